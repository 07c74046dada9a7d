"""Complex symbol timing recovery (symSyncC) without a GPU: the CPU restatement's behaviour (chunking, fault
rule, lock on pulse-shaped QPSK), the new entry points' argument checks, and the kernel's resource usage and ISA."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import composable_sdr_amd as cs
from composable_sdr_amd import _lib
import symsyncc_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, np.complex64).view(np.uint32)


def test_setters_and_complex_calls_validate_before_anything_else():
    """NULL is CSDR_ERR_INVALID for every new entry point, device or not; with a device a wrong H_len and NULL taps are too"""
    L = cs.lib()
    H = np.ones(2 * 32 * 2 * 3 + 1, f32)
    y, ny = np.zeros(32, f32), np.zeros(1, np.uint32)
    hp, yp, nyp = H.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), ny.ctypes.data_as(C.POINTER(C.c_uint32))
    assert L.csdr_symsync_set_taps(None, hp, H.size) == _lib.ERR_INVALID
    assert L.csdr_symsync_set_rnyquist(None, cs.CSDR_FIRFILT_ARKAISER, 0.5) == _lib.ERR_INVALID
    assert L.csdr_symsync_process_c(None, yp, 4, yp, nyp) == _lib.ERR_INVALID
    assert L.csdr_symsync_process_c_device(None, yp, 4, yp, yp, None) == _lib.ERR_INVALID
    if L.csdr_device_count() > 0:
        s = cs.SymSync(2, 3, 0.0, 32, lf_bw=0.01, k_out=1)
        before = s.taps()
        assert L.csdr_symsync_set_taps(s.h, hp, H.size - 1) == _lib.ERR_INVALID
        assert L.csdr_symsync_set_taps(s.h, hp, H.size + 32) == _lib.ERR_INVALID
        assert L.csdr_symsync_set_taps(s.h, None, H.size) == _lib.ERR_INVALID
        assert L.csdr_symsync_set_rnyquist(s.h, 8, 0.5) == _lib.ERR_INVALID
        assert L.csdr_symsync_set_rnyquist(s.h, cs.CSDR_FIRFILT_RRC, 0.0) == _lib.ERR_INVALID
        assert L.csdr_symsync_process_c(s.h, yp, 4, yp, None) == _lib.ERR_INVALID
        after = s.taps()
        s.close()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


def test_symsyncc_without_gpu_is_nodev():
    if cs.lib().csdr_device_count() > 0:
        r = cs.symSyncC(3, 2)._start()                         # with a device the Pipe's resource is the object
        assert r.taps_len == 12 and r.npfb == 32
        r.close()
        return
    with pytest.raises(cs.CsdrError) as e:
        cs.symSyncC(3, 2)._start()
    assert e.value.code == _lib.ERR_NODEV


def test_restatement_design_of_the_reference_settings():
    P = R.design(2, 3, 32, 0.01, 1)
    assert (P["H_len"], P["L"]) == (385, 12) and P["mf"].shape == P["dmf"].shape == (12, 32)
    assert np.abs(P["H"] * P["dH"]).max() == pytest.approx(0.06, rel=1e-6)
    assert np.array_equal(P["mf"][-1], P["H"][:32]) and np.array_equal(P["mf"][0], P["H"][11 * 32:12 * 32])
    # sum h^2 = k npfb over the prototype: every one of the npfb matched sub-filters carries about k of it
    assert float(np.sum(P["H"].astype(np.float64) ** 2)) == pytest.approx(64.0, rel=1e-6)
    s = R.SymSyncC(1)
    assert s.dl[0] == s.rate[0] == f32(2.0) and s.hist.dtype == np.complex64


def test_restatement_chunking_is_bit_identical():
    x, _ = R.psk(800, 2, seed=2)
    one = R.run_calls(x, [x.size])[0][0]
    for c in (1, 7, 333):
        calls = [c] * (x.size // c) + ([x.size % c] if x.size % c else [])
        got = R.run_calls(x, calls)[0][0]
        assert np.array_equal(_bits(got), _bits(one)), c


def test_restatement_real_input_equals_the_real_restatement():
    """CF32 rows with a zero imaginary part run the real synchroniser's arithmetic on the same banks: q's second product is 0"""
    import symsync_restatement as S
    x, _ = R.psk(500, 2, bits_per_symbol=1, seed=5)
    P = R.design(2, 3, 32, 0.01, 1)
    yc = R.run_calls(x.real.astype(np.complex64), [x.size], banks=(P["mf"], P["dmf"]))[0][0]
    yr = S.run_calls(x.real.astype(f32), [x.size], k=2, m=3, M=32, lf_bw=0.01, k_out=1, banks=(P["mf"], P["dmf"]))[0][0]
    assert np.array_equal(yc.real.view(np.uint32), yr.view(np.uint32)) and not yc.imag.any()


def test_restatement_fault_rule_del_not_positive_stops_and_sticks():
    """a steep, huge decaying exponential keeps q at -1 and drives del to <= 0: the stream stops within the call, is flagged and
    stays silent; the other stream is untouched; reset clears the flag.  The GPU is not driven into the rule"""
    n = 4096
    r = (1e36 * np.exp(-np.arange(n) / 100.0)).astype(f32)
    x, _ = R.psk(n // 2 + 40, 2, seed=3)
    X = np.stack([(r * (1 + 1j)).astype(np.complex64), x[:n]])
    s = R.SymSyncC(2, lf_bw=0.05)
    y, ny = s.process(X)
    assert s.fault.tolist() == [True, False]
    assert 0 < ny[0] <= n and not (s.dl[0] > 0)
    y2, ny2 = s.process(X)
    assert ny2[0] == 0 and ny2[1] > 0 and s.fault.tolist() == [True, False]
    got = np.concatenate([y[1, :ny[1]], y2[1, :ny2[1]]])
    want = R.run_calls(np.concatenate([x[:n], x[:n]]), [n, n], lf_bw=0.05)[0][0]
    assert np.array_equal(_bits(got), _bits(want))
    s.reset()
    assert not s.fault.any() and s.dl[0] == f32(2.0)


def test_restatement_fault_rule_capacity():
    """k_out = k asks for one output per input sample; a transmitter 3000 ppm fast needs more than n outputs in a call of n
    samples: the stream fills the call's capacity, stops and stays flagged"""
    x, _ = R.psk(1500, 2, ppm=3000.0, seed=4)
    s = R.SymSyncC(1, k_out=2)
    y, ny = s.process(x)
    assert s.fault[0] and ny[0] == x.size and s.dl[0] < f32(1.0)
    y2, ny2 = s.process(x[:100])
    assert ny2[0] == 0 and s.fault[0]


LOCK = [(2, 3, 1, R.ARKAISER, 0.37, 200.0), (4, 3, 1, R.ARKAISER, 1.6, -200.0), (4, 4, 1, R.RRC, 2.3, 200.0),
        (4, 3, 2, R.ARKAISER, 3.1, 150.0)]


@pytest.mark.parametrize("k,m,k_out,ftype,offset,ppm", LOCK)
def test_timing_recovery_locks_on_qpsk(k, m, k_out, ftype, offset, ppm):
    """3000 QPSK symbols, npfb 32, lf_bw 0.01: no decision error after the first 500 symbols at the best lag, the final rate
    within 1e-3 of k / (k_out (1 + ppm 1e-6)) and an EVM against the best complex gain of at most 0.05.
    The f32 restatement gives EVM 0.018, 0.025, 0.008 and 0.032 for the four cases (0.05 is the issue's bound: twice the
    worst of a cruder f64 model; the residue is the short filter's ISI)"""
    x, sym = R.psk(3000, k, m, ftype, 0.5, offset, ppm, seed=1)
    outs, _, marks, s = R.run_calls(x, [x.size], k=k, m=m, M=32, lf_bw=0.01, k_out=k_out, ftype=ftype, beta=0.5)
    e, n, lag, evm = R.decide(outs[0], marks[0], sym, 500)
    want = k / (k_out * (1.0 + ppm * 1e-6))
    print(f"({k},{m},{k_out},{ftype},{offset},{ppm}): {e} errors in {n} symbols (lag {lag}), EVM {evm:.4f}, "
          f"rate {s.rate[0]:.6f} (want {want:.6f})")
    assert not s.fault.any()
    assert e == 0 and n >= 2400
    assert abs(float(s.rate[0]) - want) <= 1e-3
    assert evm <= 0.05


def test_symsyncc_kernel_has_no_scratch_and_no_contraction(tmp_path):
    """k_symsyncc keeps its state and the staged block in registers / LDS; its only fused multiply-adds are the two correctly
    rounded divisions' v_div_scale / v_div_fmas / v_div_fixup sequences (re and im of y = mf / k)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "composable_sdr_amd", "csrc", "kernels_symsyncc.hip")
    out = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-c", src, "-o", str(tmp_path / "ssc.o"),
                          "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    blocks = {b.splitlines()[0]: b for b in re.split(r"remark: Function Name: ", out.stderr)[1:]}
    names = [n for n in blocks if "k_symsyncc" in n]
    assert len(names) == 1
    b = blocks[names[0]]
    assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0
    assert int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) == 0
    asm = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", src, "-o", "-"],
                         capture_output=True, text=True, timeout=600).stdout
    assert "v_div_scale_f32" in asm and "v_div_fmas_f32" in asm and "v_div_fixup_f32" in asm
    ndiv = len(re.findall(r"^\s+v_div_fixup_f32", asm, re.M))
    fmas = re.findall(r"^\s+(v_fma\w*|v_fmac\w*|v_mac\w*|v_mad\w*f32|v_pk_fma\w*)", asm, re.M)
    assert 2 <= ndiv and len(fmas) <= 5 * ndiv, (ndiv, fmas)       # each division's Newton-Raphson steps only
    assert ndiv <= 4, ndiv
    assert "ds_read_b64" in asm or "ds_read2_b64" in asm            # the windows are read a pair at a time
