"""pskTracker and symTracker without a GPU: the contract's sine and cosine against their restatement and f64, the
f32 restatement's lock on impaired BPSK / QPSK, its equaliser on two-path channels, the composition behind the symbol
synchroniser's restatement, chunking and parity, the C ABI's life-cycle and symbols, the kernel's resources and the Pipe's
marshalling."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import composable_sdr_amd as cs
from composable_sdr_amd import _lib, pipes
import psktrack_cases as K
import psktrack_restatement as R
import symsyncc_restatement as SC
import test_pipes_marshal_cpu as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, c64, u32 = np.float32, np.complex64, np.uint32
NAMES = ["csdr_psktrack_new", "csdr_psktrack_restart", "csdr_psktrack_process", "csdr_psktrack_process_device",
         "csdr_psktrack_get_state", "csdr_psktrack_get_design", "csdr_psktrack_destroy", "csdr_sincos_word"]
GOOD = (2, 2, 0, 9, 0.05, 0, 200, 9e-4, 0.02, 1, 16)
BAD = [(3, 2, 0, 9, 0.05, 0, 200, 9e-4, 0.02, 1, 16), (2, 1, 0, 9, 0.05, 0, 200, 9e-4, 0.02, 1, 16),
       (2, 2, 0, 8, 0.05, 0, 200, 9e-4, 0.02, 1, 16), (2, 2, 0, 19, 0.05, 0, 200, 9e-4, 0.02, 1, 16),
       (2, 2, 2, 9, 0.05, 0, 200, 9e-4, 0.02, 1, 16), (2, 2, 0, 9, float("nan"), 0, 200, 9e-4, 0.02, 1, 16),
       (2, 2, 0, 9, 0.05, 2, 200, 9e-4, 0.02, 1, 16), (2, 2, 0, 9, 0.05, 0, 200, 2.0, 0.02, 1, 16),
       (2, 2, 0, 9, 0.05, 0, 200, 9e-4, -0.1, 1, 16), (2, 2, 0, 9, 0.05, 0, 200, 9e-4, 0.02, 0, 16)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- sine and cosine
def test_sincos_word_equals_the_restatement_and_stays_within_2_to_the_minus_21():
    """the 2^20 words i << 12 and 10^5 random words: csdr_sincos_word and the numpy restatement agree bit for bit, and the
    largest error against f64 is 1.08e-7 (measured; the cap is 2^-21 = 4.8e-7, fm_common.h's atan2 has 1.2e-7)"""
    w = np.concatenate([np.arange(1 << 20, dtype=np.uint64) << 12,
                        np.random.default_rng(1).integers(0, 1 << 32, 100000, dtype=np.uint64)]).astype(u32)
    s, c = R.sincos_word(w)
    fn = _lib.lib().csdr_sincos_word
    gs, gc = C.c_float(), C.c_float()
    ps, pc = C.byref(gs), C.byref(gc)
    hs, hc = np.empty(w.size, f32), np.empty(w.size, f32)
    for i, v in enumerate(w.tolist()):
        fn(v, ps, pc)
        hs[i], hc[i] = gs.value, gc.value
    assert np.array_equal(_bits(hs), _bits(s)) and np.array_equal(_bits(hc), _bits(c))
    a = w.astype(np.float64) * (2.0 * np.pi / 2.0 ** 32)
    err = max(float(np.abs(s - np.sin(a)).max()), float(np.abs(c - np.cos(a)).max()))
    print(f"sincos_word: max |error| = {err:.3e}")
    assert err <= 2.0 ** -21
    assert fn(0, None, pc) == _lib.ERR_INVALID
    s1, c1 = cs.sincos_word(1 << 30)                            # a quarter turn
    assert (s1, c1) == (1, 0) and cs.sincos_word(0) == (0, 1)


def test_word_rounds_clamps_and_drops_nan():
    v = np.array([0.0, 1e-9, 1e-6, -1e-6, 10.0, -10.0, np.inf, -np.inf, np.nan, 2.4 * np.pi / 2 ** 31], f32)
    got = R.word(v).astype(np.int64)
    got = np.where(got >= 1 << 31, got - (1 << 32), got)
    assert got.tolist() == [0, 1, 684, -684, 1 << 30, -(1 << 30), 1 << 30, -(1 << 30), 0, 2]


# ---------------------------------------------------------------------------------------------------------------- lock
CONFIGS = [dict(sps=1), dict(sps=2, eq_len=9, eq_mode=R.DD), dict(sps=2, eq_len=9, eq_mode=R.CM)]


@pytest.mark.parametrize("bits", [1, 2])
@pytest.mark.parametrize("cfg", CONFIGS, ids=["sps1", "sps2-dd9", "sps2-cm9"])
def test_the_f32_restatement_locks(bits, cfg):
    """3000 symbols, RRC 0.25 m 5, ideal timing, at the three (offset, phase, amplitude) conditions: no decision error after
    the first 500 symbols at the best rotation, EVM (against the best real gain) <= 0.05, final freq within 2 % of the offset
    (of 0.002 cycles per symbol where the offset is 0: the loop's jitter does not depend on the offset).
    Measured, f32 restatement: 0 errors everywhere; EVM 0.0116 .. 0.0119 at sps 1, 0.0155 .. 0.0168 with the equaliser; freq off by
    at most 0.61 % (QPSK, constant modulus), 0.22 % (QPSK, decision-directed), 0.05 % elsewhere.  The f64 twin gives the same
    figures to the digits shown."""
    X, pts, num = K.rows(3000, bits, cfg["sps"], seed=bits)
    y, k, _, s = R.run_calls(X, [X.shape[1]], bits=bits, **cfg)
    f = s.freq_cycles_per_symbol()
    for r, (offset, _, _) in enumerate(K.CONDITIONS):
        e, n, evm = K.score(y[r], k[r], pts, num, bits, 500)
        rel = abs(f[r] - offset) / max(abs(offset), 0.002)
        print(f"bits {bits} {cfg} {K.CONDITIONS[r]}: {e} errors in {n}, EVM {evm:.4f}, freq {f[r]:.6f} ({100 * rel:.2f} %)")
        assert e == 0 and n >= 2400
        assert evm <= 0.05
        assert rel <= 0.02


def test_the_f64_twin_runs_the_same_loop():
    """the twin differs from the f32 restatement by rounding only: same decisions, soft symbols within 1e-4"""
    X, _, _ = K.rows(600, 2, 2, seed=3, conditions=K.CONDITIONS[1:2])
    kw = dict(bits=2, sps=2, eq_len=9, eq_mode=R.DD, eq_delay=100)
    y32, k32, _, _ = R.run_calls(X, [X.shape[1]], **kw)
    y64, k64, _, _ = R.run_calls(X, [X.shape[1]], dtype=np.float64, **kw)
    assert y64[0].dtype == np.complex128 and np.array_equal(k32[0], k64[0])
    assert np.abs(y32[0] - y64[0]).max() < 1e-4


# ---------------------------------------------------------------------------------------------------------------- equaliser
@pytest.mark.parametrize("bits", [1, 2])
@pytest.mark.parametrize("ch", [0, 1])
def test_the_equaliser_on_two_path_channels(ch, bits):
    """[1, 0.3 e^j] and [1, 0, 0.3 e^j] in T/2 taps: decision-directed with 9 taps makes no error after 500 symbols and at most
    half the EVM of sps 1 without an equaliser on the same signal; constant modulus makes no error (its EVM is recorded).
    Measured (none / DD / CM): channel 0 BPSK 0.192 / 0.031 / 0.131, QPSK 0.185 / 0.033 / 0.038; channel 1 BPSK 0.305 / 0.036 /
    0.264, QPSK 0.300 / 0.038 / 0.046 (constant modulus leaves BPSK's quadrature component alone)"""
    X2, pts, num = K.rows(3000, bits, 2, seed=40 + bits, channel=K.CHANNELS[ch])
    evm = {}
    for name, X, cfg in (("none", X2[:, ::2], dict(sps=1)), ("dd", X2, dict(sps=2, eq_len=9, eq_mode=R.DD)),
                         ("cm", X2, dict(sps=2, eq_len=9, eq_mode=R.CM))):
        y, k, _, _ = R.run_calls(X, [X.shape[1]], bits=bits, **cfg)
        res = [K.score(y[r], k[r], pts, num, bits, 500) for r in range(len(K.CONDITIONS))]
        evm[name] = [v[2] for v in res]
        print(f"channel {ch} bits {bits} {name}: errors {[v[0] for v in res]}, EVM {[round(v[2], 4) for v in res]}")
        if name != "none":
            assert all(v[0] == 0 and v[1] >= 2400 for v in res)
    assert all(d <= 0.5 * n for d, n in zip(evm["dd"], evm["none"]))


# ---------------------------------------------------------------------------------------------------------------- composition
def test_behind_the_symbol_synchronisers_restatement():
    """symsyncc_restatement (RRC 0.25, m 4, k 4, npfb 16, k_out 2, lf_bw 0.01) then this restatement (BPSK, sps 2, 9 taps,
    constant modulus, phase = SYMTRACK_PHASE): 4000 BPSK symbols of unit amplitude, timing offset 1.6 samples, 100 ppm, carrier
    0.001 cycles per symbol.  The synchroniser's loop instants are its even outputs, which is SYMTRACK_PHASE = 0.  No error
    after the first 1000 symbols at the best rotation; measured: 0 errors in 2991, freq 0.0009998 cycles per symbol.
    Used: lf_bw 0.01, phase 0 (the values the issue chose; neither had to be varied)."""
    x, sym = SC.psk(4000, 4, 4, SC.RRC, 0.25, 1.6, 100.0, bits_per_symbol=1, seed=7)
    x = (x * np.exp(2j * np.pi * 0.001 * np.arange(x.size) / 4)).astype(c64)
    outs, _, marks, s = SC.run_calls(x, [x.size], k=4, m=4, M=16, lf_bw=0.01, k_out=2, ftype=SC.RRC, beta=0.25)
    assert not s.fault.any()
    at = np.nonzero(marks[0])[0]
    assert at.size > 3900 and np.all(at % 2 == pipes.SYMTRACK_PHASE)
    y, k, _, t = R.run_calls(outs[0], [outs[0].size], bits=1, sps=2, phase=pipes.SYMTRACK_PHASE, eq_len=9, eq_mode=R.CM)
    got = k[0][1000:]
    best = None
    for lag in range(960, 1040):
        for flip in (0, 1):
            want = (sym[lag:lag + got.size].real < 0).astype(u32) ^ flip
            n = min(want.size, got.size)
            e = int(np.sum(want[:n] != got[:n]))
            if n >= 2900 and (best is None or e < best[0]):
                best = (e, n, lag)
    f = float(t.freq_cycles_per_symbol()[0])
    print(f"composite: {best[0]} errors in {best[1]} (lag {best[2]}), freq {f:.7f}")
    assert best[0] == 0
    assert abs(f - 0.001) <= 0.02 * 0.002


# ---------------------------------------------------------------------------------------------------------------- chunking
@pytest.mark.parametrize("cfg", [dict(bits=2, sps=2, phase=1, eq_len=9, eq_mode=R.DD, eq_delay=50), dict(bits=2, sps=2, phase=0),
                                 dict(bits=1, sps=1)], ids=["sps2-eq9-phase1", "sps2-noeq", "sps1"])
def test_restatement_chunking_and_parity_are_bit_identical(cfg):
    X, _, _ = K.rows(1500, cfg["bits"], cfg["sps"], seed=9, channel=K.CHANNELS[0])
    N = X.shape[1]
    rng = np.random.default_rng(4)
    calls = [0, 1, 333, 7] + rng.integers(0, 701, 40).tolist()
    calls = calls[:int(np.searchsorted(np.cumsum(calls), N))]
    calls.append(N - sum(calls))
    assert sum(c % 2 for c in calls) >= 3 and 0 in calls
    y1, k1, c1, s1 = R.run_calls(X, [N], **cfg)
    y2, k2, c2, s2 = R.run_calls(X, calls, **cfg)
    assert c1.sum(axis=0).tolist() == c2.sum(axis=0).tolist() and abs(int(c1.sum(axis=0)[0]) - N / cfg["sps"]) < 1
    for r in range(3):
        assert np.array_equal(_bits(y1[r]), _bits(y2[r])) and np.array_equal(k1[r], k2[r])
    assert np.array_equal(s1.theta, s2.theta) and np.array_equal(s1.freq, s2.freq) and np.array_equal(_bits(s1.w), _bits(s2.w))


def test_phase_names_the_sample_under_the_centre_tap():
    """with the unit centre tap and no adaptation, output j is input sample 2 j + phase for every equaliser length"""
    x = (np.arange(1, 65) + 0j).astype(c64)
    for L in (0, 3, 5, 9, 17):
        for phase in (0, 1):
            s = R.PskTrack(1, bits=1, sps=2, phase=phase, eq_len=L, eq_delay=1 << 30, pll_bw=0.0, agc_bw=0.0)
            y, _, ny = s.process(x)
            c = (L - 1) // 2 if L else 0
            out = y[0, :ny[0]]
            lead = len([t for t in range(c) if (t + c) % 2 == phase])      # outputs whose centre sample precedes the row: zeros
            assert ny[0] == 32 and not out[:lead].any(), (L, phase)
            assert np.array_equal(out[lead:], x[phase::2][:32 - lead]), (L, phase)


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_the_new_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "csdr.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", cs.lib_path()], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, hdr) and n in _lib.SIGNATURES and n in exported, n
    assert not [n for n in NAMES if "_create" in n or "_open" in n or n.endswith(("_reset", "_rewind"))]


def test_new_validates_before_it_looks_for_a_device():
    L = _lib.lib()
    h = C.c_void_p()
    rc = L.csdr_psktrack_new(*GOOD, C.byref(h))
    if L.csdr_device_count() > 0:
        _lib.check(rc)
        assert h.value and L.csdr_psktrack_destroy(h) == 0
    else:
        with pytest.raises(cs.CsdrError) as e:
            _lib.check(rc)
        assert e.value.code == _lib.ERR_NODEV and "no CPU fallback" in str(e.value) and not h.value
    for bad in BAD:
        h = C.c_void_p()
        with pytest.raises(cs.CsdrError) as e:
            _lib.check(L.csdr_psktrack_new(*bad, C.byref(h)))
        assert e.value.code == _lib.ERR_INVALID and "psktrack: bad arguments" in str(e.value) and not h.value, bad
    assert L.csdr_psktrack_new(*GOOD, None) == _lib.ERR_INVALID


def test_null_handles():
    L = _lib.lib()
    buf = np.zeros(16, c64)
    p = buf.ctypes.data
    assert L.csdr_psktrack_destroy(None) == 0
    assert L.csdr_psktrack_restart(None) == _lib.ERR_INVALID
    assert L.csdr_psktrack_process(None, p, 4, None, p, None, p) == _lib.ERR_INVALID
    assert L.csdr_psktrack_process_device(None, p, 4, None, p, None, p, None) == _lib.ERR_INVALID
    assert L.csdr_psktrack_get_state(None, 0, None, None, None, None, None) == _lib.ERR_INVALID
    assert L.csdr_psktrack_get_design(None, None, None, None, None) == _lib.ERR_INVALID


def test_pipes_without_a_gpu_are_nodev():
    if cs.lib().csdr_device_count() > 0:
        r = cs.pskTracker(2, 2, 0, 9)._start()
        assert r.design()[2] == 9 and r.state()[3] == 0
        r.close()
        return
    for pipe in (cs.pskTracker(1), cs.symTracker(4, 4)):
        with pytest.raises(cs.CsdrError) as e:
            pipe._start()
        assert e.value.code == _lib.ERR_NODEV


# ---------------------------------------------------------------------------------------------------------------- resources
def test_kernel_has_no_spills_and_no_scratch(tmp_path):
    """k_psktrack keeps its state and the staged block in registers, weights and window in LDS"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "composable_sdr_amd", "csrc", "kernels_psktrack.hip")
    out = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-c", src, "-o", str(tmp_path / "pt.o"),
                          "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    blocks = {b.splitlines()[0]: b for b in re.split(r"remark: Function Name: ", out.stderr)[1:]}
    names = [n for n in blocks if "k_psktrack" in n]
    assert len(names) == 1
    b = blocks[names[0]]
    assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0
    assert int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) == 0
    assert int(re.search(r"SGPRs Spill: (\d+)", b).group(1)) == 0
    assert "Dynamic Stack: False" in b


# ---------------------------------------------------------------------------------------------------------------- marshalling
H0 = 0xB000


@pytest.fixture
def L(monkeypatch):
    fake = M.RecordingLib()
    fake.report["csdr_psktrack_new"] = lambda *a: (H0,)         # the stand-in knows `create` and `open` only
    monkeypatch.setattr(pipes, "lib", lambda: fake)
    return fake


def test_pipe_marshals_rows_of_unequal_length(L):
    pipe = cs.pskTracker(2, 2, 1, 9, eq_mode=cs.CSDR_PSKTRACK_EQ_CM, nchan=3, max_samples=512)
    r = pipe._start()
    assert L.calls == [("csdr_psktrack_new", (2, 2, 1, 9, 0.05, 1, 200, 9e-4, 0.02, 3, 512, M.REFH))] and r.h.value == H0
    L.fill["csdr_psktrack_process"] = (6, lambda h, x, n, nx, y, sym, ny: [nx._arr[c] // 2 if nx is not None else n // 2 for c in range(3)])
    rows = [np.arange(5) + 1j, np.zeros(0), M._strided(c64, 8)]
    mark = len(L.calls)
    got = pipe._process(r, rows)
    A = M.A
    assert L.since(mark) == [("csdr_psktrack_process", (H0, A(c64, 3, 8), 8, A(u32, 3), A(c64, 3, 8), 0, A(u32, 3)))]
    x, nx = L.raw[-1][1]._arr, L.raw[-1][3]._arr
    assert nx.tolist() == [5, 0, 8] and np.array_equal(x[0], np.r_[rows[0], 0, 0, 0]) and not x[1].any() and np.array_equal(x[2], rows[2])
    assert isinstance(got, list) and [g.shape for g in got] == [(2,), (0,), (4,)] and all(g.dtype == c64 for g in got)
    mark = len(L.calls)
    got = pipe._process(r, M._strided(c64, 3, 6))               # one 2-D array: every row holds n, no counts array
    assert L.since(mark) == [("csdr_psktrack_process", (H0, A(c64, 3, 6), 6, 0, A(c64, 3, 6), 0, A(u32, 3)))]
    assert isinstance(got, list) and [g.shape for g in got] == [(3,)] * 3
    y, sym, ny = r.process_rows(np.zeros((3, 4), c64), symbols=True)
    assert L.calls[-1] == ("csdr_psktrack_process", (H0, A(c64, 3, 4), 4, 0, A(c64, 3, 4), A(u32, 3, 4), A(u32, 3)))
    assert sym.shape == (3, 4) and sym.dtype == u32 and ny.tolist() == [2, 2, 2]
    mark = len(L.calls)
    for bad in ([np.zeros(4, c64)] * 2, np.zeros((2, 4), c64), np.zeros(7, c64)):
        with pytest.raises(cs.CsdrError) as e:
            pipe._process(r, bad)
        assert e.value.code == _lib.ERR_INVALID
    assert L.since(mark) == []
    r.process_device(M.X, 8, M.Z, M.Y, 0, M.Z + 64, M.S)
    r.restart()
    assert L.since(mark) == [("csdr_psktrack_process_device", (H0, M.X, 8, M.Z, M.Y, 0, M.Z + 64, M.S)), ("csdr_psktrack_restart", (H0,))]
    mark = len(L.calls)
    pipe._done(r)
    pipe._done(r)
    assert L.since(mark) == [("csdr_psktrack_destroy", (H0,))]
    for use in (lambda: r.h, lambda: pipe._process(r, rows), r.restart):
        with pytest.raises(cs.CsdrError) as e:
            use()
        assert e.value.code == _lib.ERR_INVALID and "psktrack already destroyed" in str(e.value)


def test_one_row_pipe_takes_and_returns_one_array(L):
    pipe = cs.pskTracker(1, nchan=1, max_samples=64)
    r = pipe._start()
    assert L.calls == [("csdr_psktrack_new", (1, 1, 0, 0, 0.05, 0, 200, 9e-4, 0.02, 1, 64, M.REFH))]
    L.fill["csdr_psktrack_process"] = (6, lambda h, x, n, nx, y, sym, ny: [n])
    got = pipe._process(r, M._strided(c64, 9))
    assert L.calls[-1] == ("csdr_psktrack_process", (H0, M.A(c64, 9), 9, 0, M.A(c64, 1, 9), 0, M.A(u32, 1)))
    assert isinstance(got, np.ndarray) and got.shape == (9,) and got.dtype == c64
    pipe._done(r)
