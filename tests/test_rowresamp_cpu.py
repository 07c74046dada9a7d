"""The row resampler (csdr_rowresamp_*, "csdr rowresamp v1") as far as it shows without a GPU: the design
function against the numpy design, the filter property of the interpolated bank, the integer timing, the launch shape, the
premises of the GPU tests' bounds on the restatements alone, the life-cycle of the handle, the names of the C ABI and the
kernel's register budget."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fsk_restatement as F
import rowresamp_restatement as R
from rowresamp_cases import (AS_DB, CASES, FSK_BW, FSK_K, FSK_LAG, IDS, RATES, fsk_rows, length, rows as _rows, samples_for, shape as _shape,
                             tile_cuts)
import composable_sdr_amd as cs
from composable_sdr_amd import _lib
from composable_sdr_amd import RowResamp, rowResampler, firdes_rowresamp  # noqa: F401  (nothing here runs without them)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
f32 = np.float32
INF, NAN = float("inf"), float("nan")
NAMES = ["csdr_rowresamp_design", "csdr_rowresamp_launch_shape", "csdr_rowresamp_open", "csdr_rowresamp_max_out", "csdr_rowresamp_count",
         "csdr_rowresamp_process", "csdr_rowresamp_process_device", "csdr_rowresamp_rewind", "csdr_rowresamp_get_design",
         "csdr_rowresamp_get_time", "csdr_rowresamp_destroy"]
LDS_LIMIT = 160 * 1024


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---------------------------------------------------------------------------- the design
@pytest.mark.parametrize("m", [1, 7])
@pytest.mark.parametrize("as_db", [40.0, 60.0, 80.0])
def test_design_equals_the_numpy_design(m, as_db):
    for rate in RATES:
        bank, delta = cs.firdes_rowresamp(rate, m, as_db)
        want, want_delta = R.design(rate, m, as_db)
        assert delta == want_delta == R.delta_of(rate)
        D = 1 if rate >= 1 else int(np.ceil(1.0 / rate))
        assert R.D_of(delta) == D and bank.dtype == f32 and bank.shape == want.shape == (257, 2 * m * D)
        ulp = float(np.spacing(f32(np.abs(want).max())))
        err = float(np.abs(bank.astype(np.float64) - want.astype(f32).astype(np.float64)).max())
        assert err <= 2 * ulp, (rate, err / ulp)
        assert np.array_equal(bank[256, :-1], bank[0, 1:])                 # row 256 is row 0 one sample later


def _response(bank):
    """(f, |H(f)|) for 0 <= f <= 8 cycles per input sample on a grid of 2^-12: the frequency response of the bank as the
    continuous kernel the resampler applies: the taps g[b + 256 j] at tau = j + b / 256, joined by straight lines (the mu
    interpolation): the transform of the samples (a zero-padded FFT) times that of the triangle, sinc^2(f / 256) / 256"""
    bank = np.asarray(bank, np.float64)
    g = np.concatenate([bank[:256].T.reshape(-1), bank[256, -1:]])
    f = np.arange(8 * 4096 + 1) / 4096.0
    return f, np.sinc(f / 256.0) ** 2 / 256.0 * np.abs(np.fft.rfft(g, n=256 * 4096)[:f.size])


@pytest.mark.parametrize("m", [1, 7])
@pytest.mark.parametrize("as_db", [40.0, 60.0, 80.0])
def test_the_interpolated_bank_is_the_low_pass_it_was_designed_as(m, as_db):
    """|H| deviates from 1 by at most 1.5 delta_r up to fc - tw / 2 and stays below 1.5 delta_r from fc + tw / 2 to 8, with
    delta_r = 10^(-as / 20) and Kaiser's transition width tw = (as - 7.95) / (14.36 P).  Measured at m = 7: at most 1.17 delta_r.
    At m = 1 (P = 2 .. 16 taps per phase) Kaiser's width formula, an asymptotic fit, is too narrow: 1.97 delta_r in the pass band
    and 1.58 in the stop band with tw; with 1.5 tw both stay below 1.0, and that wider band edge is what m = 1 is held to."""
    delta_r = 10.0 ** (-as_db / 20.0)
    worst_p = worst_s = 0.0
    for rate in RATES:
        bank, delta = cs.firdes_rowresamp(rate, m, as_db)
        P, fc = bank.shape[1], R.fc_of(rate)
        tw = (1.5 if m == 1 else 1.0) * (as_db - 7.95) / (14.36 * P)
        f, H = _response(bank)
        if fc - tw / 2 > 0:
            worst_p = max(worst_p, float(np.abs(H[f <= fc - tw / 2] - 1.0).max()))
        worst_s = max(worst_s, float(H[f >= fc + tw / 2].max()))
    print(f"rowresamp m {m} as {as_db:g}: pass band {worst_p / delta_r:.3f} delta_r, stop band {worst_s / delta_r:.3f} delta_r")
    assert worst_p <= 1.5 * delta_r and worst_s <= 1.5 * delta_r


# ---------------------------------------------------------------------------- the integer timing
@pytest.mark.parametrize("rate", RATES)
def test_counts_add_up_for_every_splitting(rate):
    delta = R.delta_of(rate)
    rng = np.random.default_rng(int(rate * 1000))
    for n in (1, 37, 3000, 100003):
        whole = R.count(0, delta, n)
        assert whole == -(-(n << 32) // delta)                            # the outputs at times below n: ceil(n 2^32 / delta)
        for _ in range(5):
            T, total, left = 0, 0, n
            while left:
                c = int(min(left, rng.integers(0, 40) if rng.random() < 0.7 else rng.integers(0, left + 1)))
                got, T = R.step(T, delta, c)
                assert 0 <= T < delta + (1 << 32)
                total, left = total + got, left - c
            assert total == whole


def test_samples_for_is_the_shortest_call_with_that_many_outputs():
    for rate in RATES:
        delta = R.delta_of(rate)
        for T in (0, 1, delta - 1):
            for c in (1, 2, 511, 1024):
                k = samples_for(T, delta, c)
                assert R.count(T, delta, k) >= c and R.count(T, delta, k - 1) < c


# ---------------------------------------------------------------------------- the launch shape
@pytest.mark.parametrize("rate", RATES)
def test_every_shape_fits_the_lds_and_covers_the_call(rate):
    delta = R.delta_of(rate)
    for m in (1, 4, 7, 8):
        if m * R.D_of(delta) > 56:
            continue
        P = R.P_of(delta, m)
        for cplx in (True, False):
            one = _shape(rate, m, cplx, 1, 1, 256)
            TO, W = one["TO"], one["window"]
            assert one["P"] == P and TO in (512, 1024) and one["lds"] == 4 * 265 * P + (8 if cplx else 4) * W <= LDS_LIMIT
            assert 1 <= one["wgs_per_cu"] <= 4 and one["wgs_per_cu"] * one["lds"] <= LDS_LIMIT
            for T in (0, 1, delta - 1):
                for n_out in (1, TO - 1, TO, TO + 1, 3 * TO + 5):
                    for nchan, cus in ((1, 256), (3, 7), (300, 256), (700, 8)):
                        s = _shape(rate, m, cplx, n_out, nchan, cus, T)
                        items = s["tiles"] * nchan
                        assert s["tiles"] == -(-n_out // TO)                 # tile i is outputs [i TO, min((i + 1) TO, n_out)): each output once
                        assert s["runs"] <= cus * s["wgs_per_cu"] and s["runs"] * s["items_per_run"] >= items
                        assert (s["runs"] - 1) * s["items_per_run"] < items  # no empty workgroup
                        assert s["items_per_run"] == 1 or items > cus * s["wgs_per_cu"]
                    for tile in range(-(-n_out // TO)):
                        o0, o1 = tile * TO, min((tile + 1) * TO, n_out)
                        first, last = (T + o0 * delta) >> 32, (T + (o1 - 1) * delta) >> 32
                        assert last - first + P <= W, (rate, m, T, n_out, tile)   # samples first - (P - 1) .. last fit the window
    assert _shape(rate, 1, True, 0, 5, 256)["runs"] == 0


def test_launch_shape_refuses_bad_arguments():
    s = (C.c_uint32 * 8)()
    L = _lib.lib()
    for args in ((0.1, 7, 1, 10, 1, 256, 0), (9.0, 7, 1, 10, 1, 256, 0), (0.48, 0, 1, 10, 1, 256, 0), (0.48, 9, 1, 10, 1, 256, 0),
                 (0.125, 8, 1, 10, 1, 256, 0), (0.48, 7, 1, 10, 0, 256, 0), (0.48, 7, 1, 10, 1, 0, 0), (NAN, 7, 1, 10, 1, 256, 0)):
        assert L.csdr_rowresamp_launch_shape(*args, s) == _lib.ERR_INVALID, args
    assert L.csdr_rowresamp_launch_shape(0.48, 7, 1, 10, 1, 256, 0, None) == _lib.ERR_INVALID


# ---------------------------------------------------------------------------- the premises of the GPU tests' bounds
@pytest.mark.parametrize("rate,m,cplx", CASES, ids=IDS)
def test_the_f32_yardstick_stays_within_the_element_bound(rate, m, cplx):
    """|yardstick - truth| <= (P + 3) 2^-24 A_k for every element: the bound the GPU tests hold the kernel to leaves an f32
    evaluation in the kernel's order of operations this much room"""
    bank, delta = cs.firdes_rowresamp(rate, m, AS_DB)
    x = _rows(1, length(rate, m), cplx, 5)
    truth, A = R.truth(bank, delta, x)
    ratio = R.worst_ratio(R.yardstick(bank, delta, x), truth, A, bank.shape[1])
    print(f"rowresamp yardstick rate {rate:.4g} m {m} {'c' if cplx else 'r'}: worst ratio {ratio:.3f}")
    assert truth.shape[1] == R.count(0, delta, x.shape[1]) and ratio <= 1.0
    assert len(tile_cuts(rate, m, x.shape[1])) == 4 and min(tile_cuts(rate, m, x.shape[1])) > 0


def test_the_f64_chain_of_the_end_to_end_case_decodes_without_error():
    """2-FSK at 25 / 3 samples per symbol behind 4 zeros, resampled by 0.48 in f64 with the f32 bank, demodulated at 4 samples
    per symbol: delay (21) plus padding (4) is 25 samples = 3 symbols, and from symbol 3 on every decision is right"""
    sym, x = fsk_rows()
    bank, delta = cs.firdes_rowresamp(0.48, 7, AS_DB)
    assert bank.shape[1] // 2 + 4 == 25
    y, _ = R.truth(bank, delta, x)
    got, E = F.demod_ref(y.astype(np.complex64), 1, FSK_K, FSK_BW)
    ns = got.shape[1]
    assert ns >= 399
    errors = int((got[:, FSK_LAG:] != sym[:, :ns - FSK_LAG]).sum())
    E = np.sort(E[:, FSK_LAG:], axis=-1)
    margin = float(((E[..., 1] - E[..., 0]) / E[..., 1]).min())
    print(f"rowresamp end to end in f64: {errors} errors of {ns - FSK_LAG} symbols per row, smallest margin {margin:.2f} of the larger bin")
    assert errors == 0


# ---------------------------------------------------------------------------- life-cycle, as test_pfbch2_cpu.py has it
GOOD = [
    (0.48, 7, 60.0, 0.0, 1, 3, 16),
    (0.125, 7, 120.0, 0.1, 0, 1, 1),
    (8.0, 8, 40.0, 0.0, 1, 2, 1 << 10),
]
BAD = [
    (0.1249, 7, 60.0, 0.0, 1, 1, 16),             # rate outside 1/8 .. 8 or not finite
    (8.01, 7, 60.0, 0.0, 1, 1, 16),
    (0.0, 7, 60.0, 0.0, 1, 1, 16),
    (-1.0, 7, 60.0, 0.0, 1, 1, 16),
    (NAN, 7, 60.0, 0.0, 1, 1, 16),
    (INF, 7, 60.0, 0.0, 1, 1, 16),
    (0.48, 0, 60.0, 0.0, 1, 1, 16),               # m outside 1 .. 8
    (0.48, 9, 60.0, 0.0, 1, 1, 16),
    (0.125, 8, 60.0, 0.0, 1, 1, 16),              # m D = 64 > 56
    (0.48, 7, 0.0, 0.0, 1, 1, 16),                # as_db outside (0, 120] or not finite
    (0.48, 7, -60.0, 0.0, 1, 1, 16),
    (0.48, 7, 120.5, 0.0, 1, 1, 16),
    (0.48, 7, INF, 0.0, 1, 1, 16),
    (0.48, 7, NAN, 0.0, 1, 1, 16),
    (0.48, 7, 60.0, -0.1, 1, 1, 16),              # fc < 0, >= 0.5 or not finite
    (0.48, 7, 60.0, 0.5, 1, 1, 16),
    (0.48, 7, 60.0, NAN, 1, 1, 16),
    (0.48, 7, 60.0, 0.0, 1, 0, 16),               # nchan = 0
    (0.48, 7, 60.0, 0.0, 1, 1, 0),                # max_samples outside 1 .. 2^28
    (0.48, 7, 60.0, 0.0, 1, 1, (1 << 28) + 1),
]


@pytest.mark.parametrize("good", GOOD, ids=[str(i) for i in range(len(GOOD))])
def test_valid_arguments_need_a_device_and_nothing_else(good):
    h = C.c_void_p()
    rc = _lib.lib().csdr_rowresamp_open(*good, C.byref(h))
    if _lib.lib().csdr_device_count() > 0:
        _lib.check(rc)
        assert h.value
        assert _lib.lib().csdr_rowresamp_destroy(h) == 0
    else:
        with pytest.raises(cs.CsdrError) as e:
            _lib.check(rc)
        assert e.value.code == _lib.ERR_NODEV and "no CPU fallback" in str(e.value)
        assert not h.value


@pytest.mark.parametrize("bad", BAD, ids=[str(i) for i in range(len(BAD))])
def test_invalid_arguments_are_refused_before_the_device_is_looked_for(bad):
    h = C.c_void_p()
    with pytest.raises(cs.CsdrError) as e:
        _lib.check(_lib.lib().csdr_rowresamp_open(*bad, C.byref(h)))
    assert e.value.code == _lib.ERR_INVALID
    assert not h.value


def test_a_null_out_pointer_is_refused_and_the_design_takes_null_pointers():
    L = _lib.lib()
    assert L.csdr_rowresamp_open(0.48, 7, 60.0, 0.0, 1, 1, 16, None) == _lib.ERR_INVALID
    assert L.csdr_rowresamp_design(0.48, 7, 60.0, 0.0, None, None, None) == 0
    P, delta = C.c_uint32(), C.c_uint64()
    assert L.csdr_rowresamp_design(0.48, 7, 60.0, 0.0, C.byref(P), C.byref(delta), None) == 0
    assert P.value == 42 and delta.value == R.delta_of(0.48)
    for args in ((0.1, 7, 60.0, 0.0), (0.48, 9, 60.0, 0.0), (0.125, 8, 60.0, 0.0), (0.48, 7, 0.0, 0.0), (0.48, 7, 121.0, 0.0),
                 (0.48, 7, 60.0, 0.5), (0.48, 7, INF, 0.0), (0.48, 7, 60.0, NAN), (NAN, 7, 60.0, 0.0)):
        assert L.csdr_rowresamp_design(*args, C.byref(P), C.byref(delta), None) == _lib.ERR_INVALID, args
    with pytest.raises(cs.CsdrError):
        cs.firdes_rowresamp(9.0)


def test_destroy_takes_null_and_rewind_and_the_calls_refuse_it():
    L = _lib.lib()
    assert L.csdr_rowresamp_destroy(None) == 0
    assert L.csdr_rowresamp_rewind(None) == _lib.ERR_INVALID
    n, t = C.c_uint32(), C.c_uint64()
    x = np.zeros(4, np.complex64)
    assert L.csdr_rowresamp_process(None, _p(x), 2, _p(x), C.byref(n)) == _lib.ERR_INVALID
    assert L.csdr_rowresamp_process_device(None, _p(x), 2, _p(x), C.byref(n), None) == _lib.ERR_INVALID
    assert L.csdr_rowresamp_count(None, 2, C.byref(n)) == _lib.ERR_INVALID
    assert L.csdr_rowresamp_get_design(None, None, None, None, None) == _lib.ERR_INVALID
    assert L.csdr_rowresamp_get_time(None, C.byref(t)) == _lib.ERR_INVALID
    assert L.csdr_rowresamp_max_out(None, 2) == 0


def test_the_pipe_needs_a_device_and_nothing_else():
    pipe = cs.rowResampler(0.48, nchan=3)
    if _lib.lib().csdr_device_count() > 0:
        pipe._done(pipe._start())
    else:
        with pytest.raises(cs.CsdrError) as e:
            pipe._start()
        assert e.value.code == _lib.ERR_NODEV and "no CPU fallback" in str(e.value)


# ---------------------------------------------------------------------------- the names
def test_every_name_is_declared_bound_and_exported_and_none_is_a_create_or_a_reset():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "csdr.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(csdr_[a-z0-9_]+)\s*\(", src))
    lib = C.CDLL(cs.lib_path())
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("csdr_rowresamp_")) == sorted(NAMES)
    for n in NAMES:
        assert n in declared and hasattr(lib, n), n
        # test_block_lifecycle_cpu.py pins the set of names with `_create` in them and of names that end in `_reset`; this block's
        # constructor is `open` and its reset is `rewind`, and this file holds its life-cycle cases
        assert "_create" not in n and not n.endswith("_reset"), n
    for n in ("RowResamp", "rowResampler", "firdes_rowresamp"):
        assert hasattr(cs, n), n


# ---------------------------------------------------------------------------- the build
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_k_rowresamp_has_no_scratch_and_no_spills(tmp_path):
    """The FIR loop keeps two running sums, a window pointer and a bank pointer per output: nothing of it may live in scratch"""
    src = os.path.join(ROOT, "composable_sdr_amd", "csrc")
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-c", os.path.join(src, "kernels_rowresamp.hip"),
                          "-o", str(tmp_path / "rr.o"), "-Rpass-analysis=kernel-resource-usage"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    blocks = [b for b in re.split(r"remark: Function Name: ", out.stderr)[1:] if "k_rowresamp" in b.splitlines()[0]]
    assert len(blocks) == 4                               # k_rowresamp<CF32 | F32> and k_rowresamp_hist<CF32 | F32>
    for b in blocks:
        assert int(re.search(r"SGPRs Spill: (\d+)", b).group(1)) == 0 and int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) == 0, b[:600]
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, b[:600]
        # four workgroups of 512 threads per CU (RRS_MAX_WGS_PER_CU, where the bank is small) are 8 waves per SIMD: at most 64 VGPRs
        assert int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1)) == 8, b[:600]
