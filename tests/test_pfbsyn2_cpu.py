"""The synthesizer of the 2x-oversampled bank (csdr_pfbsyn2_*) as far as it shows without a GPU: the restatements
of tests/pfbsyn2_restatement.py agree with each other and do not depend on the chunking, the design function equals the numpy
design, the round trip through analyzer and synthesizer that pins both cutoff rules, the launch shape, the life-cycle of the
handle, the names of the C ABI, and three deliberate faults of the f32 restatement that the bounds of the GPU tests catch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pfbch2_restatement as A
import pfbsyn2_restatement as S
from pfbsyn2_cases import CUTS, FRAMES, rows, runs_frames, shape as _shape
import composable_sdr_amd as cs
from composable_sdr_amd import _lib
from composable_sdr_amd import Firpfbch2Synth, firpfbch2Synthesizer, firdes_pfbsyn2  # noqa: F401  (nothing here runs without them)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
INF, NAN = float("inf"), float("nan")
NAMES = ["csdr_pfbsyn2_design", "csdr_pfbsyn2_launch_shape", "csdr_pfbsyn2_open_kaiser", "csdr_pfbsyn2_open_taps", "csdr_pfbsyn2_process",
         "csdr_pfbsyn2_process_device", "csdr_pfbsyn2_rewind", "csdr_pfbsyn2_get_taps", "csdr_pfbsyn2_delay", "csdr_pfbsyn2_destroy"]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _noise_rows(M, frames, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((M, frames)) + 1j * rng.standard_normal((M, frames))) / np.sqrt(2.0)


# ---------------------------------------------------------------------------- the restatements
@pytest.mark.parametrize("M,m", [(4, 1), (8, 3), (16, 7), (256, 2)])
def test_the_structural_form_equals_the_closed_form(M, m):
    g = S.design(M, m, 80.0)[:2 * M * m]
    Y = _noise_rows(M, 37, M + m)
    ref, got = S.truth(g, Y, M), S.structural(g, Y, M, m)
    err = float(np.abs(got - ref).max()) / float(np.abs(ref).max())
    print(f"pfbsyn2 structural vs closed form M {M} m {m}: {err:.2e}")
    assert ref.shape == got.shape == (37 * (M // 2),) and err <= 1e-11


def test_the_restatements_do_not_depend_on_the_chunking():
    """sample s of a longer stream is sample s of a shorter one, and the calls a stream is cut into do not show, bit for bit"""
    M, m = 8, 3
    g = S.design(M, m, 80.0)[:2 * M * m]
    Y = _noise_rows(M, 40, 5)
    P = M // 2
    a, b = S.truth(g, Y, M)[:23 * P], S.truth(g, Y[:, :23], M)            # a matrix product: the library may order its sums by shape
    assert np.abs(a - b).max() <= 1e-13 * np.abs(a).max()
    for prec in (64, 32):
        one = S.structural(g, Y, M, m, prec)
        assert np.array_equal(one[:23 * P], S.structural(g, Y[:, :23], M, m, prec))
        for cuts in ([40], [1] * 40, [3, 0, 11, 1, 25], [12, 28]):             # shorter and longer than the reach of 4 m = 12 frames
            assert np.array_equal(one, S.structural(g, Y, M, m, prec, cuts=cuts)), (prec, cuts)


# ---------------------------------------------------------------------------- the design
@pytest.mark.parametrize("M,m", [(4, 1), (8, 3), (64, 7), (256, 8)])
def test_design_equals_the_numpy_design(M, m):
    L = 2 * M * m
    for fc in (0.0, 0.6 / M):
        g = cs.firdes_pfbsyn2(M, m, 80.0, fc)
        want = S.design(M, m, 80.0, float(f32(fc)) if fc else float(f32(0.5) / f32(M)))   # the C ABI takes fc as a float
        assert g.dtype == np.float32 and g.shape == (L,)
        ulp = float(np.spacing(f32(np.abs(want).max())))
        err = float(np.abs(g.astype(np.float64) - want[:L].astype(f32).astype(np.float64)).max())
        print(f"pfbsyn2 design M {M} m {m} fc {fc:g}: {err / ulp:.2f} ulp of the largest tap")
        assert err <= 2 * ulp
        total = float(g.astype(np.float64).sum()) + float(g[0])            # the dropped tap mirrors the first: all 2 M m + 1 sum to M
        assert abs(total - M) <= 1e-6 * M, total
    # fc = 0 is the synthesizer's rule, half the analyzer's cutoff, and the same design function
    assert np.array_equal(cs.firdes_pfbsyn2(M, m, 80.0, 0.0).view(np.uint32), cs.firdes_pfbsyn2(M, m, 80.0, 0.5 / M).view(np.uint32))
    assert np.array_equal(cs.firdes_pfbsyn2(M, m, 80.0, 0.0).view(np.uint32), cs.firdes_pfbch2(M, m, 80.0, 0.5 / M).view(np.uint32))
    assert not np.array_equal(cs.firdes_pfbsyn2(M, m, 80.0, 0.0), cs.firdes_pfbch2(M, m, 80.0, 0.0))


# ---------------------------------------------------------------------------- the round trip that pins both cutoff rules
def _rt_frames(m):
    return 16 * m + 64


@pytest.mark.parametrize("M,m,as_db,rel_max,gain_tol", [(16, 7, 80.0, 1e-4, 1e-4), (64, 7, 80.0, 1e-4, 1e-4), (256, 7, 80.0, 1e-4, 1e-4),
                                                        (32, 7, 100.0, 3e-5, None)])
def test_analysis_then_synthesis_returns_the_input(M, m, as_db, rel_max, gain_tol):
    """analyzer cut at 1 / M, synthesizer cut at 0.5 / M, f64: the input comes back D = 2 M m - M / 2 + 1 samples late with
    unit gain.  Measured: (16, 7, 80) 4.26e-5, gain 1.000023; (64, 7, 80) 4.29e-5, 1.000023; (256, 7, 80) 4.35e-5, 1.000024;
    (32, 7, 100) 1.11e-5, 1.000010"""
    rel, gain, D = S.roundtrip(M, m, as_db, A.stream(M, _rt_frames(m), 3))
    print(f"pfbsyn2 round trip M {M} m {m} As {as_db:g}: D {D} rel-RMS {rel:.3e} gain {gain:.6f}")
    assert D == 2 * M * m - M // 2 + 1 == S.delay(M, m)
    assert rel <= rel_max
    if gain_tol is not None:
        assert abs(gain - 1.0) <= gain_tol


@pytest.mark.parametrize("scale", [0.5, 0.75, 1.0])
def test_equal_cutoffs_on_both_sides_do_not_return_the_input(scale):
    """the property tells the recalled rules (1 / M and 0.5 / M) apart from their neighbours: either rule put in the other's
    place, or both moved to the middle.  Measured: 0.159 at 0.5 / M on both sides, 0.623 at 0.75 / M, 0.946 at 1 / M"""
    M, m = 16, 7
    rel, gain, _ = S.roundtrip(M, m, 80.0, A.stream(M, _rt_frames(m), 3), fc_a=scale / M, fc_s=scale / M)
    print(f"pfbsyn2 round trip with {scale:g} / M on both sides: rel-RMS {rel:.3f} gain {gain:.3f}")
    assert rel > 0.1


def test_the_property_pins_the_pair_of_cutoffs_not_which_side_has_which():
    """what the round trip does not tell: with the two rules exchanged (analyzer 0.5 / M, synthesizer 1 / M) the input comes back
    just as well (measured 4.30e-5, gain 1.000024).  That the analyzer has the wider filter stays as recalled"""
    M, m = 16, 7
    rel, gain, _ = S.roundtrip(M, m, 80.0, A.stream(M, _rt_frames(m), 3), fc_a=0.5 / M, fc_s=1.0 / M)
    print(f"pfbsyn2 round trip with the rules exchanged: rel-RMS {rel:.3e} gain {gain:.6f}")
    assert rel <= 1e-4 and abs(gain - 1.0) <= 1e-4


def test_the_wrong_delay_does_not_return_the_input():
    """D is pinned too: one sample off and the round trip is as wrong as white noise against itself shifted"""
    M, m = 16, 7
    L, D = 2 * M * m, S.delay(M, m)
    x = A.stream(M, _rt_frames(m), 3).astype(np.complex128)
    xh = S.truth(S.design(M, m, 80.0)[:L], A.truth(A.design(M, m, 80.0)[:L], x, M), M)
    for d in (D - 1, D + 1):
        a, b = x[L:x.size - d], xh[L + d:]
        assert np.sqrt(np.mean(np.abs(b - a) ** 2) / np.mean(np.abs(a) ** 2)) > 0.5


# ---------------------------------------------------------------------------- the launch shape
def test_every_shape_fits_the_lds_and_covers_the_call():
    for M in (4, 8, 16, 32, 64, 128, 256):
        for m in range(1, 9):
            one = _shape(M, m, 1, 256)
            L, F = 2 * M * m, one["F"]
            assert F >= 16 and F * M == 4096                                        # row pieces of 128 bytes or more, no idle wave
            # the carry, V and the twiddles as float2, the taps as float
            assert one["lds"] == 8 * (L - M // 2 + F * (M + (1 if F >= 32 else 2)) + M // 4) + 4 * L <= 160 * 1024
            assert 1 <= one["wgs_per_cu"] <= 2 and one["wgs_per_cu"] * one["lds"] <= 160 * 1024
            for cus in (1, 7, 256):
                for frames in (1, F - 1, F, F + 1, 3 * F + 1, cus * F, 2 * cus * one["wgs_per_cu"] * F + 1, runs_frames(M, m, cus)):
                    s = _shape(M, m, frames, cus)
                    assert s["tiles"] == -(-frames // F)
                    assert s["runs"] <= cus * s["wgs_per_cu"] and s["runs"] * s["tiles_per_run"] >= s["tiles"]
                    assert (s["runs"] - 1) * s["tiles_per_run"] < s["tiles"]       # no empty workgroup
                    assert s["tiles_per_run"] == 1 or s["tiles"] > cus * s["wgs_per_cu"]    # a short call spreads over the CUs
    assert _shape(256, 7, 0, 256)["runs"] == 0
    assert _shape(256, 7, 1, 256)["wgs_per_cu"] == 2 and _shape(256, 8, 1, 256)["wgs_per_cu"] == 2
    print("pfbsyn2 workgroups per CU:", {(M, m): _shape(M, m, 1, 256)["wgs_per_cu"] for M, m in ((256, 7), (256, 8), (32, 7), (4, 1))},
          "LDS bytes:", {(M, m): _shape(M, m, 1, 256)["lds"] for M, m in ((256, 7), (256, 8), (32, 7), (4, 1))})


@pytest.mark.parametrize("M,m", [(4, 1), (256, 7)])
def test_the_runs_case_of_the_gpu_tests_walks_runs_and_ends_ragged(M, m):
    for cus in (8, 256, 304):
        s = _shape(M, m, runs_frames(M, m, cus), cus)
        assert s["tiles_per_run"] >= 2 and s["tiles"] // s["tiles_per_run"] >= 3 and runs_frames(M, m, cus) % s["F"] == 5


def test_launch_shape_refuses_bad_arguments():
    s = (C.c_uint32 * 6)()
    for args in ((3, 1, 10, 256), (512, 1, 10, 256), (8, 0, 10, 256), (8, 9, 10, 256), (8, 3, 10, 0)):
        assert _lib.lib().csdr_pfbsyn2_launch_shape(*args, s) == _lib.ERR_INVALID
    assert _lib.lib().csdr_pfbsyn2_launch_shape(8, 3, 10, 256, None) == _lib.ERR_INVALID


# ---------------------------------------------------------------------------- life-cycle, as test_pfbch2_cpu.py has it
TAPS = np.ones(2 * 4 * 1, f32)
BAD_TAPS = np.array([1, 1, 1, NAN, 1, 1, 1, 1], f32)
GOOD = [
    ("csdr_pfbsyn2_open_kaiser", (4, 1, 60.0, 0.0, 16)),
    ("csdr_pfbsyn2_open_kaiser", (256, 8, 80.0, 0.003, 1)),
    ("csdr_pfbsyn2_open_taps", (_p(TAPS), 4, 1, 16)),
]
BAD = [
    ("csdr_pfbsyn2_open_kaiser", (2, 1, 60.0, 0.0, 16)),            # M below 4
    ("csdr_pfbsyn2_open_kaiser", (512, 1, 60.0, 0.0, 16)),          # M above 256
    ("csdr_pfbsyn2_open_kaiser", (12, 1, 60.0, 0.0, 16)),           # M not a power of two
    ("csdr_pfbsyn2_open_kaiser", (8, 0, 60.0, 0.0, 16)),            # m outside 1 .. 8
    ("csdr_pfbsyn2_open_kaiser", (8, 9, 60.0, 0.0, 16)),
    ("csdr_pfbsyn2_open_kaiser", (8, 3, 0.0, 0.0, 16)),             # as_db <= 0 or not finite
    ("csdr_pfbsyn2_open_kaiser", (8, 3, -60.0, 0.0, 16)),
    ("csdr_pfbsyn2_open_kaiser", (8, 3, INF, 0.0, 16)),
    ("csdr_pfbsyn2_open_kaiser", (8, 3, NAN, 0.0, 16)),
    ("csdr_pfbsyn2_open_kaiser", (8, 3, 60.0, -0.1, 16)),           # fc < 0, >= 0.5 or not finite
    ("csdr_pfbsyn2_open_kaiser", (8, 3, 60.0, 0.5, 16)),
    ("csdr_pfbsyn2_open_kaiser", (8, 3, 60.0, NAN, 16)),
    ("csdr_pfbsyn2_open_kaiser", (8, 3, 60.0, 0.0, 0)),             # max_frames = 0
    ("csdr_pfbsyn2_open_kaiser", (256, 3, 60.0, 0.0, (1 << 23) + 1)),   # max_frames M above 2^31
    ("csdr_pfbsyn2_open_taps", (None, 4, 1, 16)),                   # null taps
    ("csdr_pfbsyn2_open_taps", (_p(BAD_TAPS), 4, 1, 16)),           # a non-finite tap
    ("csdr_pfbsyn2_open_taps", (_p(TAPS), 4, 1, 0)),
    ("csdr_pfbsyn2_open_taps", (_p(TAPS), 6, 1, 16)),
    ("csdr_pfbsyn2_open_taps", (_p(TAPS), 4, 0, 16)),
]


@pytest.mark.parametrize("name,good", GOOD, ids=[f"{n[len('csdr_pfbsyn2_'):]}-{i}" for i, (n, _) in enumerate(GOOD)])
def test_valid_arguments_need_a_device_and_nothing_else(name, good):
    h = C.c_void_p()
    rc = getattr(_lib.lib(), name)(*good, C.byref(h))
    if _lib.lib().csdr_device_count() > 0:
        _lib.check(rc)
        assert h.value
        assert _lib.lib().csdr_pfbsyn2_destroy(h) == 0
    else:
        with pytest.raises(cs.CsdrError) as e:
            _lib.check(rc)
        assert e.value.code == _lib.ERR_NODEV and "no CPU fallback" in str(e.value)
        assert not h.value


@pytest.mark.parametrize("name,bad", BAD, ids=[f"{n[len('csdr_pfbsyn2_'):]}-{i}" for i, (n, _) in enumerate(BAD)])
def test_invalid_arguments_are_refused_before_the_device_is_looked_for(name, bad):
    h = C.c_void_p()
    with pytest.raises(cs.CsdrError) as e:
        _lib.check(getattr(_lib.lib(), name)(*bad, C.byref(h)))
    assert e.value.code == _lib.ERR_INVALID
    assert not h.value


def test_a_null_out_pointer_and_a_null_design_buffer_are_refused():
    assert _lib.lib().csdr_pfbsyn2_open_kaiser(4, 1, 60.0, 0.0, 16, None) == _lib.ERR_INVALID
    assert _lib.lib().csdr_pfbsyn2_open_taps(_p(TAPS), 4, 1, 16, None) == _lib.ERR_INVALID
    assert _lib.lib().csdr_pfbsyn2_design(4, 1, 60.0, 0.0, None) == _lib.ERR_INVALID
    g = np.empty(8, f32)
    for args in ((3, 1, 60.0, 0.0), (4, 9, 60.0, 0.0), (4, 1, 0.0, 0.0), (4, 1, 60.0, 0.5), (4, 1, INF, 0.0), (4, 1, 60.0, NAN)):
        assert _lib.lib().csdr_pfbsyn2_design(*args, _p(g)) == _lib.ERR_INVALID, args


def test_destroy_takes_null_and_rewind_and_the_calls_refuse_it():
    L = _lib.lib()
    assert L.csdr_pfbsyn2_destroy(None) == 0
    assert L.csdr_pfbsyn2_rewind(None) == _lib.ERR_INVALID
    n = C.c_uint32()
    x = np.zeros(4, np.complex64)
    y = np.zeros(4, np.complex64)
    assert L.csdr_pfbsyn2_process(None, _p(y), 1, _p(x), C.byref(n)) == _lib.ERR_INVALID
    assert L.csdr_pfbsyn2_process_device(None, _p(y), 1, _p(x), None) == _lib.ERR_INVALID
    assert L.csdr_pfbsyn2_get_taps(None, _p(x)) == _lib.ERR_INVALID
    assert L.csdr_pfbsyn2_delay(None) == 0


def test_the_pipe_needs_a_device_and_nothing_else():
    pipe = cs.firpfbch2Synthesizer(8)
    if _lib.lib().csdr_device_count() > 0:
        pipe._done(pipe._start())
    else:
        with pytest.raises(cs.CsdrError) as e:
            pipe._start()
        assert e.value.code == _lib.ERR_NODEV and "no CPU fallback" in str(e.value)
    with pytest.raises(cs.CsdrError) as e:
        cs.Firpfbch2Synth(np.ones(10, f32), 4, 1)                  # 10 taps are not 2 M m = 8
    assert e.value.code == _lib.ERR_INVALID


# ---------------------------------------------------------------------------- the names
def test_every_name_is_declared_bound_and_exported_and_none_is_a_create_or_a_reset():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "csdr.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(csdr_[a-z0-9_]+)\s*\(", src))
    lib = C.CDLL(cs.lib_path())
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("csdr_pfbsyn2_")) == sorted(NAMES)
    assert sorted(n for n in declared if n.startswith("csdr_pfbsyn2_")) == sorted(NAMES)
    for n in NAMES:
        assert hasattr(lib, n), n
        # test_pfbch2_cpu.py pins the names that begin with csdr_pfbch2_, test_block_lifecycle_cpu.py the names with `_create` in
        # them and the names that end in `_reset`; this block's life-cycle cases are in this file
        assert not n.startswith("csdr_pfbch2_") and "_create" not in n and "_reset" not in n, n
    for n in ("Firpfbch2Synth", "firpfbch2Synthesizer", "firdes_pfbsyn2"):
        assert hasattr(cs, n), n


# ---------------------------------------------------------------------------- faults the GPU bounds have to catch
def _ratios(got, truth, yard, M):
    a, b, _, _ = A.ratios(S.by_phase(got, M), S.by_phase(truth, M), S.by_phase(yard, M), M)
    return a, b


@pytest.mark.parametrize("M,m", [(4, 1), (32, 7), (256, 7)])
def test_the_bounds_of_the_gpu_tests_catch_three_faults(M, m):
    """the f32 restatement with a fault in it, under the rule test_pfbsyn2_gpu.py applies to the kernel (per output phase, per
    element): one tap of one phase off by 2^-10; the parity flipped behind a call boundary; a halo that starts one frame late at
    a run start.  Each has to leave the bound (ratio > 1) while the path without the fault stays below one half of it"""
    P = M // 2
    g = cs.firdes_pfbsyn2(M, m, 80.0, 0.0)
    Y = rows(M, m, FRAMES, 100 * M + m)
    truth, yard = S.truth(g, Y, M), S.yardstick(g, Y, M, m)
    clean = _ratios(S.structural(g, Y, M, m, 32, cuts=CUTS), truth, yard, M)
    assert max(clean) < 0.5, clean
    bad_tap = g.copy()
    bad_tap[(P - 1) + 1 * P] += f32(2.0 ** -10)                    # phase r = P - 1, tap n = 1
    faults = {"tap": S.structural(bad_tap, Y, M, m, 32, cuts=CUTS),
              "parity": S.structural(g, Y, M, m, 32, cuts=CUTS, mutate="parity"),
              "halo": S.structural(g, Y, M, m, 32, cuts=CUTS, mutate="halo")}
    for name, got in faults.items():
        a, b = _ratios(got, truth, yard, M)
        print(f"pfbsyn2 M {M} m {m} fault {name}: ratios (a) {a:.3g} (b) {b:.3g}; clean {clean[0]:.3f} {clean[1]:.3f}")
        assert max(a, b) > 1.0, (name, a, b)
