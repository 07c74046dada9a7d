"""The 2x-oversampled channelizer (csdr_pfbch2_*) as far as it shows without a GPU: the restatements of
tests/pfbch2_restatement.py agree with each other, the design function equals the numpy design, the documented crossing of
neighbouring channels at the channel centres, the launch shape, the life-cycle of the handle and the names of the C ABI."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pfbch2_restatement as R
from pfbch2_cases import runs_frames, shape as _shape
import composable_sdr_amd as cs
from composable_sdr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
INF, NAN = float("inf"), float("nan")
NAMES = ["csdr_pfbch2_design", "csdr_pfbch2_launch_shape", "csdr_pfbch2_open_kaiser", "csdr_pfbch2_open_taps", "csdr_pfbch2_process",
         "csdr_pfbch2_process_device", "csdr_pfbch2_rewind", "csdr_pfbch2_get_taps", "csdr_pfbch2_destroy"]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _noise(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)


# ---------------------------------------------------------------------------- the restatements
@pytest.mark.parametrize("M,m", [(4, 1), (8, 3), (16, 7), (256, 2)])
def test_the_structural_form_equals_the_closed_form(M, m):
    h = R.design(M, m, 80.0)[:2 * M * m]
    x = _noise(37 * (M // 2), M + m)
    ref, got = R.truth(h, x, M), R.structural(h, x, M, m)
    err = float(np.abs(got - ref).max()) / float(np.abs(ref).max())
    print(f"pfbch2 structural vs closed form M {M} m {m}: {err:.2e}")
    assert ref.shape == got.shape == (M, 37) and err <= 1e-11


def test_the_restatements_do_not_depend_on_the_chunking_of_their_own_definition():
    """frame t of a longer stream is frame t of a shorter one (x[s < 0] = 0 and nothing else carried)"""
    M, m = 8, 3
    h = R.design(M, m, 80.0)[:2 * M * m]
    x = _noise(40 * (M // 2), 5)
    a, b = R.truth(h, x, M)[:, :23], R.truth(h, x[:23 * (M // 2)], M)      # a matrix product: the library may order its sums by shape
    assert np.abs(a - b).max() <= 1e-13 * np.abs(a).max()
    assert np.array_equal(R.yardstick(h, x, M, m)[:, :23], R.yardstick(h, x[:23 * (M // 2)], M, m))


# ---------------------------------------------------------------------------- the design
@pytest.mark.parametrize("M,m", [(4, 1), (8, 3), (64, 7), (256, 8)])
def test_design_equals_the_numpy_design(M, m):
    L = 2 * M * m
    for fc in (0.0, 0.6 / M):
        h = cs.firdes_pfbch2(M, m, 80.0, fc)
        want = R.design(M, m, 80.0, float(f32(fc)))                # the C ABI takes fc as a float
        assert h.dtype == np.float32 and h.shape == (L,)
        ulp = float(np.spacing(f32(np.abs(want).max())))
        err = float(np.abs(h.astype(np.float64) - want[:L].astype(f32).astype(np.float64)).max())
        print(f"pfbch2 design M {M} m {m} fc {fc:g}: {err / ulp:.2f} ulp of the largest tap")
        assert err <= 2 * ulp
        # the dropped tap is the mirror image of the first (the design is symmetric): all 2 M m + 1 sum to M
        assert abs(want[L] - want[0]) <= 1e-12 * M
        total = float(h.astype(np.float64).sum()) + float(h[0])
        assert abs(total - M) <= 1e-6 * M, total
    assert np.array_equal(cs.firdes_pfbch2(M, m, 80.0, 0.0).view(np.uint32), cs.firdes_pfbch2(M, m, 80.0, 1.0 / M).view(np.uint32))


@pytest.mark.parametrize("M,m", [(4, 2), (16, 7)])
def test_neighbours_cross_at_the_channel_centres(M, m):
    """A tone at channel k0's centre comes out of row k0 with the prototype's DC gain / M and out of both neighbours at one
    half (the -6 dB point of a Kaiser design is its cutoff, fc = 1 / M at fc = 0), once the window of 4 m frames is full"""
    h = cs.firdes_pfbch2(M, m, 80.0, 0.0).astype(np.float64)
    k0, frames = 1, 4 * m + 8
    x = np.exp(2j * np.pi * k0 * np.arange(frames * (M // 2)) / M)
    y = np.abs(R.truth(h, x, M)[:, 4 * m:])
    assert np.abs(y[k0] - h.sum() / M).max() <= 1e-12
    for k in ((k0 - 1) % M, (k0 + 1) % M):
        print(f"pfbch2 M {M} m {m}: neighbour {k} of a tone at the centre of {k0}: {y[k].mean():.5e}")
        assert np.abs(y[k] - 0.5).max() <= 0.01


# ---------------------------------------------------------------------------- the launch shape
def test_every_shape_fits_the_lds_and_covers_the_call():
    for M in (4, 8, 16, 32, 64, 128, 256):
        for m in range(1, 9):
            one = _shape(M, m, 1, 256)
            L, F = 2 * M * m, one["F"]
            assert F >= 16 and F * M == 4096                                        # row pieces of 128 bytes or more, no idle wave
            assert one["lds"] == 8 * (L - M // 2 + F * (M // 2) + F * (M + (1 if F >= 32 else 2)) + M // 4) <= 160 * 1024
            assert 1 <= one["wgs_per_cu"] <= 2 and one["wgs_per_cu"] * one["lds"] <= 160 * 1024
            for cus in (1, 7, 256):
                for frames in (1, F - 1, F, F + 1, 3 * F + 1, cus * F, 2 * cus * one["wgs_per_cu"] * F + 1, runs_frames(M, m, cus)):
                    s = _shape(M, m, frames, cus)
                    assert s["tiles"] == -(-frames // F)
                    assert s["runs"] <= cus * s["wgs_per_cu"] and s["runs"] * s["tiles_per_run"] >= s["tiles"]
                    assert (s["runs"] - 1) * s["tiles_per_run"] < s["tiles"]       # no empty workgroup
                    assert s["tiles_per_run"] == 1 or s["tiles"] > cus * s["wgs_per_cu"]    # a short call spreads over the CUs
    assert _shape(256, 7, 0, 256)["runs"] == 0
    print("pfbch2 workgroups per CU:", {(M, m): _shape(M, m, 1, 256)["wgs_per_cu"] for M, m in ((256, 7), (256, 8), (32, 7), (4, 1))},
          "LDS bytes:", {(M, m): _shape(M, m, 1, 256)["lds"] for M, m in ((256, 7), (256, 8), (32, 7), (4, 1))})


@pytest.mark.parametrize("M,m", [(4, 1), (256, 7)])
def test_the_runs_case_of_the_gpu_tests_walks_runs_and_ends_ragged(M, m):
    for cus in (8, 256, 304):
        s = _shape(M, m, runs_frames(M, m, cus), cus)
        assert s["tiles_per_run"] >= 2 and s["tiles"] // s["tiles_per_run"] >= 3 and runs_frames(M, m, cus) % s["F"] == 5


def test_launch_shape_refuses_bad_arguments():
    s = (C.c_uint32 * 6)()
    for args in ((3, 1, 10, 256), (512, 1, 10, 256), (8, 0, 10, 256), (8, 9, 10, 256), (8, 3, 10, 0)):
        assert _lib.lib().csdr_pfbch2_launch_shape(*args, s) == _lib.ERR_INVALID
    assert _lib.lib().csdr_pfbch2_launch_shape(8, 3, 10, 256, None) == _lib.ERR_INVALID


# ---------------------------------------------------------------------------- life-cycle, as test_block_lifecycle_cpu.py has it
TAPS = np.ones(2 * 4 * 1, f32)
BAD_TAPS = np.array([1, 1, 1, NAN, 1, 1, 1, 1], f32)
GOOD = [
    ("csdr_pfbch2_open_kaiser", (4, 1, 60.0, 0.0, 16)),
    ("csdr_pfbch2_open_kaiser", (256, 8, 80.0, 0.003, 1)),
    ("csdr_pfbch2_open_taps", (_p(TAPS), 4, 1, 16)),
]
BAD = [
    ("csdr_pfbch2_open_kaiser", (2, 1, 60.0, 0.0, 16)),            # M below 4
    ("csdr_pfbch2_open_kaiser", (512, 1, 60.0, 0.0, 16)),          # M above 256
    ("csdr_pfbch2_open_kaiser", (12, 1, 60.0, 0.0, 16)),           # M not a power of two
    ("csdr_pfbch2_open_kaiser", (8, 0, 60.0, 0.0, 16)),            # m outside 1 .. 8
    ("csdr_pfbch2_open_kaiser", (8, 9, 60.0, 0.0, 16)),
    ("csdr_pfbch2_open_kaiser", (8, 3, 0.0, 0.0, 16)),             # as_db <= 0 or not finite
    ("csdr_pfbch2_open_kaiser", (8, 3, -60.0, 0.0, 16)),
    ("csdr_pfbch2_open_kaiser", (8, 3, INF, 0.0, 16)),
    ("csdr_pfbch2_open_kaiser", (8, 3, NAN, 0.0, 16)),
    ("csdr_pfbch2_open_kaiser", (8, 3, 60.0, -0.1, 16)),           # fc < 0, >= 0.5 or not finite
    ("csdr_pfbch2_open_kaiser", (8, 3, 60.0, 0.5, 16)),
    ("csdr_pfbch2_open_kaiser", (8, 3, 60.0, NAN, 16)),
    ("csdr_pfbch2_open_kaiser", (8, 3, 60.0, 0.0, 0)),             # max_frames = 0
    ("csdr_pfbch2_open_taps", (None, 4, 1, 16)),                   # null taps
    ("csdr_pfbch2_open_taps", (_p(BAD_TAPS), 4, 1, 16)),           # a non-finite tap
    ("csdr_pfbch2_open_taps", (_p(TAPS), 4, 1, 0)),
    ("csdr_pfbch2_open_taps", (_p(TAPS), 6, 1, 16)),
    ("csdr_pfbch2_open_taps", (_p(TAPS), 4, 0, 16)),
]


@pytest.mark.parametrize("name,good", GOOD, ids=[f"{n[len('csdr_pfbch2_'):]}-{i}" for i, (n, _) in enumerate(GOOD)])
def test_valid_arguments_need_a_device_and_nothing_else(name, good):
    h = C.c_void_p()
    rc = getattr(_lib.lib(), name)(*good, C.byref(h))
    if _lib.lib().csdr_device_count() > 0:
        _lib.check(rc)
        assert h.value
        assert _lib.lib().csdr_pfbch2_destroy(h) == 0
    else:
        with pytest.raises(cs.CsdrError) as e:
            _lib.check(rc)
        assert e.value.code == _lib.ERR_NODEV and "no CPU fallback" in str(e.value)
        assert not h.value


@pytest.mark.parametrize("name,bad", BAD, ids=[f"{n[len('csdr_pfbch2_'):]}-{i}" for i, (n, _) in enumerate(BAD)])
def test_invalid_arguments_are_refused_before_the_device_is_looked_for(name, bad):
    h = C.c_void_p()
    with pytest.raises(cs.CsdrError) as e:
        _lib.check(getattr(_lib.lib(), name)(*bad, C.byref(h)))
    assert e.value.code == _lib.ERR_INVALID
    assert not h.value


def test_a_null_out_pointer_and_a_null_design_buffer_are_refused():
    assert _lib.lib().csdr_pfbch2_open_kaiser(4, 1, 60.0, 0.0, 16, None) == _lib.ERR_INVALID
    assert _lib.lib().csdr_pfbch2_open_taps(_p(TAPS), 4, 1, 16, None) == _lib.ERR_INVALID
    assert _lib.lib().csdr_pfbch2_design(4, 1, 60.0, 0.0, None) == _lib.ERR_INVALID
    h = np.empty(8, f32)
    for args in ((3, 1, 60.0, 0.0), (4, 9, 60.0, 0.0), (4, 1, 0.0, 0.0), (4, 1, 60.0, 0.5), (4, 1, INF, 0.0), (4, 1, 60.0, NAN)):
        assert _lib.lib().csdr_pfbch2_design(*args, _p(h)) == _lib.ERR_INVALID, args


def test_destroy_takes_null_and_rewind_and_the_calls_refuse_it():
    L = _lib.lib()
    assert L.csdr_pfbch2_destroy(None) == 0
    assert L.csdr_pfbch2_rewind(None) == _lib.ERR_INVALID
    n = C.c_uint32()
    x = np.zeros(4, np.complex64)
    assert L.csdr_pfbch2_process(None, _p(x), 2, _p(x), C.byref(n)) == _lib.ERR_INVALID
    assert L.csdr_pfbch2_process_device(None, _p(x), 2, _p(x), None) == _lib.ERR_INVALID
    assert L.csdr_pfbch2_get_taps(None, _p(x)) == _lib.ERR_INVALID


def test_the_pipe_needs_a_device_and_nothing_else():
    pipe = cs.firpfbch2Channelizer(8)
    if _lib.lib().csdr_device_count() > 0:
        pipe._done(pipe._start())
    else:
        with pytest.raises(cs.CsdrError) as e:
            pipe._start()
        assert e.value.code == _lib.ERR_NODEV and "no CPU fallback" in str(e.value)
    with pytest.raises(cs.CsdrError) as e:
        cs.Firpfbch2(np.ones(10, f32), 4, 1)                       # 10 taps are not 2 M m = 8
    assert e.value.code == _lib.ERR_INVALID


# ---------------------------------------------------------------------------- the names
def test_every_name_is_declared_bound_and_exported_and_none_is_a_create_or_a_reset():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "csdr.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(csdr_[a-z0-9_]+)\s*\(", src))
    lib = C.CDLL(cs.lib_path())
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("csdr_pfbch2_")) == sorted(NAMES)
    for n in NAMES:
        assert n in declared and hasattr(lib, n), n
        # test_block_lifecycle_cpu.py pins the set of names with `_create` in them and of names that end in `_reset` to the
        # fifteen blocks it has cases for; this block's constructors are `open` and its reset is `rewind`, and this file holds
        # its life-cycle cases
        assert "_create" not in n and not n.endswith("_reset"), n
    for n in ("Firpfbch2", "firpfbch2Channelizer", "firdes_pfbch2"):
        assert hasattr(cs, n), n
