"""The 2x-oversampled channelizer (csdr_pfbch2_*, k_pfb2) on the GPU, all through the C ABI, against the f64
closed form of tests/pfbch2_restatement.py under the per-channel / per-element rule of DESIGN.md 4.6 (the f32 restatement is the
yardstick), and against itself bit for bit wherever the contract says the output does not depend on something: the chunking,
the run and tile a frame falls into, a rewind, the constructor, host versus device entry.

Input: complex white noise of unit variance plus a tone of amplitude 0.25, 0.45 / M above channel 1's centre, in the transition
band the block exists for.  Every test runs under a time limit of its own: a watchdog thread ends the process if a GPU call does
not come back."""
import ctypes as C
import faulthandler
import functools
import subprocess

import numpy as np
import pytest

import pfbch2_restatement as R
from host_exe import host_exe
from pfbch2_cases import runs_frames, shape as _shape

pytestmark = pytest.mark.gpu

cs = pytest.importorskip("composable_sdr_amd")
from composable_sdr_amd import _lib  # noqa: E402

f32 = np.float32
LIMIT_S = 120
SHAPES = [(4, 1), (8, 3), (32, 7), (64, 2), (256, 7), (256, 8)]
IDS = [f"M{M}-m{m}" for M, m in SHAPES]
CUTS = [37, 1, 0, 9, 67]                  # frames per call: shorter than the window of 4 m frames, empty, odd (the parity is carried)
FRAMES = sum(CUTS)


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _same(got, want, what=""):
    assert got.dtype == want.dtype == np.complex64 and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    assert np.array_equal(g, w), (what, int((g != w).sum()), g.size)


def _cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@functools.lru_cache(maxsize=None)
def _case(M, m, frames=FRAMES):
    """(input, taps, one call's output, the f64 truth, the f32 yardstick); computed once, never written to"""
    x = R.stream(M, frames, 100 * M + m)
    h = cs.Firpfbch2.kaiser(M, m, 80.0, 0.0, max_frames=frames)
    taps, y = h.taps(), h.process(x)
    h.close()
    out = (x, taps, y, R.truth(taps, x, M), R.yardstick(taps, x, M, m))
    for a in out:
        a.setflags(write=False)
    return out


def _in_calls(h, x, M, cuts):
    P = M // 2
    pos, rows = 0, []
    for c in cuts:
        rows.append(h.process(x[pos * P:(pos + c) * P]))
        assert rows[-1].shape == (M, c)
        pos += c
    assert pos * P == x.size
    return np.concatenate(rows, axis=1)


def _parity(tag, M, got, truth, yard):
    assert np.isfinite(got.view(f32)).all(), tag
    a, b, ya, yb = R.ratios(got, truth, yard, M)
    print(f"pfbch2 {tag}: worst per-channel ratio (a) {a:.3f} (yardstick term {ya:.2f} of the bound), "
          f"worst per-element ratio (b) {b:.3f} (yardstick term {yb:.2f} of the bound)")
    assert a <= 1.0 and b <= 1.0, (tag, a, b)


@pytest.mark.parametrize("M,m", SHAPES, ids=IDS)
def test_parity_with_the_closed_form(M, m):
    x, taps, y, truth, yard = _case(M, m)
    assert y.shape == truth.shape == yard.shape == (M, FRAMES)
    _parity(f"M {M} m {m}, {FRAMES} frames", M, y, truth, yard)


@pytest.mark.parametrize("M,m", SHAPES, ids=IDS)
def test_one_call_equals_many_bit_for_bit(M, m):
    x, taps, y, _, _ = _case(M, m)
    h = cs.Firpfbch2.kaiser(M, m, 80.0, 0.0, max_frames=max(CUTS))
    got = _in_calls(h, x, M, CUTS)
    h.close()
    _same(got, y, f"M {M} m {m} cuts {CUTS}")


@pytest.mark.parametrize("M,m", [(4, 1), (256, 7)], ids=["M4-m1", "M256-m7"])
def test_runs_of_tiles_and_a_ragged_last_tile(M, m):
    """one call in which at least three workgroups walk two tiles each and the last tile has 5 frames: against the truth, and
    bit for bit against the same stream in calls of 33 frames (which start every frame somewhere else in a tile and a run)"""
    frames = runs_frames(M, m, _cus())
    s = _shape(M, m, frames, _cus())
    assert s["tiles_per_run"] >= 2 and s["tiles"] // s["tiles_per_run"] >= 3 and frames % s["F"] == 5, s
    x, taps, y, truth, yard = _case(M, m, frames)
    _parity(f"M {M} m {m}, {frames} frames in {s['runs']} runs of {s['tiles_per_run']} tiles", M, y, truth, yard)
    h = cs.Firpfbch2.kaiser(M, m, 80.0, 0.0, max_frames=33)
    got = _in_calls(h, x, M, [33] * (frames // 33) + ([frames % 33] if frames % 33 else []))
    h.close()
    _same(got, y, f"M {M} m {m} calls of 33 frames")


@pytest.mark.parametrize("M,m", [(8, 3), (256, 7)], ids=["M8-m3", "M256-m7"])
def test_rewind_gives_the_state_after_open(M, m):
    x, taps, y, _, _ = _case(M, m)
    P = M // 2
    h = cs.Firpfbch2.kaiser(M, m, 80.0, 0.0, max_frames=FRAMES)
    h.process(x[:37 * P])                          # an odd number of frames: history and parity both differ from the open state
    h.rewind()
    got = h.process(x)
    h.rewind()
    h.rewind()
    again = _in_calls(h, x, M, CUTS)
    h.close()
    _same(got, y, "after rewind")
    _same(again, y, "after two rewinds, in calls")


@pytest.mark.parametrize("M,m", [(4, 1), (64, 2)], ids=["M4-m1", "M64-m2"])
def test_open_taps_with_the_designed_taps_equals_open_kaiser(M, m):
    x, taps, y, _, _ = _case(M, m)
    _same(taps.view(np.complex64), cs.firdes_pfbch2(M, m, 80.0, 0.0).view(np.complex64), "get_taps")
    h = cs.Firpfbch2(cs.firdes_pfbch2(M, m, 80.0, 0.0), M, m, max_frames=FRAMES)
    got = h.process(x)
    back = h.taps()
    h.close()
    _same(got, y, "open_taps")
    _same(back.view(np.complex64), taps.view(np.complex64), "the taps given")


@pytest.mark.parametrize("M,m", [(8, 3), (256, 8)], ids=["M8-m3", "M256-m8"])
def test_process_device_on_a_stream_of_the_callers_equals_process(M, m):
    import torch
    x, taps, y, _, _ = _case(M, m)
    P = M // 2
    h = cs.Firpfbch2.kaiser(M, m, 80.0, 0.0, max_frames=FRAMES)
    d_x = torch.from_numpy(np.ascontiguousarray(x).view(f32).reshape(-1, 2).copy()).cuda()
    d_y = [torch.zeros((M, c, 2), device="cuda", dtype=torch.float32) for c in (37, 77)]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        h.process_device(d_x.data_ptr(), 37 * P, d_y[0].data_ptr(), s.cuda_stream)
        h.process_device(d_x.data_ptr() + 8 * 37 * P, 77 * P, d_y[1].data_ptr(), s.cuda_stream)
    s.synchronize()
    got = np.concatenate([t.cpu().numpy().view(np.complex64)[..., 0] for t in d_y], axis=1)
    h.close()
    _same(got, y, "process_device")


def test_refused_calls_leave_the_stream_where_it_was():
    M, m = 8, 3
    x, taps, y, _, _ = _case(M, m)
    P = M // 2
    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(L.csdr_pfbch2_open_kaiser(M, m, 80.0, 0.0, 64, C.byref(h)))
    out = np.empty((M, 64), np.complex64)
    n = C.c_uint32(12345)
    rows, pos = [], 0

    def good(c):
        nonlocal pos
        _lib.check(L.csdr_pfbch2_process(h, _p(x[pos * P:]), c * P, _p(out), C.byref(n)))
        assert n.value == c
        rows.append(out.reshape(-1)[:M * c].reshape(M, c).copy())
        pos += c

    good(37)
    n.value = 12345
    assert L.csdr_pfbch2_process(h, _p(x), 9 * P + 1, _p(out), C.byref(n)) == _lib.ERR_SIZE          # not a multiple of M / 2
    assert "multiple" in L.csdr_last_error().decode()
    assert L.csdr_pfbch2_process(h, _p(x), 65 * P, _p(out), C.byref(n)) == _lib.ERR_SIZE             # more than max_frames
    assert L.csdr_pfbch2_process(h, None, 9 * P, _p(out), C.byref(n)) == _lib.ERR_INVALID
    assert L.csdr_pfbch2_process(h, _p(x), 9 * P, None, C.byref(n)) == _lib.ERR_INVALID
    assert L.csdr_pfbch2_process(h, _p(x), 9 * P, _p(out), None) == _lib.ERR_INVALID
    assert L.csdr_pfbch2_process_device(h, None, 9 * P, None, None) == _lib.ERR_INVALID
    assert L.csdr_pfbch2_process_device(h, _p(x), 9 * P + 2, _p(out), None) == _lib.ERR_SIZE
    assert L.csdr_pfbch2_get_taps(h, None) == _lib.ERR_INVALID
    assert n.value == 12345
    good(1)
    good(0)
    good(9)
    good(64)
    good(3)
    assert L.csdr_pfbch2_destroy(h) == 0
    _same(np.concatenate(rows, axis=1), y, "around refused calls")


def test_the_pipe_composes_with_the_fm_demodulator():
    M, m = 8, 7
    x = R.stream(M, FRAMES, 9)
    P = M // 2
    pipe = cs.compose(cs.fmDemodulator(0.3, nchan=M, max_samples=FRAMES), cs.firpfbch2Channelizer(M, max_frames=FRAMES))
    r = pipe._start()
    got = [pipe._process(r, x[:37 * P]), pipe._process(r, x[37 * P:])]
    pipe._done(r)
    h = cs.Firpfbch2.kaiser(M, m, 80.0, 0.0, max_frames=FRAMES)
    fm = cs.fmDemodulator(0.3, nchan=M, max_samples=FRAMES)
    rf = fm._start()
    want = [fm._process(rf, h.process(x[:37 * P])), fm._process(rf, h.process(x[37 * P:]))]
    fm._done(rf)
    h.close()
    for g, w in zip(got, want):
        assert g.dtype == w.dtype == np.float32 and g.shape == w.shape and g.shape[0] == M
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32))
    rows = cs.firpfbch2Channelizer(M)
    rr = rows._start()
    out = rows._process(rr, x)
    empty = rows._process(rr, np.empty(0, np.complex64))
    rows._done(rr)
    assert isinstance(out, list) and len(out) == M and all(o.shape == (FRAMES,) and o.dtype == np.complex64 for o in out)
    assert len(empty) == 1 and empty[0].size == 0


def test_the_host_program_writes_the_python_pipes_bytes(tmp_path):
    M, m = 8, 3
    x, taps, y, _, _ = _case(M, m)
    src, dst = tmp_path / "in.cf32", tmp_path / "out"
    x.tofile(src)
    cuts = [c for c in CUTS if c]
    subprocess.run([host_exe("pfbch2_host"), f"{M}:{m}:80:0", ",".join(str(c) for c in cuts), str(src), str(dst)], check=True, timeout=LIMIT_S)
    for k in range(M):
        got = np.fromfile(f"{dst}_ch{k}.cf32", dtype=np.complex64)
        _same(got, np.ascontiguousarray(y[k]), f"row {k}")
