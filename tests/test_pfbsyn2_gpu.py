"""The synthesizer of the 2x-oversampled bank (csdr_pfbsyn2_*, k_pfb2s) on the GPU, all through the C ABI: against
the f64 closed form of tests/pfbsyn2_restatement.py under the per-row / per-element rule of DESIGN.md 4.6 (the f32 restatement is
the yardstick; a "row" is one output phase r, so that a single wrong branch is not diluted), against itself bit for bit wherever
the contract says the output does not depend on something (the chunking, the run and tile a frame falls into, a rewind, the
constructor, host versus device entry), and behind the analyzer, where the round trip has to return the input.

Input: the analyzer's f64 closed form of pfbch2_restatement.stream, rounded to CF32: realistic rows, computed on the CPU; the GPU
analyzer is in the loop only in the round-trip and host-program tests.  Every test runs under a time limit of its own: a watchdog
thread ends the process if a GPU call does not come back."""
import ctypes as C
import faulthandler
import functools
import subprocess

import numpy as np
import pytest

import pfbch2_restatement as A
import pfbsyn2_restatement as S
from host_exe import host_exe
from pfbsyn2_cases import CUTS, FRAMES, SHAPES, rows as _rows, runs_frames, shape as _shape

pytestmark = pytest.mark.gpu

cs = pytest.importorskip("composable_sdr_amd")
from composable_sdr_amd import _lib  # noqa: E402
from composable_sdr_amd import Firpfbch2Synth, firpfbch2Synthesizer, firdes_pfbsyn2  # noqa: E402,F401  (nothing here runs without them)

f32 = np.float32
LIMIT_S = 120
IDS = [f"M{M}-m{m}" for M, m in SHAPES]


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
    """(rows, taps, one call's output, the f64 truth, the f32 yardstick); computed once, never written to"""
    Y = _rows(M, m, frames, 100 * M + m)
    h = cs.Firpfbch2Synth.kaiser(M, m, 80.0, 0.0, max_frames=frames)
    taps, x = h.taps(), h.process(Y)
    h.close()
    out = (Y, taps, x, S.truth(taps, Y, M), S.yardstick(taps, Y, M, m))
    for a in out:
        a.setflags(write=False)
    return out


def _in_calls(h, Y, M, cuts):
    pos, parts = 0, []
    for c in cuts:
        parts.append(h.process(Y[:, pos:pos + c]))
        assert parts[-1].shape == (c * (M // 2),)
        pos += c
    assert pos == Y.shape[1]
    return np.concatenate(parts)


def _parity(tag, M, got, truth, yard):
    assert np.isfinite(got.view(f32)).all(), tag
    a, b, ya, yb = A.ratios(S.by_phase(got, M), S.by_phase(truth, M), S.by_phase(yard, M), M)
    print(f"pfbsyn2 {tag}: worst per-phase ratio (a) {a:.3f} (yardstick term {ya:.2f} of the bound), "
          f"worst per-element ratio (b) {b:.3f} (yardstick term {yb:.2f} of the bound)")
    assert a <= 1.0 and b <= 1.0, (tag, a, b)


@pytest.mark.parametrize("M,m", SHAPES, ids=IDS)
def test_parity_with_the_closed_form(M, m):
    Y, taps, x, truth, yard = _case(M, m)
    assert x.shape == truth.shape == yard.shape == (FRAMES * (M // 2),)
    _parity(f"M {M} m {m}, {FRAMES} frames", M, x, truth, yard)


@pytest.mark.parametrize("M,m", SHAPES, ids=IDS)
def test_one_call_equals_many_bit_for_bit(M, m):
    Y, taps, x, _, _ = _case(M, m)
    h = cs.Firpfbch2Synth.kaiser(M, m, 80.0, 0.0, max_frames=max(CUTS))
    got = _in_calls(h, Y, M, CUTS)
    h.close()
    _same(got, x, f"M {M} m {m} cuts {CUTS}")


@pytest.mark.parametrize("M,m", [(4, 1), (256, 7)], ids=["M4-m1", "M256-m7"])
def test_runs_of_tiles_and_a_ragged_last_tile(M, m):
    """one call in which at least three workgroups walk two tiles each and the last tile has 5 frames: against the truth, and
    bit for bit against the same stream in calls of 33 frames (which start every frame somewhere else in a tile and a run)"""
    frames = runs_frames(M, m, _cus())
    s = _shape(M, m, frames, _cus())
    assert s["tiles_per_run"] >= 2 and s["tiles"] // s["tiles_per_run"] >= 3 and frames % s["F"] == 5, s
    Y, taps, x, truth, yard = _case(M, m, frames)
    _parity(f"M {M} m {m}, {frames} frames in {s['runs']} runs of {s['tiles_per_run']} tiles", M, x, truth, yard)
    h = cs.Firpfbch2Synth.kaiser(M, m, 80.0, 0.0, max_frames=33)
    got = _in_calls(h, Y, M, [33] * (frames // 33) + ([frames % 33] if frames % 33 else []))
    h.close()
    _same(got, x, f"M {M} m {m} calls of 33 frames")


@pytest.mark.parametrize("M,m", [(8, 3), (256, 7)], ids=["M8-m3", "M256-m7"])
def test_rewind_gives_the_state_after_open(M, m):
    Y, taps, x, _, _ = _case(M, m)
    h = cs.Firpfbch2Synth.kaiser(M, m, 80.0, 0.0, max_frames=FRAMES)
    h.process(Y[:, :37])                           # an odd number of frames: history and parity both differ from the open state
    h.rewind()
    got = h.process(Y)
    h.rewind()
    h.rewind()
    again = _in_calls(h, Y, M, CUTS)
    h.close()
    _same(got, x, "after rewind")
    _same(again, x, "after two rewinds, in calls")


@pytest.mark.parametrize("M,m", [(4, 1), (64, 2)], ids=["M4-m1", "M64-m2"])
def test_open_taps_with_the_designed_taps_equals_open_kaiser(M, m):
    Y, taps, x, _, _ = _case(M, m)
    _same(taps.view(np.complex64), cs.firdes_pfbsyn2(M, m, 80.0, 0.0).view(np.complex64), "get_taps")
    h = cs.Firpfbch2Synth(cs.firdes_pfbsyn2(M, m, 80.0, 0.0), M, m, max_frames=FRAMES)
    got = h.process(Y)
    back = h.taps()
    h.close()
    _same(got, x, "open_taps")
    _same(back.view(np.complex64), taps.view(np.complex64), "the taps given")


@pytest.mark.parametrize("M,m", [(8, 3), (256, 8)], ids=["M8-m3", "M256-m8"])
def test_process_device_on_a_stream_of_the_callers_equals_process(M, m):
    import torch
    Y, taps, x, _, _ = _case(M, m)
    P = M // 2
    h = cs.Firpfbch2Synth.kaiser(M, m, 80.0, 0.0, max_frames=FRAMES)
    cuts = (37, 77)
    d_y = [torch.from_numpy(np.ascontiguousarray(Y[:, a:a + c]).view(f32).reshape(M, c, 2).copy()).cuda() for a, c in zip((0, 37), cuts)]
    d_x = [torch.zeros((c * P, 2), device="cuda", dtype=torch.float32) for c in cuts]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for dy, dx, c in zip(d_y, d_x, cuts):
            h.process_device(dy.data_ptr(), c, dx.data_ptr(), s.cuda_stream)
    s.synchronize()
    got = np.concatenate([t.cpu().numpy().view(np.complex64)[..., 0] for t in d_x])
    assert h.delay() == 2 * M * m - M // 2 + 1
    h.close()
    _same(got, x, "process_device")


def test_refused_calls_leave_the_stream_where_it_was():
    M, m = 8, 3
    Y, taps, x, _, _ = _case(M, m)
    P = M // 2
    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(L.csdr_pfbsyn2_open_kaiser(M, m, 80.0, 0.0, 64, C.byref(h)))
    out = np.empty(64 * P, np.complex64)
    n = C.c_uint32(12345)
    parts, pos = [], 0

    def good(c):
        nonlocal pos
        y = np.ascontiguousarray(Y[:, pos:pos + c])
        _lib.check(L.csdr_pfbsyn2_process(h, _p(y), c, _p(out), C.byref(n)))
        assert n.value == c * P
        parts.append(out[:c * P].copy())
        pos += c

    good(37)
    n.value = 12345
    y9 = np.ascontiguousarray(Y[:, :9])
    big = np.zeros((M, 65), np.complex64)
    assert L.csdr_pfbsyn2_process(h, _p(big), 65, _p(out), C.byref(n)) == _lib.ERR_SIZE              # more than max_frames
    assert "max" in L.csdr_last_error().decode()
    assert L.csdr_pfbsyn2_process(h, None, 9, _p(out), C.byref(n)) == _lib.ERR_INVALID
    assert L.csdr_pfbsyn2_process(h, _p(y9), 9, None, C.byref(n)) == _lib.ERR_INVALID
    assert L.csdr_pfbsyn2_process(h, _p(y9), 9, _p(out), None) == _lib.ERR_INVALID
    assert L.csdr_pfbsyn2_process(h, _p(out), 9, _p(out), C.byref(n)) == _lib.ERR_INVALID            # the same buffer
    assert L.csdr_pfbsyn2_process_device(h, None, 9, None, None) == _lib.ERR_INVALID
    assert L.csdr_pfbsyn2_process_device(h, _p(out), 9, _p(out), None) == _lib.ERR_INVALID
    assert L.csdr_pfbsyn2_process_device(h, _p(y9), 65, _p(out), None) == _lib.ERR_SIZE
    assert L.csdr_pfbsyn2_get_taps(h, None) == _lib.ERR_INVALID
    assert n.value == 12345
    assert L.csdr_pfbsyn2_delay(h) == 2 * M * m - P + 1
    good(1)
    good(0)
    good(9)
    good(64)
    good(3)
    assert L.csdr_pfbsyn2_destroy(h) == 0
    _same(np.concatenate(parts), x, "around refused calls")


# ---------------------------------------------------------------------------- behind the analyzer
@functools.lru_cache(maxsize=None)
def _round_trip_f64(M, m, frames):
    x = A.stream(M, frames, 3)
    x.setflags(write=False)
    return x, S.roundtrip(M, m, 80.0, x)


@pytest.mark.parametrize("M,m", [(16, 7), (64, 7), (256, 7)], ids=["M16-m7", "M64-m7", "M256-m7"])
def test_the_composed_pipes_return_the_input(M, m):
    """firpfbch2Synthesizer . firpfbch2Channelizer over three unequal chunks: xh[s + D] against x[s] behind the first L samples,
    rel-RMS <= 1.5 x the f64 figure of the same stream (measured: 4.3e-5 at 80 dB) + 20 d U (f32 head-room for two transforms)"""
    frames = 16 * m + 64
    P, L, d = M // 2, 2 * M * m, float(np.log2(M))
    x, (rel64, gain64, D) = _round_trip_f64(M, m, frames)
    pipe = cs.compose(cs.firpfbch2Synthesizer(M, m, 80.0, max_frames=frames), cs.firpfbch2Channelizer(M, m, 80.0, max_frames=frames))
    r = pipe._start()
    cuts = [41, 1, frames - 42]
    parts, pos = [], 0
    for c in cuts:
        parts.append(pipe._process(r, x[pos * P:(pos + c) * P]))
        pos += c
    assert pipe._process(r, np.empty(0, np.complex64)).size == 0
    pipe._done(r)
    xh = np.concatenate(parts)
    assert xh.dtype == np.complex64 and xh.shape == x.shape
    syn = cs.Firpfbch2Synth.kaiser(M, m, 80.0)
    assert syn.delay() == D == 2 * M * m - P + 1
    syn.close()
    a, b = x[L:x.size - D].astype(np.complex128), xh[L + D:].astype(np.complex128)
    rel = float(np.sqrt(np.mean(np.abs(b - a) ** 2) / np.mean(np.abs(a) ** 2)))
    gain = float(np.abs(np.vdot(a, b)) / np.vdot(a, a).real)
    bound = 1.5 * rel64 + 20.0 * d * A.U
    print(f"pfbsyn2 round trip on the GPU M {M} m {m}: rel-RMS {rel:.3e} (f64 {rel64:.3e}, bound {bound:.3e}) gain {gain:.6f} (f64 {gain64:.6f})")
    assert rel <= bound


def test_the_host_program_writes_the_python_pipes_bytes(tmp_path):
    M, m = 8, 3
    P = M // 2
    x = A.stream(M, FRAMES, 11)
    src, dst = tmp_path / "in.cf32", tmp_path / "out.cf32"
    x.tofile(src)
    cuts = [c for c in CUTS if c]
    subprocess.run([host_exe("pfbsyn2_host"), f"{M}:{m}:80", ",".join(str(c) for c in cuts), str(src), str(dst)], check=True, timeout=LIMIT_S)
    pipe = cs.compose(cs.firpfbch2Synthesizer(M, m, 80.0, max_frames=max(cuts)), cs.firpfbch2Channelizer(M, m, 80.0, max_frames=max(cuts)))
    r = pipe._start()
    parts, pos = [], 0
    for c in cuts:
        parts.append(pipe._process(r, x[pos * P:(pos + c) * P]))
        pos += c
    pipe._done(r)
    _same(np.fromfile(dst, dtype=np.complex64), np.concatenate(parts), "pfbsyn2_host")


# ---------------------------------------------------------------------------- life-cycle, as test_block_lifecycle_gpu.py has it
def _assert_same_bits(got, want, what):
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert g.dtype == w.dtype and g.shape == w.shape and g.size > 0, (what, g.dtype, w.dtype, g.shape, w.shape)
    assert g.tobytes() == w.tobytes(), what


@pytest.mark.parametrize("kind", ["class", "pipe"])
def test_two_handles_are_independent_and_close_is_idempotent(kind):
    M, m = 8, 3
    Y = _case(M, m)[0]
    y1, y2 = Y[:, :77], Y[:, 77:]
    if kind == "class":
        make, run, done = (lambda: cs.Firpfbch2Synth.kaiser(M, m, 80.0, max_frames=FRAMES)), (lambda r, y: r.process(y)), (lambda r: r.close())
    else:
        pipe = cs.firpfbch2Synthesizer(M, m, 80.0, max_frames=FRAMES)
        make, run, done = pipe._start, pipe._process, pipe._done
    a, b = make(), make()
    _assert_same_bits(run(a, y1), run(b, y1), "two fresh handles, the same input")
    done(b)
    got = run(a, y2)                                          # the survivor goes on from its own state, in its own buffers
    c = make()
    run(c, y1)
    _assert_same_bits(got, run(c, y2), "the survivor of a destroy against a third fresh handle")
    for r in (a, b, c):
        done(r)
        done(r)                                               # a second close (a second _done) is fine
    for r in (a, b, c):
        for use in (lambda: r.h, lambda: r.process(y1)):
            with pytest.raises(cs.CsdrError) as e:
                use()
            assert e.value.code == _lib.ERR_INVALID and "already destroyed" in str(e.value)


def test_create_close_cycles_without_a_call():
    pipe = cs.firpfbch2Synthesizer(8)
    for _ in range(3):
        cs.Firpfbch2Synth.kaiser(256, 8, 80.0, max_frames=16).close()
        pipe._done(pipe._start())
