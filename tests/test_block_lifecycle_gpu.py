"""The life-cycle the eighteen block handles of include/csdr.h share, on the GPU: two handles of one configuration are
independent (the same input gives the same bits; destroying one leaves the other's state and buffers alone), close is
idempotent, a closed object refuses work, and create / close cycles without a call in between are clean.  For the ten blocks
that carry their state in a ping-pong pair: a refused call leaves the state alone, and a reset (or rewind) gives the state
of a fresh handle whichever side of the pair is current.  For the fifteen cases on nchan rows: a chunk that is no [rows][n] is
refused by the Pipe layer and leaves the state alone.

One case per block kind (real and complex where a block has both) in the smallest configuration its own GPU test uses,
nchan = 3 where the block takes nchan, calls of 3000 and 1000 samples per row (multiples of every k and decimation here,
whole frames at M = 8) from a seeded generator.  Every comparison is of bits: the same calls on the same state give the same
bits for every block.
Every test runs under a time limit of its own: a watchdog thread ends the process if a GPU call does not come back."""
import faulthandler

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

cs = pytest.importorskip("composable_sdr_amd")
from composable_sdr_amd import _lib                           # noqa: E402

f32, c64 = np.float32, np.complex64
LIMIT_S = 120
NCHAN, MAXN, N1, N2 = 3, 4096, 3000, 1000


@pytest.fixture(autouse=True)
def _time_limit(monkeypatch):
    monkeypatch.setenv("CSDR_QUIET", "1")                     # the resampler prints its design otherwise
    faulthandler.dump_traceback_later(LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


class Case:
    """make() -> resource; run(r, x) / lazy(r, x) -> tuple of arrays (lazy: the call that takes the lazily allocated buffer);
    done(r); rows: nchan of the input, 0 for a block of one stream ([n] arrays); is_class: r is one of the handle-owning
    classes (it has .h), not the resource of a function-style Pipe.  For a block whose state is a ping-pong pair, pair = (input
    elements per sample of max_samples, the k, decimation or M / 2 that a call's length is a multiple of, or 0); reset(r): the
    block's reset or rewind, where it has one"""

    def __init__(self, name, make, run, done, dtype, rows, lazy=None, is_class=False, pair=None, reset=None):
        self.name, self.make, self.run, self.done, self.dtype, self.rows = name, make, run, done, dtype, rows
        self.lazy, self.is_class, self.pair, self.reset = lazy or run, is_class, pair, reset


def _pipe(name, pipe, dtype, rows, pair=None):
    return Case(name, pipe._start, lambda r, x: (pipe._process(r, x),), pipe._done, dtype, rows, pair=pair)


def _obj(name, make, dtype, rows, run=None, lazy=None, pair=None, reset=None):
    return Case(name, make, run or (lambda r, x: (r.process(x),)), lambda r: r.close(), dtype, rows, lazy, True, pair, reset)


def _reset(r):
    r.reset()


def _rewind(r):
    r.rewind()


CASES = [
    _pipe("dcblock", cs.dcBlocker(max_samples=MAXN), c64, 0),
    _pipe("nco-down", cs.mixDown(0.1, max_samples=MAXN), c64, 0),
    _pipe("nco-up", cs.mixUp(0.123, max_samples=MAXN), c64, 0),
    _pipe("agc", cs.automaticGainControl(-35.0, nchan=NCHAN, max_samples=MAXN), c64, NCHAN),
    _pipe("freqdem", cs.fmDemodulator(0.3, nchan=NCHAN, max_samples=MAXN), c64, NCHAN, pair=(1, 0)),
    _pipe("iirfilt", cs.iirFilter(2, 0.025, nchan=NCHAN, max_samples=MAXN), f32, NCHAN, pair=(1, 0)),
    _pipe("firdecim", cs.firDecimator(4, nchan=NCHAN, max_samples=MAXN), f32, NCHAN, pair=(1, 4)),
    _pipe("resamp", cs.resampler(0.3, 60.0, max_samples=MAXN), c64, 0),
    _pipe("ampdem", cs.amDemodulator(nchan=NCHAN, max_samples=MAXN), c64, NCHAN, pair=(1, 0)),
    _obj("fmstereo", lambda: cs.FmStereo(192e3, 4, nchan=NCHAN, max_samples=MAXN), f32, NCHAN),
    _obj("symsync", lambda: cs.SymSync(4, 4, 0.0, 64, nchan=NCHAN, max_samples=MAXN), f32, NCHAN, run=lambda r, x: tuple(r.process(x))),
    _obj("firhilb-decim", lambda: cs.FirHilb(max_samples=MAXN), f32, 0, run=lambda r, x: (r.decim(x),), pair=(2, 0),
         reset=_reset),
    _obj("firhilb-interp", lambda: cs.FirHilb(max_samples=MAXN), c64, 0, run=lambda r, x: (r.interp(x),), pair=(1, 0),
         reset=_reset),
    _obj("fskdem", lambda: cs.FskDem(1, 8, 0.25, nchan=NCHAN, max_samples=MAXN), c64, NCHAN,
         lazy=lambda r, x: r.process_rows(x, energy=True)),
    _obj("firfilt-real", lambda: cs.FirFilt(np.ones(5, f32), 1.0, is_complex=False, nchan=NCHAN, max_samples=MAXN), f32, NCHAN,
         pair=(1, 0), reset=_reset),
    _obj("firfilt-complex", lambda: cs.FirFilt.kaiser(21, 0.1, 60.0, is_complex=True, nchan=NCHAN, max_samples=MAXN), c64, NCHAN,
         pair=(1, 0), reset=_reset),
    _obj("gmskdem", lambda: cs.GmskDem(4, 3, 0.3, nchan=NCHAN, max_samples=MAXN), c64, NCHAN,
         lazy=lambda r, x: r.process_rows(x, soft=True), pair=(1, 4), reset=_reset),
    _obj("iirsos-real", lambda: cs.IirSos.prototype(3, 0.1, is_complex=False, nchan=NCHAN, max_samples=MAXN), f32, NCHAN),
    _obj("iirsos-complex", lambda: cs.IirSos.prototype(3, 0.1, is_complex=True, nchan=NCHAN, max_samples=MAXN), c64, NCHAN),
    # the analyzer counts its calls in samples (max_frames M / 2 = MAXN of them), the synthesizer in frames: rows of MAXN at most
    _obj("pfbch2", lambda: cs.Firpfbch2.kaiser(8, 3, max_frames=MAXN // 4), c64, 0, pair=(1, 4), reset=_rewind),
    _obj("pfbsyn2", lambda: cs.Firpfbch2Synth.kaiser(8, 3, max_frames=MAXN), c64, 8, pair=(1, 0), reset=_rewind),
    _obj("rowresamp", lambda: cs.RowResamp(0.48, 7, complex=True, nchan=NCHAN, max_samples=MAXN), c64, NCHAN, pair=(1, 0),
         reset=_rewind),
]
PAIRS = [c for c in CASES if c.pair]                          # the ten blocks with a ping-pong pair: seven older ones, the three newest
RESETS = [c for c in PAIRS if c.reset]
ROWED = [c for c in CASES if c.rows > 1]                      # the fifteen cases whose chunks are [rows][n]


def _input(case, n, seed):
    shape = (case.rows, n) if case.rows else (n,)
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape)
    if case.dtype is c64:
        x = x + 1j * rng.standard_normal(shape)
    return (0.5 * x).astype(case.dtype)


def _assert_same_bits(got, want, what):
    assert len(got) == len(want) and len(got) >= 1, what
    for g, w in zip(got, want):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape and g.size > 0, (what, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), what


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_two_handles_are_independent_and_close_is_idempotent(case):
    x, x2 = _input(case, N1, 1), _input(case, N2, 2)
    a, b = case.make(), case.make()
    _assert_same_bits(case.run(a, x), case.run(b, x), "two fresh handles, the same input")
    case.done(b)
    got = case.lazy(a, x2)                                    # the survivor goes on from its own state, in its own buffers
    c = case.make()
    case.run(c, x)
    _assert_same_bits(got, case.lazy(c, x2), "the survivor of a destroy against a third fresh handle")
    for r in (a, b, c):
        case.done(r)
        case.done(r)                                          # a second close (a second _done) is fine
    if case.is_class:
        for r in (a, b, c):
            for use in (lambda: r.h, lambda: case.run(r, x)):
                with pytest.raises(cs.CsdrError) as e:
                    use()
                assert e.value.code == _lib.ERR_INVALID and "already destroyed" in str(e.value)
    else:
        assert not a.h and not b.h and not c.h


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_create_close_cycles_without_a_call(case):
    for _ in range(3):
        case.done(case.make())


def test_resampler_rate_zero_owns_no_device_memory_and_still_lives_the_same_life():
    pipe = cs.resampler(0.0, max_samples=MAXN)
    x = _input(CASES[0], N1, 3)
    a, b = pipe._start(), pipe._start()
    assert np.array_equal(pipe._process(a, x), x) and np.array_equal(pipe._process(b, x), x)
    pipe._done(b)
    assert np.array_equal(pipe._process(a, x[:N2]), x[:N2])
    pipe._done(a)
    pipe._done(a)
    pipe._done(b)
    for _ in range(3):
        pipe._done(pipe._start())


@pytest.mark.parametrize("case", PAIRS, ids=[c.name for c in PAIRS])
def test_a_refused_call_leaves_the_state_alone(case):
    """calls A, refused ones, B against A, B on a fresh handle.  Refused: max + 1 samples per row and, where a call's length
    has to be a multiple of something, the first multiple past max and a length below max that is no multiple"""
    xa, xb = _input(case, N1, 1), _input(case, N2, 2)
    unit, step = case.pair
    refused = [(MAXN + 1) * unit] + ([MAXN + step, N2 + step // 2] if step else [])
    a, b = case.make(), case.make()
    want = case.run(b, xa), case.run(b, xb)
    _assert_same_bits(case.run(a, xa), want[0], "call A")
    for n in refused:
        with pytest.raises(cs.CsdrError) as e:
            case.run(a, _input(case, n, 3))
        assert e.value.code == _lib.ERR_SIZE, (n, str(e.value))
    _assert_same_bits(case.run(a, xb), want[1], "call B behind the refused calls")
    case.done(a)
    case.done(b)


@pytest.mark.parametrize("case", ROWED, ids=[c.name for c in ROWED])
def test_a_ragged_chunk_is_refused_and_leaves_the_state_alone(case):
    """a flat chunk of rows * 1000 + 1 elements is no [rows][n]: the Pipe layer refuses it (ERR_INVALID) before the library is
    called, so the call behind it gives the bits of a handle that never saw it"""
    x1, x2 = _input(case, N2, 1), _input(case, N2, 2)
    a, b = case.make(), case.make()
    _assert_same_bits(case.run(a, x1), case.run(b, x1), "the first call")
    ragged = np.append(_input(case, N2, 3).reshape(-1), case.dtype(0.25))
    assert ragged.shape == (case.rows * N2 + 1,) and ragged.dtype == case.dtype
    with pytest.raises(cs.CsdrError) as e:
        case.run(a, ragged)
    assert e.value.code == _lib.ERR_INVALID, str(e.value)
    _assert_same_bits(case.run(a, x2), case.run(b, x2), "the second call, behind the refused chunk on one of the two")
    case.done(a)
    case.done(b)


@pytest.mark.parametrize("case", RESETS, ids=[c.name for c in RESETS])
def test_reset_after_one_call_and_after_two_calls_both_give_the_create_state(case):
    """one call leaves the pair on its second side, two calls on its first: the call after the reset equals a fresh handle's"""
    xa, xb = _input(case, N1, 1), _input(case, N2, 2)
    fresh = case.make()
    want = case.run(fresh, xa)
    case.done(fresh)
    for calls in ((xa,), (xa, xb)):
        r = case.make()
        for x in calls:
            case.run(r, x)
        case.reset(r)
        _assert_same_bits(case.run(r, xa), want, f"the call behind a reset after {len(calls)} call(s)")
        case.done(r)
