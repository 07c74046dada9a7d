"""What composable_sdr_amd/pipes.py hands to the C ABI, without a GPU and without the built library: `pipes.lib` is replaced by
a stand-in whose every attribute is a callable that records (name, arguments) and returns 0.  A create or open writes a
non-null handle through the byref it is given, and a call that reports a count writes the count the block's rule predicts.

In the record a pointer is an integer (c_void_p(v) and v are equal, None and 0 are equal), an array is
("array", dtype, shape, C-contiguous), a byref is ("ref", the type's name) and a ctypes array is ("carray", type, values).

For each of the eighteen blocks and Chain, through the public class or Pipe: the create call and its scalars; for chunks of
[nchan][n] (strided, of the wrong dtype) and flat [nchan * n] the entry point, the n it gets, dtype / shape / contiguity of input
and output and the returned shape; every device entry point's argument list; close twice and work after close; and the ragged
chunk (nchan = 2, 7 elements), which is refused before the library is called.  nchan in {1, 2, 3}, n in {0, k, 2 k + 1} with k the
block's samples per symbol or decimation: the places a `//` can go wrong."""
import ctypes as C
import re

import numpy as np
import pytest

import composable_sdr_amd as cs
from composable_sdr_amd import _lib, pipes, sharded

f32, c64, u32 = np.dtype(np.float32), np.dtype(np.complex64), np.dtype(np.uint32)
H0, MAXN = 0xA000, 512
X, Y, Z, S = 0x1000, 0x2000, 0x3000, 0x77
REF32, REF64, REFH = ("ref", "c_uint"), ("ref", "c_ulong"), ("ref", "c_void_p")
assert C.c_uint32 is C.c_uint and C.c_uint64 is C.c_ulong


def _array_of(arg):
    """the numpy array behind a pointer that ndarray.ctypes.data_as made, or None"""
    arr = getattr(arg, "_arr", None)
    return arr if isinstance(arr, np.ndarray) else None


def _norm(a):
    arr = _array_of(a)
    if arr is not None:
        return ("array", arr.dtype, arr.shape, bool(arr.flags.c_contiguous))
    if hasattr(a, "_obj"):
        return ("ref", type(a._obj).__name__)
    if a is None:
        return 0
    if isinstance(a, C.c_void_p):
        return a.value or 0
    if isinstance(a, C.Array):
        return ("carray", a._type_.__name__, a.raw if a._type_ is C.c_char else list(a))
    if isinstance(a, (np.integer, np.floating)):
        return a.item()
    return a


def A(dtype, *shape):
    return ("array", dtype, tuple(shape), True)


class RecordingLib:
    """report[name](*args) -> the values for the call's byrefs, in order; fill[name] = (i, f): argument i's array gets f(*args);
    returns[name](*args) -> the call's return value instead of 0"""

    def __init__(self):
        self.calls, self.raw, self.report, self.fill, self.returns = [], [], {}, {}, {}
        self._next = H0

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, tuple(_norm(a) for a in args)))
            self.raw.append(args)
            if re.search(r"_(create|open)(_[a-z]+)?$", name):
                args[-1]._obj.value = self._next
                self._next += 0x10
            if name in self.report:
                for ref, v in zip([a for a in args if hasattr(a, "_obj")], self.report[name](*args)):
                    ref._obj.value = v
            if name in self.fill:
                i, f = self.fill[name]
                _array_of(args[i])[...] = f(*args)
            return self.returns[name](*args) if name in self.returns else 0
        return fn

    def since(self, mark):
        return self.calls[mark:]


@pytest.fixture
def L(monkeypatch):
    fake = RecordingLib()
    monkeypatch.setattr(pipes, "lib", lambda: fake)
    monkeypatch.setattr(sharded, "lib", lambda: fake)
    return fake


def _invalid(e, text):
    assert e.value.code == _lib.ERR_INVALID and text in str(e.value), str(e.value)


def _strided(dtype, *shape):
    """[..][n] of twice the precision, every second element of [..][2 n]: wrong dtype, not contiguous"""
    wide = np.complex128 if dtype == c64 else np.float64
    base = np.arange(int(np.prod(shape)) * 2, dtype=np.float64).reshape(shape[:-1] + (2 * shape[-1],)).astype(wide)
    x = base[..., ::2]
    assert x.shape == shape and x.dtype != dtype and (x.size < 2 or not x.flags.c_contiguous)
    return x


# ---------------------------------------------------------------------------------------------------------------- the row blocks
class Row:
    """One block on `nchan` rows.  make(nchan) -> (resource, process(a), done()); create(nchan) -> (entry, scalars before the
    handle's byref); entry(h, x, n, y, *tail); rule(n) -> elements per output row; layout: "like" (y and the result laid out as
    the caller's chunk), "first" (y [nchan][m]; the result is y, or its first row for a one-dimensional chunk) or "split" (y
    [nchan][m]; the result is the list of rows cut to the reported counts, or the first of them); before(h, nchan, n): the calls
    ahead of the entry point; rig(L, nchan): what the stand-in reports"""

    def __init__(self, name, block, make, create, entry, dtype, out_dtype, k=5, rule=lambda n: n, layout="like", tail=lambda nchan, n: (),
                 is_class=True, nchans=(1, 2, 3), before=lambda h, nchan, n: [], rig=lambda L, nchan: None, after_create=lambda h: []):
        self.name, self.block, self.make, self.create, self.entry, self.dtype, self.out_dtype = name, block, make, create, entry, dtype, out_dtype
        self.k, self.rule, self.layout, self.tail, self.is_class, self.nchans = k, rule, layout, tail, is_class, nchans
        self.before, self.rig, self.after_create = before, rig, after_create


def _of_pipe(pipe):
    def make(nchan):
        p = pipe(nchan)
        r = p._start()
        return r, (lambda a: p._process(r, a)), (lambda: p._done(r))
    return make


def _of_class(ctor, method="process"):
    def make(nchan):
        r = ctor(nchan)
        return r, getattr(r, method), r.close
    return make


def _first_gen(name, block, pipe, scalars, dtype, out_dtype, entry="process", nchans=(1, 2, 3), **kw):
    return Row(name, block, _of_pipe(pipe), lambda nchan: (f"csdr_{block}_create", scalars(nchan)), f"csdr_{block}_{entry}", dtype, out_dtype,
               is_class=False, nchans=nchans, **kw)


def _rig_count(entry, count):
    """the entry point reports count(nchan, n) through its byref"""
    def rig(L, nchan):
        L.report[entry] = lambda h, x, n, *rest: (count(nchan, n),)
    return rig


def _rig_symsync(entry):
    def rig(L, nchan):
        L.fill[entry] = (4, lambda h, x, n, y, ny: n // 2)
    return rig


def _rig_rowresamp(L, nchan):
    L.report["csdr_rowresamp_count"] = lambda h, n, ref: (n * 48 // 100,)
    L.report["csdr_rowresamp_process"] = lambda h, x, n, y, ref: (n * 48 // 100,)


ROWS = [
    _first_gen("dcblock", "dcblock", lambda nchan: cs.dcBlocker(0.001, MAXN), lambda nchan: (0.001, MAXN), c64, c64, nchans=(1,)),
    _first_gen("nco-down", "nco", lambda nchan: cs.mixDown(0.1, MAXN), lambda nchan: (0.1, MAXN), c64, c64, entry="mix_down", nchans=(1,)),
    _first_gen("nco-up", "nco", lambda nchan: cs.mixUp(0.123, MAXN), lambda nchan: (0.123, MAXN), c64, c64, entry="mix_up", nchans=(1,)),
    _first_gen("agc", "agc", lambda nchan: cs.automaticGainControl(-35.0, nchan, MAXN), lambda nchan: (-35.0, nchan, MAXN), c64, c64),
    _first_gen("freqdem", "freqdem", lambda nchan: cs.fmDemodulator(0.3, nchan, MAXN), lambda nchan: (0.3, nchan, MAXN), c64, f32),
    _first_gen("iirfilt", "iirfilt", lambda nchan: cs.iirFilter(2, 0.025, 0.0, 10.0, 10.0, nchan, MAXN),
               lambda nchan: (2, 0.025, 0.0, 10.0, 10.0, nchan, MAXN), f32, f32),
    _first_gen("firdecim", "firdecim", lambda nchan: cs.firDecimator(4, nchan, MAXN), lambda nchan: (4, nchan, MAXN), f32, f32, k=4,
               rule=lambda n: n // 4),
    _first_gen("ampdem", "ampdem", lambda nchan: cs.amDemodulator(nchan, MAXN, 0.7), lambda nchan: (0.7, nchan, MAXN), c64, f32),
    Row("fmstereo", "fmstereo", _of_class(lambda nchan: cs.FmStereo(192e3, 4, nchan, MAXN)),
        lambda nchan: ("csdr_fmstereo_create", (192000.0, 4, nchan, MAXN)), "csdr_fmstereo_process", f32, f32, k=4,
        rule=lambda n: 2 * (n // 4), tail=lambda nchan, n: (REF32,),
        rig=_rig_count("csdr_fmstereo_process", lambda nchan, n: nchan * 2 * (n // 4))),
    Row("symsync", "symsync", _of_class(lambda nchan: cs.SymSync(4, 3, 0.25, 16, nchan, MAXN, lf_bw=0.02, k_out=1)),
        lambda nchan: ("csdr_symsync_create", (4, 3, 0.25, 16, 0.02, 1, nchan, MAXN)), "csdr_symsync_process", f32, f32, k=4,
        layout="split", tail=lambda nchan, n: (A(u32, nchan),), rig=_rig_symsync("csdr_symsync_process")),
    Row("symsyncc", "symsync", _of_pipe(lambda nchan: cs.symSyncC(3, 2, nchan, MAXN)),
        lambda nchan: ("csdr_symsync_create", (2, 3, 0.0, 32, 0.01, 1, nchan, MAXN)), "csdr_symsync_process_c", c64, c64, k=2,
        layout="split", tail=lambda nchan, n: (A(u32, nchan),), rig=_rig_symsync("csdr_symsync_process_c"),
        after_create=lambda h: [("csdr_symsync_set_rnyquist", (h, cs.CSDR_FIRFILT_ARKAISER, 0.5))]),
    Row("fskdem", "fskdem", _of_class(lambda nchan: cs.FskDem(2, 8, 0.25, nchan, MAXN)),
        lambda nchan: ("csdr_fskdem_create", (2, 8, 0.25, nchan, MAXN)), "csdr_fskdem_process", c64, u32, k=8, rule=lambda n: n // 8,
        layout="first", tail=lambda nchan, n: (0, REF32), rig=_rig_count("csdr_fskdem_process", lambda nchan, n: nchan * (n // 8))),
    Row("gmskdem", "gmskdem", _of_class(lambda nchan: cs.GmskDem(4, 3, 0.3, nchan, MAXN)),
        lambda nchan: ("csdr_gmskdem_create", (4, 3, 0.3, nchan, MAXN)), "csdr_gmskdem_process", c64, u32, k=4, rule=lambda n: n // 4,
        layout="first", tail=lambda nchan, n: (0, REF32), rig=_rig_count("csdr_gmskdem_process", lambda nchan, n: nchan * (n // 4))),
    Row("firfilt-taps-real", "firfilt", _of_class(lambda nchan: cs.FirFilt(np.ones(5), 0.5, False, nchan, MAXN)),
        lambda nchan: ("csdr_firfilt_create_taps", (A(f32, 5), 5, 0.5, 0, nchan, MAXN)), "csdr_firfilt_process", f32, f32),
    Row("firfilt-kaiser-complex", "firfilt", _of_class(lambda nchan: cs.FirFilt.kaiser(21, 0.1, 60.0, 0.0, True, nchan, MAXN)),
        lambda nchan: ("csdr_firfilt_create_kaiser", (21, 0.1, 60.0, 0.0, 1, nchan, MAXN)), "csdr_firfilt_process", c64, c64),
    Row("iirsos-prototype-real", "iirsos", _of_class(lambda nchan: cs.IirSos.prototype(3, 0.1, 0.0, 10.0, 10.0, False, nchan, MAXN)),
        lambda nchan: ("csdr_iirsos_create_prototype", (3, 0.1, 0.0, 10.0, 10.0, 0, nchan, MAXN)), "csdr_iirsos_process", f32, f32),
    Row("iirsos-sos-complex", "iirsos", _of_class(lambda nchan: cs.IirSos(np.ones((2, 3)), np.ones((2, 3)), True, nchan, MAXN)),
        lambda nchan: ("csdr_iirsos_create_sos", (A(f32, 6), A(f32, 6), 2, 1, nchan, MAXN)), "csdr_iirsos_process", c64, c64),
    Row("rowresamp", "rowresamp", _of_class(lambda nchan: cs.RowResamp(0.48, 7, 60.0, 0.0, True, nchan, MAXN)),
        lambda nchan: ("csdr_rowresamp_open", (0.48, 7, 60.0, 0.0, 1, nchan, MAXN)), "csdr_rowresamp_process", c64, c64, k=25,
        rule=lambda n: n * 48 // 100, layout="first", tail=lambda nchan, n: (REF32,),
        before=lambda h, nchan, n: [("csdr_rowresamp_count", (h, n, REF32))], rig=_rig_rowresamp),
]


def _chunks(row, nchan, n):
    """(chunk, its shape at the library) for [nchan][n] strided and of the wrong dtype, and flat [nchan * n] as it should be"""
    yield _strided(row.dtype, nchan, n), (nchan, n)
    yield np.zeros(nchan * n, dtype=row.dtype), (nchan * n,)


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_row_block_create_calls_shapes_and_close(L, row):
    for nchan in row.nchans:
        mark = len(L.calls)
        r, process, done = row.make(nchan)
        entry, scalars = row.create(nchan)
        h = r.h.value
        assert L.since(mark) == [(entry, scalars + (REFH,))] + row.after_create(h), (row.name, nchan)
        row.rig(L, nchan)
        for n in (0, row.k, 2 * row.k + 1):
            m = row.rule(n)
            for a, x_shape in _chunks(row, nchan, n):
                flat = len(x_shape) == 1
                if row.layout == "like":
                    y_shape = x_shape if m == n else ((nchan * m,) if flat else (nchan, m))
                else:
                    y_shape = (nchan, m)
                mark = len(L.calls)
                got = process(a)
                what = (row.name, nchan, n, x_shape)
                want = (row.entry, (h, A(row.dtype, *x_shape), n, A(row.out_dtype, *y_shape)) + row.tail(nchan, n))
                assert L.since(mark) == row.before(h, nchan, n) + [want], what
                if row.layout == "split":
                    rows = [got] if flat else got
                    assert isinstance(got, np.ndarray if flat else list) and len(rows) == (1 if flat else nchan), what
                    assert all(g.shape == (n // 2,) and g.dtype == row.out_dtype for g in rows), what
                else:
                    assert isinstance(got, np.ndarray) and got.dtype == row.out_dtype, what
                    assert got.shape == ((m,) if row.layout == "first" and flat else y_shape), what
        mark = len(L.calls)
        done()
        done()                                                  # a second close is fine, and is one destroy
        assert L.since(mark) == [(f"csdr_{row.block}_destroy", (h,))], (row.name, nchan)
        if row.is_class or row.name == "symsyncc":
            for use in (lambda: r.h, lambda: process(np.zeros(nchan * row.k, dtype=row.dtype))):
                with pytest.raises(cs.CsdrError) as e:
                    use()
                _invalid(e, f"{row.block} already destroyed")
            assert L.since(mark + 1) == []
        else:
            assert not r.h


@pytest.mark.parametrize("row", [r for r in ROWS if 2 in r.nchans], ids=[r.name for r in ROWS if 2 in r.nchans])
def test_a_ragged_chunk_is_refused_before_the_library_is_called(L, row):
    """nchan = 2 and 7 elements: no [2][n].  Before, the library got n = 3 and the caller an array whose last element nobody wrote"""
    r, process, done = row.make(2)
    row.rig(L, 2)
    mark = len(L.calls)
    for a in (np.zeros(7, dtype=row.dtype), _strided(row.dtype, 7)):
        with pytest.raises(cs.CsdrError) as e:
            process(a)
        _invalid(e, f"{row.block}: a chunk of shape (7,), not [2][n]")
    assert L.since(mark) == []
    assert np.shape(process(np.zeros(8, dtype=row.dtype)))      # the object goes on working
    done()


def test_second_outputs_of_the_symbol_demodulators(L):
    for make, kw, entry, per in ((lambda: cs.FskDem(2, 8, 0.25, 3, MAXN), "energy", "csdr_fskdem_process", (4,)),
                                 (lambda: cs.GmskDem(8, 3, 0.3, 3, MAXN), "soft", "csdr_gmskdem_process", ())):
        r = make()
        L.report[entry] = lambda h, x, n, sym, e, ref: (3 * (n // 8),)
        for n in (0, 8, 17):
            mark = len(L.calls)
            sym, e = r.process_rows(_strided(c64, 3, n), **{kw: True})
            assert L.since(mark) == [(entry, (r.h.value, A(c64, 3, n), n, A(u32, 3, n // 8), A(f32, 3, n // 8, *per), REF32))]
            assert sym.shape == (3, n // 8) and sym.dtype == u32 and e.shape == (3, n // 8) + per and e.dtype == f32
        r.close()


def test_rowresamp_keeps_its_stricter_shape_check(L):
    r = cs.RowResamp(0.48, nchan=2, max_samples=MAXN)
    mark = len(L.calls)
    for a in (np.zeros((4, 3), c64), np.zeros((2, 2, 3), c64), np.zeros((1, 12), c64), np.zeros(7, c64)):
        with pytest.raises(cs.CsdrError) as e:
            r.process(a)
        _invalid(e, f"rowresamp: a chunk of shape {a.shape}, not [2][n]")
    assert L.since(mark) == []
    r.close()


# ---------------------------------------------------------------------------------------------------------------- the other blocks
def test_resampler_allocates_max_out_and_returns_the_reported_count(L):
    pipe = cs.resampler(0.3, 60.0, MAXN)
    r = pipe._start()
    h = r.h.value
    assert L.calls == [("csdr_resamp_create", (0.3, 60.0, MAXN, REFH))]
    L.returns["csdr_resamp_max_out"] = lambda h, n: n + 2
    L.report["csdr_resamp_process"] = lambda h, x, n, y, ref: (n // 3,)
    for n in (0, 3, 7):
        for a in (_strided(c64, n), np.zeros(n, c64)):
            mark = len(L.calls)
            got = pipe._process(r, a)
            assert L.since(mark) == [("csdr_resamp_max_out", (h, n)), ("csdr_resamp_process", (h, A(c64, n), n, A(c64, n + 2), REF32))]
            assert got.shape == (n // 3,) and got.dtype == c64 and got.base is None
    mark = len(L.calls)
    pipe._done(r)
    pipe._done(r)
    assert L.since(mark) == [("csdr_resamp_destroy", (h,))] and not r.h


def test_firhilb_halves_and_doubles(L):
    r = cs.FirHilb(5, 60.0, MAXN)
    h = r.h.value
    assert L.calls == [("csdr_firhilb_create", (5, 60.0, MAXN, REFH))]
    for n in (0, 2, 5):
        for length in (2 * n, 2 * n + 1):                       # `length div 2` drops an odd last float
            for a in (_strided(f32, length), np.zeros(length, f32)):
                mark = len(L.calls)
                got = r.decim(a)
                assert L.since(mark) == [("csdr_firhilb_decim", (h, A(f32, length), n, A(c64, n)))]
                assert got.shape == (n,) and got.dtype == c64
        for a in (_strided(c64, n), np.zeros(n, c64)):
            mark = len(L.calls)
            got = r.interp(a)
            assert L.since(mark) == [("csdr_firhilb_interp", (h, A(c64, n), n, A(f32, 2 * n)))]
            assert got.shape == (2 * n,) and got.dtype == f32
    mark = len(L.calls)
    r.reset()
    r.close()
    r.close()
    assert L.since(mark) == [("csdr_firhilb_reset", (h,)), ("csdr_firhilb_destroy", (h,))]
    for use in (lambda: r.decim(np.zeros(4, f32)), lambda: r.interp(np.zeros(4, c64)), r.reset):
        with pytest.raises(cs.CsdrError) as e:
            use()
        _invalid(e, "firhilb already destroyed")


BANKS = [(cs.Firpfbch2, "pfbch2"), (cs.Firpfbch2Synth, "pfbsyn2")]


@pytest.mark.parametrize("cls,block", BANKS, ids=[b for _, b in BANKS])
def test_bank_objects_both_constructors_getters_and_close(L, cls, block):
    M, m = 8, 3
    for bad in (np.zeros(2 * M * m + 1), np.zeros(0)):
        with pytest.raises(cs.CsdrError) as e:
            cls(bad, M, m)
        _invalid(e, f"{block}: {bad.size} taps, not 2 M m = 48")
    assert L.calls == []
    a = cls(np.zeros((2 * m, M)), M, m, 64)                    # float64 and [2 m][M]: converted and flattened
    b = cls.kaiser(M, m, 80.0, 0.0, 64)
    assert L.calls == [(f"csdr_{block}_open_taps", (A(f32, 2 * M * m), M, m, 64, REFH)),
                       (f"csdr_{block}_open_kaiser", (M, m, 80.0, 0.0, 64, REFH))]
    for r in (a, b):
        h = r.h.value
        assert type(r) is cls and (r.M, r.m) == (M, m)
        mark = len(L.calls)
        assert r.taps().shape == (2 * M * m,)
        r.rewind()
        r.close()
        r.close()
        assert L.since(mark) == [(f"csdr_{block}_get_taps", (h, A(f32, 2 * M * m))), (f"csdr_{block}_rewind", (h,)),
                                 (f"csdr_{block}_destroy", (h,))]
        for use in (r.taps, r.rewind, lambda: r.process(np.zeros((M, 4), c64)), lambda: r.process_device(X, 4, Y)):
            with pytest.raises(cs.CsdrError) as e:
                use()
            _invalid(e, f"{block} already destroyed")


def test_pfbch2_process_and_the_channelizer_pipes_list(L):
    M = 8
    pipe = cs.firpfbch2Channelizer(M, 3, 80.0, 0.0, 64)
    r = pipe._start()
    h = r.h.value
    L.report["csdr_pfbch2_process"] = lambda h, x, n, y, ref: (n // (M // 2),)
    for frames in (0, 1, 3):
        n = frames * (M // 2)
        for a in (_strided(c64, n), np.zeros((frames, M // 2), c64)):
            mark = len(L.calls)
            y = r.process(a)
            assert L.since(mark) == [("csdr_pfbch2_process", (h, A(c64, n), n, A(c64, M, frames), REF32))]
            assert y.shape == (M, frames) and y.dtype == c64
            mark = len(L.calls)
            rows = pipe._process(r, a)
            if n == 0:                                          # [empty], and the library is not called
                assert L.since(mark) == [] and len(rows) == 1 and rows[0].shape == (0,) and rows[0].dtype == c64
            else:
                assert len(L.since(mark)) == 1 and isinstance(rows, list) and len(rows) == M
                assert all(row.shape == (frames,) and row.dtype == c64 for row in rows)
    pipe._done(r)


def test_pfbsyn2_process_and_the_synthesizer_pipes_rows(L):
    M = 8
    pipe = cs.firpfbch2Synthesizer(M, 3, 80.0, 0.0, 64)
    r = pipe._start()
    h = r.h.value
    L.report["csdr_pfbsyn2_process"] = lambda h, y, frames, x, ref: (frames * (M // 2),)
    for frames in (0, 1, 3):
        for a in (_strided(c64, M, frames), np.zeros((M, frames), c64)):
            mark = len(L.calls)
            x = r.process(a)
            assert L.since(mark) == [("csdr_pfbsyn2_process", (h, A(c64, M, frames), frames, A(c64, frames * (M // 2)), REF32))]
            assert x.shape == (frames * (M // 2),) and x.dtype == c64
            mark = len(L.calls)
            x = pipe._process(r, list(a))
            assert x.shape == (frames * (M // 2),) and len(L.since(mark)) == (1 if frames else 0)
    assert pipe._process(r, [np.empty(0, c64)]).shape == (0,)   # what the channelizer yields for an empty chunk
    mark = len(L.calls)
    for a in (np.zeros(M * 4, c64), np.zeros((M + 1, 4), c64)):
        with pytest.raises(cs.CsdrError) as e:
            r.process(a)
        _invalid(e, f"pfbsyn2: a chunk of shape {a.shape}, not [{M}][frames]")
    assert L.since(mark) == []
    pipe._done(r)


def test_chain_create_process_submit_collect_and_close(L):
    ch = cs.Chain(channels=4, demod="fm", kf=0.25, max_frames=64)
    h = ch.h.value
    assert L.calls == [("csdr_chain_cfg_default", (("ref", "ChainCfg"), 4)), ("csdr_chain_create", (("ref", "ChainCfg"), REFH))]
    cfg = L.raw[1][0]._obj
    assert (cfg.channels, cfg.demod, cfg.max_frames, cfg.flags, cfg.dc_block) == (4, _lib.DEMOD_FM, 64, _lib.FLAG_QUIET, 1)
    assert cfg.kf == np.float32(0.25) and cfg.pfb_m == 7
    L.report["csdr_chain_process"] = lambda h, x, n, out, ref: (n,)
    L.report["csdr_chain_collect"] = lambda h, ref: (12,)
    for nf in (0, 1, 3):
        for a in (_strided(c64, 4 * nf), np.zeros(4 * nf, c64)):
            mark = len(L.calls)
            out = ch.process(a)
            assert L.since(mark) == [("csdr_chain_process", (h, A(c64, 4 * nf), 4 * nf, A(f32, 4, nf), REF32))]
            assert out.shape == (4, nf) and out.dtype == f32
    mark = len(L.calls)
    outs = [ch.submit(_strided(c64, 12)), ch.submit(np.zeros(12, c64))]
    assert [ch.collect() is o for o in outs] == [True, True]
    submit = ("csdr_chain_submit", (h, A(c64, 12), 12, A(f32, 4, 3)))
    assert L.since(mark) == [submit, submit, ("csdr_chain_collect", (h, REF32)), ("csdr_chain_collect", (h, REF32))]
    mark = len(L.calls)
    ch.submit(np.zeros(12, c64))
    ch.reset()
    ch.seek_frames(32)
    assert ch._pending == []
    ch.close()
    ch.close()
    assert L.since(mark) == [submit, ("csdr_chain_reset", (h,)), ("csdr_chain_seek_frames", (h, 32)), ("csdr_chain_destroy", (h,))]
    for use in (lambda: ch.process(np.zeros(4, c64)), lambda: ch.process_device(X, 4, Y), lambda: ch.submit(np.zeros(4, c64)), ch.reset):
        with pytest.raises(cs.CsdrError) as e:
            use()
        _invalid(e, "chain already destroyed")


def test_firpfbch_channelizer_pipe_yields_the_list_of_rows(L):
    pipe = cs.firpfbchChannelizer(4, max_frames=64)
    r = pipe._start()
    cfg = L.raw[1][0]._obj
    assert (cfg.channels, cfg.dc_block, cfg.demod) == (4, 0, _lib.DEMOD_NONE)
    L.report["csdr_chain_process"] = lambda h, x, n, out, ref: (n,)
    mark = len(L.calls)
    rows = pipe._process(r, np.zeros(0, c64))
    assert L.since(mark) == [] and len(rows) == 1 and rows[0].shape == (0,) and rows[0].dtype == c64
    rows = pipe._process(r, _strided(c64, 12))
    assert L.since(mark) == [("csdr_chain_process", (r.h.value, A(c64, 12), 12, A(c64, 4, 3), REF32))]
    assert isinstance(rows, list) and len(rows) == 4 and all(row.shape == (3,) and row.dtype == c64 for row in rows)
    pipe._done(r)


# ---------------------------------------------------------------------------------------------------------------- the two-call getters
def test_two_call_getters_ask_for_the_sizes_then_fill(L):
    L.report["csdr_gmskdem_get_design"] = lambda *a: (25,)
    L.report["csdr_rowresamp_design"] = L.report["csdr_rowresamp_get_design"] = lambda *a: (14, 8947849)
    g = cs.GmskDem(4, 3, 0.3)
    r = cs.RowResamp(0.48)
    mark = len(L.calls)
    assert g.design().shape == (25,)
    assert L.since(mark) == [("csdr_gmskdem_get_design", (g.h.value, REF32, 0)), ("csdr_gmskdem_get_design", (g.h.value, 0, A(f32, 25)))]
    mark = len(L.calls)
    bank, delta = cs.firdes_rowresamp(0.48, 7, 60.0, 0.0)
    assert bank.shape == (257, 14) and bank.dtype == f32 and delta == 8947849
    assert L.since(mark) == [("csdr_rowresamp_design", (0.48, 7, 60.0, 0.0, REF32, REF64, 0)),
                             ("csdr_rowresamp_design", (0.48, 7, 60.0, 0.0, 0, 0, A(f32, 257, 14)))]
    mark = len(L.calls)
    bank, delta = r.design()
    assert bank.shape == (257, 14) and delta == 8947849
    assert L.since(mark) == [("csdr_rowresamp_get_design", (r.h.value, REF32, REF64, 0, 0)),
                             ("csdr_rowresamp_get_design", (r.h.value, 0, 0, 0, A(f32, 257, 14)))]
    g.close()
    r.close()


# ---------------------------------------------------------------------------------------------------------------- device entry points
def _comm():
    return sharded.Comm(0, 1, bytes(_lib.COMM_ID_BYTES))


# (make, method, arguments, keyword arguments, entry point, the arguments behind the handle)
DEVICE = [
    (lambda: cs.FmStereo(192e3, 4), "process_device", (X, 8, Y), {}, "csdr_fmstereo_process_device", (X, 8, Y, REF32, 0)),
    (lambda: cs.FmStereo(192e3, 4), "process_device", (X, 8, Y, S), {}, "csdr_fmstereo_process_device", (X, 8, Y, REF32, S)),
    (lambda: cs.SymSync(4), "process_device", (X, 8, Y, Z), {}, "csdr_symsync_process_device", (X, 8, Y, Z, 0)),
    (lambda: cs.SymSync(4), "process_device", (X, 8, Y, Z), {"stream": S}, "csdr_symsync_process_device", (X, 8, Y, Z, S)),
    (lambda: cs.SymSync(4), "process_c_device", (X, 8, Y, Z), {}, "csdr_symsync_process_c_device", (X, 8, Y, Z, 0)),
    (lambda: cs.SymSync(4), "process_c_device", (X, 8, Y, Z, S), {}, "csdr_symsync_process_c_device", (X, 8, Y, Z, S)),
    (lambda: cs.FirHilb(), "decim_device", (X, 8, Y), {}, "csdr_firhilb_decim_device", (X, 8, Y, 0)),
    (lambda: cs.FirHilb(), "interp_device", (X, 8, Y, S), {}, "csdr_firhilb_interp_device", (X, 8, Y, S)),
    (lambda: cs.FskDem(2, 8, 0.25), "process_device", (X, 8, Y), {}, "csdr_fskdem_process_device", (X, 8, Y, 0, 0)),
    (lambda: cs.FskDem(2, 8, 0.25), "process_device", (X, 8, Y, Z, S), {}, "csdr_fskdem_process_device", (X, 8, Y, Z, S)),
    (lambda: cs.GmskDem(4, 3, 0.3), "process_device", (X, 8, Y), {"stream": S}, "csdr_gmskdem_process_device", (X, 8, Y, 0, S)),
    (lambda: cs.GmskDem(4, 3, 0.3), "process_device", (X, 8, Y), {"d_soft_ptr": Z}, "csdr_gmskdem_process_device", (X, 8, Y, Z, 0)),
    (lambda: cs.FirFilt(np.ones(3)), "process_device", (X, 8, Y), {}, "csdr_firfilt_process_device", (X, 8, Y, 0)),
    (lambda: cs.FirFilt.kaiser(21, 0.1), "process_device", (X, 8, X, S), {}, "csdr_firfilt_process_device", (X, 8, X, S)),
    (lambda: cs.IirSos.prototype(3, 0.1), "process_device", (X, 8, Y), {}, "csdr_iirsos_process_device", (X, 8, Y, 0)),
    (lambda: cs.IirSos(np.ones(3), np.ones(3)), "process_device", (X, 8, X, S), {}, "csdr_iirsos_process_device", (X, 8, X, S)),
    (lambda: cs.Chain(channels=4), "process_device", (X, 8, Y), {}, "csdr_chain_process_device", (X, 8, Y, REF32, 0)),
    (lambda: cs.Chain(channels=4), "process_device", (X, 8, Y, S), {}, "csdr_chain_process_device", (X, 8, Y, REF32, S)),
    (lambda: cs.Chain(channels=4), "submit_device", (X, 8, Y), {}, "csdr_chain_submit_device", (X, 8, Y, REF32, 0)),
    (lambda: cs.Chain(channels=4), "submit_device", (X, 8, Y, Z), {}, "csdr_chain_submit_device", (X, 8, Y, REF32, Z)),
    (lambda: cs.Chain(channels=4), "wait_device", (), {}, "csdr_chain_wait_device", (0,)),
    (lambda: cs.Chain(channels=4), "wait_device", (S,), {}, "csdr_chain_wait_device", (S,)),
    (lambda: cs.Firpfbch2.kaiser(8, 3), "process_device", (X, 8, Y), {}, "csdr_pfbch2_process_device", (X, 8, Y, 0)),
    (lambda: cs.Firpfbch2(np.zeros(48), 8, 3), "process_device", (X, 8, Y, S), {}, "csdr_pfbch2_process_device", (X, 8, Y, S)),
    (lambda: cs.Firpfbch2Synth.kaiser(8, 3), "process_device", (X, 8, Y), {}, "csdr_pfbsyn2_process_device", (X, 8, Y, 0)),
    (lambda: cs.Firpfbch2Synth(np.zeros(48), 8, 3), "process_device", (X, 8, Y, S), {}, "csdr_pfbsyn2_process_device", (X, 8, Y, S)),
    (lambda: cs.RowResamp(0.48), "process_device", (X, 8, Y), {}, "csdr_rowresamp_process_device", (X, 8, Y, REF32, 0)),
    (lambda: cs.RowResamp(0.48), "process_device", (X, 8, Y, S), {}, "csdr_rowresamp_process_device", (X, 8, Y, REF32, S)),
    (_comm, "allreduce_f32", (X, 10), {}, "csdr_comm_allreduce_f32", (X, 10, 0)),
    (_comm, "allreduce_f32", (X, 10, S), {}, "csdr_comm_allreduce_f32", (X, 10, S)),
    (_comm, "broadcast", (X, 64), {}, "csdr_comm_broadcast", (X, 64, 0, 0)),
    (_comm, "broadcast", (X, 64, 2, S), {}, "csdr_comm_broadcast", (X, 64, 2, S)),
    (_comm, "hybrid_exchange", (X, Y, 4, [32, 32]), {}, "csdr_hybrid_exchange", (X, Y, 4, ("carray", "c_uint", [32, 32]), 8, 0)),
    (_comm, "hybrid_exchange", (X, Y, 4, [32], 4, S), {}, "csdr_hybrid_exchange", (X, Y, 4, ("carray", "c_uint", [32]), 4, S)),
]


@pytest.mark.parametrize("make,method,args,kw,entry,want", DEVICE, ids=[f"{i:02d}-{d[4][5:]}" for i, d in enumerate(DEVICE)])
def test_device_entry_points_pass_integers_straight_through(L, make, method, args, kw, entry, want):
    r = make()
    L.report[entry] = lambda *a: (5,)
    mark = len(L.calls)
    got = getattr(r, method)(*args, **kw)
    assert L.since(mark) == [(entry, (r.h.value,) + want)]
    assert got == (5 if REF32 in want else None)
    r.close()


def test_comm_create_and_close(L):
    with pytest.raises(ValueError):
        sharded.Comm(0, 1, b"short")
    comm = _comm()
    h = comm.h.value
    assert L.calls == [("csdr_comm_create", (0, 1, ("carray", "c_char", bytes(_lib.COMM_ID_BYTES)), -1, REFH))]
    assert (comm.rank, comm.world) == (0, 1)
    comm.close()
    comm.close()
    assert L.calls[1:] == [("csdr_comm_destroy", (h,))]
