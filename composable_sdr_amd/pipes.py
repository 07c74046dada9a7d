"""Host-side mirror of the reference's DSP blocks (src/ComposableSDR/Liquid.chs) and of
the Pipe protocol (src/ComposableSDR/Types.hs:51-55, 93-131) over the C ABI.

A Pipe is (start, process, done); `start` creates the native object, `process` maps one
array to one array, `done` destroys it -- exactly the life-cycle addPipe/unPipe drive.
Names follow the reference: dcBlocker, mixDown, mixUp, automaticGainControl,
fmDemodulator, firpfbchChannelizer.  `Chain` is the fused replacement for
`mix . mux (replicate nch demod) . firpfbchChannelizer nc` (apps/SoapySDR.hs:218-225).

Every block that works on `nchan` rows takes its arrays through `_rows`, the one place that says how a caller's array is read
as [nchan][n] and how long the output rows are.  Device entry points take raw device pointers and streams as plain integers.
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import CsdrError, check, lib, DEMOD_AM, DEMOD_FM, DEMOD_NONE, DEMOD_WBFM


def _c64(x):
    return np.ascontiguousarray(x, dtype=np.complex64)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Pipe:
    """Pipe {_start, _process, _done} (Types.hs:51-55)."""

    def __init__(self, start, process, done):
        self._start, self._process, self._done = start, process, done

    # Category instance: (.) = compose (Types.hs:101-103); `self . other` runs other first
    def __matmul__(self, other):
        return compose(self, other)


def compose(p1, p2):
    """compose (Types.hs:93-99): process = process2 >=> process1; done2 before done1."""
    def start():
        return (p1._start(), p2._start())

    def process(r, a):
        return p1._process(r[0], p2._process(r[1], a))

    def done(r):
        p2._done(r[1])
        p1._done(r[0])
    return Pipe(start, process, done)


# Category instance: id (Types.hs:101-102)
idPipe = Pipe(lambda: None, lambda r, a: a, lambda r: None)


def unPipe(pipe):
    """unPipe (Types.hs:109-115): create the pipe's resource NOW and hand back
    (stream transformer = S.mapM (process r), cleanup = dest r).  The caller runs
    `cleanup` after the stream has been folded (SoapySDR.hs:206, :282)."""
    r = pipe._start()

    def process(stream):
        for a in stream:
            yield pipe._process(r, a)

    return process, (lambda: pipe._done(r))


class _Handle:
    """Owns one native handle; destroy is idempotent."""

    def __init__(self, h, destroy):
        self.h, self._destroy = h, destroy

    def close(self):
        if self.h:
            check(self._destroy(self.h))
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _new_handle(block, *args, create="create"):
    """csdr_<block>_<create>(*args, &h) -> the owner of the new handle"""
    h = C.c_void_p()
    check(getattr(lib(), f"csdr_{block}_{create}")(*args, C.byref(h)))
    return _Handle(h, getattr(lib(), f"csdr_{block}_destroy"))


def _handle_pipe(block, args, process):
    """a function-style Pipe: `start` creates the csdr_<block> handle from `args`, `process(r, a)` uses r.h, `done` closes it"""
    return Pipe(lambda: _new_handle(block, *args), process, lambda r: r.close())


def _method_pipe(make, method="process"):
    """a Pipe over an object's method: `start` makes the object, `process` calls the method, `done` closes the object"""
    return Pipe(make, lambda r, a: getattr(r, method)(a), lambda r: r.close())


def _rows(block, a, dtype, nchan, out_dtype=None, out_len=None, plane=False, strict=False):
    """The one row marshaller: the caller's array `a` as contiguous `dtype` rows [nchan][n] -> (x, n, y), y the uninitialised
    output of `out_dtype` (default: `dtype`) with `out_len(n)` (default: n) elements per row.  A flat array is rows of
    size // nchan; a size that is no multiple of nchan is refused before anything is called (`strict`: so is an array that is
    neither flat nor [nchan][n]).  y is [nchan][out_len(n)] for `plane`, else laid out as the caller laid out `a`"""
    x = np.ascontiguousarray(a, dtype=dtype)
    if x.size % nchan or (strict and (x.ndim > 2 or (x.ndim == 2 and x.shape[0] != nchan))):
        raise CsdrError(_lib.ERR_INVALID, f"{block}: a chunk of shape {x.shape}, not [{nchan}][n]")
    n = x.size // nchan
    m = n if out_len is None else out_len(n)
    if plane:
        shape = (nchan, m)
    elif out_len is None:
        shape = x.shape
    else:
        shape = x.shape[:-1] + (m,) if x.ndim > 1 else (nchan * m,)
    return x, n, np.empty(shape, dtype=out_dtype or dtype)


def _row_pipe(block, args, dtype, out_dtype, nchan=1, out_len=None, entry="process"):
    """a function-style Pipe over csdr_<block>_<entry>(h, x, n, y) on `nchan` rows: the first-generation blocks"""
    def process(r, a):
        x, n, y = _rows(block, a, dtype, nchan, out_dtype, out_len)
        check(getattr(lib(), f"csdr_{block}_{entry}")(r.h, _ptr(x), n, _ptr(y)))
        return y
    return _handle_pipe(block, args, process)


def _split_rows(y, counts, a):
    """(y [nchan][n], counts [nchan]) -> the list of nchan arrays y[c, :counts[c]], or the one array when the caller's `a` is [n]"""
    out = [y[c, :counts[c]] for c in range(len(counts))]
    return out[0] if np.ndim(a) == 1 else out


def _channel_list(process, a):
    """what a channelizer Pipe yields for the chunk `a`: the rows of process(x) as a list; [empty] for an empty chunk"""
    x = _c64(a)
    return list(process(x)) if x.size else [np.empty(0, dtype=np.complex64)]


def _sized(fn, args, sizes, alloc):
    """A two-call getter: fn(*args, *&sizes, NULL) reports the sizes (None: not asked for), fn(*args, NULL .., buffer) fills the
    buffer that `alloc` makes from them.  Returns the buffer"""
    check(fn(*args, *[None if s is None else C.byref(s) for s in sizes], None))
    buf = alloc(*[s.value for s in sizes if s is not None])
    check(fn(*args, *[None] * len(sizes), _ptr(buf)))
    return buf


class _Owner:
    """Base of the classes that own one native csdr_<_block> handle in `_h`: `h` refuses a closed object, `close` is idempotent"""
    _block = None

    @classmethod
    def _adopt(cls, handle, *state):
        """an object of this class around a handle that is already made (the alternate constructors); `state` goes to _state"""
        self = cls.__new__(cls)
        self._h = handle
        self._state(*state)
        return self

    @property
    def h(self):
        if not self._h.h:
            raise CsdrError(_lib.ERR_INVALID, f"{self._block} already destroyed")
        return self._h.h

    def _get(self, entry, *args):
        """csdr_<_block>_<entry>(h, *args)"""
        return getattr(lib(), f"csdr_{self._block}_{entry}")(self.h, *args)

    def _call(self, entry, *args):
        check(self._get(entry, *args))

    def close(self):
        self._h.close()


class _Resettable(_Owner):
    """... whose C ABI has csdr_<_block>_reset"""

    def reset(self):
        self._call("reset")


def dcBlocker(alpha=0.0005, max_samples=1 << 20):
    """dcBlocker (Liquid.chs:575-589): iirfilt_crcf_create_dc_blocker(0.0005)."""
    return _row_pipe("dcblock", (alpha, max_samples), np.complex64, np.complex64)


def mixDown(f, max_samples=1 << 20):
    """mixDown f (Liquid.chs:798-799): y = x * conj(nco)."""
    return _row_pipe("nco", (f, max_samples), np.complex64, np.complex64, entry="mix_down")


def mixUp(f, max_samples=1 << 20):
    """mixUp f (Liquid.chs:808-809): y = x * nco."""
    return _row_pipe("nco", (f, max_samples), np.complex64, np.complex64, entry="mix_up")


def automaticGainControl(tres, nchan=1, max_samples=4096):
    """automaticGainControl tres (Liquid.chs:727-728); nchan independent instances, input
    and output channel-major [nchan][n] (1-D arrays are treated as one channel)."""
    return _row_pipe("agc", (tres, nchan, max_samples), np.complex64, np.complex64, nchan)


def fmDemodulator(kf, nchan=1, max_samples=4096):
    """fmDemodulator kf (Liquid.chs:333-334)."""
    return _row_pipe("freqdem", (kf, nchan, max_samples), np.complex64, np.float32, nchan)


def iirFilter(n, fc, f0=0.0, ap=10.0, as_db=10.0, nchan=1, max_samples=4096):
    """iirFilter n fc f0 ap as (Liquid.chs:629-638): real-valued Butterworth low-pass (order 2 is what the
    reference instantiates, as the WBFM de-emphasis)."""
    return _row_pipe("iirfilt", (n, fc, f0, ap, as_db, nchan, max_samples), np.float32, np.float32, nchan)


def firDecimator(m, nchan=1, max_samples=4096):
    """firDecimator m (Liquid.chs:500-501): Kaiser decimator (semi-length 10, 60 dB), n div m samples out."""
    return _row_pipe("firdecim", (m, nchan, max_samples), np.float32, np.float32, nchan, lambda n: n // m)


def amDemodulator(nchan=1, max_samples=4096, mod_index=0.8):
    """amDemodulator (Liquid.chs:468-469): ampmodem_create 0.8 DSB, carrier present."""
    return _row_pipe("ampdem", (mod_index, nchan, max_samples), np.complex64, np.float32, nchan)


def wbFMDemodulator(quadRate, decim, max_samples=4096):
    """wbFMDemodulator quadRate decim = firDecimator decim . iirDeemph . fmDemodulator 0.6 (Liquid.chs:653-656)"""
    return compose(firDecimator(decim, max_samples=max_samples),
                   compose(iirFilter(2, 5000.0 / quadRate, 0.0, 10.0, 10.0, max_samples=max_samples),
                           fmDemodulator(0.6, max_samples=max_samples)))


def resampler(r, as_db=60.0, max_samples=1 << 20):
    """resampler r as (Liquid.chs:115-117): Pipe IO (Array CF32) (Array CF32) with a variable-length output
    (`shrinkToFit` to the count msresamp_crcf_execute reports, :79-98).  r == 0 is the identity."""
    def process(rh, a):
        x, n, y = _rows("resamp", a, np.complex64, 1, out_len=lambda n: int(lib().csdr_resamp_max_out(rh.h, n)))
        n_out = C.c_uint32()
        check(lib().csdr_resamp_process(rh.h, _ptr(x), n, _ptr(y), C.byref(n_out)))
        return y.reshape(-1)[:n_out.value].copy()
    return _handle_pipe("resamp", (r, as_db, max_samples), process)


class FmStereo(_Resettable):
    """The `csdr_fmstereo_*` object: stereoFMDecoder quadRate decim on `nchan` independent F32 MPX streams (include/csdr.h)."""
    _block = "fmstereo"

    def __init__(self, quadRate, decim, nchan=1, max_samples=1 << 16):
        self._h = _new_handle("fmstereo", float(quadRate), int(decim), int(nchan), int(max_samples))
        self.decim, self.nchan = int(decim), int(nchan)

    @property
    def delay(self):
        return int(self._get("get_delay"))

    @property
    def taps_len(self):
        return int(self._get("get_taps_len"))

    def pll(self, chan=0):
        th, d = C.c_uint32(), C.c_uint32()
        self._call("get_pll", chan, C.byref(th), C.byref(d))
        return th.value, d.value

    def process(self, mpx):
        """[nchan][n] (or [n] for one stream) F32 -> [nchan][2 (n // decim)] (or [2 (n // decim)]) interleaved L, R."""
        x, n, y = _rows("fmstereo", mpx, np.float32, self.nchan, out_len=lambda n: 2 * (n // self.decim))
        n_out = C.c_uint32()
        self._call("process", _ptr(x), n, _ptr(y), C.byref(n_out))
        assert n_out.value == y.size, (n_out.value, y.size)
        return y

    def process_device(self, d_mpx_ptr, n, d_lr_ptr, stream=0):
        """Device-resident variant: raw device pointers (ints), enqueues on `stream`; returns the element count."""
        n_out = C.c_uint32()
        self._call("process_device", d_mpx_ptr, n, d_lr_ptr, C.byref(n_out), stream)
        return n_out.value

    def kernel_times(self):
        """us of the last call's front, pll, back, deemph, decim kernels (needs CSDR_DIAG=1 CSDR_FMS_TIME=1 at create)"""
        t = (C.c_float * 5)()
        self._call("kernel_times", t)
        return list(t)


def stereoFMDecoder(quadRate, decim, nchan=1, max_samples=1 << 16):
    """stereoFMDecoder quadRate decim (Liquid.chs:1069-1078) as a Pipe from F32 MPX arrays ([nchan][n], or [n]) to interleaved
    stereo L, R, L, R ... ([nchan][2 (n div decim)]).  The wire delay is a constant d samples (deviation)."""
    return _method_pipe(lambda: FmStereo(quadRate, decim, nchan, max_samples))


CSDR_FIRFILT_ARKAISER, CSDR_FIRFILT_RRC = 7, 9          # liquid's numbers, as Liquid.chs:225 and :160 pass them


def firdes_rnyquist(ftype, k, m, beta, dt=0.0):
    """liquid_firdes_prototype(ftype, k, m, beta, dt) for CSDR_FIRFILT_ARKAISER or CSDR_FIRFILT_RRC (`csdr_firdes_rnyquist`):
    2 k m + 1 taps as F32, evaluated in f64 and rounded once.  No GPU needed"""
    h = np.empty(2 * max(int(k), 0) * max(int(m), 0) + 1, dtype=np.float32)
    check(lib().csdr_firdes_rnyquist(int(ftype), int(k), int(m), float(beta), float(dt), _ptr(h)))
    return h


class SymSync(_Resettable):
    """The `csdr_symsync_*` object: symSyncR k m beta npfb (set_lf_bw lf_bw, set_output_rate k_out) on `nchan` independent F32
    streams (include/csdr.h), or, through `process_c`, symsync_crcf on CF32 streams.  The
    first process call after create, reset or a setter fixes the sample type."""
    _block = "symsync"

    def __init__(self, k, m=4, beta=0.0, npfb=64, nchan=1, max_samples=1 << 16, lf_bw=0.05, k_out=2):
        self._h = _new_handle("symsync", int(k), int(m), float(beta), int(npfb), float(lf_bw), int(k_out), int(nchan), int(max_samples))
        self.k, self.npfb, self.nchan = int(k), int(npfb), int(nchan)

    @property
    def taps_len(self):
        return int(self._get("get_taps_len"))

    def taps(self):
        """(mf, dmf), each [h_sub_len][npfb] as the kernel holds them"""
        L = self.taps_len
        mf, dmf = np.empty((L, self.npfb), np.float32), np.empty((L, self.npfb), np.float32)
        self._call("get_taps", _ptr(mf), _ptr(dmf))
        return mf, dmf

    def state(self, chan=0):
        """(tau, rate, del, q_hat) of stream `chan`; raises CsdrError (ERR_SIZE) when the stream is faulted"""
        v = [C.c_float() for _ in range(4)]
        self._call("get_state", chan, *[C.byref(a) for a in v])
        return tuple(np.float32(a.value) for a in v)

    def _sync(self, entry, x, dtype):
        x, n, y = _rows("symsync", x, dtype, self.nchan, plane=True)
        ny = np.zeros(self.nchan, dtype=np.uint32)
        self._call(entry, _ptr(x), n, _ptr(y), ny.ctypes.data_as(C.POINTER(C.c_uint32)))
        return y, ny

    def process_rows(self, x):
        """[nchan][n] (or [n]) F32 -> (y [nchan][n], counts [nchan]): row c holds counts[c] outputs"""
        return self._sync("process", x, np.float32)

    def process(self, x):
        """[nchan][n] -> a list of nchan arrays (their lengths vary); [n] -> one array"""
        return _split_rows(*self.process_rows(x), x)

    def process_device(self, d_x_ptr, n, d_y_ptr, d_ny_ptr, stream=0):
        """Device-resident variant: raw device pointers (ints) for x [nchan][n], y [nchan][n], counts [nchan]; enqueues on
        `stream`"""
        self._call("process_device", d_x_ptr, n, d_y_ptr, d_ny_ptr, stream)

    def set_taps(self, H):
        """symsync_create(k, npfb, H, H_len): new banks from the prototype H (2 npfb k m + 1 taps); the state as after create"""
        H = np.ascontiguousarray(H, dtype=np.float32).reshape(-1)
        self._call("set_taps", _ptr(H), H.size)

    def set_rnyquist(self, ftype, beta):
        """symsync_create_rnyquist(ftype, k, m, beta, npfb): firdes_rnyquist(ftype, k npfb, m, beta) as the prototype"""
        self._call("set_rnyquist", int(ftype), float(beta))

    def process_c(self, x):
        """[nchan][n] (or [n]) complex64 -> (y complex64 [nchan][n], counts [nchan]): row c holds counts[c] outputs"""
        return self._sync("process_c", x, np.complex64)

    def process_c_device(self, d_x_ptr, n, d_y_ptr, d_ny_ptr, stream=0):
        """Device-resident variant of process_c: raw device pointers (ints) for x, y [nchan][n] CF32 and counts [nchan];
        enqueues on `stream`"""
        self._call("process_c_device", d_x_ptr, n, d_y_ptr, d_ny_ptr, stream)


def _symsyncc(m, k, nchan, max_samples):
    s = SymSync(k, m, 0.0, 32, nchan, max_samples, lf_bw=0.01, k_out=1)
    try:
        s.set_rnyquist(CSDR_FIRFILT_ARKAISER, 0.5)
    except Exception:
        s.close()
        raise
    return s


def symSyncC(m, k, nchan=1, max_samples=1 << 16):
    """symSyncC m k (Liquid.chs:177-242: symsync_crcf_create_rnyquist(ARKAISER, k, m, 0.5, 32), lf_bw 0.01 and output rate 1
    left at symsync_create's defaults) as a Pipe from complex64 arrays ([nchan][n], or [n]) to the synchronised symbols: a
    list of per-stream arrays, or one array for [n].  It composes behind firpfbchChannelizer's rows"""
    return Pipe(lambda: _symsyncc(m, k, nchan, max_samples), lambda r, a: _split_rows(*r.process_c(a), a), lambda r: r.close())


def symSyncR(k, m=4, beta=0.0, M=64, nchan=1, max_samples=1 << 16):
    """symSyncR k m beta M (Liquid.chs:244-282: set_lf_bw 0.05, set_output_rate 2) as a Pipe from F32 arrays ([nchan][n], or
    [n]) to the synchronised samples: a list of per-stream arrays, or one array for [n]"""
    return _method_pipe(lambda: SymSync(k, m, beta, M, nchan, max_samples))


def fmDemWithSync(k, nchan=1, max_samples=1 << 16):
    """fmDemWithSync k = symSyncR k 4 0 64 . fmDemodulator (0.02 * k) (Liquid.chs:431-437), the product taken in np.float32"""
    kf = float(np.float32(0.02) * np.float32(k))
    return compose(symSyncR(k, 4, 0.0, 64, nchan, max_samples), fmDemodulator(kf, nchan, max_samples))


CSDR_PSKTRACK_EQ_DD, CSDR_PSKTRACK_EQ_CM = 0, 1       # eq_mode: decision-directed, constant modulus


def sincos_word(w):
    """(sin, cos) of the uint32 phase word `w` (2^32 = one turn) as k_psktrack computes them (`csdr_sincos_word`, DESIGN.md
    4.20), F32.  No GPU needed"""
    s, c = C.c_float(), C.c_float()
    check(lib().csdr_sincos_word(int(w) & 0xffffffff, C.byref(s), C.byref(c)))
    return np.float32(s.value), np.float32(c.value)


class PskTrack(_Owner):
    """The `csdr_psktrack_*` object: power normaliser, carrier PLL, T/2 equaliser and BPSK / QPSK decisions on `nchan` independent
    CF32 rows of their own lengths (include/csdr.h): the part of symTracker behind the symbol synchroniser."""
    _block = "psktrack"

    def __init__(self, bits, sps=1, phase=0, eq_len=0, eq_mu=0.05, eq_mode=CSDR_PSKTRACK_EQ_DD, eq_delay=200, pll_bw=9e-4,
                 agc_bw=0.02, nchan=1, max_samples=1 << 16):
        self._h = _new_handle("psktrack", int(bits), int(sps), int(phase), int(eq_len), float(eq_mu), int(eq_mode), int(eq_delay),
                              float(pll_bw), float(agc_bw), int(nchan), int(max_samples), create="new")
        self.bits, self.sps, self.eq_len, self.nchan = int(bits), int(sps), int(eq_len), int(nchan)

    def restart(self):
        """back to the state right after the constructor"""
        self._call("restart")

    def state(self, chan=0):
        """(theta, freq, p, symbols so far, weights complex64 [eq_len]) of row `chan`; theta and freq are uint32 phase words"""
        th, fr, n, p = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_float()
        w = np.zeros(self.eq_len, dtype=np.complex64)
        self._call("get_state", chan, C.byref(th), C.byref(fr), C.byref(p), C.byref(n), _ptr(w))
        return th.value, fr.value, np.float32(p.value), n.value, w

    def design(self):
        """(alpha, beta, eq_len, LDS bytes per workgroup)"""
        a, b, L, lds = C.c_float(), C.c_float(), C.c_uint32(), C.c_uint32()
        self._call("get_design", C.byref(a), C.byref(b), C.byref(L), C.byref(lds))
        return np.float32(a.value), np.float32(b.value), L.value, lds.value

    def _marshal(self, rows):
        """a list of nchan rows of their own lengths -> (x [nchan][n] zero-padded, counts [nchan]); an array -> (it, None)"""
        if not isinstance(rows, (list, tuple)):
            return rows, None
        if len(rows) != self.nchan:
            raise CsdrError(_lib.ERR_INVALID, f"psktrack: a chunk of {len(rows)} rows, not {self.nchan}")
        rows = [np.asarray(r, dtype=np.complex64).reshape(-1) for r in rows]
        nx = np.array([r.size for r in rows], dtype=np.uint32)
        x = np.zeros((self.nchan, int(nx.max())), dtype=np.complex64)
        for c, r in enumerate(rows):
            x[c, :r.size] = r
        return x, nx

    def process_rows(self, rows, symbols=False):
        """a list of nchan CF32 rows (lengths may differ), or [nchan][n] (or [n]) -> (y complex64 [nchan][n], counts [nchan]), with
        symbols=True (y, sym uint32 [nchan][n], counts): row c holds counts[c] outputs"""
        a, nx = self._marshal(rows)
        x, n, y = _rows("psktrack", a, np.complex64, self.nchan, plane=True, strict=True)
        sym = np.empty((self.nchan, n), dtype=np.uint32) if symbols else None
        ny = np.zeros(self.nchan, dtype=np.uint32)
        self._call("process", _ptr(x), n, None if nx is None else _ptr(nx), _ptr(y), None if sym is None else _ptr(sym), _ptr(ny))
        return (y, sym, ny) if symbols else (y, ny)

    def process(self, rows):
        """-> the list of nchan arrays of soft symbols d; one array for [n]"""
        y, ny = self.process_rows(rows)
        return _split_rows(y, ny, np.empty((0, 0)) if isinstance(rows, (list, tuple)) else rows)

    def process_device(self, d_x_ptr, n, d_nx_ptr, d_y_ptr, d_sym_ptr, d_ny_ptr, stream=0):
        """Device-resident variant: raw device pointers (ints) for x [nchan][n] CF32, the rows' sample counts [nchan] uint32 (0:
        every row holds n), y [nchan][n] CF32, symbols [nchan][n] uint32 (0: not wanted) and counts [nchan]; enqueues on `stream`"""
        self._call("process_device", d_x_ptr, n, d_nx_ptr or None, d_y_ptr, d_sym_ptr or None, d_ny_ptr, stream)


def pskTracker(bits, sps=1, phase=0, eq_len=0, eq_mu=0.05, eq_mode=CSDR_PSKTRACK_EQ_DD, eq_delay=200, pll_bw=9e-4, agc_bw=0.02,
               nchan=1, max_samples=1 << 16):
    """pskTracker as a Pipe from a list of nchan CF32 rows of their own lengths, as symSyncC yields them (or one
    array [nchan][n], or [n]), to the list of per-row soft symbols (or one array for [n])"""
    return _method_pipe(lambda: PskTrack(bits, sps, phase, eq_len, eq_mu, eq_mode, eq_delay, pll_bw, agc_bw, nchan, max_samples))


SYMTRACK_PHASE = 0          # the output parity of csdr_symsync at k_out = 2 that is the symbol instant


class SymTrack:
    """symTracker m k (Liquid.chs:158-175: symtrack_cccf_create(RRC, k, m, 0.25, BPSK)) as the composition of two blocks on `nchan`
    rows: SymSync(k, m, npfb 16, lf_bw, k_out 2) with the RRC 0.25 banks, then PskTrack(bits 1, sps 2, eq_len 9, constant
    modulus).  The synchroniser's rows and counts stay on the device: the second block is enqueued behind the first on one
    stream.  Deviations: no agc_crcf in front, so the input should be near unit rms, and lf_bw 0.01."""

    def __init__(self, m, k, nchan=1, max_samples=1 << 16, lf_bw=0.01, bits=1, eq_len=9, eq_mode=CSDR_PSKTRACK_EQ_CM):
        import torch
        self._torch = torch
        self.nchan, self.max_n = int(nchan), int(max_samples)
        self.sync = SymSync(k, m, 0.0, 16, nchan, max_samples, lf_bw=lf_bw, k_out=2)
        self.track = None
        try:
            self.sync.set_rnyquist(CSDR_FIRFILT_RRC, 0.25)
            self.track = PskTrack(bits, 2, SYMTRACK_PHASE, eq_len, eq_mode=eq_mode, nchan=nchan, max_samples=max_samples)
            dev = dict(device="cuda")
            self._mid = torch.empty(2 * self.nchan * self.max_n, dtype=torch.float32, **dev)
            self._y = torch.empty(2 * self.nchan * self.max_n, dtype=torch.float32, **dev)
            self._cnt = torch.empty(2 * self.nchan, dtype=torch.int32, **dev)
        except Exception:
            self.close()
            raise

    def process(self, x):
        """[nchan][n] (or [n]) complex64 -> the list of nchan arrays of soft symbols; one array for [n]"""
        torch = self._torch
        a, n, _ = _rows("symtrack", x, np.complex64, self.nchan, plane=True)
        if n > self.max_n:
            raise CsdrError(_lib.ERR_SIZE, f"symtrack: {n} samples > max {self.max_n}")
        stream = torch.cuda.current_stream().cuda_stream
        d_x = torch.from_numpy(a.view(np.float32).reshape(-1)).cuda()
        d_mid_n, d_ny = self._cnt[:self.nchan], self._cnt[self.nchan:]
        self.sync.process_c_device(d_x.data_ptr(), n, self._mid.data_ptr(), d_mid_n.data_ptr(), stream)
        self.track.process_device(self._mid.data_ptr(), n, d_mid_n.data_ptr(), self._y.data_ptr(), 0, d_ny.data_ptr(), stream)
        ny = d_ny.cpu().numpy().astype(np.uint32)
        y = self._y[:2 * self.nchan * n].cpu().numpy().view(np.complex64).reshape(self.nchan, n)
        return _split_rows(y, ny, x)

    def close(self):
        for o in (self.track, self.sync):
            if o is not None:
                o.close()


def symTracker(m, k, nchan=1, max_samples=1 << 16, lf_bw=0.01):
    """symTracker m k (Liquid.chs:173-175) as a Pipe from complex64 arrays ([nchan][n], or [n]) at k samples per symbol to the
    tracked BPSK soft symbols: a list of per-row arrays, or one array for [n]"""
    return _method_pipe(lambda: SymTrack(m, k, nchan, max_samples, lf_bw))


class FirHilb(_Resettable):
    """The `csdr_firhilb_*` object: firhilbf_create m As (firhilbCreate, Liquid.chs:520-525, fixes 5 and 60), a half-band Hilbert
    transform driven as a 2:1 real-to-complex decimator and a 1:2 complex-to-real interpolator on shared windows
    (include/csdr.h).  `max_samples` is the largest call in complex samples."""
    _block = "firhilb"

    def __init__(self, m=5, as_db=60.0, max_samples=1 << 16):
        self._h = _new_handle("firhilb", int(m), float(as_db), int(max_samples))
        self.m = int(m)

    @property
    def taps_len(self):
        return int(self._get("get_taps_len"))

    def taps(self):
        """the 2 m quadrature-branch taps hq, oldest sample first"""
        hq = np.empty(self.taps_len, np.float32)
        self._call("get_taps", _ptr(hq))
        return hq

    def decim(self, x):
        """firhilbDecim (Liquid.chs:530-534): F32 [2 n (+ 1)] -> CF32 [n]; `length div 2` drops an odd last float"""
        x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
        n = x.size // 2
        y = np.empty(n, dtype=np.complex64)
        self._call("decim", _ptr(x), n, _ptr(y))
        return y

    def interp(self, x):
        """firhilbInterp (Liquid.chs:539-543): CF32 [n] -> F32 [2 n]"""
        x = _c64(x).reshape(-1)
        y = np.empty(2 * x.size, dtype=np.float32)
        self._call("interp", _ptr(x), x.size, _ptr(y))
        return y

    def decim_device(self, d_x_ptr, n, d_y_ptr, stream=0):
        """Device-resident variant: raw device pointers (ints) for 2 n floats in, n complex out; enqueues on `stream`"""
        self._call("decim_device", d_x_ptr, n, d_y_ptr, stream)

    def interp_device(self, d_x_ptr, n, d_y_ptr, stream=0):
        """Device-resident variant: n complex in, 2 n floats out"""
        self._call("interp_device", d_x_ptr, n, d_y_ptr, stream)


def realToComplex(m=5, as_db=60.0, max_samples=1 << 16):
    """realToComplex (Liquid.chs:536-537) as a Pipe from F32 arrays to CF32 arrays of half the length"""
    return _method_pipe(lambda: FirHilb(m, as_db, max_samples), "decim")


def complexToReal(m=5, as_db=60.0, max_samples=1 << 16):
    """complexToReal (Liquid.chs:545-546) as a Pipe from CF32 arrays to F32 arrays of twice the length"""
    return _method_pipe(lambda: FirHilb(m, as_db, max_samples), "interp")


class _SymbolDem(_Owner):
    """What FskDem and GmskDem share: `nchan` CF32 rows of n samples in, n // k uint32 symbols per row out, and on request a
    second F32 output of `per` values per symbol (a NULL pointer: not wanted)"""

    def _symbols(self, x, second, per=()):
        x, n, sym = _rows(self._block, x, np.complex64, self.nchan, np.uint32, lambda n: n // self.k, plane=True)
        e = np.empty(sym.shape + per, dtype=np.float32) if second else None
        n_out = C.c_uint32()
        self._call("process", _ptr(x), n, _ptr(sym), _ptr(e) if second else None, C.byref(n_out))
        assert n_out.value == sym.size, (n_out.value, sym.size)
        return (sym, e) if second else sym

    def process(self, x):
        """[nchan][n] -> symbols [nchan][n // k]; [n] -> [n // k]"""
        sym = self.process_rows(x)
        return sym[0] if np.ndim(x) == 1 else sym

    def _device(self, d_x_ptr, n, d_sym_ptr, d_second_ptr, stream):
        self._call("process_device", d_x_ptr, n, d_sym_ptr, d_second_ptr or None, stream)


class FskDem(_SymbolDem):
    """The `csdr_fskdem_*` object: fskDemodulator m k bw (Liquid.chs:336-382) on `nchan` independent CF32 streams: M = 2^m
    tones, k samples per symbol (include/csdr.h).  A call of n samples per row yields n // k symbols per row
    and drops the last n % k samples; nothing is carried between calls."""
    _block = "fskdem"

    def __init__(self, m, k, bw, nchan=1, max_samples=1 << 16):
        self._h = _new_handle("fskdem", int(m), int(k), float(bw), int(nchan), int(max_samples))
        self.m, self.k, self.M, self.nchan = int(m), int(k), 1 << int(m), int(nchan)

    def design(self):
        """(K, demod_map): the transform size and the bin of each of the M tones"""
        K = C.c_uint32()
        dmap = np.empty(self.M, dtype=np.uint32)
        self._call("get_design", C.byref(K), _ptr(dmap))
        return K.value, dmap

    def process_rows(self, x, energy=False):
        """[nchan][n] (or [n]) CF32 -> symbols [nchan][n // k] uint32, or with energy=True (symbols, E [nchan][n // k][M])"""
        return self._symbols(x, energy, (self.M,))

    def process_device(self, d_x_ptr, n, d_sym_ptr, d_energy_ptr=0, stream=0):
        """Device-resident variant: raw device pointers (ints) for x [nchan][n] CF32, symbols [nchan][n // k] uint32 and,
        unless 0, energies [nchan][n // k][M] F32; enqueues on `stream`"""
        self._device(d_x_ptr, n, d_sym_ptr, d_energy_ptr, stream)


def fskDemodulator(m, k, bw, nchan=1, max_samples=1 << 16):
    """fskDemodulator m k bw (Liquid.chs:378-382) as a Pipe from CF32 arrays ([nchan][n], or [n]) to uint32 symbols
    ([nchan][n div k], or [n div k]); the n mod k samples left over in a chunk are dropped, as there (Liquid.chs:367-376)"""
    return _method_pipe(lambda: FskDem(m, k, bw, nchan, max_samples))


def firdes_kaiser(n, fc, as_db=60.0):
    """liquid_firdes_kaiser(n, fc, as_db, 0) (`csdr_firdes_kaiser`): n taps as F32, evaluated in f64 and rounded once.  No GPU needed"""
    h = np.empty(max(int(n), 0), dtype=np.float32)
    check(lib().csdr_firdes_kaiser(int(n), float(fc), float(as_db), 0.0, _ptr(h)))
    return h


def fir_groupdelay(h, fc):
    """firfilt_crcf_groupdelay (Liquid.chs:879) of the taps h at the normalised frequency fc (`csdr_fir_groupdelay`).  No GPU needed"""
    h = np.ascontiguousarray(h, dtype=np.float32).reshape(-1)
    gd = C.c_float()
    check(lib().csdr_fir_groupdelay(_ptr(h), h.size, float(fc), C.byref(gd)))
    return gd.value


class _RowFilter(_Resettable):
    """What FirFilt and IirSos share: `nchan` rows of CF32 (`is_complex`) or F32 samples, as many out as in"""

    def _state(self, is_complex, nchan):
        self.is_complex, self.nchan = bool(is_complex), int(nchan)
        self.dtype = np.complex64 if self.is_complex else np.float32

    def process(self, x):
        """[nchan][n] -> [nchan][n]; [n] -> [n]"""
        x, n, y = _rows(self._block, x, self.dtype, self.nchan)
        self._call("process", _ptr(x), n, _ptr(y))
        return y


def _filter_shape(is_complex, nchan, max_samples):
    return int(bool(is_complex)), int(nchan), int(max_samples)


class FirFilt(_RowFilter):
    """The `csdr_firfilt_*` object: firfilt_crcf (`is_complex`, CF32 rows) or firfilt_rrrf (F32 rows) with real taps on `nchan`
    independent rows: y[t] = scale * sum_i taps[i] x[t - i], the last len(taps) - 1 samples of a row carried from call to call
    (include/csdr.h).  `FirFilt.kaiser` is firfiltCreateCKaiser (Liquid.chs:889-895)."""
    _block = "firfilt"

    def __init__(self, taps, scale=1.0, is_complex=True, nchan=1, max_samples=1 << 16):
        t = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
        self._h = _new_handle("firfilt", _ptr(t), t.size, float(scale), *_filter_shape(is_complex, nchan, max_samples), create="create_taps")
        self._state(is_complex, nchan)

    @classmethod
    def kaiser(cls, n, fc, as_db=60.0, mu=0.0, is_complex=True, nchan=1, max_samples=1 << 16):
        """the taps of firdes_kaiser(n, fc, as_db) and the scale 2 fc"""
        return cls._adopt(_new_handle("firfilt", int(n), float(fc), float(as_db), float(mu), *_filter_shape(is_complex, nchan, max_samples),
                                      create="create_kaiser"), is_complex, nchan)

    @property
    def taps_len(self):
        return int(self._get("get_taps_len"))

    def taps(self):
        """(taps F32 [L], scale)"""
        t = np.empty(self.taps_len, np.float32)
        s = C.c_float()
        self._call("get_taps", _ptr(t), C.byref(s))
        return t, np.float32(s.value)

    def process_device(self, d_x_ptr, n, d_y_ptr, stream=0):
        """Device-resident variant: raw device pointers (ints) for x and y, [nchan][n] each; enqueues on `stream`"""
        self._call("process_device", d_x_ptr, n, d_y_ptr, stream)


def firFilterCKaiser(n, fc, as_db=60.0, mu=0.0, nchan=1, max_samples=1 << 16):
    """firFilterCKaiser n fc as mu (Liquid.chs:897-916 over firfiltCreateCKaiser, :889-895) as a Pipe of CF32 arrays
    ([nchan][n], or [n])"""
    return _method_pipe(lambda: FirFilt.kaiser(n, fc, as_db, mu, True, nchan, max_samples))


def firFilterC(taps, scale=1.0, nchan=1, max_samples=1 << 16):
    """firFilterC f (Liquid.chs:868-887): firfilt_crcf as a Pipe of CF32 arrays; the liquid object f is its taps and scale here"""
    return _method_pipe(lambda: FirFilt(taps, scale, True, nchan, max_samples))


def firFilterR(taps, scale=1.0, nchan=1, max_samples=1 << 16):
    """firFilterR f (Liquid.chs:955-957): firfilt_rrrf as a Pipe of F32 arrays; the liquid object f is its taps and scale here"""
    return _method_pipe(lambda: FirFilt(taps, scale, False, nchan, max_samples))


def _firdes_gmsk(fn, k, m, bt):
    k, m = int(k), int(m)
    h = np.empty(2 * k * m + 1 if 0 < k <= 64 and 0 < m <= 8 else 1, dtype=np.float32)
    check(fn(k, m, float(bt), _ptr(h)))
    return h


def firdes_gmsktx(k, m, bt):
    """The GMSK transmit pulse (`csdr_firdes_gmsktx`): a rectangle of one symbol through a Gaussian of bandwidth-time product
    bt, 2 k m + 1 taps as F32 that sum to one, evaluated in f64 and rounded once.  No GPU needed"""
    return _firdes_gmsk(lib().csdr_firdes_gmsktx, k, m, bt)


def firdes_gmskrx(k, m, bt):
    """This library's GMSK receive filter (`csdr_firdes_gmskrx`, not liquid_firdes_gmskrx): the 2 k m + 1 taps of least energy
    whose cascade with firdes_gmsktx(k, m, bt) is 1 at the centre and 0 at the other symbol instants of its span; exactly
    symmetric F32, evaluated in f64 and rounded once.  No GPU needed"""
    return _firdes_gmsk(lib().csdr_firdes_gmskrx, k, m, bt)


def firFilterRNyquist(k, m, beta, mu=0.0, nchan=1, max_samples=1 << 16):
    """firFilterRNyquist k m beta mu (Liquid.chs:935-953, which hard-codes LIQUID_FIRFILT_GMSKRX and the scale 1 / k) as a Pipe
    of F32 arrays: firFilterR(firdes_gmskrx(k, m, beta), 1 / k).  mu != 0 is refused, as in the other designs"""
    if float(mu) != 0.0:
        raise CsdrError(_lib.ERR_INVALID, "firFilterRNyquist: mu != 0 is not supported")
    return firFilterR(firdes_gmskrx(k, m, beta), 1.0 / int(k), nchan, max_samples)


class GmskDem(_SymbolDem, _Resettable):
    """The `csdr_gmskdem_*` object: gmskdem_create(k, m, bt) (Liquid.chs:384-429; liquid's argument order) on `nchan`
    independent CF32 streams: k samples per symbol, a receive filter of 2 k m + 1 taps (firdes_gmskrx), one bit per symbol
    (include/csdr.h).  A call takes a multiple of k samples per row and yields n // k symbols per row; the last
    2 k m + 1 samples of a row are carried from call to call."""
    _block = "gmskdem"

    def __init__(self, k, m, bt, nchan=1, max_samples=1 << 16):
        self._h = _new_handle("gmskdem", int(k), int(m), float(bt), int(nchan), int(max_samples))
        self.k, self.m, self.nchan = int(k), int(m), int(nchan)

    def design(self):
        """the receive filter's taps, F32 [2 k m + 1]"""
        return _sized(lib().csdr_gmskdem_get_design, (self.h,), (C.c_uint32(),), lambda L: np.empty(L, dtype=np.float32))

    def process_rows(self, x, soft=False):
        """[nchan][n] (or [n]) CF32 -> symbols [nchan][n // k] uint32, or with soft=True (symbols, d [nchan][n // k] F32)"""
        return self._symbols(x, soft)

    def process_device(self, d_x_ptr, n, d_sym_ptr, d_soft_ptr=0, stream=0):
        """Device-resident variant: raw device pointers (ints) for x [nchan][n] CF32, symbols [nchan][n // k] uint32 and,
        unless 0, soft values [nchan][n // k] F32; enqueues on `stream`"""
        self._device(d_x_ptr, n, d_sym_ptr, d_soft_ptr, stream)


def gmskDemodulator(m, k, bw, nchan=1, max_samples=1 << 16):
    """gmskDemodulator m k bw (Liquid.chs:428-429; the reference's argument order, which hands `k m bw` on to gmskdem_create,
    :409) as a Pipe from CF32 arrays ([nchan][n], or [n]) to uint32 bits ([nchan][n div k], or [n div k]); n not a multiple
    of k is refused, as there (:421)"""
    return _method_pipe(lambda: GmskDem(k, m, bw, nchan, max_samples))


def iirdes_butter_lowpass(n, fc):
    """Butterworth low-pass of order n (1 .. 16) at fc in (0, 0.5) as second-order sections (`csdr_iirdes_butter_lowpass`):
    (b, a), F32 [ceil(n / 2)][3] each with a0 = 1, every section of unit DC gain, evaluated in f64 and rounded once.  No GPU
    needed"""
    S = (max(int(n), 0) + 1) // 2
    b, a = np.zeros((S, 3), np.float32), np.zeros((S, 3), np.float32)
    check(lib().csdr_iirdes_butter_lowpass(int(n), float(fc), _ptr(b), _ptr(a)))
    return b, a


class IirSos(_RowFilter):
    """The `csdr_iirsos_*` object: a cascade of 1 .. 8 second-order sections with real coefficients on `nchan` independent rows
    of CF32 (`is_complex`, iirfilt_crcf: re and im filtered alike) or F32 samples, every section's state carried from call to
    call (include/csdr.h).  `IirSos(b, a)` takes the caller's sections ([S][3] each, divided by their a0);
    `IirSos.prototype` is iirfilt_*_create_prototype(BUTTER, LOWPASS, SOS, n, fc, ..) (Liquid.chs:594-608)."""
    _block = "iirsos"

    def __init__(self, b, a, is_complex=True, nchan=1, max_samples=1 << 16):
        b = np.ascontiguousarray(b, dtype=np.float32).reshape(-1)
        a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
        if b.size != a.size or b.size % 3:
            raise CsdrError(_lib.ERR_INVALID, "iirsos: b and a must be [S][3] each")
        self._h = _new_handle("iirsos", _ptr(b), _ptr(a), b.size // 3, *_filter_shape(is_complex, nchan, max_samples), create="create_sos")
        self._state(is_complex, nchan)

    @classmethod
    def prototype(cls, n, fc, f0=0.0, ap=10.0, as_db=10.0, is_complex=True, nchan=1, max_samples=1 << 16):
        """the sections of iirdes_butter_lowpass(n, fc); f0, ap and as_db are accepted and ignored"""
        return cls._adopt(_new_handle("iirsos", int(n), float(fc), float(f0), float(ap), float(as_db),
                                      *_filter_shape(is_complex, nchan, max_samples), create="create_prototype"), is_complex, nchan)

    @property
    def nsec(self):
        return int(self._get("get_nsec"))

    def sos(self):
        """(b, a): F32 [S][3] each, as the handle runs them (a0 = 1)"""
        S = self.nsec
        b, a = np.empty((S, 3), np.float32), np.empty((S, 3), np.float32)
        self._call("get_sos", _ptr(b), _ptr(a))
        return b, a

    def process_device(self, d_x_ptr, n, d_y_ptr, stream=0):
        """Device-resident variant: raw device pointers (ints) for x and y, [nchan][n] each (the same buffer or disjoint ones);
        enqueues on `stream`"""
        self._call("process_device", d_x_ptr, n, d_y_ptr, stream)


def iirCFilter(n, fc, f0=0.0, ap=10.0, as_db=10.0, nchan=1, max_samples=1 << 16):
    """iirCFilter n fc f0 ap as (Liquid.chs:600-608): order-n Butterworth low-pass (iirfilt_crcf) as a Pipe of CF32 arrays
    ([nchan][n], or [n])"""
    return _method_pipe(lambda: IirSos.prototype(n, fc, f0, ap, as_db, True, nchan, max_samples))


def iirFilterN(n, fc, f0=0.0, ap=10.0, as_db=10.0, nchan=1, max_samples=1 << 16):
    """iirCFilter's design on F32 arrays for any order 1 .. 16 (`iirFilter` itself stays the order-2 `csdr_iirfilt` object)"""
    return _method_pipe(lambda: IirSos.prototype(n, fc, f0, ap, as_db, False, nchan, max_samples))


def iirFilterSOS(b, a, complex=False, nchan=1, max_samples=1 << 16):
    """The caller's own second-order sections b, a ([S][3] each, S <= 8: a Chebyshev, elliptic or notch design brought from
    elsewhere) as a Pipe of F32 or (complex) CF32 arrays; a liquid iirfilt object is its sections here"""
    return _method_pipe(lambda: IirSos(b, a, complex, nchan, max_samples))


@dataclass
class ChainConfig:
    channels: int = 1
    dc_block: bool = True
    dc_alpha: float = 0.0005
    agc: float = 0.0            # -a; 0 = off
    demod: str = "none"         # "none" (DeNo) | "fm" (DeNBFM kf) | "am" (DeAM) | "wbfm" (DeWBFM decim)
    decim: int = 4              # DeWBFM decim
    deemph_fc: float = 0.025    # 5000 / quadRate (Liquid.chs:655)
    kf: float = 0.3
    mix: bool = False
    chan_first: int = 0
    chan_count: int = 0
    chan_stride: int = 0        # G > 1: interleaved ownership, channels chan_first + G*m (pruned DFT)
    device: int = -1
    max_frames: int = 4096
    flags: int = _lib.FLAG_QUIET
    pfb_m: int = 7
    pfb_as: float = 80.0
    tail_only: bool = False     # CSDR_FLAG_TAIL_ONLY: the per-channel tail alone on a channel-major CF32 plane [channels][nf]
    dft_backward: bool = False  # CSDR_FLAG_DFT_BACKWARD: the analyzer's transform as e^{+j} (row k = forward row (M - k) mod M); include/csdr.h


class Chain(_Resettable):
    """The fused chain object behind `csdr_chain_*`."""
    _block = "chain"

    def __init__(self, cfg: ChainConfig = None, **kw):
        cfg = cfg or ChainConfig(**kw)
        self.cfg = cfg
        c = _lib.ChainCfg()
        lib().csdr_chain_cfg_default(C.byref(c), cfg.channels)
        c.channels = cfg.channels
        c.dc_block, c.dc_alpha = int(cfg.dc_block), cfg.dc_alpha
        c.agc_threshold_db = cfg.agc
        c.demod = {"none": DEMOD_NONE, "fm": DEMOD_FM, "am": DEMOD_AM, "wbfm": DEMOD_WBFM}[cfg.demod]
        c.wbfm_decim, c.deemph_fc = cfg.decim, cfg.deemph_fc
        c.kf, c.mix = cfg.kf, int(cfg.mix)
        c.chan_first, c.chan_count = cfg.chan_first, cfg.chan_count
        c.chan_stride = cfg.chan_stride
        c.device, c.max_frames, c.flags = cfg.device, cfg.max_frames, cfg.flags | (_lib.FLAG_TAIL_ONLY if cfg.tail_only else 0) | (_lib.FLAG_DFT_BACKWARD if cfg.dft_backward else 0)
        c.pfb_m, c.pfb_as = cfg.pfb_m, cfg.pfb_as
        self._h = _new_handle("chain", C.byref(c))
        self._pending = []                              # (x, out) of the chunks between submit and collect
        self.M = cfg.channels
        self.C = cfg.channels // cfg.chan_stride if cfg.chan_stride > 1 else (cfg.chan_count or (cfg.channels - cfg.chan_first))
        self.mixed = bool(cfg.mix) and self.M > 1
        self.out_dtype = np.float32 if cfg.demod in ("fm", "am", "wbfm") else np.complex64
        self.decim = cfg.decim if cfg.demod == "wbfm" else 1

    @property
    def path(self):
        return self._get("path").decode()

    @property
    def taps(self):
        n = self.M * 2 * self.cfg.pfb_m
        t = np.zeros(n, dtype=np.float32)
        got = self._get("get_taps", _ptr(t), n)
        return t[:max(got, 0)]

    @property
    def nco(self):
        th, d = C.c_uint32(), C.c_uint32()
        self._call("get_nco", C.byref(th), C.byref(d))
        return th.value, d.value

    def out_shape(self, n_in):
        nf = n_in // self.M // self.decim
        return (nf,) if self.mixed else (self.C, nf)

    def process(self, x):
        """One compacted chunk (host arrays) -> channel-major [C][nf] (or [nf] when mixing)."""
        x = _c64(x)
        out = np.empty(self.out_shape(x.size), dtype=self.out_dtype)
        n_out = C.c_uint32()
        self._call("process", _ptr(x), x.size, _ptr(out), C.byref(n_out))
        if x.size == 0:
            return out
        assert n_out.value == out.size, (n_out.value, out.size)
        return out

    def process_device(self, d_in_ptr, n_in, d_out_ptr, stream=0):
        """Device-resident variant: raw device pointers (ints), enqueues on `stream`."""
        n_out = C.c_uint32()
        check(lib().csdr_chain_process_device(self.h, d_in_ptr, n_in, d_out_ptr, C.byref(n_out), stream))
        return n_out.value

    # ---- pipelined device entry point (csdr_chain_submit_device / csdr_chain_wait_device)
    def submit_device(self, d_in_ptr, n_in, d_out_ptr, ready_event=0):
        """Queue one HBM-resident chunk on the handle's own streams; consecutive chunks' launches may overlap (include/csdr.h).
        `d_in_ptr` must stay untouched and `d_out_ptr` unread until wait_device()."""
        n_out = C.c_uint32()
        check(lib().csdr_chain_submit_device(self.h, d_in_ptr, n_in, d_out_ptr, C.byref(n_out), ready_event))
        return n_out.value

    def independent_launches(self):
        return self._get("debug_independent_launches")

    def wait_device(self, stream=None):
        """Host (stream=None) or `stream` waits for every chunk queued with submit_device()."""
        self._call("wait_device", stream)

    # ---- asynchronous host-buffer entry point (csdr_chain_submit / csdr_chain_collect)
    def submit(self, x, out=None):
        """Queue one chunk; `x` / `out` should come from host_array() (page-locked) for full PCIe speed.  Returns `out`,
        which is valid after the matching collect()."""
        x = _c64(x)
        if out is None:
            out = np.empty(self.out_shape(x.size), dtype=self.out_dtype)
        self._call("submit", _ptr(x), x.size, _ptr(out))
        self._pending.append((x, out))                   # keep the buffers alive until collect
        return out

    def collect(self):
        """Wait for the oldest submitted chunk; returns its output array."""
        n_out = C.c_uint32()
        self._call("collect", C.byref(n_out))
        x, out = self._pending.pop(0)
        assert n_out.value == out.size or x.size == 0, (n_out.value, out.size)
        return out

    def status(self):
        """raises CsdrError if a device-side inter-workgroup wait timed out since the last check"""
        self._call("status")

    def kernel_time(self):
        ms, n = C.c_double(), C.c_uint32()
        name = self._get("kernel_time", C.byref(ms), C.byref(n))
        return name.decode(), ms.value, n.value

    def agc_stats(self):
        """(segments checked, segments recomputed) of the time-parallel AGC tail since create"""
        a, b = C.c_uint32(), C.c_uint32()
        self._call("debug_agc", C.byref(a), C.byref(b))
        return a.value, b.value

    def agc_tile_major_calls(self):
        """calls since create whose AGC tail ran on a tile-major plane (k_agc_spec_tm)"""
        return self._get("debug_agc_tile_major_calls")

    def reset(self):
        super().reset()
        self._pending = []                              # the native side abandons chunks still in flight

    def seek_frames(self, frames):
        """reset, then continue as if `frames` frames of the stream had already gone by"""
        self._call("seek_frames", int(frames))
        self._pending = []

    def close(self):
        self._pending = []
        super().close()


class host_array:
    """numpy view of page-locked host memory from csdr_host_alloc (freed with the object)."""

    def __init__(self, shape, dtype):
        self.dtype = np.dtype(dtype)
        n = int(np.prod(shape)) * self.dtype.itemsize
        self.p = lib().csdr_host_alloc(n)
        if not self.p:
            raise CsdrError(_lib.ERR_NOMEM, "csdr_host_alloc failed")
        buf = (C.c_char * n).from_address(self.p)
        buf._csdr_owner = _PinnedBlock(self.p)          # the block lives as long as any numpy view of it (views keep `buf` as their base)
        self.a = np.frombuffer(buf, dtype=self.dtype).reshape(shape)


class _PinnedBlock:
    def __init__(self, p):
        self.p = p

    def __del__(self):
        try:
            if self.p:
                lib().csdr_host_free(self.p)
                self.p = None
        except Exception:
            pass


def firpfbchChannelizer(n, **kw):
    """firpfbchChannelizer n (Liquid.chs:864-866): Pipe IO (Array CF32) [Array CF32].
    Output is the list of n per-channel arrays the reference produces by slicing one
    channel-major buffer (Liquid.chs:850-862); an empty input yields [empty]."""
    return Pipe(lambda: Chain(ChainConfig(channels=n, dc_block=False, **kw)), lambda r, a: _channel_list(r.process, a),
                lambda r: r.close())


def _firdes_bank2(fn, M, m, as_db, fc):
    M, m = int(M), int(m)
    h = np.empty(2 * M * m if 0 < M <= 256 and 0 < m <= 8 else 1, dtype=np.float32)
    check(fn(M, m, float(as_db), float(fc), _ptr(h)))
    return h


def firdes_pfbch2(M, m, as_db=80.0, fc=0.0):
    """The prototype of the 2x-oversampled channelizer (`csdr_pfbch2_design`): the first 2 M m of the 2 M m + 1 Kaiser taps of
    cutoff fc (0: the analyzer's rule 1 / M) that sum to M, evaluated in f64 and rounded once.  No GPU needed"""
    return _firdes_bank2(lib().csdr_pfbch2_design, M, m, as_db, fc)


def firdes_pfbsyn2(M, m, as_db=80.0, fc=0.0):
    """The prototype of the 2x-oversampled synthesizer (`csdr_pfbsyn2_design`): firdes_pfbch2's Kaiser design with fc = 0 meaning
    the synthesizer's rule 0.5 / M, half the analyzer's cutoff.  No GPU needed"""
    return _firdes_bank2(lib().csdr_pfbsyn2_design, M, m, as_db, fc)


class _Bank2(_Owner):
    """What the two 2x-oversampled bank objects share: M channels over a prototype of 2 M m taps, the caller's (`cls(taps, M, m)`)
    or the block's own Kaiser design (`cls.kaiser`); `taps` reads it back, `rewind` is the reset"""

    def __init__(self, taps, M, m, max_frames=1 << 16):
        self._state(M, m)
        t = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
        if t.size != 2 * self.M * self.m:
            raise CsdrError(_lib.ERR_INVALID, f"{self._block}: {t.size} taps, not 2 M m = {2 * self.M * self.m}")
        self._h = _new_handle(self._block, _ptr(t), self.M, self.m, int(max_frames), create="open_taps")

    def _state(self, M, m):
        self.M, self.m = int(M), int(m)

    @classmethod
    def kaiser(cls, M, m=7, as_db=80.0, fc=0.0, max_frames=1 << 16):
        """the taps of the block's design function: firdes_pfbch2(M, m, as_db, fc) for Firpfbch2, firdes_pfbsyn2(M, m, as_db, fc)
        for Firpfbch2Synth"""
        return cls._adopt(_new_handle(cls._block, int(M), int(m), float(as_db), float(fc), int(max_frames), create="open_kaiser"), M, m)

    def taps(self):
        t = np.empty(2 * self.M * self.m, np.float32)
        self._call("get_taps", _ptr(t))
        return t

    def rewind(self):
        """back to the state right after the object was made (firpfbch2_crcf_reset)"""
        self._call("rewind")


class Firpfbch2(_Bank2):
    """The `csdr_pfbch2_*` object: liquid's firpfbch2_crcf analyzer (which the reference does not import), M channels at twice
    the critical rate: every M / 2 input samples give one frame, rows are channel-major and centred on 2 pi k / M
    (include/csdr.h).  `Firpfbch2(taps, M, m)` takes a prototype of 2 M m taps, `Firpfbch2.kaiser` designs it."""
    _block = "pfbch2"

    def process(self, x):
        """[n] CF32, n a multiple of M / 2 -> [M][n / (M / 2)] CF32"""
        x = _c64(x).reshape(-1)
        y = np.empty((self.M, x.size // (self.M // 2)), dtype=np.complex64)
        frames = C.c_uint32()
        self._call("process", _ptr(x), x.size, _ptr(y), C.byref(frames))
        assert frames.value == y.shape[1], (frames.value, y.shape)
        return y

    def process_device(self, d_x_ptr, n, d_y_ptr, stream=0):
        """Device-resident variant: raw device pointers (ints) for x [n] and y [M][n / (M / 2)]; enqueues on `stream`"""
        self._call("process_device", d_x_ptr, n, d_y_ptr, stream)


def firpfbch2Channelizer(M, m=7, as_db=80.0, fc=0.0, max_frames=1 << 16):
    """The 2x-oversampled counterpart of firpfbchChannelizer: Pipe IO (Array CF32) [Array CF32], the list of M per-channel
    arrays, each at 2 / M of the input rate; an empty input yields [empty], as there"""
    return Pipe(lambda: Firpfbch2.kaiser(M, m, as_db, fc, max_frames), lambda r, a: _channel_list(r.process, a), lambda r: r.close())


class Firpfbch2Synth(_Bank2):
    """The `csdr_pfbsyn2_*` object: the synthesizer side of liquid's firpfbch2_crcf, the way back from Firpfbch2's rows to one
    stream: every frame of M values gives M / 2 samples, and Firpfbch2.kaiser followed by Firpfbch2Synth.kaiser returns its
    input `delay()` samples late (include/csdr.h).  `Firpfbch2Synth(taps, M, m)` takes a prototype of 2 M m taps,
    `Firpfbch2Synth.kaiser` designs it."""
    _block = "pfbsyn2"

    def delay(self):
        """samples by which the analyzer followed by this synthesizer delays a stream: 2 M m - M / 2 + 1"""
        return int(self._get("delay"))

    def process(self, y):
        """[M][frames] CF32 -> [frames M / 2] CF32"""
        y = _c64(y)
        if y.ndim != 2 or y.shape[0] != self.M:
            raise CsdrError(_lib.ERR_INVALID, f"pfbsyn2: a chunk of shape {y.shape}, not [{self.M}][frames]")
        x = np.empty(y.shape[1] * (self.M // 2), dtype=np.complex64)
        n = C.c_uint32()
        self._call("process", _ptr(y), y.shape[1], _ptr(x), C.byref(n))
        assert n.value == x.size, (n.value, x.shape)
        return x

    def process_device(self, d_y_ptr, frames, d_x_ptr, stream=0):
        """Device-resident variant: raw device pointers (ints) for y [M][frames] and x [frames M / 2]; enqueues on `stream`"""
        self._call("process_device", d_y_ptr, frames, d_x_ptr, stream)


def firpfbch2Synthesizer(M, m=7, as_db=80.0, fc=0.0, max_frames=1 << 16):
    """The way back from firpfbch2Channelizer: Pipe IO [Array CF32] (Array CF32), from the M per-channel arrays of a chunk (a list
    or an [M][frames] array) to frames M / 2 samples; [empty], which the channelizer yields for an empty input, gives empty"""
    def process(r, rows):
        if sum(np.asarray(a).size for a in rows) == 0:
            return np.empty(0, dtype=np.complex64)
        return r.process(np.stack([_c64(a).reshape(-1) for a in rows]))
    return Pipe(lambda: Firpfbch2Synth.kaiser(M, m, as_db, fc, max_frames), process, lambda r: r.close())


def _rowresamp_design(fn, args, delay=()):
    """(bank F32 [257][P], delta) through the entry point fn(*args, &P, &delta, *delay, bank)"""
    P, delta = C.c_uint32(), C.c_uint64()
    bank = _sized(fn, args, (P, delta, *delay), lambda P, delta: np.empty((257, P), dtype=np.float32))
    return bank, int(delta.value)


def firdes_rowresamp(rate, m=7, as_db=60.0, fc=0.0):
    """The design of the row resampler (`csdr_rowresamp_design`, "csdr rowresamp v1"): (bank F32 [257][P], delta),
    delta = llround(2^32 / rate) Q32.32 input samples per output and P = 2 m D taps per phase.  No GPU needed"""
    return _rowresamp_design(lib().csdr_rowresamp_design, (float(rate), int(m), float(as_db), float(fc)))


class RowResamp(_Owner):
    """The `csdr_rowresamp_*` object: liquid's resamp_crcf (`complex`, CF32 rows) or resamp_rrrf (F32 rows) on `nchan` independent
    rows that share one rate and one clock: [nchan][n] in, [nchan][n_out] out, n_out the same for every row and known before the
    call (`count`).  The last P - 1 samples of a row and the time of the next output are carried from call to call, and the
    output does not depend on how the stream is cut into calls (include/csdr.h)."""
    _block = "rowresamp"

    def __init__(self, rate, m=7, as_db=60.0, fc=0.0, complex=True, nchan=1, max_samples=1 << 16):
        self._h = _new_handle("rowresamp", float(rate), int(m), float(as_db), float(fc), int(bool(complex)), int(nchan), int(max_samples),
                              create="open")
        self.is_complex, self.nchan = bool(complex), int(nchan)
        self.dtype = np.complex64 if self.is_complex else np.float32

    def design(self):
        """(bank F32 [257][P], delta)"""
        return _rowresamp_design(lib().csdr_rowresamp_get_design, (self.h,), delay=(None,))

    def delay(self):
        """the group delay in input samples: m D"""
        d = C.c_uint32()
        self._call("get_design", None, None, C.byref(d), None)
        return int(d.value)

    def time(self):
        """T: the Q32.32 time of the next output relative to the first sample of the next call"""
        t = C.c_uint64()
        self._call("get_time", C.byref(t))
        return int(t.value)

    def count(self, n):
        """outputs per row that the next call of n samples per row yields"""
        n_out = C.c_uint32()
        self._call("count", int(n), C.byref(n_out))
        return int(n_out.value)

    def max_out(self, n):
        """room per row that a call of n samples may need, whatever the time it starts at"""
        return int(self._get("max_out", int(n)))

    def rewind(self):
        """back to the state right after the object was made (resamp_crcf_reset)"""
        self._call("rewind")

    def process(self, x):
        """[nchan][n] -> [nchan][n_out]; [n] -> [n_out]"""
        x, n, y = _rows("rowresamp", x, self.dtype, self.nchan, out_len=self.count, plane=True, strict=True)
        n_out = C.c_uint32()
        self._call("process", _ptr(x), n, _ptr(y), C.byref(n_out))
        assert n_out.value == y.shape[1], (n_out.value, y.shape)
        return y[0] if x.ndim == 1 else y

    def process_device(self, d_x_ptr, n, d_y_ptr, stream=0):
        """Device-resident variant: raw device pointers (ints) for x [nchan][n] and y [nchan][n_out]; enqueues on `stream` and
        returns n_out without synchronising"""
        n_out = C.c_uint32()
        self._call("process_device", d_x_ptr, int(n), d_y_ptr, C.byref(n_out), stream)
        return int(n_out.value)


def rowResampler(rate, m=7, as_db=60.0, fc=0.0, complex=True, nchan=1, max_samples=1 << 16):
    """The arbitrary-rate resampler on rows as a Pipe of [nchan][n] arrays (CF32, or F32 with complex=False; [n] for one row):
    what turns the channelizers' fs / M into the whole number of samples per symbol that fskDemodulator, gmskDemodulator and the
    symbol synchronisers take, or into an audio rate"""
    return _method_pipe(lambda: RowResamp(rate, m, as_db, fc, complex, nchan, max_samples))
