"""numpy restatement of the FIR filter of DESIGN.md 4.13 (csdr_firfilt_*: firFilterC / firFilterR / firFilterCKaiser,
Liquid.chs:868-916, 955-957).  No GPU, no oracle.

  filter_f32(taps, scale, x, hist)   k_firfilt's arithmetic, operation for operation: per output acc = +0, then for
                                     i = 0 .. L - 1 in that order acc = acc + taps[i] * x[t - i] (the product rounded to f32,
                                     then the sum), y = scale * acc; complex samples: the same on re and im separately
  filter_f64(taps, scale, x, hist)   the same sum in f64 (the f32 taps, scale and samples taken as they are)
  bound(taps, scale, x, hist)        (L + 2) 2^-24 |scale| sum_i |taps[i]| |x[t - i]| per output: L rounded products summed in
                                     order plus the scale's rounding (valid for L <= 2048); for complex samples per component
  response(taps, scale, f)           H(f) = scale sum_i taps[i] e^{-2 pi j f i} in f64

x is [n] or [rows][n], F32 or CF32; hist is None (zeros: the state after create / reset) or the L - 1 samples in front of x
([L - 1] or [rows][L - 1]).  The two filters return (y, new_hist): new_hist is the last L - 1 samples of (hist | x), what the
next call has to be given."""
import numpy as np

f32 = np.float32


def _rows(x, dtype=None):
    x = np.asarray(x)
    if dtype is None:
        dtype = np.complex64 if np.iscomplexobj(x) else np.float32
    x = x.astype(dtype, copy=False)
    return (x.reshape(1, -1) if x.ndim == 1 else x), x.ndim == 1


def _extended(taps, x, hist):
    taps = np.asarray(taps, f32).reshape(-1)
    rows, one = _rows(x)
    H = taps.size - 1
    if hist is None:
        hist = np.zeros((rows.shape[0], H), rows.dtype)
    hist = _rows(hist, rows.dtype)[0]
    assert hist.shape == (rows.shape[0], H), (hist.shape, rows.shape, H)
    return taps, np.concatenate([hist, rows], axis=1), rows.shape[1], one


def _planes(ext):
    """the component planes of [rows][H + n] samples: (re, im) or (x,)"""
    if np.iscomplexobj(ext):
        return [np.ascontiguousarray(ext.real), np.ascontiguousarray(ext.imag)]
    return [ext]


def _complex_of(re, im, dtype):
    y = np.empty(re.shape, dtype)
    y.real, y.imag = re, im
    return y


def filter_f32(taps, scale, x, hist=None):
    taps, ext, n, one = _extended(taps, x, hist)
    L, H = taps.size, taps.size - 1
    s = f32(scale)
    out = []
    for p in _planes(ext):
        acc = np.zeros((p.shape[0], n), f32)
        for i in range(L):
            prod = taps[i] * p[:, H - i:H - i + n]                 # f32 * f32 -> f32: rounded once
            acc = acc + prod                                       # rounded once
        out.append(s * acc)
    y = _complex_of(out[0], out[1], np.complex64) if len(out) == 2 else out[0]
    new_hist = ext[:, ext.shape[1] - H:]
    return (y[0], new_hist[0]) if one else (y, new_hist)


def filter_f64(taps, scale, x, hist=None):
    taps, ext, n, one = _extended(taps, x, hist)
    L, H = taps.size, taps.size - 1
    out = []
    for p in _planes(ext):
        p = p.astype(np.float64)
        acc = np.zeros((p.shape[0], n), np.float64)
        for i in range(L):
            acc = acc + float(taps[i]) * p[:, H - i:H - i + n]
        out.append(float(f32(scale)) * acc)
    y = _complex_of(out[0], out[1], np.complex128) if len(out) == 2 else out[0]
    new_hist = ext[:, ext.shape[1] - H:]
    return (y[0], new_hist[0]) if one else (y, new_hist)


def bound(taps, scale, x, hist=None):
    """per output (per component for complex samples: a list of one or two arrays)"""
    taps, ext, n, one = _extended(taps, x, hist)
    L, H = taps.size, taps.size - 1
    out = []
    for p in _planes(ext):
        p = np.abs(p.astype(np.float64))
        acc = np.zeros((p.shape[0], n), np.float64)
        for i in range(L):
            acc = acc + abs(float(taps[i])) * p[:, H - i:H - i + n]
        b = (L + 2) * 2.0 ** -24 * abs(float(f32(scale))) * acc
        out.append(b[0] if one else b)
    return out


def components(y):
    """the component arrays of a filter output, in the order bound() lists them"""
    y = np.asarray(y)
    return [y.real, y.imag] if np.iscomplexobj(y) else [y]


def response(taps, scale, f):
    taps = np.asarray(taps, np.float64).reshape(-1)
    return float(f32(scale)) * np.sum(taps * np.exp(-2j * np.pi * float(f) * np.arange(taps.size)))
