"""The order-n IIR filter (csdr_iirsos_*) restated in numpy: the Butterworth low-pass design in f64 and the
sequential f32 cascade the kernel is compared with.

Design (plain mathematics, nothing recalled): analog prototype poles exp(+-j theta_i), theta_i = (2 (i + 1) + n - 1) pi / (2 n)
for i < floor(n / 2), and -1 for odd n; bilinear transform with pre-warping m = tan(pi fc): p_d = (1 + m p) / (1 - m p); all
zeros at -1.  One section per conjugate pair in the order i = 0, 1, .. (highest Q first), A = [1, -2 Re p_d, |p_d|^2],
B = g [1, 2, 1]; for odd n a first-order section last, A = [1, -p_d, 0], B = g [1, 1, 0]; g gives every section unit DC gain:
(1 + a1 + a2) / 4 = |1 - p_d|^2 / 4 = m^2 / |1 - m p|^2 for a pair and (1 - p_d) / 2 = m / (1 + m) for the real pole."""
import numpy as np

f32 = np.float32


def butter_lowpass_sos64(n, fc):
    """(b, a) in f64, [ceil(n / 2)][3] each"""
    n = int(n)
    m = np.tan(np.pi * float(fc))
    b, a = [], []
    for i in range(n // 2):
        theta = (2 * (i + 1) + n - 1) * np.pi / (2 * n)
        p = complex(np.cos(theta), np.sin(theta))
        den = abs(1.0 - m * p) ** 2
        pd = (1.0 + m * p) * np.conj(1.0 - m * p) / den
        g = m * m / den
        a.append([1.0, -2.0 * pd.real, abs(1.0 + m * p) ** 2 / den])
        b.append([g, 2.0 * g, g])
    if n & 1:
        pd, g = (1.0 - m) / (1.0 + m), m / (1.0 + m)
        a.append([1.0, -pd, 0.0])
        b.append([g, g, 0.0])
    return np.array(b, np.float64), np.array(a, np.float64)


def butter_lowpass_sos(n, fc):
    """the same rounded once to F32, as csdr_iirdes_butter_lowpass returns it"""
    b, a = butter_lowpass_sos64(n, fc)
    return b.astype(f32), a.astype(f32)


def response(b, a, w):
    """H(e^{jw}) of the cascade b, a ([S][3]) at the angular frequencies w, in f64"""
    z = np.exp(-1j * np.asarray(w, np.float64))
    b, a = np.asarray(b, np.float64), np.asarray(a, np.float64)
    H = np.ones(z.shape, np.complex128)
    for bs, as_ in zip(b, a):
        H *= (bs[0] + bs[1] * z + bs[2] * z * z) / (as_[0] + as_[1] * z + as_[2] * z * z)
    return H


def butter_magnitude(n, fc, w):
    """|H| of the order-n Butterworth low-pass through the bilinear transform: 1 / sqrt(1 + (tan(w / 2) / tan(pi fc))^(2 n))"""
    return 1.0 / np.sqrt(1.0 + (np.tan(np.asarray(w, np.float64) / 2.0) / np.tan(np.pi * float(fc))) ** (2 * int(n)))


def rounding_bound(b64, a64, w):
    """First-order bound on |H32(w) - H(w)| when every coefficient of the f64 design b64, a64 is rounded once to f32: a
    coefficient moves by at most half an ulp of its f32 value, so section s = B_s / A_s moves by at most
    (dB_s + |H_s| dA_s) / |A_s| with dB_s, dA_s the sums of those half ulps (|z^-k| = 1), and the cascade by
        |H(w)| sum_s (dB_s / |B_s(w)| + dA_s / |A_s(w)|).
    For a narrow low-pass A_s(1) = 1 + a1 + a2 is of the order (2 pi fc)^2 while a1 is near -2: that is where the room goes"""
    z = np.exp(-1j * np.asarray(w, np.float64))
    half_ulp = lambda c: 0.5 * np.spacing(np.abs(np.asarray(c, np.float64).astype(f32))).astype(np.float64)
    H = np.abs(response(b64, a64, w))
    rel = np.zeros(z.shape)
    for bs, as_ in zip(np.asarray(b64, np.float64), np.asarray(a64, np.float64)):
        dB, dA = half_ulp(bs).sum(), half_ulp(as_[1:]).sum()
        B, A = np.abs(bs[0] + bs[1] * z + bs[2] * z * z), np.abs(as_[0] + as_[1] * z + as_[2] * z * z)
        rel += dB / B + dA / A
    return H * rel


def filter_f32(b, a, x, state=None):
    """The sequential f32 cascade, direct form II, no contraction: per section and sample
        v0 = (x - a1 v1) - a2 v2;  y = (b0 v0 + b1 v1) + b2 v2;  (v1, v2) <- (v0, v1)
    on the rows of x ([C][n] or [n], F32 or CF32: re and im alike).  state [S][2][C] (+ re/im), zeros when None.
    Returns (y, state)"""
    b, a = np.asarray(b, f32).reshape(-1, 3), np.asarray(a, f32).reshape(-1, 3)
    x = np.asarray(x)
    cplx = np.iscomplexobj(x)
    xr = np.ascontiguousarray(x, np.complex64 if cplx else f32)
    rows = xr.reshape(int(np.prod(xr.shape[:-1])), xr.shape[-1])          # [n] is one row
    # components as independent real rows
    comp = np.concatenate([rows.real, rows.imag]) if cplx else rows
    comp = np.ascontiguousarray(comp, f32)
    S, R, n = b.shape[0], comp.shape[0], comp.shape[1]
    st = np.zeros((S, 2, R), f32) if state is None else np.array(state, f32, copy=True)
    cur = comp
    for s in range(S):
        b0, b1, b2, a1, a2 = b[s, 0], b[s, 1], b[s, 2], a[s, 1], a[s, 2]
        v1, v2 = st[s, 0].copy(), st[s, 1].copy()
        out = np.empty_like(cur)
        for t in range(n):
            v0 = (cur[:, t] - a1 * v1) - a2 * v2
            out[:, t] = (b0 * v0 + b1 * v1) + b2 * v2
            v2, v1 = v1, v0
        st[s, 0], st[s, 1] = v1, v2
        cur = out
    if cplx:
        y = (cur[:R // 2] + 1j * cur[R // 2:]).astype(np.complex64)
    else:
        y = cur
    return y.reshape(xr.shape), st


def filter_f64(b, a, x):
    """truth: the same f32 coefficients run in f64 by scipy.signal.lfilter, section by section, from zero state"""
    from scipy.signal import lfilter
    b, a = np.asarray(b, f32).reshape(-1, 3).astype(np.float64), np.asarray(a, f32).reshape(-1, 3).astype(np.float64)
    y = np.asarray(x).astype(np.complex128 if np.iscomplexobj(x) else np.float64)
    for bs, as_ in zip(b, a):
        y = lfilter(bs, as_, y, axis=-1)
    return y
