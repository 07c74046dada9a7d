"""numpy restatement of the 2x-oversampled channelizer of DESIGN.md 4.17 (csdr_pfbch2_*: liquid's firpfbch2_crcf analyzer as
recalled, which the reference does not import).  No GPU, no product code.

M channels (a power of two), semi-length m, a real prototype h[0 .. L - 1] with L = 2 m M; P = M / 2 input samples per frame;
frame t (counted from the start of the stream) has the newest sample n_t = (t + 1) P - 1; x[s < 0] = 0.

  truth(h, x, M)                 (i)   the closed form in f64, a matrix product per block of frames:
                                       y_k[t] = (1 / M) sum_{i < L} h[i] x[n_t - i] e^{+2 pi j k (i + t P) / M}
                                       (no window, no parity, no transform: the phasors are looked up by k (i + t P) mod M)
  structural(h, x, M, m, prec)   (ii)  prec = 64: liquid's structure in f64.  M windows of 2 m samples; sample s is pushed into
                                       window (M - 1 - s) mod M, so a frame's P pushes go to the upper half on even frames and
                                       to the lower half on odd ones; branch i takes the dot product of h_sub_i[n] = h[i + n M]
                                       with window i (odd frames) or window (i + P) mod M (even frames); the DFT input is
                                       rotated by P on odd frames; a backward DFT scaled by 1 / M (np.fft.ifft)
                                 (iii) prec = 32: the same with the kernel's accumulation, acc = fma(h, x, acc) from +0 with
                                       the oldest sample first (the fma as an f64 product and sum rounded to f32: the product is
                                       exact, the double rounding differs from fmaf in rare last bits) and a complex64 ifft.
                                       This is the yardstick for the GPU kernel's error, not its bit pattern
  design(M, m, as_db, fc)        (iv)  the prototype in f64: 2 M m + 1 taps sinc(2 fc t) w_kaiser(t), fc = 1 / M when 0 is
                                       given, scaled to sum M (liquid's sincf cosine product below 0.01)
All of them return [M][frames] (design: [2 M m + 1])."""
import numpy as np

f32 = np.float32


def _frames(x, M):
    x = np.asarray(x).reshape(-1)
    P = M // 2
    assert x.size % P == 0, (x.size, P)
    return x, P, x.size // P


def truth(h, x, M, block=512):
    h = np.asarray(h, np.float64).reshape(-1)
    x, P, T = _frames(x, M)
    L = h.size
    xp = np.concatenate([np.zeros(L - P, np.complex128), x.astype(np.complex128)])
    # xp[t P + j] is x[n_t - i] with i = L - 1 - j.  The phasor has the period M in i and L is a multiple of M, so the terms of
    # equal j mod M are added first and the sum over i becomes an M x M matrix product: the same sum, 2 m times cheaper
    b = np.arange(M)
    k = np.arange(M)
    E = np.exp(2j * np.pi * ((k[:, None] * ((L - 1 - b) % M)[None, :]) % M) / M)
    hr = h[::-1]
    y = np.empty((M, T), np.complex128)
    win = np.lib.stride_tricks.sliding_window_view(xp, L)[::P] if T else None
    for t0 in range(0, T, block):
        t = np.arange(t0, min(t0 + block, T))
        g = (win[t0:t0 + t.size] * hr[None, :]).reshape(t.size, L // M, M).sum(axis=1)
        rot = np.exp(2j * np.pi * ((k[:, None] * ((t * P) % M)[None, :]) % M) / M)
        y[:, t0:t0 + t.size] = rot * (E @ g.T) / M
    return y


def structural(h, x, M, m, prec=64):
    assert prec in (32, 64)
    real, cplx = (np.float64, np.complex128) if prec == 64 else (np.float32, np.complex64)
    h = np.asarray(h).reshape(-1).astype(real)
    x, P, T = _frames(x, M)
    assert h.size == 2 * m * M
    H = 2 * m * M
    xp = np.concatenate([np.zeros(H, cplx), x.astype(cplx)])     # xp[H + s] = x[s]
    t = np.arange(T)
    n_t = (t + 1) * P - 1
    i = np.arange(M)
    u = np.empty((T, M), cplx)
    for par in (0, 1):
        tt = t[par::2]
        if not tt.size:
            continue
        c = (i + (P if par == 0 else 0)) % M                                  # the window branch i reads
        newest = n_t[tt][:, None] - ((n_t[tt][:, None] - (M - 1 - c)[None, :]) % M)   # the last sample pushed into it
        acc_re = np.zeros((tt.size, M), real)
        acc_im = np.zeros((tt.size, M), real)
        for n in range(2 * m - 1, -1, -1):                                    # oldest sample first
            s = xp[H + newest - n * M]
            hn = h[i + n * M][None, :]
            if prec == 64:
                acc_re = acc_re + hn * s.real
                acc_im = acc_im + hn * s.imag
            else:
                acc_re = (hn.astype(np.float64) * s.real.astype(np.float64) + acc_re.astype(np.float64)).astype(f32)
                acc_im = (hn.astype(np.float64) * s.imag.astype(np.float64) + acc_im.astype(np.float64)).astype(f32)
        v = np.empty((tt.size, M), cplx)
        v.real, v.imag = acc_re, acc_im
        u[par::2] = np.roll(v, P, axis=1) if par else v                       # u[(i + P) mod M] = v[i] on odd frames
    y = np.fft.ifft(u, axis=1)               # numpy >= 2 transforms complex64 in f32; an older numpy would do it in f64,
    return np.ascontiguousarray(y.astype(cplx).T)   # a finer yardstick and so a tighter bound, never a looser one


def yardstick(h, x, M, m):
    return structural(h, x, M, m, prec=32)


def _bessel_i0(z):
    z = np.asarray(z, np.float64)
    q, term, total = 0.25 * z * z, np.ones_like(z), np.ones_like(z)
    for k in range(1, 200):
        term = term * q / (k * k)
        total = total + term
    return total


def kaiser_beta(as_db):
    as_db = abs(float(as_db))
    if as_db > 50.0:
        return 0.1102 * (as_db - 8.7)
    if as_db > 21.0:
        return 0.5842 * (as_db - 21.0) ** 0.4 + 0.07886 * (as_db - 21.0)
    return 0.0


def design(M, m, as_db, fc=0.0):
    N = 2 * M * m + 1
    fc = 1.0 / M if fc == 0 else float(fc)
    t = np.arange(N, dtype=np.float64) - 0.5 * (N - 1)
    z = 2.0 * fc * t
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(np.abs(z) < 0.01, np.cos(np.pi * z / 2) * np.cos(np.pi * z / 4) * np.cos(np.pi * z / 8),
                        np.sin(np.pi * z) / (np.pi * z))
    r = 2.0 * t / (N - 1)
    beta = kaiser_beta(as_db)
    w = _bessel_i0(beta * np.sqrt(np.maximum(1.0 - r * r, 0.0))) / _bessel_i0(beta)
    hd = sinc * w
    return hd * (M / hd.sum())


def relrms(y, ref):
    """per channel: rms(y - ref) / rms(ref)"""
    d = np.asarray(y, np.complex128) - ref
    return np.sqrt((np.abs(d) ** 2).mean(axis=1) / (np.abs(ref) ** 2).mean(axis=1))


U = 2.0 ** -24


def ratios(got, ref, yard, M):
    """The per-channel / per-element rule of DESIGN.md 4.6 with d = log2 M (one rounding per radix-2 stage on every path):
      (a) every channel:  relrms_c(got) <= 2 max_c relrms_c(yardstick) + d U
      (b) every element:  |got - truth| <= 4 max |yardstick - truth| + 6 d U rms(truth)
    Returns (worst (a) ratio, worst (b) ratio, the yardstick's share of bound (a), of bound (b))"""
    d = float(np.log2(M))
    ya = 2.0 * float(relrms(yard, ref).max())
    yb = 4.0 * float(np.abs(np.asarray(yard, np.complex128) - ref).max())
    bound_a = ya + d * U
    bound_b = yb + 6.0 * d * U * float(np.sqrt(np.mean(np.abs(ref) ** 2)))
    return (float(relrms(got, ref).max()) / bound_a, float(np.abs(np.asarray(got, np.complex128) - ref).max()) / bound_b,
            ya / bound_a, yb / bound_b)


def stream(M, frames, seed):
    """the test input: complex white noise of unit variance and a tone of amplitude 0.25, 0.45 / M above channel 1's centre (in
    the transition band between channels 1 and 2), as CF32"""
    rng = np.random.default_rng(seed)
    n = frames * (M // 2)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)
    x = x + 0.25 * np.exp(2j * np.pi * (1.45 / M) * np.arange(n))
    return x.astype(np.complex64)
