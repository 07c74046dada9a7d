"""numpy restatement of liquid-dsp 1.3.2's fskdem (fskDemodulator m k bw, Liquid.chs:336-382) as recalled:
unpinned.  No GPU, no oracle.

  design(m, k, bw)         fskdem_create's K and demod_map, in f32 as liquid computes them
  table(K)                 W[t] = e^{-2 pi i t / K}: f64, rounded once to f32 (what csdr_fskdem_create builds)
  demod_ref(x, m, k, bw)   the algorithm as liquid states it, in f64: a zero-padded K-point FFT, |X[demod_map[s]]|, first maximum
  demod_f32(x, m, k, bw)   k_fskdem's arithmetic, operation for operation: the f32 table indexed by (b j) mod K, four multiplies,
                           one subtraction and one addition per product, each sum from +0 over j = 0 .. k - 1, sqrt in f32,
                           `s == 0 or v > vmax`
  fskmod(sym, m, k, bw)    liquid's fskmod for test signals: one NCO whose phase runs on across symbols

x is [n] or [rows][n]; n // k symbols per row, the n % k samples at the end of a row are dropped (Liquid.chs:367-376)."""
import math

import numpy as np

f32 = np.float32


def roundf(v):
    """C roundf of one f32: half away from zero (evaluated in f64, where |v| + 0.5 is exact)"""
    v = float(v)
    return f32(math.copysign(math.floor(abs(v) + 0.5), v))


def design(m, k, bw):
    """(K, demod_map [M] uint32)"""
    M = 1 << m
    bw = f32(bw)
    M2 = f32(0.5) * f32(M - 1)
    df = bw / M2
    K_min, K_max = k, max(16, 4 * k)
    K, err_min = K_min, f32(0)
    for K_hat in range(K_min, K_max + 1):
        v = f32(0.5) * df * f32(K_hat)
        err = abs(roundf(v) - v)
        if K_hat == K_min or err < err_min:
            K, err_min = K_hat, err
        if err < f32(1e-6):
            break
    dmap = np.zeros(M, np.uint32)
    for i in range(M):
        freq = (f32(i) - M2) * bw / M2
        idx = freq * f32(K)
        dmap[i] = int(roundf(idx + f32(K) if idx < 0 else idx)) % K      # % K: a wrapped index that rounds to K is bin 0
    return K, dmap


def table(K):
    a = 2.0 * np.pi * np.arange(K, dtype=np.float64) / float(K)
    return np.cos(a).astype(f32), (-np.sin(a)).astype(f32)


def _symbols(x, k):
    x = np.asarray(x, np.complex64)
    rows = x.reshape(1, -1) if x.ndim == 1 else x
    ns = rows.shape[1] // k
    return rows[:, :ns * k].reshape(rows.shape[0] * ns, k), (rows.shape[0], ns), x.ndim == 1


def _shape(sym, E, shp, one):
    sym, E = sym.reshape(shp), E.reshape(shp + (E.shape[-1],))
    return (sym[0], E[0]) if one else (sym, E)


def demod_ref(x, m, k, bw):
    """(symbols, magnitudes [..][M]) in f64"""
    K, dmap = design(m, k, bw)
    xs, shp, one = _symbols(x, k)
    X = np.fft.fft(xs.astype(np.complex128), n=K, axis=1)
    E = np.abs(X[:, dmap.astype(np.int64)])
    return _shape(np.argmax(E, axis=1).astype(np.uint32), E, shp, one)


def demod_f32(x, m, k, bw):
    """(symbols uint32, magnitudes [..][M] f32), bit for bit what k_fskdem writes"""
    K, dmap = design(m, k, bw)
    wr, wi = table(K)
    xs, shp, one = _symbols(x, k)
    xr, xi = np.ascontiguousarray(xs.real.T), np.ascontiguousarray(xs.imag.T)        # [k][symbols]
    N, M = xs.shape[0], 1 << m
    E = np.empty((N, M), f32)
    for s in range(M):
        b, t = int(dmap[s]), 0
        ar, ai = np.zeros(N, f32), np.zeros(N, f32)
        for j in range(k):
            pr = xr[j] * wr[t] - xi[j] * wi[t]
            pi = xr[j] * wi[t] + xi[j] * wr[t]
            ar = ar + pr
            ai = ai + pi
            t += b
            if t >= K:
                t -= K
        E[:, s] = np.sqrt(ar * ar + ai * ai)
    sym, vmax = np.zeros(N, np.uint32), E[:, 0].copy()
    for s in range(1, M):                                                           # s == 0 || v > vmax
        up = E[:, s] > vmax
        sym[up] = s
        vmax[up] = E[up, s]
    return _shape(sym, E, shp, one)


def bound(x, k):
    """(k + 8) 2^-24 sum_j |x_j| per symbol: k rounded products with a rounded table entry and k accumulations"""
    xs, shp, one = _symbols(x, k)
    B = (k + 8) * 2.0 ** -24 * np.abs(xs.astype(np.complex128)).sum(axis=1)
    return B.reshape(shp)[0] if one else B.reshape(shp)


def fskmod(sym, m, k, bw):
    """fskmod_modulate: k samples of e^{j theta} per symbol, theta stepping by (s - M2) 2 pi bw / M2 and never reset"""
    M2 = 0.5 * ((1 << m) - 1)
    dphi = (np.asarray(sym, np.float64) - M2) * 2.0 * np.pi * bw / M2
    steps = np.repeat(dphi, k)
    theta = np.concatenate([[0.0], np.cumsum(steps)[:-1]])
    return np.exp(1j * theta).astype(np.complex64)


def awgn(n, snr_db, rng):
    """complex white noise of power 10^(-snr_db / 10) (against a unit-power signal)"""
    s = 10.0 ** (-snr_db / 20.0) / np.sqrt(2.0)
    return (s * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
