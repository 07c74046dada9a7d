"""numpy restatement (f64) of the GMSK designs and demodulator of DESIGN.md 4.15 (csdr_firdes_gmsktx / csdr_firdes_gmskrx /
csdr_gmskdem_*), and a GMSK synthesiser of its own.  Nothing here calls the library."""
import math

import numpy as np


def firdes_gmsktx(k, m, bt):
    """the Gaussian-filtered rectangular frequency pulse, 2 k m + 1 taps that sum to one (f64)"""
    c = 2.0 * math.pi * bt / math.sqrt(math.log(2.0))
    q = lambda x: 0.5 * math.erfc(x / math.sqrt(2.0))                     # noqa: E731
    g = np.array([q(c * (i / k - m - 0.5)) - q(c * (i / k - m + 0.5)) for i in range(2 * k * m + 1)])
    return g / g.sum()


def _constraints(g, k, m):
    L = g.size
    A = np.zeros((2 * m + 1, L))
    for j in range(-m, m + 1):
        for i in range(L):
            idx = L - 1 + j * k - i
            if 0 <= idx < L:
                A[j + m, i] = g[idx]
    return A


def firdes_gmskrx(k, m, bt):
    """the r of least sum r^2 with (g * r)[L - 1] = 1 and (g * r)[L - 1 + j k] = 0, 0 < |j| <= m, made symmetric (f64)"""
    A = _constraints(firdes_gmsktx(k, m, bt), k, m)
    e = np.zeros(2 * m + 1)
    e[m] = 1.0
    r = A.T @ np.linalg.solve(A @ A.T, e)
    return 0.5 * (r + r[::-1])


def condition(k, m, bt):
    A = _constraints(firdes_gmsktx(k, m, bt), k, m)
    return float(np.linalg.cond(A @ A.T))


def phases(x, L):
    """phi[t] = arg(conj(x[t - 1]) x[t]) for t = -(L - 1) .. n - 1 of each row of x [C][n], in front of it L zeros; the
    operations in fm_sample_rn's order, so that the signed zeros out of a zero history agree.  Returns (phi, previous sample)"""
    x = np.atleast_2d(np.asarray(x)).astype(np.complex128)
    X = np.concatenate([np.zeros((x.shape[0], L), np.complex128), x], axis=1)
    xp, xc = X[:, :-1], X[:, 1:]
    re = xp.real * xc.real + xp.imag * xc.imag
    im = xp.real * xc.imag + (-(xp.imag * xc.real))
    return np.arctan2(im, re), xp


def assert_usable(x, L):
    """no sample's phase step lies in (3, pi): there the f32 and the f64 angle could wrap differently.  An exact +-pi out of an
    all-zero previous sample is allowed"""
    phi, xp = phases(x, L)
    bad = (np.abs(phi) > 3.0) & ~((xp == 0) & (np.abs(phi) == np.pi))
    assert not bad.any(), int(bad.sum())


def demod(x, r, k):
    """x [C][n] (n a multiple of k) from fresh state -> (d [C][n / k] f64, mag [C][n / k] = sum_i |r[i] phi[s k - i]|)"""
    r = np.asarray(r, np.float64)
    L = r.size
    phi, _ = phases(x, L)                                                 # phi[:, j] is t = j - (L - 1)
    n = phi.shape[1] - (L - 1)
    assert n % k == 0
    d = np.stack([np.convolve(p, r)[L - 1:L - 1 + n:k] for p in phi])
    mag = np.stack([np.convolve(np.abs(p), np.abs(r))[L - 1:L - 1 + n:k] for p in phi])
    return d, mag


def tolerance(r, mag):
    """|soft - d64| <= E_phi sum |r| + (L + 2) 2^-24 sum_i |r_i phi_i|: E_phi = 4e-7 rad is fm_common.h's 1.2e-7 (evaluation) +
    6e-9 (fit) for atan2f_rn plus 1.7e-7 for the two rounded products of conj(x') x; the second term is L products and L sums
    in f32 with the f32 rounding of the taps"""
    r = np.asarray(r, np.float64)
    return 4e-7 * np.abs(r).sum() + (r.size + 2) * 2.0 ** -24 * mag


def gmskmod(bits, k, m, bt, offset=0.0, snr_db=None, amp=1.0, rng=None, phase0=0.0):
    """GMSK of modulation index 0.5: the phase steps are sum_s a_s (pi / 2) g[t - s k] + offset, a_s = 2 bit_s - 1, for
    t < len(bits) k; symbol s reaches the receive filter's output at symbol s + 2 m.  CF32 of amplitude amp whose phase starts
    at phase0, noise at snr_db below it"""
    bits = np.asarray(bits)
    a = np.zeros(bits.size * k)
    a[::k] = 2.0 * bits - 1.0
    inc = 0.5 * math.pi * np.convolve(a, firdes_gmsktx(k, m, bt))[:a.size] + offset
    x = amp * np.exp(1j * (phase0 + np.cumsum(inc)))
    if snr_db is not None:
        s = amp * 10.0 ** (-snr_db / 20.0) / math.sqrt(2.0)
        x = x + s * (rng.standard_normal(x.size) + 1j * rng.standard_normal(x.size))
    return x.astype(np.complex64)
