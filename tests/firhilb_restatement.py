"""CPU restatement of realToComplex / complexToReal (Liquid.chs:503-546), liquid's firhilbf as DESIGN.md 4.11 states it.  Test
infrastructure: the checker of tests/test_firhilb_*.py.

It performs the kernel's f32 operations in the kernel's order (kernels_firhilb.hip), so the two agree bit for bit:
  the quadrature branch: products in f32, summed j = 0 .. 2m-1 (oldest sample first) starting from the first product
  (np.cumsum is sequential); no fused multiply-add; the delay branch is a copy.
The design is restated in float64 (design(m, As)); the GPU tests hand the handle's f32 taps in.
"""
import math

import numpy as np

from symsync_restatement import _bessel_i0, _kaiser_beta

f32 = np.float32


def firdes_kaiser_f64(n, fc, As, wden):
    """liquid_firdes_kaiser(n, fc, As, 0) in f64 with the Kaiser window's argument 2 t / wden, term for term as design.cpp's"""
    beta = _kaiser_beta(As)
    ib = _bessel_i0(beta)
    h = np.empty(n, np.float64)
    for i in range(n):
        t = float(i) - 0.5 * float(n - 1)
        x = 2.0 * fc * t
        if abs(x) < 0.01:
            sinc = math.cos(math.pi * x / 2) * math.cos(math.pi * x / 4) * math.cos(math.pi * x / 8)
        else:
            sinc = math.sin(math.pi * x) / (math.pi * x)
        r = 2.0 * t / wden
        a = 1.0 - r * r
        h[i] = sinc * _bessel_i0(beta * math.sqrt(a if a > 0 else 0.0)) / ib
    return h


def design(m=5, As=60.0):
    """firhilbf_create(m, As) in f64: h = liquid_firdes_kaiser(4 m + 1, 0.25, As, 0); h[i] <- Im(h[i] e^{j pi t / 2}), t = i - 2 m;
    hq[j] = h[h_len - i - 1] for i = 1, 3, 5, ... (j = 0 .. 2m-1).  t is odd at those taps, so the factor is exactly +-1.
    The window's argument is 2 t / h_len (design.cpp's design_firhilb says why)."""
    h_len = 4 * m + 1
    h = firdes_kaiser_f64(h_len, 0.25, As, float(h_len))
    hq = np.empty(2 * m, np.float64)
    for j in range(2 * m):
        i = h_len - (2 * j + 1) - 1
        t = i - 2 * m
        hq[j] = h[i] if t % 4 == 1 else -h[i]
    return hq


class FirHilb:
    """one firhilbf: two windows of 2 m floats shared by decim (2 n reals -> n complex) and interp (n complex -> 2 n reals)"""

    def __init__(self, m=5, As=60.0, taps=None):
        self.m = m
        self.hq = design(m, As).astype(f32) if taps is None else np.asarray(taps, f32).copy()
        assert self.hq.size == 2 * m
        self.reset()

    def reset(self):
        self.w0 = np.zeros(2 * self.m, f32)          # index 0 oldest; the delay branch
        self.w1 = np.zeros(2 * self.m, f32)          # the quadrature branch

    def _run(self, to_w1, to_w0):
        """push to_w1[p] to w1 and to_w0[p] to w0 for every p: (quadrature outputs, delay outputs)"""
        n, m, H = to_w1.size, self.m, 2 * self.m
        e1 = np.concatenate([self.w1, np.asarray(to_w1, f32)])
        e0 = np.concatenate([self.w0, np.asarray(to_w0, f32)])
        self.w1, self.w0 = e1[n:].copy(), e0[n:].copy()
        if n == 0:
            return np.empty(0, f32), np.empty(0, f32)
        W = np.lib.stride_tricks.sliding_window_view(e1, H)[1:n + 1]        # after push p: e1[p + 1 .. p + 2m]
        yq = np.cumsum(W * self.hq[None, :], axis=1, dtype=f32)[:, -1]
        yi = e0[m:m + n]                                                    # w0[m - 1] after push p: e0[p + m]
        return yq, yi

    def decim(self, x):
        """per pair (x0, x1): push x0 to w1, yq = sum_j hq[j] w1[j]; push x1 to w0, yi = w0[m - 1]; yi + j yq"""
        x = np.asarray(x, f32).reshape(-1)
        n = x.size // 2
        yq, yi = self._run(x[0:2 * n:2], x[1:2 * n:2])
        y = np.empty(n, np.complex64)
        y.real, y.imag = yi, yq
        return y

    def interp(self, x):
        """per x: push Im x to w0, y[0] = w0[m - 1]; push Re x to w1, y[1] = sum_j hq[j] w1[j]"""
        x = np.asarray(x, np.complex64).reshape(-1)
        yq, yi = self._run(x.real, x.imag)
        y = np.empty(2 * x.size, f32)
        y[0::2], y[1::2] = yi, yq
        return y


def run_calls(obj, x, calls, interp=False):
    """x through obj in calls of the given sizes (complex samples each): the concatenated output"""
    step = 1 if interp else 2
    out, pos = [], 0
    for c in calls:
        a = x[pos:pos + step * c]
        pos += step * c
        out.append(obj.interp(a) if interp else obj.decim(a))
    return np.concatenate(out) if out else np.empty(0, f32 if interp else np.complex64)


def band_limited(N, seed=11, ntones=31):
    """31 unit tones spread evenly over 0.1 .. 0.4 cycles per real sample with seeded phases, scaled to unit power: (x, its
    quadrature) -- the same tones as sines"""
    n = np.arange(N)
    rng = np.random.default_rng(seed)
    fs, ph = np.linspace(0.1, 0.4, ntones), rng.uniform(0, 2 * np.pi, ntones)
    arg = 2 * np.pi * fs[:, None] * n[None, :] + ph[:, None]
    g = 1.0 / np.sqrt(ntones / 2)
    return np.cos(arg).sum(axis=0) * g, np.sin(arg).sum(axis=0) * g
