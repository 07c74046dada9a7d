"""CPU restatement of pskTracker ("csdr psktrack v1", include/csdr.h), vectorised over rows.  Test infrastructure:
the checker of tests/test_psktrack_*.py.

PskTrack(dtype=f32) performs k_psktrack's f32 operations in the kernel's order (kernels_psktrack.hip, psktrack_common.h): every
product and sum below is one rounded f32 operation, divisions and square roots are correctly rounded, nothing is contracted.
PskTrack(dtype=f64) is the twin of the same loop in f64 with libm's sine and cosine: it keeps the integer phase words, the word()
quantisation and every rule, and serves the property tests."""
import math

import numpy as np

f32 = np.float32
DD, CM = 0, 1                                             # eq_mode: decision-directed, constant-modulus
PLL_BW, AGC_BW, EQ_MU, EQ_DELAY = 9e-4, 0.02, 0.05, 200   # the defaults of include/csdr.h
P_MIN = f32(2.0 ** -100)                                  # floor of the power estimate
EQ_EPS = f32(2.0 ** -20)                                  # eps of the normalised LMS
K_ANGLE = f32(math.pi * 2.0 ** -31)                       # radians per unit of the 29-bit remainder: (pi / 4) / 2^29
W_SCALE = f32(2.0 ** 31 / math.pi)                        # phase words per radian
W_MAX = 2.0 ** 30
S1, S2, S3 = f32(-1.6666654611e-1), f32(8.3321608736e-3), f32(-1.9515295891e-4)
C1, C2, C3 = f32(4.166664568298827e-2), f32(-1.388731625493765e-3), f32(2.443315711809948e-5)
A_QPSK = f32(0.70710677)


def sincos_word(w):
    """(sin, cos) of the phase word w (2^32 = one turn) as csdr_sincos_word computes them, bit for bit: octant o = w >> 29,
    remainder r = w & (2^29 - 1), reflected to 2^29 - r in the odd octants; a = f32(r) K_ANGLE in [0, pi / 4]; z = a a;
    sin a = ((((S3 z + S2) z + S1) z) a) + a and cos a = (1 - 0.5 z) + ((((C3 z + C2) z + C1) z) z), every operation rounded;
    octants 1, 2, 5, 6 swap the two, sin is negated in octants 4 .. 7, cos in octants 2 .. 5"""
    w = np.atleast_1d(np.asarray(w, np.uint32))
    o = (w >> np.uint32(29)).astype(np.int32)
    r = (w & np.uint32(0x1fffffff)).astype(np.int32)
    r = np.where(o & 1, np.int32(0x20000000) - r, r).astype(np.int32)
    a = r.astype(f32) * K_ANGLE
    z = a * a
    p = S3 * z
    p = p + S2
    p = p * z
    p = p + S1
    p = p * z
    p = p * a
    s = p + a
    q = C3 * z
    q = q + C2
    q = q * z
    q = q + C1
    q = q * z
    q = q * z
    c = (f32(1) - f32(0.5) * z) + q
    swap = ((o + 1) >> 1) & 1
    sn, cs = np.where(swap, c, s), np.where(swap, s, c)
    sn = np.where(o >= 4, -sn, sn)
    cs = np.where(((o + 2) >> 2) & 1, -cs, cs)
    return sn.astype(f32), cs.astype(f32)


def word(v, ft=f32):
    """radians -> phase words: one product by 2^31 / pi in `ft`, NaN -> 0, clamped to +-2^30, rounded to the nearest integer
    (ties to even), as uint32 modulo 2^32"""
    f = np.asarray(v, ft) * ft(W_SCALE)
    f = np.where(f == f, f, ft(0))
    f = np.where(f > ft(W_MAX), ft(W_MAX), np.where(f < ft(-W_MAX), ft(-W_MAX), f))
    return (np.rint(f).astype(np.int64) & 0xffffffff).astype(np.uint32)


class PskTrack:
    """nchan independent rows; process(x complex [nchan][n], nx [nchan] or None) -> (y [nchan][n], sym uint32 [nchan][n], ny)"""

    def __init__(self, nchan=1, bits=1, sps=1, phase=0, eq_len=0, eq_mu=EQ_MU, eq_mode=DD, eq_delay=EQ_DELAY, pll_bw=PLL_BW,
                 agc_bw=AGC_BW, dtype=f32):
        assert bits in (1, 2) and sps in (1, 2) and phase in (0, 1) and eq_mode in (DD, CM)
        assert eq_len == 0 or (sps == 2 and eq_len % 2 == 1 and 3 <= eq_len <= 17)
        self.C, self.bits, self.sps, self.phase, self.L, self.mode, self.delay = nchan, bits, sps, phase, eq_len, eq_mode, eq_delay
        self.ft = ft = dtype
        self.ct = np.complex64 if ft is f32 else np.complex128
        self.mu, self.agc_bw = ft(f32(eq_mu)), ft(f32(agc_bw))
        self.alpha = ft(f32(pll_bw))
        self.beta = ft(np.sqrt(f32(pll_bw)))                     # f32 sqrt, correctly rounded
        self.restart()

    def restart(self):
        C, L, ft = self.C, self.L, self.ft
        self.p = np.ones(C, ft)
        self.theta = np.zeros(C, np.uint32)
        self.freq = np.zeros(C, np.uint32)
        self.par = np.zeros(C, np.uint32)
        self.nsym = np.zeros(C, np.uint32)
        self.wr, self.wi = np.zeros((C, L), ft), np.zeros((C, L), ft)
        if L:
            self.wr[:, (L - 1) // 2] = 1
        self.br, self.bi = np.zeros((C, L), ft), np.zeros((C, L), ft)      # the window, oldest sample first

    @property
    def w(self):
        return (self.wr + 1j * self.wi).astype(self.ct)

    def _sincos(self, th):
        if self.ft is f32:
            return sincos_word(th)
        a = th.astype(np.float64) * (2.0 * math.pi / 2.0 ** 32)
        return np.sin(a), np.cos(a)

    def process(self, x, nx=None):
        C, L, ft = self.C, self.L, self.ft
        x = np.asarray(x, self.ct).reshape(C, -1)
        n = x.shape[1]
        nx = np.full(C, n, np.int64) if nx is None else np.minimum(np.asarray(nx, np.int64), n)
        xr, xi = np.ascontiguousarray(x.real).astype(ft), np.ascontiguousarray(x.imag).astype(ft)
        yr, yi = np.zeros((C, n), ft), np.zeros((C, n), ft)
        sym = np.zeros((C, n), np.uint32)
        cnt = np.zeros(C, np.int64)
        one, half, A = ft(1), ft(0.5), ft(A_QPSK)
        cpar = ((L - 1) // 2) & 1 if L else 0
        err = np.seterr(all="ignore")
        for t in range(int(nx.max()) if C else 0):
            a = np.nonzero(t < nx)[0]
            vr, vi = xr[a, t], xi[a, t]
            # 1. power normaliser
            m2 = vr * vr + vi * vi
            p = self.p[a] + self.agc_bw * (m2 - self.p[a])
            p = np.where(p < ft(P_MIN), ft(P_MIN), p)
            self.p[a] = p
            g = np.sqrt(p)
            vr, vi = vr / g, vi / g
            # 2. derotation
            s, c = self._sincos(self.theta[a])
            ur = vr * c + vi * s
            ui = vi * c - vr * s
            self.theta[a] = self.theta[a] + self.freq[a]
            # 3. window and symbol decimation
            if L:
                self.br[a, :-1], self.bi[a, :-1] = self.br[a, 1:], self.bi[a, 1:]
                self.br[a, -1], self.bi[a, -1] = ur, ui
            inst = np.ones(a.size, bool) if self.sps == 1 else ((self.par[a] + cpar) & 1) == self.phase
            self.par[a] ^= np.uint32(1)
            if not inst.any():
                continue
            i = a[inst]
            if L:
                br, bi, wr, wi = self.br[i], self.bi[i], self.wr[i], self.wi[i]
                dr, di, E = np.zeros(i.size, ft), np.zeros(i.size, ft), np.zeros(i.size, ft)
                for j in range(L):
                    dr = dr + (wr[:, j] * br[:, j] + wi[:, j] * bi[:, j])
                    di = di + (wr[:, j] * bi[:, j] - wi[:, j] * br[:, j])
                    E = E + (br[:, j] * br[:, j] + bi[:, j] * bi[:, j])
            else:
                dr, di = ur[inst], ui[inst]
            # 4. decision
            bI = dr < 0
            if self.bits == 1:
                hr, hi = np.where(bI, -one, one), np.zeros(i.size, ft)
                k = bI.astype(np.uint32)
            else:
                bQ = di < 0
                hr, hi = np.where(bI, -A, A), np.where(bQ, -A, A)
                k = bI.astype(np.uint32) | (bQ.astype(np.uint32) << np.uint32(1))
            # 5. phase error and PLL
            e = di * hr - dr * hi
            self.freq[i] = self.freq[i] + word(self.alpha * e, ft)
            self.theta[i] = self.theta[i] + word(self.beta * e, ft)
            # 6. equaliser update
            if L:
                u = self.nsym[i] >= self.delay
                if self.mode == DD:
                    er, ei = hr - dr, hi - di
                else:
                    r = np.sqrt(dr * dr + di * di)
                    ok = r > 0
                    rs = np.where(ok, r, one)
                    er, ei = np.where(ok, dr / rs - dr, 0).astype(ft), np.where(ok, di / rs - di, 0).astype(ft)
                gn = self.mu / (E + ft(EQ_EPS))
                for j in range(L):
                    nr = wr[:, j] + gn * (er * br[:, j] + ei * bi[:, j])
                    ni = wi[:, j] + gn * (er * bi[:, j] - ei * br[:, j])
                    wr[:, j], wi[:, j] = np.where(u, nr, wr[:, j]), np.where(u, ni, wi[:, j])
                self.wr[i], self.wi[i] = wr, wi
            self.nsym[i] = self.nsym[i] + (self.nsym[i] != np.uint32(0xffffffff)).astype(np.uint32)
            # 7. output
            yr[i, cnt[i]], yi[i, cnt[i]], sym[i, cnt[i]] = dr, di, k
            cnt[i] += 1
        np.seterr(**err)
        y = np.empty((C, n), self.ct)
        y.real, y.imag = yr, yi
        return y, sym, cnt.astype(np.uint32)

    def freq_cycles_per_symbol(self):
        """the loop's frequency word as cycles per symbol, signed"""
        return self.freq.astype(np.int32).astype(np.float64) * self.sps / 2.0 ** 32


def run_calls(x, calls, **kw):
    """x [nchan][N] (or [N]) through one PskTrack in calls of the given lengths: (y per row, symbols per row, counts, the object)"""
    x = np.asarray(x)
    X = x.reshape(1, -1) if x.ndim == 1 else x
    s = PskTrack(X.shape[0], **kw)
    ys, ks, counts, pos = [[] for _ in X], [[] for _ in X], [], 0
    for c in calls:
        y, k, ny = s.process(X[:, pos:pos + c])
        pos += c
        counts.append(ny.copy())
        for r in range(X.shape[0]):
            ys[r].append(y[r, :ny[r]])
            ks[r].append(k[r, :ny[r]])
    return [np.concatenate(v) for v in ys], [np.concatenate(v) for v in ks], np.array(counts), s
