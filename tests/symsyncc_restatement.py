"""CPU restatement of symSyncC m k (Liquid.chs:177-242), liquid's symsync_crcf as DESIGN.md 4.16 states it, vectorised over
streams; the two root-Nyquist prototype designs in f64; and a generator of pulse-shaped QPSK / BPSK with a timing offset and a
clock error.  Test infrastructure: the checker of tests/test_rnyquist_cpu.py and tests/test_symsyncc_*.py.

SymSyncC performs the kernel's f32 operations in the kernel's order (k_symsyncc in kernels_symsyncc.hip), so the two agree bit
for bit: re and im of a dot product are independent sums, products in f32, summed oldest sample first starting from the first
product; y = (mf.re / k, mf.im / k) correctly rounded; q = mf.re dmf.re + mf.im dmf.im, two rounded products and one add,
clipped to +-1; the loop filter, tau / bf / b and the fault rule exactly as symsync_restatement.SymSync has them."""
import math

import numpy as np

import symsync_restatement as S

f32 = np.float32
ARKAISER, RRC = 7, 9                                          # liquid's LIQUID_FIRFILT_ numbers


# ---- the prototype designs, f64 ---------------------------------------------------------------------------------------
def rrc_f64(k, m, beta, dt=0.0):
    """liquid_firdes_rrcos(k, m, beta, dt): the closed form, 2 k m + 1 taps"""
    n = 2 * k * m + 1
    h = np.empty(n, np.float64)
    for i in range(n):
        z = (i + dt) / k - m
        g = 1.0 - 16.0 * beta * beta * z * z
        if abs(z) < 1e-12:
            h[i] = 1.0 - beta + 4.0 * beta / math.pi
        elif abs(g) < 1e-8:
            a = math.pi / (4.0 * beta)
            h[i] = beta / math.sqrt(2.0) * ((1.0 + 2.0 / math.pi) * math.sin(a) + (1.0 - 2.0 / math.pi) * math.cos(a))
        else:
            h[i] = (math.sin(math.pi * z * (1.0 - beta)) + 4.0 * beta * z * math.cos(math.pi * z * (1.0 + beta))) / (math.pi * z * g)
    return h


def _bessel_i0(z):
    """symsync_restatement._bessel_i0 on an array: the same power series, every element summed until it has converged"""
    q = 0.25 * z * z
    term, s = np.ones_like(z), np.ones_like(z)
    for k in range(1, 200):
        term = term * (q / (float(k) * float(k)))
        s = s + term
        if np.all(term < 1e-18 * s):
            break
    return s


def kaiser_f64(n, fc, As, dt=0.0):
    """symsync_restatement.firdes_kaiser_f64 with liquid's fractional sample offset: t = i - (n - 1) / 2 + dt"""
    beta = S._kaiser_beta(As)
    t = np.arange(n, dtype=np.float64) - 0.5 * float(n - 1) + dt
    x = 2.0 * fc * t
    xs = np.where(np.abs(x) < 0.01, 1.0, x)
    sinc = np.where(np.abs(x) < 0.01, np.cos(math.pi * x / 2) * np.cos(math.pi * x / 4) * np.cos(math.pi * x / 8),
                    np.sin(math.pi * xs) / (math.pi * xs))
    r = 2.0 * t / float(n - 1)
    return sinc * _bessel_i0(beta * np.sqrt(np.maximum(1.0 - r * r, 0.0))) / S._bessel_i0(beta)


def arkaiser_rho_hat(m, beta):
    lb = math.log(beta)
    c0 = 0.762886 + 0.067663 * math.log(m)
    c1 = 0.065515
    c2 = math.log(1.0 - 0.088 * math.pow(m, -1.6))
    return c0 + c1 * lb + c2 * lb * lb


def rkaiser_f64(k, m, beta, rho, dt=0.0):
    """the r-Kaiser family: a Kaiser low-pass whose transition band is rho of the excess bandwidth, scaled to sum h^2 = k"""
    n = 2 * k * m + 1
    kf = 0.5 * (1.0 + beta * (1.0 - rho)) / k
    dl = beta * rho / k
    As = 14.26 * dl * n + 7.95
    h = kaiser_f64(n, kf, As, dt)
    return h * math.sqrt(k / float(np.sum(h * h)))


def arkaiser_f64(k, m, beta, dt=0.0):
    return rkaiser_f64(k, m, beta, arkaiser_rho_hat(m, beta), dt)


def rnyquist_f64(ftype, k, m, beta, dt=0.0):
    return rrc_f64(k, m, beta, dt) if ftype == RRC else arkaiser_f64(k, m, beta, dt)


def isi_rms(h, k, m):
    """rms of (h * h) at the 2 m multiples of k on one side of its centre, relative to the centre (the other side mirrors it)"""
    g = np.convolve(h, h)
    c = (g.size - 1) // 2
    e = g[c + k * np.arange(1, 2 * m + 1)] / g[c]
    return float(np.sqrt(np.mean(e * e)))


# ---- the synchroniser -------------------------------------------------------------------------------------------------
def banks_from_prototype(H, M):
    """symsync_create(k, M, H, H_len) behind the prototype, as design.cpp's symsync_set_prototype: (dH, mf, dmf)"""
    H = np.asarray(H, f32)
    H_len = H.size
    L = H_len // M
    dH = np.empty(H_len, f32)
    dH[1:-1] = H[2:] - H[:-2]
    dH[0] = H[1] - H[H_len - 1]
    dH[H_len - 1] = H[0] - H[H_len - 2]
    dH = dH * (f32(0.06) / np.abs(H * dH).max())
    rev = np.array([[p + (L - 1 - j) * M for p in range(M)] for j in range(L)])
    return dH, H[rev], dH[rev]


def design(k=2, m=3, M=32, lf_bw=0.01, k_out=1, ftype=ARKAISER, beta=0.5):
    """symsync_create_rnyquist(ftype, k, m, beta, M) + set_lf_bw + set_output_rate: symsync_restatement.design's dictionary
    with the banks of the root-Nyquist prototype designed at k M samples per symbol"""
    P = S.design(k, m, M, lf_bw, k_out)
    P["H"] = rnyquist_f64(ftype, k * M, m, beta).astype(f32)
    P["dH"], P["mf"], P["dmf"] = banks_from_prototype(P["H"], M)
    return P


class SymSyncC(S.SymSync):
    """nchan independent symsync_crcf streams; process(x complex64 [nchan][n]) -> (y complex64 [nchan][n], ny [nchan])"""

    def __init__(self, nchan=1, k=2, m=3, M=32, lf_bw=0.01, k_out=1, ftype=ARKAISER, beta=0.5, banks=None):
        self.P = design(k, m, M, lf_bw, k_out, ftype, beta) if banks is None else S.design(k, m, M, lf_bw, k_out)
        if banks is not None:
            mf, dmf = banks
            self.P["mf"] = np.asarray(mf, f32).reshape(self.P["L"], M)
            self.P["dmf"] = np.asarray(dmf, f32).reshape(self.P["L"], M)
        self.C = nchan
        self.reset()

    def reset(self):
        super().reset()
        self.hist = np.zeros((self.C, self.P["L"] - 1), np.complex64)

    def process(self, x):
        P, C = self.P, self.C
        x = np.asarray(x, np.complex64).reshape(C, -1)
        n = x.shape[1]
        L, M, k_out = P["L"], P["M"], P["k_out"]
        mfb, dmfb = P["mf"], P["dmf"]
        kf, fM = f32(P["k"]), f32(M)
        b0, b1, b2, a1, a2, ra = P["b0"], P["b1"], P["b2"], P["a1"], P["a2"], P["rate_adj"]
        ext = np.concatenate([self.hist, x], axis=1)
        er, ei = np.ascontiguousarray(ext.real), np.ascontiguousarray(ext.imag)
        yr, yi = np.zeros((C, n), f32), np.zeros((C, n), f32)
        lo = np.zeros((C, n), bool)
        cnt = np.zeros(C, np.int64)
        run = ~self.fault
        err = np.seterr(over="ignore", invalid="ignore")
        dot = lambda h, w: np.cumsum(h * w, axis=1, dtype=f32)[:, -1]  # noqa: E731
        for t in range(n):
            if not run.any():
                break
            Wr, Wi = er[:, t:t + L], ei[:, t:t + L]
            b = self.b.copy()
            live = run.copy()
            while True:
                live &= b < M
                over = live & ((cnt >= n) | (b < 0))
                if over.any():
                    run &= ~over
                    live &= ~over
                idx = np.nonzero(live)[0]
                if idx.size == 0:
                    break
                bi = b[idx]
                hm = mfb[:, bi].T
                mr, mi = dot(hm, Wr[idx]), dot(hm, Wi[idx])
                yr[idx, cnt[idx]] = mr / kf
                yi[idx, cnt[idx]] = mi / kf
                upd = self.decim[idx] == k_out
                lo[idx[upd], cnt[idx[upd]]] = True
                cnt[idx] += 1
                if upd.any():
                    u = idx[upd]
                    self.decim[u] = 0
                    hd = dmfb[:, bi[upd]].T
                    dr, di = dot(hd, Wr[u]), dot(hd, Wi[u])
                    q = mr[upd] * dr + mi[upd] * di
                    q = np.where(q > f32(1), f32(1), np.where(q < f32(-1), f32(-1), q)).astype(f32)
                    v2 = self.v1[u]
                    self.v1[u] = self.v0[u]
                    self.v0[u] = (q - a1 * self.v1[u]) - a2 * v2
                    self.q_hat[u] = (b0 * self.v0[u] + b1 * self.v1[u]) + b2 * v2
                    self.rate[u] = self.rate[u] + ra * self.q_hat[u]
                    self.dl[u] = self.rate[u] + self.q_hat[u]
                    bad = u[~(self.dl[u] > 0)]
                    run[bad] = False
                    live[bad] = False
                    idx = np.nonzero(live)[0]
                self.decim[idx] += 1
                self.tau[idx] = self.tau[idx] + self.dl[idx]
                self.bf[idx] = self.tau[idx] * fM
                bad = idx[~(self.bf[idx] < f32(8388608.0))]
                run[bad] = False
                live[bad] = False
                ok = idx[self.bf[idx] < f32(8388608.0)]
                b[ok] = S._roundf(self.bf[ok])
            done = run
            self.tau[done] = self.tau[done] - f32(1)
            self.bf[done] = self.bf[done] - fM
            self.b[done] = b[done] - M
        np.seterr(**err)
        self.fault |= ~run
        self.hist = ext[:, n:].copy()
        self.loop_out = lo
        y = np.empty((C, n), np.complex64)
        y.real, y.imag = yr, yi
        return y, cnt


def run_calls(x, calls, **kw):
    """x [nchan][N] (or [N]) through one SymSyncC in calls of the given lengths: (outputs per stream, counts [ncalls][nchan],
    loop-instant masks per stream, the object)"""
    x = np.asarray(x, np.complex64)
    X = x.reshape(1, -1) if x.ndim == 1 else x
    s = SymSyncC(X.shape[0], **kw)
    outs = [[] for _ in range(X.shape[0])]
    marks = [[] for _ in range(X.shape[0])]
    counts, pos = [], 0
    for c in calls:
        y, ny = s.process(X[:, pos:pos + c])
        pos += c
        counts.append(ny.copy())
        for r in range(X.shape[0]):
            outs[r].append(y[r, :ny[r]])
            marks[r].append(s.loop_out[r, :ny[r]])
    outs = [np.concatenate(o) if o else np.empty(0, np.complex64) for o in outs]
    marks = [np.concatenate(o) if o else np.empty(0, bool) for o in marks]
    return outs, np.array(counts), marks, s


# ---- synthetic signals ------------------------------------------------------------------------------------------------
def psk(nsym, k, m=3, ftype=ARKAISER, beta=0.5, offset=0.37, ppm=200.0, bits_per_symbol=2, seed=0, amp=1.0):
    """QPSK (or BPSK) symbols shaped by the root-Nyquist prototype designed at 32 k samples per symbol and sampled at
    round((i (1 + ppm 1e-6) + offset) 32) of that grid, i.e. a transmitter whose clock runs ppm slow against the receiver's
    k samples per symbol, the first symbol `offset` samples early; scaled to unit mean power times amp.
    (samples complex64, symbols complex128 of unit modulus)"""
    rng = np.random.default_rng(seed)
    if bits_per_symbol == 2:
        sym = ((2.0 * rng.integers(0, 2, nsym) - 1.0) + 1j * (2.0 * rng.integers(0, 2, nsym) - 1.0)) / math.sqrt(2.0)
    else:
        sym = (2.0 * rng.integers(0, 2, nsym) - 1.0) + 0j
    ov = 32
    kk = k * ov
    h = rnyquist_f64(ftype, kk, m, beta)
    n = int((nsym - 2 * m - 2) * k)
    pos = np.round((np.arange(n) * (1.0 + ppm * 1e-6) + offset) * ov).astype(np.int64)
    # s(p) = sum_j sym[j] h[p - j kk]: the 2 m + 1 symbols whose pulse covers fine-grid position p
    x = np.zeros(n, np.complex128)
    j0 = pos // kk
    for d in range(-2 * m, 1):
        j = j0 + d
        t = pos - j * kk
        ok = (j >= 0) & (j < nsym) & (t >= 0) & (t < h.size)
        x[ok] += sym[j[ok]] * h[t[ok]]
    x *= amp / math.sqrt(float(np.mean(np.abs(x) ** 2)))
    return x.astype(np.complex64), sym


def decide(y, marks, sym, skip):
    """QPSK decisions at the loop instants after `skip` of them against the transmitted symbols at the best lag (within 64
    symbols of `skip`) and the best complex gain: (errors, compared, lag, evm).  evm = rms |y - g sym| / |g|, g the
    least-squares gain; a decision is the pair of signs of y / g"""
    s = np.asarray(y, np.complex128)[marks][skip:]
    best = None
    for lag in range(max(0, skip - 64), skip + 64):
        ref = sym[lag:lag + s.size]
        n = min(ref.size, s.size)
        if n < 16:
            break
        g = np.vdot(ref[:n], s[:n]) / np.vdot(ref[:n], ref[:n])
        z = s[:n] / g
        e = int(np.sum((np.sign(z.real) != np.sign(ref[:n].real)) | ((np.sign(z.imag) != np.sign(ref[:n].imag)) & (ref[:n].imag != 0))))
        evm = float(np.sqrt(np.mean(np.abs(z - ref[:n]) ** 2)))
        if best is None or (e, evm) < (best[0], best[3]):
            best = (e, n, lag, evm)
    return best
