"""CPU restatement of symSyncR k m beta M (Liquid.chs:244-282), liquid's symsync_rrrf as DESIGN.md 4.10 states it, vectorised
over streams, and a generator of synthetic FSK.  Test infrastructure: the checker of tests/test_symsync_*.py.

It performs the kernel's f32 operations in the kernel's order (k_symsync in kernels_symsync.hip), so the two agree bit for bit:
  dot products: products in f32, summed oldest sample first starting from the first product (np.cumsum is sequential);
  no fused multiply-add anywhere; y = mf / k correctly rounded; b = C roundf(bf), done as floor(|bf| + 0.5) in f64;
  the loop filter in direct form II, v0 = (q - a1 v1) - a2 v2 and q_hat = (b0 v0 + b1 v1) + b2 v2;
  the capacity and fault rule: a stream that would take del <= 0, reach bf >= 2^23, index a bank below 0 or write more than
  the call's n outputs stops for that call and stays faulted (0 outputs per call) until reset.
The design (prototype in f64 rounded once, the rest in f32) is restated too; the GPU tests can also hand the handle's banks in.
"""
import math

import numpy as np

f32 = np.float32


def _bessel_i0(z):
    """I0 by its power series, as design.cpp's bessel_i0"""
    q, term, s = 0.25 * z * z, 1.0, 1.0
    for k in range(1, 200):
        term *= q / (float(k) * float(k))
        s += term
        if term < 1e-18 * s:
            break
    return s


def _kaiser_beta(As):
    As = abs(As)
    if As > 50.0:
        return 0.1102 * (As - 8.7)
    if As > 21.0:
        return 0.5842 * math.pow(As - 21.0, 0.4) + 0.07886 * (As - 21.0)
    return 0.0


def firdes_kaiser_f64(n, fc, As):
    """liquid_firdes_kaiser(n, fc, As, 0) in f64, term for term as design.cpp's firdes_kaiser"""
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
        r = 2.0 * t / float(n - 1)
        a = 1.0 - r * r
        h[i] = sinc * _bessel_i0(beta * math.sqrt(a if a > 0 else 0.0)) / ib
    return h


def design(k=4, m=4, M=64, lf_bw=0.05, k_out=2):
    """symsync_rrrf_create_kaiser(k, m, beta, M) + set_lf_bw(lf_bw) + set_output_rate(k_out); beta is ignored"""
    H_len = 2 * M * k * m + 1
    L = H_len // M
    fc = f32(0.75) / f32(k * M)
    H = (firdes_kaiser_f64(H_len, float(fc), 40.0) * 1.5).astype(f32)
    dH = np.empty(H_len, f32)
    dH[1:-1] = H[2:] - H[:-2]
    dH[0] = H[1] - H[H_len - 1]
    dH[H_len - 1] = H[0] - H[H_len - 2]
    hdh = np.abs(H * dH)
    s = f32(0.06) / hdh.max()
    dH = dH * s
    rev = np.array([[p + (L - 1 - j) * M for p in range(M)] for j in range(L)])
    alpha = f32(1.0) - f32(lf_bw)
    lb = f32(0.22) * f32(lf_bw)
    A0 = f32(1.0) - f32(0.5) * alpha
    A1 = -(f32(0.495) * alpha)
    return dict(k=k, m=m, M=M, k_out=k_out, H_len=H_len, L=L, H=H, dH=dH, mf=H[rev], dmf=dH[rev],
                b0=lb / A0, b1=f32(0.0) / A0, b2=f32(0.0) / A0, a1=A1 / A0, a2=f32(0.0) / A0,
                rate_adj=f32(0.5 * float(f32(lf_bw))), rate0=f32(k) / f32(k_out))


def _roundf(x):
    """C roundf (half away from zero) of f32 values, as an int"""
    x = x.astype(np.float64)
    return (np.copysign(np.floor(np.abs(x) + 0.5), x)).astype(np.int64)


class SymSync:
    """nchan independent symsync_rrrf streams; process(x [nchan][n]) -> (y [nchan][n], ny [nchan]), cap = n per call"""

    def __init__(self, nchan=1, k=4, m=4, M=64, lf_bw=0.05, k_out=2, banks=None):
        self.P = design(k, m, M, lf_bw, k_out)
        if banks is not None:
            mf, dmf = banks
            self.P["mf"] = np.asarray(mf, f32).reshape(self.P["L"], M)
            self.P["dmf"] = np.asarray(dmf, f32).reshape(self.P["L"], M)
        self.C = nchan
        self.reset()

    def reset(self):
        C, P = self.C, self.P
        z = lambda: np.zeros(C, f32)  # noqa: E731
        self.tau, self.bf, self.q_hat, self.v0, self.v1 = z(), z(), z(), z(), z()
        self.rate = np.full(C, P["rate0"], f32)
        self.dl = self.rate.copy()
        self.b = np.zeros(C, np.int64)
        self.decim = np.zeros(C, np.int64)
        self.fault = np.zeros(C, bool)
        self.hist = np.zeros((C, P["L"] - 1), f32)

    def process(self, x):
        """one call on [nchan][n] (or [n] for one stream); also sets self.loop_out, True where an output was a loop instant"""
        P, C = self.P, self.C
        x = np.asarray(x, f32).reshape(C, -1)
        n = x.shape[1]
        L, M, k_out = P["L"], P["M"], P["k_out"]
        mfb, dmfb = P["mf"], P["dmf"]
        kf, fM = f32(P["k"]), f32(M)
        b0, b1, b2, a1, a2, ra = P["b0"], P["b1"], P["b2"], P["a1"], P["a2"], P["rate_adj"]
        ext = np.concatenate([self.hist, x], axis=1)
        y = np.zeros((C, n), f32)
        lo = np.zeros((C, n), bool)
        cnt = np.zeros(C, np.int64)
        run = ~self.fault
        err = np.seterr(over="ignore", invalid="ignore")     # a stream driven to overflow clips q to +-1, as the kernel does
        for t in range(n):
            if not run.any():
                break
            W = ext[:, t:t + L]
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
                w = W[idx]
                mf = np.cumsum(mfb[:, bi].T * w, axis=1, dtype=f32)[:, -1]
                y[idx, cnt[idx]] = mf / kf
                upd = self.decim[idx] == k_out
                lo[idx[upd], cnt[idx[upd]]] = True
                cnt[idx] += 1
                if upd.any():
                    u = idx[upd]
                    self.decim[u] = 0
                    dmf = np.cumsum(dmfb[:, bi[upd]].T * w[upd], axis=1, dtype=f32)[:, -1]
                    q = mf[upd] * dmf
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
                b[ok] = _roundf(self.bf[ok])
            done = run                                     # every live stream left its while loop with b >= M
            self.tau[done] = self.tau[done] - f32(1)
            self.bf[done] = self.bf[done] - fM
            self.b[done] = b[done] - M
        np.seterr(**err)
        self.fault |= ~run
        self.hist = ext[:, n:].copy()
        self.loop_out = lo
        return y, cnt


def run_calls(x, calls, **kw):
    """x [nchan][N] (or [N]) through one SymSync in calls of the given lengths: (outputs per stream, counts [ncalls][nchan],
    loop-instant masks per stream, the object)"""
    x = np.asarray(x, f32)
    one = x.ndim == 1
    X = x.reshape(1, -1) if one else x
    s = SymSync(X.shape[0], **kw)
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
    outs = [np.concatenate(o) if o else np.empty(0, f32) for o in outs]
    marks = [np.concatenate(o) if o else np.empty(0, bool) for o in marks]
    return outs, np.array(counts), marks, s


# ---- synthetic signals ------------------------------------------------------------------------------------------------
def nrz_fsk_iq(nsym, k=4, offset=0.37, ppm=200.0, dev=0.1, seed=0, snr_db=None, ovs=8):
    """continuous-phase binary FSK at k (1 + ppm 1e-6) samples per symbol, the first symbol starting `offset` samples late:
    complex baseband (unit amplitude, deviation +-dev cycles per sample) and the bits.  The NRZ frequency pulse has raised-
    cosine edges k / 2 samples long; the phase is integrated on an `ovs` times finer grid."""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, nsym)
    sps = k * (1.0 + ppm * 1e-6)
    n = int((nsym - 1) * sps)
    t = np.arange(n * ovs, dtype=np.float64) / ovs
    sym = np.clip(np.floor((t - offset) / sps).astype(np.int64), 0, nsym - 1)
    f = dev * (2.0 * bits[sym] - 1.0)
    w = np.hanning(k // 2 * ovs + 2)[1:-1]
    f = np.convolve(f, w / w.sum(), mode="same").reshape(n, ovs).mean(axis=1)
    x = np.exp(2j * np.pi * np.cumsum(f))
    if snr_db is not None:
        s = 10 ** (-snr_db / 20) / np.sqrt(2)
        x = x + s * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return x.astype(np.complex64), bits


def freqdem(x, kf):
    """freqdem: arg(x[t] conj(x[t-1])) / (2 pi kf) with x[-1] = 0 (f64, rounded once)"""
    x = np.asarray(x, np.complex128)
    prev = np.concatenate([[0], x[:-1]])
    return (np.angle(x * np.conj(prev)) / (2 * np.pi * kf)).astype(f32)


def decide(y, marks, bits, skip):
    """hard decisions at the loop instants after `skip` of them, aligned to the transmitted bits by the best lag (within 64
    symbols of `skip`): (errors, compared, lag, eye), eye = min |y| / mean |y| over the decisions"""
    s = y[marks][skip:]
    d = (s > 0).astype(np.int64)
    best = None
    for lag in range(max(0, skip - 64), skip + 64):
        ref = bits[lag:lag + d.size]
        m = min(ref.size, d.size)
        if m < 16:
            break
        e = int(np.sum(ref[:m] != d[:m]))
        if best is None or e < best[0]:
            best = (e, m, lag)
    e, m, lag = best
    a = np.abs(s[:m])
    return e, m, lag, float(a.min() / a.mean())
