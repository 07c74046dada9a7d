"""CPU restatement of stereoFMDecoder' quadRate decim (Liquid.chs:959-1078) with the constant wire delay of DESIGN.md 4.9,
and a generator of synthetic stereo broadcasts.  Test infrastructure: the checker of tests/test_fmstereo_*.py.

Per stream, on the F32 MPX x (the freqdem output):
  N = round(q / 1350) taps for every FIR (Haskell `round`, half-even); d = round(fir_group_delay(pilot FIR, 100 / q))
  s[t] = x[t - d] (0 before the stream start): the wire
  p    = mixUp ncoF . firPilot . mixDown ncoF (x + 0j)         two fresh VCO NCOs at phase 0 (O.Nco)
  pllStep per sample (float32 scalars, in the reference's order) -> u[t] = s[t] cos(phase(theta_SS))
  lmr  = 2 Re firLMR(u), lpr = Re firLPR(s); (L, R) = (lpr + lmr, lpr - lmr)
  L, R -> O.Butter2(5000 / q) -> O.FirDecim(decim), the decimator consuming floor(n / decim) decim samples per call
The FIR dot products are taken in f64 and rounded once (liquid's summation order is not reproducible anyway); the output scale
2 fc is then applied in f32, as firfilt_crcf_set_scale does.  The PLL steps through every f32 operation of nco_crcf's VCO
(oracle/csdr_oracle.c's constrain and float-phase phasor, restated here vectorised over streams and checked against the
oracle's in tests/test_fmstereo_cpu.py) and GHC's class-default atan2.  `sums="f32"` is a second rounding of the same decoder
(FIR sums accumulated in f32, the PLL's cos / sin from libm's cosf / sinf): tests/fms_cases.py takes the GPU tests' bounds
from its distance to the default.
"""
import ctypes as C
import math

import numpy as np

import oracle_lib as O

f32 = np.float32
TWO_PI = 6.283185307179586
PI_F = f32(3.14159265358979323846)
_libm = C.CDLL("libm.so.6")
for _fn in ("cosf", "sinf", "atanf"):
    getattr(_libm, _fn).restype = C.c_float
    getattr(_libm, _fn).argtypes = [C.c_float]


# ---- design -------------------------------------------------------------------------------------------------------------
def _besseli0(z):
    """the oracle's liquid_besseli0f: 32-term series sum_k ((z/2)^k / k!)^2 (oracle/csdr_oracle.c orc_besseli0)"""
    if z == 0.0:
        return 1.0
    y = 0.0
    for k in range(32):
        t = k * math.log(0.5 * z) - math.lgamma(k + 1.0)
        y += math.exp(2.0 * t)
    return y


def _kaiser_beta(As):
    As = abs(As)
    if As > 50.0:
        return 0.1102 * (As - 8.7)
    if As > 21.0:
        return 0.5842 * (As - 21.0) ** 0.4 + 0.07886 * (As - 21.0)
    return 0.0


def _sinc(x):
    if abs(x) < 0.01:
        return math.cos(math.pi * x / 2.0) * math.cos(math.pi * x / 4.0) * math.cos(math.pi * x / 8.0)
    return math.sin(math.pi * x) / (math.pi * x)


def firdes_kaiser(n, fc, As=60.0):
    """liquid_firdes_kaiser(n, fc, As, 0) evaluated in f64 and rounded once, as the oracle's PFB prototype"""
    beta = _kaiser_beta(As)
    ib = _besseli0(beta)
    h = np.empty(n, dtype=np.float32)
    for i in range(n):
        t = i - (n - 1) / 2.0
        r = 2.0 * t / (n - 1)
        a = max(1.0 - r * r, 0.0)
        h[i] = _sinc(2.0 * float(fc) * t) * (_besseli0(beta * math.sqrt(a)) / ib)
    return h


def haskell_round(v):
    """Haskell `round`: to the nearest integer, ties to even"""
    return int(np.rint(np.float64(v)))


def fir_group_delay(h, fc):
    """liquid's fir_group_delay as recalled: Re(sum i h[i] e^{j 2 pi fc i} / sum h[i] e^{j 2 pi fc i}), f32 accumulation;
    the quotient's real part as (t0 conj(t1)).re / |t1|^2 in f32 (composable_sdr_amd/csrc/design.cpp does the same)"""
    t0r = t0i = t1r = t1i = f32(0)
    for i, hi in enumerate(np.asarray(h, dtype=np.float32)):
        a = f32(TWO_PI * float(f32(fc)) * float(i))
        c, s = f32(_libm.cosf(a)), f32(_libm.sinf(a))
        hc, hs, fi = hi * c, hi * s, f32(i)
        t0r, t0i = t0r + hc * fi, t0i + hs * fi
        t1r, t1i = t1r + hc, t1i + hs
    return (t0r * t1r + t0i * t1i) / (t1r * t1r + t1i * t1i)


def design(q, decim=4):
    N = haskell_round(q / 1350.0)
    fc_p, fc_a = f32(800.0 / q), f32(15000.0 / q)
    hp, ha = firdes_kaiser(N, fc_p), firdes_kaiser(N, fc_a)
    gd = fir_group_delay(hp, f32(100.0 / q))
    ncoF = f32(19000.0 * 2.0 * math.pi / q)
    alpha = f32(9.0 / q)
    return dict(q=q, N=N, d=haskell_round(gd), group_delay=float(gd), hp=hp, ha=ha, sp=f32(2) * fc_p, sa=f32(2) * fc_a,
                ncoF=ncoF, d_nco=O.nco_constrain(ncoF), alpha=alpha, beta=f32(np.sqrt(alpha)), deemph_fc=f32(5000.0 / q), decim=decim)


# ---- the oracle's NCO arithmetic, vectorised over streams --------------------------------------------------------------
def constrain(x):
    """orc_nco_constrain on an array of f32"""
    x = np.asarray(x, dtype=np.float32)
    p = (x.astype(np.float64) * 0.159154943091895).astype(np.float32)
    fp = p - np.trunc(p).astype(np.int64).astype(np.float32)
    fp = np.where(fp < 0, (fp.astype(np.float64) + 1.0).astype(np.float32), fp)
    return ((fp * f32(4294967296.0)).astype(np.uint64) & 0xFFFFFFFF).astype(np.uint32)


def phase(theta):
    """nco_crcf_get_phase: 2 pi (float) theta / 2^32, evaluated in f64, rounded to f32"""
    return (TWO_PI * np.asarray(theta, dtype=np.uint32).astype(np.float32).astype(np.float64) / 4294967296.0).astype(np.float32)


def _cos(ph):
    return np.cos(ph.astype(np.float64)).astype(np.float32)


def _sin(ph):
    return np.sin(ph.astype(np.float64)).astype(np.float32)


def _cosf(ph):
    """libm's cosf, element by element (the rounding variant, sums="f32")"""
    return np.array([_libm.cosf(float(v)) for v in np.ravel(ph)], dtype=np.float32).reshape(np.shape(ph))


def _sinf(ph):
    return np.array([_libm.sinf(float(v)) for v in np.ravel(ph)], dtype=np.float32).reshape(np.shape(ph))


def hs_atan2(y, x):
    """GHC's class-default atan2 on Float, element-wise: atan (y / x) plus the quadrant fixes (not atan2f)"""
    y = np.asarray(y, dtype=np.float32).copy()
    x = np.asarray(x, dtype=np.float32)
    neg = ((x <= 0) & (y < 0)) | ((x < 0) & (y == 0) & np.signbit(y)) | ((x == 0) & np.signbit(x) & (y == 0) & np.signbit(y))
    y = np.where(neg, -y, y)
    with np.errstate(divide="ignore", invalid="ignore"):
        at = np.arctan((y / x).astype(np.float64)).astype(np.float32)
    r = np.where(x > 0, at,
                 np.where((x == 0) & (y > 0), PI_F / f32(2),
                          np.where((x < 0) & (y > 0), PI_F + at,
                                   np.where((y == 0) & ((x < 0) | ((x == 0) & np.signbit(x))), PI_F,
                                            np.where((x == 0) & (y == 0), y, x + y))))).astype(np.float32)
    return np.where(neg, -r, r).astype(np.float32)


# ---- the decoder -------------------------------------------------------------------------------------------------------
def _check_sums(sums):
    if sums not in ("f64", "f32"):
        raise ValueError(f"sums: {sums!r} is neither 'f64' nor 'f32'")
    return sums == "f32"


def _fir(h, x, scale, sums="f64"):
    """sums="f64": the dot products in f64, rounded once; "f32": accumulated in f32 tap by tap, every product and sum rounded"""
    if _check_sums(sums):
        h, x = np.asarray(h, np.float32), np.ascontiguousarray(x, dtype=np.float32)
        xp = np.concatenate([np.zeros(h.size - 1, np.float32), x])
        y = np.zeros(x.size, np.float32)
        for k in range(h.size):
            y = y + h[k] * xp[h.size - 1 - k: h.size - 1 - k + x.size]
    else:
        y = np.convolve(x.astype(np.float64), h.astype(np.float64))[: x.size].astype(np.float32)
    return y * scale


def front(x, P, sums="f64"):
    """x [n] F32 -> p [n] CF32 (pilot branch), s [n] (wire), lpr [n]"""
    x = np.asarray(x, dtype=np.float32)
    xm = O.Nco(P["ncoF"]).mix_down(x.astype(np.complex64))
    z = (_fir(P["hp"], xm.real, P["sp"], sums) + 1j * _fir(P["hp"], xm.imag, P["sp"], sums)).astype(np.complex64)
    p = O.Nco(P["ncoF"]).mix_up(z)
    s = np.concatenate([np.zeros(P["d"], np.float32), x])[: x.size]
    return p, s, _fir(P["ha"], s, P["sa"], sums)


def pll(p, s, P, theta=None, dtheta=None, sums="f64"):
    """pllStep over [R][n] (or [n]) streams -> u, and the end words (theta, d_theta) per stream; sums="f32" takes every cos and
    sin from libm's cosf / sinf instead of f64 rounded once"""
    cos_, sin_ = (_cosf, _sinf) if _check_sums(sums) else (_cos, _sin)
    p, s = np.atleast_2d(p), np.atleast_2d(s).astype(np.float32)
    R, n = p.shape
    th = np.zeros(R, np.uint32) if theta is None else np.asarray(theta, np.uint32).copy()
    dth = np.full(R, P["d_nco"], np.uint32) if dtheta is None else np.asarray(dtheta, np.uint32).copy()
    pr, pi = p.real.astype(np.float32), p.imag.astype(np.float32)
    u = np.empty((R, n), np.float32)
    alpha, beta = P["alpha"], P["beta"]
    for t in range(n):
        phi = phase(th)
        th_ss = constrain(f32(2) * phi)                       # ncoSS set_phase (2 phi)
        cs, sn = cos_(phi), sin_(phi)                         # ncoPE cexpf
        nsn = -sn
        re = pr[:, t] * cs - pi[:, t] * nsn                   # p * conjugate c  (Haskell's Complex (*))
        im = pr[:, t] * nsn + pi[:, t] * cs
        e = hs_atan2(im, re)
        dth = dth + constrain(e * alpha)                      # nco_crcf_pll_step: adjust_frequency, adjust_phase
        th = th + constrain(e * beta)
        th = th + dth                                         # nco_crcf_step
        u[:, t] = s[:, t] * cos_(phase(th_ss))                # Re mix_block_down ncoSS (s + 0j)
    return u, th, dth


def back(u, lpr, P, sums="f64"):
    lmr = f32(2) * _fir(P["ha"], u, P["sa"], sums)
    return lpr + lmr, lpr - lmr


def decimate_calls(y, calls, decim):
    """firDecimator decim over per-call slices of a continuous row: each call consumes floor(n / decim) decim samples"""
    fd = O.FirDecim(decim)
    out, pos = [], 0
    for n in calls:
        k = n // decim * decim
        out.append(fd.execute_block(y[pos: pos + k]))
        pos += n
    return np.concatenate(out) if out else np.zeros(0, np.float32)


def _tail(L, R, P, calls):
    """L, R -> O.Butter2 -> the per-call decimator -> interleaved L, R, and the de-emphasised planes"""
    L = O.Butter2(P["deemph_fc"]).execute_block(L)
    R = O.Butter2(P["deemph_fc"]).execute_block(R)
    Ld, Rd = decimate_calls(L, calls, P["decim"]), decimate_calls(R, calls, P["decim"])
    lr = np.empty(2 * Ld.size, np.float32)
    lr[0::2], lr[1::2] = Ld, Rd
    return lr, L, R


def decode(x, q, decim=4, calls=None, sums="f64"):
    """one stream: MPX x -> interleaved L, R as the library returns them over `calls` (sample counts per call; default one
    call), plus the PLL end words and the intermediate planes.  sums="f32" is the rounding variant: the FIR sums accumulated in
    f32 and the PLL's cos / sin from libm's cosf / sinf.  It is no better a reference than the default; the distance between the
    two measures how far the decoder's output moves under rounding alone (tests/fms_cases.py)"""
    P = design(q, decim)
    x = np.asarray(x, dtype=np.float32)
    calls = [x.size] if calls is None else list(calls)
    assert sum(calls) == x.size
    p, s, lpr = front(x, P, sums)
    u, th, dth = pll(p, s, P, sums=sums)
    L, R = back(u[0], lpr, P, sums)
    lr, L, R = _tail(L, R, P, calls)
    return lr, dict(theta=int(th[0]), dtheta=int(dth[0]), L=L, R=R, u=u[0], p=p, lpr=lpr, P=P)


def decode_rows(X, q, decim=4, calls=None, sums="f64"):
    """[R][n] streams fed in `calls` (default one call; the PLL vectorised over the rows) -> [R][2 sum(c // decim for c in calls)],
    and the PLL end words per row.  Each row is decode's of that row, bit for bit"""
    P = design(q, decim)
    X = np.asarray(X, dtype=np.float32)
    calls = [X.shape[1]] if calls is None else list(calls)
    assert sum(calls) == X.shape[1]
    fr = [front(x, P, sums) for x in X]
    u, th, dth = pll(np.stack([f[0] for f in fr]), np.stack([f[1] for f in fr]), P, sums=sums)
    out = [_tail(*back(u[r], fr[r][2], P, sums), P, calls)[0] for r in range(X.shape[0])]
    return np.stack(out), th, dth


# ---- synthetic stereo broadcasts -----------------------------------------------------------------------------------------
def stereo_mpx(n, q, fl=1000.0, fr=3000.0, pilot_offset_hz=0.0, seed=0, pilot=True):
    """MPX = 0.45 (L + R) + 0.1 cos(pilot) + 0.45 (L - R) cos(2 pilot), L a tone at fl, R a tone at fr; random pilot phase"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / q
    L, R = np.cos(2 * np.pi * fl * t), np.cos(2 * np.pi * fr * t)
    ph = 2 * np.pi * (19000.0 + pilot_offset_hz) * t + rng.uniform(0, 2 * np.pi)
    m = 0.45 * (L + R) + (0.1 * np.cos(ph) + 0.45 * (L - R) * np.cos(2 * ph) if pilot else 0.0)
    return m.astype(np.float32)


def stereo_broadcast(n, q, kf=0.8, snr_db=40.0, **kw):
    """the MPX frequency-modulated for fmDemodulator kf (phase step 2 pi kf g m per sample, g = 0.25 keeps the peak step below
    pi, so freqdem returns g m) plus white noise at snr_db; CF32"""
    m = stereo_mpx(n, q, **kw).astype(np.float64)
    rng = np.random.default_rng(kw.get("seed", 0) + 1)
    ph = np.cumsum(2 * np.pi * kf * m * 0.25)          # 0.25: peak deviation below half the sample rate
    x = np.exp(1j * ph)
    sig = 10 ** (-snr_db / 20) / np.sqrt(2)
    x = x + sig * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return x.astype(np.complex64), m


def tone_db(y, f, rate):
    """power of y at frequency f relative to its total power, dB (Hann window)"""
    y = np.asarray(y, np.float64)
    w = np.hanning(y.size)
    Y = np.abs(np.fft.rfft(y * w)) ** 2
    k = int(round(f * y.size / rate))
    band = Y[max(k - 3, 0): k + 4].sum()
    return 10 * np.log10(band / Y.sum())


def tone_power(y, f, rate):
    y = np.asarray(y, np.float64)
    w = np.hanning(y.size)
    Y = np.abs(np.fft.rfft(y * w)) ** 2
    k = int(round(f * y.size / rate))
    return Y[max(k - 3, 0): k + 4].sum()
