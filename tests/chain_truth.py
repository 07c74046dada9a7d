"""The chain up to FM, restated in numpy f64: DC blocker -> pre-mix -> polyphase branches -> DFT -> freqdem.

Conventions, all taken from oracle/csdr_oracle.c (the restatement shares no code with it):
  DC blocker   y = lfilter([1, -1], [1, -beta]), beta = f32(1) - f32(alpha) (orc_dcblock_create: a1 = -1 + alpha in f32)
  pre-mix      x_n * conj(v_n), v_n = exp(j ph_n), ph_n = f32(2 pi f32(theta_n) / 2^32), theta_n = n * dtheta mod 2^32,
               dtheta = nco_constrain(pfb_offset(M)): the phase words and their f32 phase are the contract; cos / sin in f64
  branches     X_f[j] = sum_n h[M - 1 - j + n M] d[(f - n) M + j], n = 0 .. p - 1, with the oracle's f32 taps h and zeros before the start
               (orc_pfb_analyzer_execute: sample i of a frame goes to window M - 1 - i, branch i lands in X[M - 1 - i])
  DFT          forward, unnormalised, per frame (numpy.fft.fft)
  freqdem      m_t = ref * arg(conj(r_{t-1}) r_t), r_{-1} = 0, ref = f32(1 / (2 pi kf)): the f32 value is the library's and the
               oracle's constant, so its rounding is part of the contract and not of anybody's error
M = 1 has no channelizer: the (DC-blocked) stream is the one channel.

Also here, shared by test_chain_truth_cpu.py and test_fm_phase_routes_gpu.py: the white-noise fixture, the bounds of the FM
comparison (per sample and per octant), and f32 emulations of the library's two arctangent polynomials."""
import numpy as np

import oracle_lib as O

TWO_PI = 2.0 * np.pi
U = 2.0 ** -24                       # half an ulp, relative: the rounding error of one f32 operation
WARM = 13                            # frames 0 .. p - 2 fill the 14-frame window (p = 2 m = 14)


def ref32(kf):
    """freqdem's scale as the library and the oracle hold it: one f32"""
    return float(np.float32(1.0 / (TWO_PI * float(np.float32(kf)))))


def beta_of(alpha):
    return float(np.float32(1) - np.float32(alpha))


def dc_block(x, alpha):
    from scipy.signal import lfilter
    return lfilter([1.0, -1.0], [1.0, -beta_of(alpha)], np.asarray(x, np.complex128))


def channelize(x, M, m=7, As=80.0):
    """pre-mix + analysis bank of x (complex128, whole frames) -> [M][nf] complex128"""
    x = np.asarray(x, np.complex128)
    if M == 1:
        return x.reshape(1, -1).copy()
    assert x.size % M == 0
    nf, p = x.size // M, 2 * m
    dtheta = O.nco_constrain(O.pfb_offset(M))
    theta = (np.arange(x.size, dtype=np.uint64) * np.uint64(dtheta)) & np.uint64(0xFFFFFFFF)
    ph = (TWO_PI * theta.astype(np.float32).astype(np.float64) / 2.0 ** 32).astype(np.float32).astype(np.float64)
    d = (x * (np.cos(ph) - 1j * np.sin(ph))).reshape(nf, M)
    h = O.Pfb(M, m, As).taps.astype(np.float64)
    H = h.reshape(p, M)[:, ::-1]                                     # H[n, j] = h[M - 1 - j + n M]
    dp = np.concatenate([np.zeros((p - 1, M), np.complex128), d])
    X = np.zeros((nf, M), np.complex128)
    for n in range(p):
        X += H[n] * dp[p - 1 - n:p - 1 - n + nf]
    return np.ascontiguousarray(np.fft.fft(X, axis=1).T)


def fm_angle(r):
    """arg(conj(r_{t-1}) r_t) per row, r_{-1} = 0; numpy's arctan2 follows IEEE on signed zeros as cargf does"""
    rp = np.concatenate([np.zeros((r.shape[0], 1), r.dtype), r[:, :-1]], axis=1)
    q = np.conj(rp) * r
    return np.arctan2(q.imag, q.real)


def chain_truth(x, M, dc=True, alpha=0.0005, kf=0.3, m=7, As=80.0):
    """x: complex samples (whole frames) -> (r [M][nf] complex128, fm [M][nf] float64)"""
    y = dc_block(x, alpha) if dc else np.asarray(x, np.complex128)
    r = channelize(y, M, m, As)
    return r, fm_angle(r) * ref32(kf)


# --------------------------------------------------------------------------- fixture
def noise(M, nf, seed=None, offset=0.0):
    """complex white Gaussian noise, sigma = 0.5, zero mean: every channel equally strong, the phase advance uniform on (-pi, pi].
    offset: a constant added to every sample (in f64, rounded to f32 with the sum): the DC the blocker has to take out"""
    g = np.random.Generator(np.random.PCG64(7 + M if seed is None else seed))
    z = g.standard_normal((M * nf, 2)) * (0.5 / np.sqrt(2.0))
    return (z[:, 0] + 1j * z[:, 1] + complex(offset)).astype(np.complex64)


def dc_rows(M, m=7, As=80.0):
    """the four channels a DC offset lands in (pre-mix by the PFB offset)"""
    if M == 1:
        return np.array([0])
    y = O.Chain(M, dc_block=False, pfb_m=m, pfb_as=As).process(np.ones(M * (2 * m + 4), np.complex64))
    return np.sort(np.argsort(np.abs(y[:, -1]))[-4:])


def prev(a):
    return np.concatenate([np.zeros((a.shape[0], 1), a.dtype), a[:, :-1]], axis=1)


def counted(M, nf):
    """frames that are compared: behind the window fill (frame 0 at M = 1: r' = 0 there)"""
    c = np.zeros(nf, bool)
    c[(WARM + 1 if M > 1 else 1):] = True
    return c


def kept(r, M):
    """counted samples with min(|r_t|, |r_{t-1}|) > 0.1 rms(r): the ones whose angle the octant statistics use"""
    a = np.abs(r)
    c = counted(M, r.shape[1])
    rms = np.sqrt(np.mean(a[:, c] ** 2))
    return (np.minimum(a, prev(a)) > 0.1 * rms) & c[None, :]


def octant(angle):
    """0 .. 7 for (-pi, -3pi/4], ... , (3pi/4, pi]"""
    return np.clip(np.floor((angle + np.pi) / (np.pi / 4)).astype(np.int64), 0, 7)


def fm_err(got, truth, kf):
    """signed error modulo 1/kf (+ref pi and -ref pi are the same angle)"""
    per = 1.0 / kf
    return (np.asarray(got, np.float64) - truth + per / 2) % per - per / 2


def sample_bound(r, E, phi, kf):
    """(a): |d_t| <= ref (2 (E / |r_t| + E / |r_{t-1}|) + phi).  A channel sample off by at most E turns its direction by at most
    asin(E / |r|) <= (pi / 2) E / |r|; the factor 2 also covers an FM instantiation that rounds its samples unlike the CF32 one."""
    a = np.abs(r)
    with np.errstate(divide="ignore", invalid="ignore"):        # E = 0 against r = 0: nan, a sample nobody compares
        return ref32(kf) * (2.0 * (E / a + E / prev(a)) + phi)


def octant_bias(d, angle, mask):
    """mean signed error of the masked samples per octant of the true angle, and the counts"""
    o = octant(angle)
    return (np.array([d[mask & (o == k)].mean() if (mask & (o == k)).any() else 0.0 for k in range(8)]),
            np.array([int((mask & (o == k)).sum()) for k in range(8)]))


def bias_bound(orc_bias, kf):
    """(b): twice the oracle's worst octant bias plus one evaluation error of the polynomial (1.2e-7 rad: systematic by design)"""
    return 2.0 * float(np.abs(orc_bias).max()) + ref32(kf) * 1.2e-7


# --------------------------------------------------------------------------- phi: the phase functions' own error, in radians
def _hulp(v):
    """half an f32 ulp at |v| (normal range)"""
    return 2.0 ** (np.floor(np.log2(abs(v))) - 24)


F32_PI_ERR = abs(float(np.float32(np.pi)) - np.pi)            # 8.74e-8
F32_HP_ERR = abs(float(np.float32(np.pi / 2)) - np.pi / 2)    # 4.37e-8


def _const_err(c, ref):
    """what f32(f32(c) * ref) misses c ref by, as an angle: both roundings of a pre-scaled fold constant, exactly"""
    return abs(float(np.float32(np.float32(c) * np.float32(ref))) - c * ref) / ref


def phi15(kf):
    """scaled_atan2f / fm_sample / fm_quad (degree 15, hp and pi pre-multiplied by ref), term by term in radians:
      products     re = fma(x', x, rnd(y' y)), im alike.  The inner products' errors are a vector of length <= U |y'| |r|, the two final
                   roundings one of length <= U |q|: <= 2 U |q| together, an angle of 2 U                               1.19e-7
      a            v_rcp_f32 is good to 1 ulp (2 U relative), the product mn * rcp adds U: 3 U relative on a, and
                   d atan(a) = a / (1 + a^2) (da / a) <= 1/2 (da / a)                                                    0.89e-7
      polynomial   fit 4.7e-8 + Horner evaluation in f32 (z = a a, eight fma): 1.2e-7 in all                            1.20e-7
      scalings     a * ref and p * (a ref): U relative each on t <= pi / 4                                              0.94e-7
      hp, pi       f32(f32(pi / 2) ref) and f32(f32(pi) ref) against ref pi / 2 and ref pi: the two roundings of each, taken exactly
                   for this ref (at most 4.37e-8 + half an ulp at ref pi / 2, and 8.74e-8 + half an ulp at ref pi)
      hp - t       rounds to at most half an ulp at ref pi / 2 (the result is <= ref pi / 2)
      pi - t       rounds to at most half an ulp at ref pi
    The half ulps are absolute, so they depend on where ref pi sits in its binade (1.67 at kf = 0.3, 10.0 at kf = 0.05): 7.6e-7 rad
    in all at kf = 0.3, 7.5e-7 at kf = 0.05.  copysign is exact."""
    ref = ref32(kf)
    consts = _const_err(np.pi / 2, ref) + _const_err(np.pi, ref)
    folds = (_hulp(ref * np.pi / 2) + _hulp(ref * np.pi)) / ref
    return 2 * U + 1.5 * U + 1.2e-7 + 2 * U * np.pi / 4 + consts + folds


def phi17(kf=None):
    """fast_atan2f and atan2f_rn (degree 17, folds in radians, ref applied last), term by term in radians:
      products 2 U and a 1.5 U as in phi15                                                                              2.09e-7
      polynomial   fit 2.5e-8 + Horner evaluation in f32 (nine fma): 9.5e-8 in all                                      0.95e-7
      p * a        U relative on t <= pi / 4 (atan2f_rn's upper octant is one fma: no more than this)                  0.47e-7
      hp, hp - t   4.37e-8 + half an ulp at pi / 2 (2^-24)                                                              1.03e-7
      pi, pi - t   8.74e-8 + half an ulp at pi (2^-23)                                                                  2.07e-7
      * ref        U relative on an angle <= pi                                                                         1.87e-7
    The 2^90 rescue of atan2f_rn is exact (a power of two on both factors).  No dependence on kf."""
    return 2 * U + 1.5 * U + 9.5e-8 + U * np.pi / 4 + F32_HP_ERR + 2.0 ** -24 + F32_PI_ERR + 2.0 ** -23 + U * np.pi


# --------------------------------------------------------------------------- shared references and the three FM assertions
KF = 0.3
ALPHA = 0.0005
# every (M, frames) a case of test_fm_phase_routes_gpu.py or of fused_cases.py runs on (both assert membership); the noise stream of an
# M is drawn once, at its largest frame count, and the shorter shapes are its prefixes
SHAPES = [(1, 42345), (7, 3333), (20, 533), (64, 3141), (64, 14341), (256, 405), (256, 6277), (1024, 2053), (1024, 3077), (4096, 49)]
_C = {}


def refs_of(x, M, dc, kf=KF, alpha=ALPHA):
    """truth and oracle of one input: dict(x, r, fm, angle, orc_r, orc_fm, kept, counted)"""
    r, fm = chain_truth(x, M, dc=dc, alpha=alpha, kf=kf)
    kw = dict(dc_block=dc, dc_alpha=alpha)
    return dict(x=x, r=r, fm=fm, angle=fm / ref32(kf), kept=kept(r, M), counted=np.broadcast_to(counted(M, r.shape[1]), r.shape),
                orc_r=O.Chain(M, **kw).process(x), orc_fm=O.Chain(M, demod="fm", kf=kf, **kw).process(x))


def refs(M, nf, dc, kf=KF, alpha=ALPHA, offset=0.0):
    """refs_of the noise stream's first nf frames (plus the constant `offset`), computed once (the cache holds one M at a time: the
    cases of a file come M by M)"""
    key = (M, nf, dc, kf, alpha, complex(offset))
    if key not in _C:
        if any(k[0] != M for k in _C):
            _C.clear()
        _C[key] = refs_of(noise(M, max(n for m, n in SHAPES if m == M), offset=offset)[:M * nf], M, dc, kf, alpha)
    return _C[key]


def check_fm(tag, got, R, E, phi, kf=KF, orc_bias=None, mask=None, sane=True):
    """(a), (b), (c) of test_fm_phase_routes_gpu.py on one FM output; returns (worst ratio of (a), the eight biases, bound of (b)).
    mask: the samples (a) covers (default: the counted ones with r, r' != 0)"""
    ref = ref32(kf)
    got = np.asarray(got)
    assert got.shape == R["fm"].shape, (tag, got.shape, R["fm"].shape)
    if sane:                                                         # (c); the mutation checks switch it off to see (a) and (b) fail
        assert np.isfinite(got).all(), f"{tag}: non-finite output"
        assert np.abs(got).max() <= ref * np.pi * (1 + 2.0 ** -22), (tag, float(np.abs(got).max()))
    d = fm_err(got, R["fm"], kf)
    a = np.abs(R["r"])
    m = (R["counted"] & (a > 0) & (prev(a) > 0)) if mask is None else mask
    ratio = np.abs(d[m]) / sample_bound(R["r"], E, phi, kf)[m]
    worst = float(ratio.max()) if ratio.size else 0.0
    bias, cnt = octant_bias(d, R["angle"], R["kept"] if mask is None else (R["kept"] & mask))
    if orc_bias is None:
        orc_bias, _ = octant_bias(fm_err(R["orc_fm"], R["fm"], kf), R["angle"], R["kept"])
    bb = bias_bound(orc_bias, kf)
    print(f"{tag}: E {E:.3e}  worst (a) ratio {worst:.3f}  octant bias " + " ".join(f"{b:+.1e}" for b in bias) + f"  (bound {bb:.2e})")
    return worst, bias, bb


def cf32_E(R):
    return float(np.abs(R["orc_r"].astype(np.complex128) - R["r"]).max())


# --------------------------------------------------------------------------- f32 emulations of the two polynomials
C15 = np.array([9.999993443e-01, -3.332985938e-01, 1.994656026e-01, -1.390860826e-01,
                9.642146528e-02, -5.591168255e-02, 2.186254039e-02, -4.054457881e-03], np.float32)
C17 = np.array([9.999998808e-01, -3.333259821e-01, 1.998590529e-01, -1.416121870e-01, 1.049891263e-01,
                -7.234797627e-02, 3.978060186e-02, -1.440101303e-02, 2.456645248e-03], np.float32)


def _fma(a, b, c):
    """f32 fma through f64: the product of two f32 is exact in f64; the sum rounds twice (f64, then f32), which differs from a
    true fma in about one case in 2^29: good enough for error statistics"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _rcp(x):
    return (1.0 / x.astype(np.float64)).astype(np.float32)


def _conj_mul(rp, r):
    rp, r = np.asarray(rp, np.complex64), np.asarray(r, np.complex64)
    re = _fma(rp.real, r.real, rp.imag * r.imag)
    im = _fma(rp.real, r.imag, -(rp.imag * r.real))
    return re, im


def emu_fm15(rp, r, kf, hp_rel=0.0, pi_rel=0.0):
    """fm_sample of csrc/fused_v2_common.h (= scaled_atan2f on the same products); hp_rel / pi_rel put a relative error on a fold
    constant, for the mutation checks"""
    ref = np.float32(ref32(kf))
    hp = np.float32(np.float32(np.pi / 2) * ref * np.float32(1.0 + hp_rel))
    pi = np.float32(np.float32(np.pi) * ref * np.float32(1.0 + pi_rel))
    re, im = _conj_mul(rp, r)
    mx = np.maximum(np.maximum(np.abs(re), np.abs(im)), np.float32(1e-37))
    mn = np.minimum(np.abs(re), np.abs(im))
    a = mn * _rcp(mx)
    z = a * a
    p = np.full_like(a, C15[7])
    for i in range(6, -1, -1):
        p = _fma(p, z, np.full_like(a, C15[i]))
    t = p * (a * ref)
    t = np.where(np.abs(im) > np.abs(re), hp - t, t)
    t = np.where(np.signbit(re), pi - t, t)
    return np.copysign(t, im)


def emu_fm17(rp, r, kf, hp_rel=0.0, pi_rel=0.0):
    """fm_sample_rn of csrc/fm_common.h (fast_atan2f differs in its upper octant: hp - rnd(p a) instead of one fma)"""
    ref = np.float32(ref32(kf))
    hp = np.float32(np.float32(np.pi / 2) * np.float32(1.0 + hp_rel))
    pi = np.float32(np.float32(np.pi) * np.float32(1.0 + pi_rel))
    re, im = _conj_mul(rp, r)
    ax, ay = np.abs(re), np.abs(im)
    mx, mn = np.maximum(ax, ay), np.minimum(ax, ay)
    sc = np.where(mx < np.float32(1e-30), np.float32(2.0 ** 90), np.float32(1.0)).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = (mn * sc) * _rcp(mx * sc)
    a = np.where(a == a, a, np.where(mx == 0, np.float32(0), np.float32(1))).astype(np.float32)
    z = a * a
    p = np.full_like(a, C17[8])
    for i in range(7, -1, -1):
        p = _fma(p, z, np.full_like(a, C17[i]))
    lo, hi = p * a, _fma(-p, a, np.full_like(a, hp))
    t = np.where(ay > ax, hi, lo)
    t = np.where(np.signbit(re), pi - t, t)
    return np.copysign(t, im) * ref
