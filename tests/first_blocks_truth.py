"""f64 references and seeded fixtures for the nine first-generation block Pipes (dcBlocker, mixDown / mixUp,
automaticGainControl, fmDemodulator, iirFilter, firDecimator, resampler, amDemodulator): DESIGN.md 4.6 / 4.8.

Every reference is the block's defining formula in plain numpy / scipy f64 on the F32 inputs (and on the F32 coefficients
the block publishes), so that the HIP kernel and the sequential F32 oracle can both be measured against the same truth:
    e_gpu <= 2 * e_orc + eps * max|truth|
test_first_blocks_cpu.py holds these references to the oracle; test_first_blocks_gpu.py holds the kernels to them."""
import numpy as np
from scipy.signal import lfilter

f32 = np.float32
U24 = 2.0 ** -24            # unit roundoff of F32 (half an ulp of 1)


def split(x, sizes):
    """x cut along its last axis into consecutive calls of `sizes` samples (contiguous copies)"""
    assert sum(sizes) == x.shape[-1], (sum(sizes), x.shape)
    out, pos = [], 0
    for s in sizes:
        out.append(np.ascontiguousarray(x[..., pos:pos + s]))
        pos += s
    return out


def cgauss(rng, shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2)


# --------------------------------------------------------------------------- dcBlocker
DC_SIZES = [524288, 524289, 600001, 1048576]     # 256 blocks of 2048 = 524 288: one more sample is block 257 (K = 2 per thread)
DC_ALPHAS = [0.0005, 5e-5]                       # the reference's value and the longest memory of test_chain_params_gpu.ALPHAS
DC_TAIL = 1000                                   # a second call: the state the long call left behind


def dc_input(n, seed=31):
    """strong DC (the state sits at DC / alpha), two tones and noise"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = (0.3 + 0.2j) + 0.4 * np.exp(2j * np.pi * 0.0137 * t) + 0.1 * np.exp(-2j * np.pi * 0.31 * t) + 0.05 * cgauss(rng, n)
    return x.astype(np.complex64)


def dc_truth(x, alpha):
    """y = v[n] - v[n-1], v[n] = x[n] + beta v[n-1] with the F32 beta = 1 - alpha, in f64"""
    beta = float(f32(1) - f32(alpha))
    return lfilter([1.0, -1.0], [1.0, -beta], np.asarray(x).astype(np.complex128))


# --------------------------------------------------------------------------- mixDown / mixUp
NCO_N = 1 << 20                                  # one call of dcBlocker's / mixDown's default max_samples
NCO_RAGGED = [1, 2047, 2048, 2049]               # + the rest; 2048 = samples per workgroup of k_dc_apply


def nco_input(seed=41):
    rng = np.random.default_rng(seed)
    t = np.arange(NCO_N)
    x = (0.6 + 0.3 * np.sin(2 * np.pi * t / 5003.0)) * np.exp(2j * np.pi * 0.07 * t) + 0.1 * cgauss(rng, NCO_N)
    return x.astype(np.complex64)


def nco_phase32(theta0, d_theta, n):
    """the kernel's own phase: theta_i = theta0 + i d_theta (mod 2^32), rounded to F32, times 2 pi / 2^32 in f64, rounded to F32"""
    theta = (np.uint64(theta0) + np.arange(n, dtype=np.uint64) * np.uint64(d_theta)) & np.uint64(0xFFFFFFFF)
    th32 = theta.astype(np.uint32).astype(f32)
    return (6.283185307179586 * th32.astype(np.float64) / 4294967296.0).astype(f32)


def nco_truth(x, d_theta, up, theta0=0):
    """x * exp(+-j ph) in f64 at the F32 phase nco_phase32 (up: +, down: -)"""
    ph = nco_phase32(theta0, d_theta, x.size).astype(np.float64)
    return np.asarray(x).astype(np.complex128) * np.exp((1j if up else -1j) * ph)


def nco_bound(x):
    """per-sample bound on |y - truth| for y = x * (c +- j s) in F32.
    c, s = sincosf(ph): 2 ulp each, and an ulp of a value below 1 is at most 2^-24 = U24 -> (|xr| + |xi|) * 2 U24 per component;
    the product xr c - xi s: at most four roundings (two products, the sum, one more should the compiler split a contraction), each
    relative U24, of terms whose magnitudes sum to <= |xr| + |xi| -> (|xr| + |xi|) * 4 U24 per component.
    Two components: sqrt 2 of the per-component bound, 6 U24 (|xr| + |xi|)."""
    x = np.asarray(x)
    return np.sqrt(2.0) * (np.abs(x.real).astype(np.float64) + np.abs(x.imag)) * 6 * U24


# --------------------------------------------------------------------------- automaticGainControl
# six levels as in test_agc_matches_oracle_and_squelch_decisions, moved apart so that the threshold is 15 dB from the nearest
# (-60, -50.5 | -20, -10.5, 0, +9.5 dB): there -35 dB sits 4.5 dB under the 3e-2 rows
AGC_LEVELS = np.array([1e-3, 3e-3, 0.1, 0.3, 1.0, 3.0])
AGC_THR = -35.0
# (nchan, samples per call); 16 = samples per block of k_agc's 16-byte path, 64 = channels per workgroup
AGC_CASES = [
    (1, [1] * 20 + [15, 16, 17, 31, 32, 33, 2501]),
    (3, [1, 3, 17, 33, 2501, 999]),
    (65, [2501, 999]),
    (130, [17]),
]


def agc_levels(nchan):
    """row r takes level r mod 6; a single row takes the level that drops, three rows one closed, the dropping and one open row"""
    if nchan == 1:
        return np.array([2])
    if nchan == 3:
        return np.array([1, 2, 5])
    return np.arange(nchan) % 6


def agc_input(nchan, n, seed=4):
    """the construction of test_agc_matches_oracle_and_squelch_decisions: six levels, every row its own noise, the 0.1 rows drop by
    60 dB half-way (FALL / SIGNALLO / TIMEOUT)"""
    rng = np.random.default_rng(seed + nchan)
    lv = agc_levels(nchan)
    z = AGC_LEVELS[lv][:, None] * cgauss(rng, (nchan, n))
    z[lv == 2, n // 2:] *= 1e-3
    return z.astype(np.complex64)


def agc_level_margin_db(z, thr=AGC_THR):
    """smallest distance (dB) between the threshold and the RMS level of any row's halves"""
    h = z.shape[1] // 2
    lev = [10 * np.log10(np.mean(np.abs(part.astype(np.complex128)) ** 2, axis=1)) for part in (z[:, :h], z[:, h:]) if part.shape[1]]
    return float(np.min(np.abs(np.concatenate(lev) - thr)))


# --------------------------------------------------------------------------- fmDemodulator
FM_SHAPES = [(1, 1), (3, 1), (7, 37), (5, 255), (5, 256), (5, 257), (300, 3)]      # (nchan, samples per call); 256 = threads per workgroup
FM_KF = [0.05, 0.3, 1.0]
FM_CALLS = 3


def fm_input(nchan, n, seed=2):
    """Gaussian rows of different levels; a zeroed stretch in row 1 where the stream is long enough.  Returns (z, zeros) with zeros the
    slice of row 1 that was cleared (or None)"""
    rng = np.random.default_rng(seed + 1000 * nchan + n)
    z = (10.0 ** (-(np.arange(nchan) % 5) / 2.0))[:, None] * cgauss(rng, (nchan, n))
    zeros = None
    if nchan > 1 and n >= 100:
        zeros = slice(40, 60)
        z[1, zeros] = 0
    return z.astype(np.complex64), zeros


def fm_truth(z, kf):
    """angle(conj(r') r) / (2 pi kf) in f64 with r' = 0 in front of the stream and kf the F32 value.  Returns (m, |conj(r') r|)"""
    zd = np.asarray(z).astype(np.complex128)
    prev = np.concatenate([np.zeros(zd.shape[:-1] + (1,), np.complex128), zd[..., :-1]], axis=-1)
    p = np.conj(prev) * zd
    return np.angle(p) / (2 * np.pi * float(f32(kf))), np.abs(p)


def fm_mask(z, absp):
    """the existing rule: samples whose |conj(r') r| exceeds 1e-3 of the row's mean power"""
    pw = np.mean(np.abs(np.asarray(z).astype(np.complex128)) ** 2, axis=-1, keepdims=True)
    return absp > 1e-3 * pw


def fm_bound(kf):
    """|m - truth| modulo 1 / kf.
    angle: fm_common.h states the polynomial's fit error 6e-9 rad and its evaluation error <= 1.2e-7 rad; the two products
    re = fma(a, c, b d), im = fma(a, d, -(b c)) carry two roundings each of terms that sum to <= |r'||r| = |conj(r') r| exactly, so
    each component is off by <= 2 U24 |p| and the angle by <= sqrt 2 * 2 U24 = 1.69e-7 rad whatever the cancellation.
    times ref = 1 / (2 pi kf).  ref is itself an F32 constant (relative U24) and the product with it rounds once more (half an ulp
    of the output): with |m| <= 1 / (2 kf) that is U24 / (2 kf) + U24 * 2^floor(log2(1 / (2 kf)))."""
    ref = 1.0 / (2 * np.pi * float(f32(kf)))
    out_max = 0.5 / float(f32(kf))
    half_ulp = U24 * 2.0 ** np.floor(np.log2(out_max))
    return (6e-9 + 1.2e-7 + np.sqrt(2.0) * 2 * U24) * ref + U24 * out_max + half_ulp


# --------------------------------------------------------------------------- iirFilter
IIR_FC = [0.0005, 0.0021, 0.025, 0.25, 0.45]
IIR_SIZES = [1, 15, 16, 17, 4095, 4096, 4097, 8191, 8193]       # 16 = samples per thread, 4096 = per chunk of k_biquad


def real_rows(nchan, n, seed):
    """real rows that differ in level and content: a row's own tone + its own noise"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    rows = [(1.0 + 0.7 * r) * (np.sin(2 * np.pi * (0.01 + 0.003 * r) * t + r) + 0.3 * rng.standard_normal(n)) + 0.1 * r for r in range(nchan)]
    return np.stack(rows).astype(f32)


def iir_truth(b, a, x):
    """lfilter of the oracle's F32 coefficients in f64, along the last axis"""
    return lfilter(np.asarray(b, np.float64), np.asarray(a, np.float64), np.asarray(x).astype(np.float64), axis=-1)


# --------------------------------------------------------------------------- firDecimator
FIRDECIM_M = [1, 2, 3, 5, 8, 16, 64]


def firdecim_sizes(m):
    """m, 2m: one and two outputs; 255m, 256m, 257m: around the 256 outputs of one workgroup; 3m < 20m: a call shorter than the
    history of 20m samples, then a long one"""
    return [m, 2 * m, 255 * m, 256 * m, 257 * m, 3 * m, 300 * m]


def firdecim_truth(h, x, m):
    """y[j] = sum_i h[i] x[jm - i] in f64 (x[t < 0] = 0), and the same sum of magnitudes.  Last axis."""
    h = np.asarray(h).astype(np.float64)
    x = np.atleast_2d(np.asarray(x).astype(np.float64))
    no = x.shape[-1] // m
    y = np.stack([np.convolve(r, h)[:no * m:m] for r in x])
    mag = np.stack([np.convolve(np.abs(r), np.abs(h))[:no * m:m] for r in x])
    return y, mag


# --------------------------------------------------------------------------- resampler
RESAMP_RATES = [2.0, 1.0, 0.999, 0.5, 0.4999, 0.25, 0.125, 0.01, 0.001]
RESAMP_STAGES = [0, 0, 0, 0, 1, 1, 2, 6, 9]          # half-band decimators design_msresamp puts in front of the arbitrary stage
RESAMP_AS = [(0.3, 40.0), (0.3, 80.0)]
RESAMP_N = 200000
RESAMP_MAX = 65536


def resamp_input(rate, seed=11):
    """two tones inside the output band + noise (test_resampler_pipe_matches_oracle_across_chunks, peak above 1)"""
    rng = np.random.default_rng(seed)
    t = np.arange(RESAMP_N)
    r = min(rate, 1.0)
    x = 0.8 * np.exp(2j * np.pi * 0.11 * r * t) + 0.3 * np.exp(-2j * np.pi * 0.31 * r * t) + 0.07 * cgauss(rng, RESAMP_N)
    return x.astype(np.complex64)


def resamp_splits(rate):
    """two ways to cut the same 200 000 samples: (a) twenty calls of one sample, odd sizes, one call of exactly max_samples;
    (b) at rate 0.001, 300 calls of 100 samples (one output per 1000: most return nothing), then odd pieces"""
    a = [1] * 20 + [3, 17, 255, 1023, 4097, 50001, RESAMP_MAX]
    rest = RESAMP_N - sum(a)
    a += [rest // 2 + 1, rest - rest // 2 - 1]
    b = [100] * 300 if rate == 0.001 else []
    rest = RESAMP_N - sum(b)
    while rest > 0:
        s = min(rest, 60001)
        b.append(s)
        rest -= s
    assert sum(a) == sum(b) == RESAMP_N and max(a + b) <= RESAMP_MAX
    return a, b


# --------------------------------------------------------------------------- amDemodulator
AM_SIZES = [1, 15, 16, 17, 2047, 2048, 2049, 4095, 4096, 4097] + [1] * 50     # 16 = samples per thread, 2048 = per workgroup of k_am
AM_N = sum(AM_SIZES)
# the call of 4096 samples starts at sample 10288; its second workgroup starts 2048 later and warms up over the 2048 samples before
AM_CALL0 = sum(AM_SIZES[:8])
AM_DROP = AM_CALL0 + 2048 - 100
AM_ALPHA = float(f32(0.01))
AM_BETA = float(f32(1) - f32(0.01))


def am_input(nchan, seed=5):
    """AM rows of different carrier level, envelope and noise; the drop row (the only row of one, row 1 of three) falls by 60 dB
    100 samples before the second workgroup of the 4096-sample call begins.  Returns (x, drop_row)"""
    rng = np.random.default_rng(seed + nchan)
    t = np.arange(AM_N)
    rows = []
    for r in range(nchan):
        env = 1.0 + 0.6 * np.sin(2 * np.pi * t / (97.0 + 10 * r)) + 0.2 * np.sin(2 * np.pi * t / 23.0 + r)
        rows.append((0.4 + 0.3 * r) * env * np.exp(1j * ((0.21 + 0.05 * r) * t + 0.5)) + 0.01 * (r + 1) * cgauss(rng, AM_N))
    x = np.stack(rows)
    drop_row = 0 if nchan == 1 else 1
    x[drop_row, AM_DROP:] *= 1e-3
    return x.astype(np.complex64), drop_row


def am_truth(x):
    """t = |y| (f64 hypot of the F32 parts); q_hat <- alpha t + (1 - alpha) q_hat with the F32 alpha and 1 - alpha; 2 (t - q_hat).
    Returns (out, q_hat)"""
    x = np.asarray(x)
    t = np.hypot(x.real.astype(np.float64), x.imag.astype(np.float64))
    q = lfilter([AM_ALPHA], [1.0, -AM_BETA], t, axis=-1)
    return 2.0 * (t - q), q
