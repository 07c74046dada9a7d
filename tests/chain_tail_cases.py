"""The AM and WBFM tails behind the chain handle (capi.hip chain_call: k_am; k_biquad + k_firdecim; launch_mix; the backward handle's row
reversal), per row: case table, truths, bounds and fixtures.  No GPU in here; shared by test_chain_tails_cpu.py (the oracle's own
decomposition, the truth functions, the table, six mutations) and test_chain_tails_gpu.py (the library under them).

Method: the freqdem's branch cut makes an end-to-end bound behind a low-pass useless, so the tail is isolated.  Every AM / WBFM handle
gets a TWIN of the same configuration whose output is the plane the tail reads: demod "none" for AM, demod "fm" with kf = 0.6 for WBFM
(csdr_chain_create sets eff.kf = 0.6f), always without --mix (eff.mix = 0).  Both get the same input in the same calls.
Truth: the tail restated in f64 on the twin's F32 rows, state carried over the whole stream and zero at its start:
  AM     first_blocks_truth.am_truth: t = |z|, q <- alpha t + (1 - alpha) q, 2 (t - q)
  WBFM   lfilter with O.Butter2(fc).coeffs, then y[j] = sum_i h[i] b[j decim - i] with O.FirDecim(decim).taps
  mix    the f64 sum of the rows;  backward: row k against twin row k (a backward twin is already reversed)
Yardstick: the oracle's F32 blocks (O.AmpDem; O.Butter2 + O.FirDecim) on the same twin rows, one set of objects per row over the stream.

Bounds, per row c, every sample: d_c = max_t |got - truth|, e_c = max_t |oracle - truth|, s_c = max_t |truth|
  AM     d_c <= 2 e_c + 2e-6 s_c + 0.99^2048 max_t q_c       (test_amdemodulator_chunks_rows_and_level_drop; the last term is k_am's
                                                              documented warm-up truncation, q from the f64 truth)
  WBFM   d_c <= 2 e_c + (5e-6 + 2e-6 sum|h_i|) b_c            (b_c = max_t |f64 biquad output|: test_firdecimator_every_m's term, and
                                                              test_iirfilter_chunks_rows_and_cutoffs' passed through the decimator)
  mix    per sample: the sum of the row bounds + (C - 1) 2^-24 sum_c |truth_c[t]|
A row whose bound is 0 (an all-zero plane row) must be reproduced exactly.

csdr_chain_path: the tails' texts follow the front's in the order csdr_chain_create appends them, "+dft-backward", "+am" | "+wbfm", then the
time-parallel AGC tail's "-spec" (fused fronts, whose text ends in "+agc") or "+agc-spec" (any-M): "fused-256|k_tile256<CF32>+agc+am-spec",
"generic+am+agc-spec".  The table therefore asks for "+agc", "-spec" and "+am" each on its own.

Fixtures: without the AGC chain_truth.noise (every row equally strong); with it keyed(): every third channel keyed on and off with
gaps of 200 .. 1500 frames around the squelch's 1000-sample time-out, so rows open, mute and time out inside the stream."""
from collections import namedtuple

import numpy as np
from scipy.signal import lfilter

import chain_truth as T
import first_blocks_truth as FB
import oracle_lib as O

U = 2.0 ** -24
KF_WB = 0.6
AM_TRUNC = 0.99 ** 2048
AGC_DB = 8.0                                   # the threshold of the keyed-signal AGC tests (test_agc_tail_is_bit_identical_to_sequential)


def agc_db(M):
    """the squelch threshold of the AGC cases.  A keyed carrier of keyed() comes out of the bank at 0.4 M / sqrt(M / 3): 9.8 dB at M = 20,
    14.9 at 64, 20.9 at 256, 26.9 at 1024, the noise rows at 0.028 sqrt(M), 30 dB and more below; at M = 8 the carrier has 5.8 dB and would
    never open a squelch at 8 dB, so the threshold is 2 dB there"""
    return 2.0 if M < 16 else AGC_DB

TM_KNOBS = {"CSDR_AGC_W": "512", "CSDR_AGC_L_TM": "688", "CSDR_RUN64_V2_ALL": "1", "CSDR_RUN_MIN_TILES": "1"}
TM_MIN = 2048                                  # 4 W: the shortest call agc_tail_tm_supported takes at W = 512


# --------------------------------------------------------------------------- designs and truths
_DES = {}


def design(fc, decim):
    """(b, a, h): the oracle's F32 biquad coefficients and decimator taps"""
    key = (float(np.float32(fc)), int(decim))
    if key not in _DES:
        b, a = O.Butter2(fc).coeffs
        _DES[key] = (b, a, O.FirDecim(decim).taps)
    return _DES[key]


def am_tail_truth(z):
    """(out, q_hat) [C][n] f64 of the CF32 rows z"""
    return FB.am_truth(np.atleast_2d(z))


def wbfm_tail_truth(f, fc, decim):
    """(y [C][n / decim], biquad output [C][n]) f64 of the F32 rows f"""
    b, a, h = design(fc, decim)
    f = np.atleast_2d(f)
    bq = lfilter(b.astype(np.float64), a.astype(np.float64), f.astype(np.float64), axis=-1)
    no = f.shape[1] // decim
    h64 = h.astype(np.float64)
    y = np.stack([np.convolve(r, h64)[:no * decim:decim] for r in bq]) if no else np.zeros((f.shape[0], 0))
    return y, bq


def am_tail_oracle(z):
    return np.stack([O.AmpDem().demodulate_block(r) for r in np.atleast_2d(z)])


def wbfm_tail_oracle(f, fc, decim):
    return np.stack([O.FirDecim(decim).execute_block(O.Butter2(fc).execute_block(r)) for r in np.atleast_2d(f)])


def fold32(rows):
    """the oracle's mix (orc_mix_f32): left fold over the rows in f32"""
    acc = rows[0].copy()
    for r in rows[1:]:
        acc = (acc + r).astype(np.float32)
    return acc


Ref = namedtuple("Ref", "truth orc bound")      # truth, orc [C][no]; bound [C]


def reference(demod, twin, fc=0.025, decim=4):
    """truth, oracle and row bounds of the tail behind the twin's rows"""
    twin = np.atleast_2d(twin)
    if demod == "am":
        assert twin.dtype == np.complex64, twin.dtype
        truth, q = am_tail_truth(twin)
        orc = am_tail_oracle(twin)
        e, s = np.abs(orc - truth).max(axis=1), np.abs(truth).max(axis=1)
        return Ref(truth, orc, 2 * e + 2e-6 * s + AM_TRUNC * q.max(axis=1))
    assert demod == "wbfm" and twin.dtype == np.float32, (demod, twin.dtype)
    truth, bq = wbfm_tail_truth(twin, fc, decim)
    orc = wbfm_tail_oracle(twin, fc, decim)
    h = design(fc, decim)[2]
    e = np.abs(orc - truth).max(axis=1)
    return Ref(truth, orc, 2 * e + (5e-6 + 2e-6 * float(np.abs(h.astype(np.float64)).sum())) * np.abs(bq).max(axis=1))


def _ratio(d, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(bound > 0, d / bound, np.where(d > 0, np.inf, 0.0))


def row_ratios(got, ref):
    """d_c / bound_c of every row"""
    got = np.atleast_2d(got)
    assert got.shape == ref.truth.shape, (got.shape, ref.truth.shape)
    return _ratio(np.abs(got.astype(np.float64) - ref.truth).max(axis=1), ref.bound)


def mix_ratios(got, ref):
    """per output sample of the mixed row: |got - sum_c truth_c| / (sum_c bound_c + (C - 1) U sum_c |truth_c[t]|)"""
    C = ref.truth.shape[0]
    assert got.shape == ref.truth.shape[1:], (got.shape, ref.truth.shape)
    bound = ref.bound.sum() + (C - 1) * U * np.abs(ref.truth).sum(axis=0)
    return _ratio(np.abs(got.astype(np.float64) - ref.truth.sum(axis=0)), bound)


def worst(got, ref, mixed):
    """(worst ratio, its row, or its output sample when mixing)"""
    r = mix_ratios(got, ref) if mixed else row_ratios(got, ref)
    if not r.size:
        return 0.0, 0
    i = int(np.argmax(r))
    return float(r[i]), i


# --------------------------------------------------------------------------- fixtures
_FIX = {}


def keyed(M, nf, seed=None):
    """_bursty's "bursts" signal (test_gpu_parity.py) built frame by frame: noise of 0.02 per component + every third channel a carrier
    of 0.4 / sqrt(M / 3) on its centre, keyed on and off with gaps of 200 .. 1500 frames, a slow phase wobble on top.  The carriers
    are constant over a frame, so one inverse DFT per frame places all of them: x[f M + j] = c[f M + j] sum_k A_k[f] e^(2 pi j k j / M),
    c[t] = e^(-j pi (M - 1) t / M) the offset of the channel centres (synth.channel_centre)"""
    rng = np.random.default_rng(4321 + M if seed is None else seed)
    n = M * nf
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.02
    A = np.zeros((nf, M), np.complex128)
    f = np.arange(nf)
    for k in range(1 if M > 1 else 0, M, 3):
        gate, pos, on = np.ones(nf), 0, bool(k & 1)
        while pos < nf:
            ln = int(rng.integers(200, 1500))
            gate[pos:pos + ln] = 1.0 if on else 0.0
            pos += ln
            on = not on
        A[:, k] = gate * (0.4 / np.sqrt(max(M, 3) / 3)) * np.exp(1j * (0.3 * np.sin(2 * np.pi * f / 50.0 + k) + 0.7 * k))
    t = np.arange(n, dtype=np.float64)
    x += np.exp(-1j * np.pi * (M - 1) / M * t) * (np.fft.ifft(A, axis=1) * M).reshape(-1)
    return x.astype(np.complex64)


def fixture(kind, M, nf):
    """the input of a case ("noise" | "keyed"); nobody writes into it"""
    key = (kind, M, nf)
    if key not in _FIX:
        if len(_FIX) > 3:
            _FIX.clear()
        _FIX[key] = T.noise(M, nf) if kind == "noise" else keyed(M, nf)
        _FIX[key].setflags(write=False)
    return _FIX[key]


# --------------------------------------------------------------------------- the case table
# id; group A .. E; M; demod "am" | "wbfm"; cs.Chain keywords besides demod (mix, agc, decim, deemph_fc, chan_*, dft_backward); flag names
# of composable_sdr_amd._lib (FLAG_QUIET | FLAG_TIME_KERNELS always); diagnostics knobs; calls in frames; max_frames; substrings of
# csdr_chain_path; substrings that must not be in it; per call a prefix of the timed kernel's name (None: no claim); the indices of
# the calls that take the tile-major AGC plane (None: no time-parallel AGC tail on the handle); fixture
Case = namedtuple("Case", "id group M demod kw flags knobs calls max_frames path nopath timed tm fix")


def _front(M, kind, agc=False):
    """(path substring, timed-kernel prefix) of the fused front of a whole-band handle without knobs, short calls; kind "CF32" | "FM"
    (with the AGC on every plan delivers CF32)"""
    k = "CF32" if agc else kind
    return {64: (f"fused-k_run64<{k}>", f"k_run64<{k}>"), 256: (f"fused-256|k_tile256<{k}>", f"k_tile256<{k}>"),
            1024: (f"fused-k_run1024v3<{k}>", None), 4096: (f"fused-4096|k_front4096+k_back4096<{k}>", f"k_front4096+k_back4096<{k}>")}[M]


def _case(id, group, M, demod, calls, kw=None, flags=(), knobs=None, max_frames=None, path=(), nopath=(), timed=None, tm=None, fix="noise"):
    kw = dict(kw or {})
    if demod == "wbfm":
        kw.setdefault("decim", 4)
        kw.setdefault("deemph_fc", 0.025)
    calls = list(calls)
    timed = list(timed) if isinstance(timed, (list, tuple)) else [timed] * len(calls)
    return Case(id, group, M, demod, kw, tuple(flags), dict(knobs or {}), calls, max_frames or max(calls), tuple(path) + (f"+{demod}",),
                tuple(nopath), timed, tm, fix)


def kind_of(demod):
    return "CF32" if demod == "am" else "FM"


def twin_kw(c):
    """cs.Chain keywords of the case's twin"""
    kw = {k: v for k, v in c.kw.items() if k not in ("mix", "decim", "deemph_fc")}
    kw.update(dict(demod="none") if c.demod == "am" else dict(demod="fm", kf=KF_WB))
    return kw


def rows_of(c):
    """channels the handle owns"""
    G = c.kw.get("chan_stride", 0)
    if G > 1:
        return c.M // G
    return c.kw.get("chan_count", 0) or c.M - c.kw.get("chan_first", 0)


def mixed(c):
    return bool(c.kw.get("mix")) and c.M > 1


def n_out(c, nf):
    """csdr_chain_process' *n_out of a call of nf frames"""
    no = nf // c.kw.get("decim", 1)
    return no if mixed(c) else rows_of(c) * no


def twin_key(c):
    """cases with the same key share their twin's output"""
    return (c.M, c.demod, tuple(sorted(twin_kw(c).items())), c.flags, tuple(sorted(c.knobs.items())), tuple(c.calls), c.max_frames, c.fix)


# ---- A: seams on small handles (k_run64 at M = 64), no AGC
AM_SEAMS = [1, 15, 16, 17, 2047, 2048, 2049, 4097] + [1] * 6      # 16 = samples per thread, 2048 = per workgroup of k_am; then q_in / q_out alone
WB_DECIMS, WB_FCS = (1, 2, 4, 5, 16), (0.025, 0.0021)


def wbfm_seams(d):
    """calls in frames, every one a multiple of d: one output; around the history H = 20 d (a call shorter than it, exactly it, longer);
    255, 256, 257 outputs (a workgroup of k_firdecim less one, whole, one more); around k_biquad's chunk of 4096 samples"""
    H = 20 * d
    lo, hi = (4096 - d) // d * d, -(-(4096 + d) // d) * d
    chunk = [lo, 4096, hi] if 4096 % d == 0 else [lo, 4096 // d * d, -(-4096 // d) * d, hi]
    calls = [d, H - d, H, H + d, 255 * d, 256 * d, 257 * d] + chunk
    out = []
    for f in calls:                                       # d = 16: 256 outputs are the 4096-sample chunk; d = 1: H - d = 19 stays
        if f and f not in out:
            out.append(f)
    return out


A_CASES = []
for _M in (8, 64):
    _p, _t = (_front(64, "CF32") if _M == 64 else ("generic", "k_pfb_fir"))
    A_CASES.append(_case(f"A_am_{_M}", "A", _M, "am", AM_SEAMS, path=(_p,), timed=_t))
    _p, _t = (_front(64, "FM") if _M == 64 else ("generic", "k_pfb_fir"))
    for _d in WB_DECIMS:
        for _fc in WB_FCS:
            A_CASES.append(_case(f"A_wbfm_{_M}_d{_d}_fc{_fc}", "A", _M, "wbfm", wbfm_seams(_d), kw=dict(decim=_d, deemph_fc=_fc),
                                 path=(_p,), timed=_t))

# ---- B: every route, short calls, the last ones ragged; with and without --mix
B_AM, B_WB = [96, 33, 1, 64, 7, 5], [96, 32, 4, 64, 8, 12]
B_AM_4096, B_WB_4096 = [32, 9, 1, 16, 5], [32, 8, 4, 16, 12]
# (tag, M, keywords, flags, path substring of the front (None: the fused front of M; %s: CF32 | FM), timed prefix ("fused": that front's; "1024", "shard1024": by call))
B_ROUTES = [
    ("m1", 1, {}, (), "generic", "k_dc_apply"),
    ("m7", 7, {}, (), "generic", "k_pfb_fir"),
    ("m20", 20, {}, (), "generic", "k_pfb_fir"),
    ("m64", 64, {}, (), None, "fused"),
    ("m256", 256, {}, (), None, "fused"),
    ("m1024", 1024, {}, (), None, "1024"),
    ("m4096", 4096, {}, (), None, "fused"),
    ("m512_g2", 512, dict(chan_stride=2), (), "generic+pruned-dft", "k_pfb_fir"),
    ("m256_c37_C70", 256, dict(chan_first=37, chan_count=70), (), None, "fused"),
    ("m256_g8_g7", 256, dict(chan_stride=8, chan_first=7), (), "fused-256|k_tile256<%s>+interleaved-shard", "k_run256v2<%s>/G8"),
    ("m1024_g4", 1024, dict(chan_stride=4), (), "fused-k_shard1024<%s>/G4+interleaved-shard", "shard1024"),
    ("m4096_C1024", 4096, dict(chan_count=1024), (), "generic", "k_pfb_fir"),
    ("m256_forced", 256, {}, ("FLAG_FORCE_GENERIC",), "generic", "k_pfb_fir"),
]


def timed_1024(kind, calls):
    """k_run1024v3 takes the whole-band calls of whole 4-frame tiles, k_run1024 the ragged ones"""
    return [f"k_run1024v3<{kind}>" if f % 4 == 0 else f"k_run1024<{kind}>" for f in calls]


def timed_shard1024(kind, calls, G=4):
    """kernel_choice.h shard1024_runs: k_shard1024 takes the calls of whole 4-frame tiles that hold a run of at least 16 tiles (four
    blocks of 4 tiles CF32, two of 8 tiles FM), k_run1024 the others"""
    tb, per = (8, 2) if kind == "FM" else (4, 4)
    return [f"k_shard1024<{kind}>/G{G}" if f % 4 == 0 and -(-(f // 4) // tb) // per else f"k_run1024<{kind}>" for f in calls]


B_CASES = []
for _tag, _M, _kw, _fl, _p, _t in B_ROUTES:
    for _dem in ("am", "wbfm"):
        _calls = (B_AM_4096 if _dem == "am" else B_WB_4096) if _M == 4096 else (B_AM if _dem == "am" else B_WB)
        _path = _front(_M, kind_of(_dem))[0] if _p is None else _p % kind_of(_dem) if "%s" in _p else _p
        _k = kind_of(_dem)
        _timed = (_front(_M, _k)[1] if _t == "fused" else timed_1024(_k, _calls) if _t == "1024" else
                  timed_shard1024(_k, _calls) if _t == "shard1024" else _t % _k if _t and "%s" in _t else _t)
        for _mix in (False, True):
            B_CASES.append(_case(f"B_{_dem}_{_tag}{'_mix' if _mix else ''}", "B", _M, _dem, _calls, kw=dict(_kw, mix=_mix), flags=_fl,
                                 path=(_path,), timed=_timed))

# ---- C: the AGC stagings, keyed signal
C_LONG = [1500, 36, 2000, 4, 1200, 600, 28]                 # FLAG_AGC_SEQUENTIAL: 5368 frames
C_SHORT = [100, 64, 4, 96, 36, 8] * 14                      # the row-major time-parallel tail: 84 calls, 4312 frames
C_TM = [TM_MIN, 36, TM_MIN, TM_MIN]                         # tile-major, one short row-major call in between
C_CASES = []
for _dem in ("am", "wbfm"):
    for _M in (8, 256):
        _p, _t = ("generic", "k_pfb_fir") if _M == 8 else _front(256, "CF32", agc=True)
        C_CASES.append(_case(f"C_{_dem}_seq_{_M}", "C", _M, _dem, C_LONG, kw=dict(agc=agc_db(_M)), flags=("FLAG_AGC_SEQUENTIAL",),
                             path=(_p,), nopath=("-spec",), timed=_t, fix="keyed"))
    for _M in (20, 256):
        _p, _t = ("generic", "k_pfb_fir") if _M == 20 else _front(256, "CF32", agc=True)
        C_CASES.append(_case(f"C_{_dem}_spec_{_M}", "C", _M, _dem, C_SHORT, kw=dict(agc=agc_db(_M)), path=(_p, "+agc", "-spec"), timed=_t, tm=(),
                             fix="keyed"))
    for _M, _t in ((64, "k_run64v2"), (256, "k_run256v"), (1024, "k_run1024v3<CF32>")):
        _calls = C_TM[:3] if _M == 1024 else C_TM
        _timed = [_t if f >= TM_MIN else None for f in _calls]
        for _mix in ((False, True) if _M == 256 else (False,)):
            C_CASES.append(_case(f"C_{_dem}_tm_{_M}{'_mix' if _mix else ''}", "C", _M, _dem, _calls, kw=dict(agc=agc_db(_M), mix=_mix),
                                 knobs=TM_KNOBS, max_frames=4096, path=("fused", "+agc", "-spec"), timed=_timed,
                                 tm=tuple(i for i, f in enumerate(_calls) if f >= TM_MIN), fix="keyed"))

# ---- D: backward handles, whole band, three calls
D_CASES = [_case(f"D_{_dem}_backward_{_M}", "D", _M, _dem, [96, 33, 7] if _dem == "am" else [96, 32, 8], kw=dict(dft_backward=True),
                 path=("+dft-backward",)) for _M in (20, 256) for _dem in ("am", "wbfm")]

# ---- E: entry points and state
E_CALLS = [96, 32, 64, 8, 48, 12, 100]
E_SEEK = 33
E_CASES = [_case(f"E_{_dem}_{_M}", "E", _M, _dem, E_CALLS) for _M in (20, 256) for _dem in ("am", "wbfm")]

ALL_CASES = A_CASES + B_CASES + C_CASES + D_CASES + E_CASES
