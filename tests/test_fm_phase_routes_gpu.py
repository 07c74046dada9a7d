"""The FM output of every chain route against the f64 truth (chain_truth.py), in all eight octants of the phase advance.

The chain computes m = ref * arg(conj(r') r) with four separately written phase functions, each folding the octants by hand:
  fast17    fast_atan2f (fused_common.h)            k_tile256<FM>, the seam sample of k_run64<FM>
  scaled15  scaled_atan2f (fused_common.h)          k_run64<FM>, k_pfb1024 / k_run1024 behind the DC blocker
  packed15  fm_sample / fm_quad (fused_v2_common.h) k_run256v2<FM[, G]>, k_run1024v2 / v3, k_shard1024, k_back4096
  rn17      fm_sample_rn (fm_common.h)              k_fm, k_transpose_fm (the any-M route, M = 1), k_pfb1024 without the DC blocker
The narrow-band carriers of the other chain tests keep the strong samples inside |arg| < pi / 4; here the input is white noise
(chain_truth.noise), every channel equally strong and the phase advance uniform, so every fold is exercised with samples that are
compared directly.  test_chain_truth_cpu.py asserts what this file relies on: the truth, the octant shares, the oracle's own figures.

Per route, with the DC blocker off and on (default alpha), kf = 0.3 (and 0.05 on one route per phase function); d = error against the
truth modulo 1 / kf:
  (a) every counted sample (frames behind the window fill, r and r' != 0), unweighted:
          |d_t| <= ref (2 (E / |r_t| + E / |r_t-1|) + phi)
      E: the largest |got - truth| of the route's CF32 run on the same input (itself held to the standing rule of
      test_chain_params_gpu._compare: rel-RMS <= 2 e_orc + 1e-6, per element <= 4 e_orc + 2e-5 max|truth|, and on the fused routes to
      the per-element bound (b) of fused_cases.py, |got - truth| <= 4 max|oracle - truth| + 6 d U rms(truth) per row group, which is
      what keeps a route with one channel off from buying itself a looser FM bound); where the route has no CF32 instantiation, the
      whole-band CF32 kernel of the same M.  phi: the phase function's own error, derived term by term in
      chain_truth.phi15 / phi17 (7.6e-7 and 8.5e-7 rad; a route that uses two functions takes the larger).
  (b) per octant of the true angle, the mean signed error over the kept samples (min(|r|, |r'|) > 0.1 rms):
          |mean_o| <= 2 max_o |mean_o(oracle)| + ref 1.2e-7
      This is the assertion a wrong fold constant fails: hp off by 1e-6 relative shifts four octants by 8e-7.
  (c) finite, |m| <= ref pi (1 + 2^-22).
Every case asserts the route: ch.path and the timed kernel of every call.

Power-of-two scaling (2^k, k = -44, -24, 24, 44): nothing in the linear chain rounds differently at another exponent and arg() does not
see a common factor, so the CF32 output times 2^-k and the FM output are bitwise those of the unscaled run (the oracle does exactly
that: test_chain_truth_cpu.py).  The FM equality is asserted where 2^-100 <= |conj(r') r| <= 2^101 after scaling (below, the inner
products of conj(r') r are denormal and lose bits; the top is 2^101 and not 2^100 for the 4096-channel route, whose products reach
2^100.7); outside, (c).  The any-M rows also run k = -60: products of ~2^-120, below fm_sample_rn's 1e-30 switch, compared with the
truth under (a) plus the denormal rounding of the inner products, 2^-148 / (2^-120 |r| |r'|) rad.

Zeros (DC blocker off): 30 frames of exact zeros inside the noise.  Where r or r' is exactly zero in the truth the output is 0 or
+-ref pi (the sign of a zero out of an f32 DFT is not the oracle's); elsewhere (a).  M = 1 has no DFT and gives the oracle's values.
Decaying silence (dc_alpha = 0.005): DC (0.3, 0.2), then zeros to the end of the stream; the blocker's tail takes |r| down through 2^-50, through
3e-19 (the fused functions' 1e-37 clamp on the product) and, where the stream is long enough, into denormals.  (c) everywhere; (a) on
the four channels DC lands in while min(|r|, |r'|) >= 2^-50, with E the CF32 run's largest error as everywhere else.  That error is
an absolute one (the f32 residue of the cancelled DC, some 1e-6 .. 1e-4 of max |r|, what the standing rule allows), so (a) bites on the
frames behind the step, where the filter's response to the blocker's tail is of order 1 (worst ratios 0.2 .. 0.3), and loosens as the
tail decays: below 2^-50 nothing but (c) is claimed."""
import re

import numpy as np
import pytest

import chain_truth as T
import fused_cases as F
from test_chain_params_gpu import ROUTES, TIMED, _dc_rows, _route_check
from util import knob, rel_rms

pytestmark = pytest.mark.gpu

cs = pytest.importorskip("composable_sdr_amd")
from composable_sdr_amd import _lib  # noqa: E402

KF, ALPHA = T.KF, T.ALPHA
F17, S15, P15, R17 = "fast17", "scaled15", "packed15", "rn17"
PHI = {F17: lambda kf: T.phi17(), R17: lambda kf: T.phi17(), S15: T.phi15, P15: T.phi15}

# call sizes smaller than test_chain_params_gpu's where the kernel still engages, and the phase functions a route runs
T256 = [16 * 12, 16 * 9 + 5, 64]                       # 405 frames: k_tile256 at chunk size, ragged, and a short call
R256 = [16 * 17, 16 * 8 + 5]                           # 405 frames: two runs, then one run from the carried state + 5 frames of k_tile256
WGS3 = {"CSDR_RESIDENT_WGS": "3"}
SHAPE = {  # id: (frames or None, extra knobs, phase functions)
    "tile256_fm": (T256, {}, (F17,)),
    "run256v2_fm_nowu": (R256, WGS3, (P15, F17)),
    "run256v2_fm_wu": (R256, WGS3, (P15, F17)),
    "run256v2_fm_g2": (R256, WGS3, (P15, F17)),
    "run256v2_fm_g8": (R256, WGS3, (P15, F17)),
    "run64_fm": (None, {}, (S15, F17)),
    "run1024v3_fm_nowu": (None, {}, (P15, S15, R17)),
    "shard1024_fm_g8": (None, {}, (P15, S15, R17)),
    "run1024v2_fm_g2": (None, {}, (P15, S15, R17)),
    "front4096_fm": (None, {}, (P15,)),
    "generic_m20_fm": (None, {}, (R17,)),
    "m1_fm": (None, {}, (R17,)),
}
# (id, M, Chain keywords, knobs, call sizes, timed kernel of each call, phase functions, expected path (None: _route_check decides))
CASES = []
for _r in ROUTES:
    if _r[2].get("demod") == "fm":
        _f, _k, _impl = SHAPE[_r[0]]
        CASES.append((_r[0], _r[1], _r[2], {**_r[3], **_k}, _f or _r[4], _r[5], _impl, None))
assert [c[0] for c in CASES] == list(SHAPE), [c[0] for c in CASES]
CASES += [
    ("generic_256_forced_fm", 256, dict(demod="fm", flags=TIMED | _lib.FLAG_FORCE_GENERIC), {}, T256, ["k_pfb_fir"] * 3, (R17,), None),
    ("pfb1024_fm", 1024, dict(demod="fm"), {"CSDR_NO_RUN1024": "1"}, [1024, 5, 1024], ["k_pfb1024"] * 3, (S15, R17), "generic+pfb1024"),
    ("generic_m7_fm", 7, dict(demod="fm"), {}, [2000, 1333], ["k_pfb_fir"] * 2, (R17,), None),      # k_dft_direct + k_transpose_fm
]
IDS = [c[0] for c in CASES]
KF_LOW = ["tile256_fm", "run64_fm", "run256v2_fm_nowu", "generic_m20_fm"]      # one route per phase function
ANY_M = [c for c in CASES if c[6] == (R17,)]
# the CF32 partner of a route without a CF32 instantiation: the whole band of the same M
PARTNER = {"run1024v2_fm_g2": (dict(demod="none"), {"CSDR_RUN1024_V3_RUNS": "8"})}


def _family(name):
    return re.match(r"k_[a-z_]+\d*", name).group(0).rstrip("_")


_DCR = {}


def _shard(case):
    """(g, G) of an interleaved-shard case, the shard that owns a channel next to DC; (0, 1) for a whole band"""
    M, G = case[1], case[2].get("chan_stride", 0)
    if M not in _DCR:
        _DCR[M] = _dc_rows(M)
    return (int(_DCR[M][0] % G), G) if G > 1 else (0, 1)


def _run(case, x, frames, demod, dc, alpha, kf, monkeypatch):
    """one handle, the calls `frames` on x -> (output of the case's rows, timed kernel of every call, path), route asserted.
    demod 'none': the route's CF32 partner."""
    tag, M, kw, knobs, _, want, _, want_path = case
    if len(want) != len(frames):                                     # other call sizes than the table's: every call on the first call's kernel
        want = [want[0]] * len(frames)
    kw = dict(kw)
    whole = False
    if demod == "none" and tag in PARTNER:
        kw, knobs = dict(PARTNER[tag][0]), PARTNER[tag][1]
        whole = True
    kw["demod"] = demod
    kw.setdefault("flags", TIMED)
    if kw.get("chan_stride", 0) > 1:
        kw["chan_first"] = _shard(case)[0]
    for k, v in knobs.items():
        knob(monkeypatch, k, v)
    ch = cs.Chain(channels=M, kf=kf, dc_block=dc, dc_alpha=alpha, max_frames=max(frames), **kw)
    outs, names, pos = [], [], 0
    try:
        for f in frames:
            outs.append(ch.process(x[pos * M:(pos + f) * M]))
            names.append(ch.kernel_time()[0])
            pos += f
        path = ch.path
    finally:
        ch.close()
        for k in knobs:
            monkeypatch.delenv(k, raising=False)
    got = np.concatenate(outs, axis=-1)
    if demod == "fm":
        if want_path is None:
            _route_check(tag, path, ALPHA, want, names, M, kw)
        else:
            assert path == want_path and names == want, (tag, path, names)
    else:                                                            # the partner: a CF32 kernel of the same family, on the same kind of path
        assert all("FM" not in n for n in names), (tag, names)
        assert all(w is None or _family(n) == _family(w) for w, n in zip(want, names)), (tag, path, names, want)
        assert path.startswith("fused") == (want_path is None and M in (64, 256, 1024, 4096) and
                                            not kw["flags"] & _lib.FLAG_FORCE_GENERIC), (tag, path)
    return (got[_rows(case)] if whole else got), names, path


def _rows(case):
    g, G = _shard(case)
    return slice(g, None, G)


def _sub(R, sl):
    return {k: (v[sl] if isinstance(v, np.ndarray) and v.ndim == 2 else v) for k, v in R.items()}


def _cf32_E(tag, got, R, fused=None):
    """the standing rule of test_chain_params_gpu._compare on the CF32 partner's output; returns E = max |got - truth|.
    fused = (M, band rows of the output, d): a fused route, also held to (b) of fused_cases.py"""
    assert got.shape == R["r"].shape and np.isfinite(got.view(np.float32)).all(), tag
    eg, eo = np.abs(got.astype(np.complex128) - R["r"]), np.abs(R["orc_r"].astype(np.complex128) - R["r"])
    rg, ro = rel_rms(got, R["r"]), rel_rms(R["orc_r"], R["r"])
    print(f"{tag} CF32: rel-rms {rg:.3e} (oracle {ro:.3e}); max {eg.max():.3e} (oracle {eo.max():.3e})")
    assert rg <= 2 * ro + 1e-6, (tag, rg, ro)
    assert eg.max() <= 4 * eo.max() + 2e-5 * float(np.abs(R["r"]).max()), (tag, eg.max(), eo.max())
    if fused is not None:
        M, rows, d = fused
        b = F.element_ratio(M, rows, got, R["r"], R["orc_r"], d)
        print(f"{tag} CF32: worst ratio to the per-element bound (b) of fused_cases.py (d = {d:.2f}) {b:.3f}")
        assert b <= 1.0, (tag, b)
    return float(eg.max())


def _phi(case, kf):
    return max(PHI[i](kf) for i in case[6])


# --------------------------------------------------------------------------- every route, all octants
@pytest.mark.parametrize("dc", [False, True], ids=["nodc", "dc"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fm_of_every_route_in_all_octants(case, dc, monkeypatch):
    tag, M, frames = case[0], case[1], case[4]
    nf = sum(frames)
    assert (M, nf) in T.SHAPES, (M, nf)
    for kf in [KF] + ([0.05] if tag in KF_LOW else []):
        R = _sub(T.refs(M, nf, dc, kf), _rows(case))
        x = R["x"]
        fm, names, path = _run(case, x, frames, "fm", dc, ALPHA, kf, monkeypatch)
        cf, cnames, cpath = _run(case, x, frames, "none", dc, ALPHA, kf, monkeypatch)
        g, G = _shard(case)
        fused = (M, np.arange(g, M, G), F.d_for(M, G)) if cpath.startswith("fused") else None
        E = _cf32_E(f"{tag} dc={dc} [{cpath}] {cnames}", cf, R, fused)
        worst, bias, bb = T.check_fm(f"{tag} dc={dc} kf={kf} [{path}] {names}", fm, R, E, _phi(case, kf), kf)
        assert worst <= 1.0, (tag, worst)
        assert np.abs(bias).max() <= bb, (tag, bias, bb)


# --------------------------------------------------------------------------- power-of-two scale invariance
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fm_and_cf32_are_invariant_under_power_of_two_scaling(case, monkeypatch):
    tag, M, frames = case[0], case[1], case[4]
    nf = sum(frames)
    R = _sub(T.refs(M, nf, True), _rows(case))
    x = R["x"]
    ref = T.ref32(KF)
    fm0, _, _ = _run(case, x, frames, "fm", True, ALPHA, KF, monkeypatch)
    cf0, _, _ = _run(case, x, frames, "none", True, ALPHA, KF, monkeypatch)
    q = np.abs(R["r"]) * T.prev(np.abs(R["r"]))
    bad = []
    for k in (-44, -24, 24, 44) + ((-60,) if case in ANY_M else ()):
        xs = (x * np.float32(2.0 ** k)).astype(np.complex64)
        fm, names, path = _run(case, xs, frames, "fm", True, ALPHA, KF, monkeypatch)
        cf, _, _ = _run(case, xs, frames, "none", True, ALPHA, KF, monkeypatch)
        assert np.isfinite(fm).all() and np.abs(fm).max() <= ref * np.pi * (1 + 2.0 ** -22), (tag, k)
        same_cf = np.array_equal((cf * np.float32(2.0 ** -k)).view(np.uint32), cf0.view(np.uint32))
        dom = (q * 4.0 ** k >= 2.0 ** -100) & (q * 4.0 ** k <= 2.0 ** 101)
        diff = (fm.view(np.uint32) != fm0.view(np.uint32)) & dom
        dmax = float(np.abs(T.fm_err(fm, fm0.astype(np.float64), KF))[dom].max()) if dom.any() else 0.0
        print(f"{tag} 2^{k} [{path}] {names}: CF32 {'bitwise' if same_cf else 'DIFFERS'}; FM differs on {int(diff.sum())} of {int(dom.sum())} "
              f"samples in the domain, max {dmax:.3e} = {dmax / np.spacing(np.float32(ref * np.pi)):.2f} ulp of ref pi")
        assert same_cf, (tag, k)
        if k == -60:
            # below the 1e-30 switch: against the truth, (a) + the denormal rounding of the four inner products (half a denormal ulp each)
            E = float(np.abs(cf0.astype(np.complex128) - R["r"]).max())
            a = np.abs(R["r"])
            m = R["counted"] & (a > 0) & (T.prev(a) > 0)
            with np.errstate(divide="ignore", invalid="ignore"):
                bound = T.sample_bound(R["r"], E, _phi(case, KF), KF) + ref * 2.0 ** -148 / (q * 4.0 ** k)
            ratio = float((np.abs(T.fm_err(fm, R["fm"], KF))[m] / bound[m]).max())
            print(f"{tag} 2^{k}: worst ratio against the truth {ratio:.3f}")
            assert ratio <= 1.0, (tag, k, ratio)
        elif diff.any():
            bad.append((k, int(diff.sum()), dmax))
    assert not bad, (tag, bad)


# --------------------------------------------------------------------------- zeros and decaying silence
def _calls(case, need):
    """the case's calls if they hold `need` frames, else [40, 30, 40] (k_front4096 + k_back4096 run at every call size)"""
    return case[4] if sum(case[4]) >= need else [40, 30, 40]


_Z = {}


def _refs_of(key, x, M, dc, alpha):
    if key not in _Z:
        _Z.clear()
        _Z[key] = T.refs_of(x, M, dc, KF, alpha)
    return _Z[key]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fm_across_exact_zeros(case, monkeypatch):
    tag, M = case[0], case[1]
    frames = _calls(case, 110)
    nf = sum(frames)
    x = T.noise(M, nf, seed=1000 + M).copy()
    x[40 * M:70 * M] = 0
    R = _sub(_refs_of(("zeros", M, nf), x, M, False, ALPHA), _rows(case))
    ref = T.ref32(KF)
    fm, names, path = _run(case, x, frames, "fm", False, ALPHA, KF, monkeypatch)
    cf, _, _ = _run(case, x, frames, "none", False, ALPHA, KF, monkeypatch)
    E = float(np.abs(cf.astype(np.complex128) - R["r"]).max())
    a = np.abs(R["r"])
    zero = (a == 0) | (T.prev(a) == 0)
    assert zero[:, 53:70].all() and not zero[:, 14:40].any() and not zero[:, 84:].any()
    assert np.isfinite(fm).all() and np.abs(fm).max() <= ref * np.pi * (1 + 2.0 ** -22), tag
    dz = np.minimum(np.abs(fm), np.abs(np.abs(fm) - ref * np.pi))[zero]
    rest = R["counted"] & ~zero
    ratio = float((np.abs(T.fm_err(fm, R["fm"], KF))[rest] / T.sample_bound(R["r"], E, _phi(case, KF), KF)[rest]).max())
    print(f"{tag} zeros [{path}] {names}: E {E:.3e}; on zero samples max distance to 0 / ref pi {dz.max():.3e}; elsewhere worst (a) ratio {ratio:.3f}")
    assert dz.max() <= 1e-6, (tag, dz.max())
    assert ratio <= 1.0, (tag, ratio)
    if M == 1:
        # no DFT, no filter: r is the input itself and the zeros' signs are the oracle's, so 0 or pi is decided: by the signs of the
        # neighbour's components on entering and on leaving (conj(r') (+0) has real part -0 when both are negative), 0 inside
        d = np.abs(T.fm_err(fm, R["orc_fm"].astype(np.float64), KF))[zero]
        assert d.max() <= 2 * np.spacing(np.float32(ref * np.pi)), d.max()
        assert np.all(fm[0, 41:70] == 0), fm[0, 38:72]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fm_through_decaying_silence(case, monkeypatch):
    tag, M = case[0], case[1]
    alpha = 0.005
    frames = _calls(case, 110)
    nf = sum(frames)
    # beta^M per frame: 150 binades take 150 / (-M log2 beta) frames; the silence sits at the end of the stream so that no more of
    # it than that is spent in denormals (where the any-M stream is too short for 150 binades it gets as far as it gets)
    tail = min(nf - 20, int(150 / (-M * np.log2(T.beta_of(alpha)))) + 16)
    n0 = nf - tail
    x = np.zeros(M * nf, np.complex64)
    x[:n0 * M] = 0.3 + 0.2j
    Rw = _refs_of(("decay", M, nf), x, M, True, alpha)
    R = _sub(Rw, _rows(case))
    ref = T.ref32(KF)
    fm, names, path = _run(case, x, frames, "fm", True, alpha, KF, monkeypatch)
    cf, _, _ = _run(case, x, frames, "none", True, alpha, KF, monkeypatch)
    assert np.isfinite(fm).all() and np.abs(fm).max() <= ref * np.pi * (1 + 2.0 ** -22), tag
    g, G = _shard(case)
    dcr = set(_dc_rows(M).tolist())
    rows = [i for i, c in enumerate(range(g, M, G)) if c in dcr]
    E = _cf32_E(f"{tag} decay", cf, R)
    a = np.abs(R["r"])
    dom = np.zeros(a.shape, bool)
    dom[rows, n0 + 1:] = (np.minimum(a, T.prev(a)) >= 2.0 ** -50)[rows, n0 + 1:]      # r and r' both behind the step: in front of it the
    #                                     truth is ~1e-13, the rounding residue of an f64 recurrence that holds DC / alpha, not a signal
    assert dom.sum() >= 4, (tag, int(dom.sum()))
    ratio = float((np.abs(T.fm_err(fm, R["fm"], KF))[dom] / T.sample_bound(R["r"], E, _phi(case, KF), KF)[dom]).max())
    print(f"{tag} decay [{path}] {names}: {int(dom.sum())} samples on rows {rows} down to |r| = 2^{np.log2(a[dom].min()):.1f} (stream ends at "
          f"2^{np.log2(max(a[rows, -1].max(), 1e-300)):.0f}); E {E:.3e}; worst (a) ratio {ratio:.3f}")
    assert ratio <= 1.0, (tag, ratio)
