"""The chain's DSP settings other than the defaults: dc_alpha, pfb_m and pfb_as (include/csdr.h csdr_chain_cfg), on every route.

Truth: an f64 DC blocker (scipy lfilter with beta = f32(1) - f32(alpha), the library's and the oracle's coefficient) in front of
O.Chain(M, dc_block=False, ...).  Yardstick: the f32 oracle O.Chain(M, dc_alpha=alpha, ...), whose distance to the truth sets the
bounds (the GPU may be at most 2x as far from the truth in rel-RMS, 4x per element); the constants added to them are the suite's
usual floors (CF32: 1e-6 rel-RMS, 2e-5 of max|truth| per element; FM, compared modulo 1/kf and weighted by min(|r_t|, |r_t-1|) /
max|r| as in test_chain_fm_matches_oracle: 2e-5 RMS, 2 ref 1e-4 per element).

The per-element check runs on the four channels DC lands in (all frames: every run or tile boundary of the route is inside) and on
every channel over the first 128 frames of each call.  A whole-array rel-RMS would dilute a run-start truncation by about M x run
length; here it shows.  Observed: the f32 oracle's own distance to the truth grows with 1/alpha (the filter state sits at |DC| /
alpha), e.g. ~1e-4 of max|truth| per element at alpha = 5e-5 and ~1e-7 at alpha = 0.3, so both ends are checked against their own
f32 reference rather than one fixed number.

Routes: alpha >= 0.0005 (and below ~0.15) keeps the route and kernels of the defaults; other alphas do not fit the truncation windows
of the fused kernels and of k_dc_tile (dc_window_ok) and run on the any-M route with the exact block scan, path
'...+dc-scan'.  Every case asserts the path and the timed kernel of the calls it makes."""
import numpy as np
import pytest

import oracle_lib as O
from chain_truth import dc_rows as _dc_rows      # (shared with fused_cases.py, which has to import without the library)
from util import knob, rel_rms, wrap_pm

pytestmark = pytest.mark.gpu

cs = pytest.importorskip("composable_sdr_amd")
from composable_sdr_amd import _lib  # noqa: E402

ALPHAS = [5e-5, 2e-4, 5e-4, 5e-3, 0.05, 0.3]
KF = 0.3
REF = 1.0 / (2 * np.pi * KF)
TIMED = _lib.FLAG_QUIET | _lib.FLAG_TIME_KERNELS
_X = {}


def _beta(alpha):
    return float(np.float32(1) - np.float32(alpha))


def _scan_route(alpha):
    """the handle leaves the DC shortcuts (csrc/csdr_internal.h dc_window_ok)"""
    b, b0 = _beta(alpha), _beta(0.0005)
    return b > b0 or -512.0 * np.log2(b) >= 120.0


def _input(M, nf, seed, dc=(0.3, 0.2)):
    """strong DC by default (|DC| = 0.36: a truncated state shows); the filter-design tests take the suite's usual weak one"""
    key = (M, nf, seed, dc)
    if key not in _X:
        import torch
        from synth import synth_cf32_torch
        x = synth_cf32_torch(M * nf, max(M, 4), torch.device("cuda", 0), seed=seed, dc=dc)
        _X.clear()
        _X[key] = x.cpu().numpy().view(np.complex64).reshape(-1)
    return _X[key]


def _references(x, M, alpha, demod, mix=False, m=7, As=80.0):
    from scipy.signal import lfilter
    b = _beta(alpha)
    yd = lfilter([1.0, -1.0], [1.0, -b], x.astype(np.complex128)).astype(np.complex64)
    kw = dict(demod=demod, kf=KF, mix=mix, pfb_m=m, pfb_as=As)
    truth = O.Chain(M, dc_block=False, **kw).process(yd)
    orc = O.Chain(M, dc_alpha=alpha, **kw).process(x)
    r = np.abs(O.Chain(M, dc_block=False, pfb_m=m, pfb_as=As).process(yd)) if demod == "fm" else None
    return truth, orc, r


def _compare(tag, got, truth, orc, r, rows, starts, fm):
    """the rules of the module docstring; rows: the channels of `got` DC lands in; starts: first frame of every call"""
    assert got.shape == truth.shape == orc.shape, (got.shape, truth.shape)
    assert np.isfinite(got).all(), f"{tag}: non-finite output"
    if fm:
        rmin = np.minimum(r, np.concatenate([np.zeros((r.shape[0], 1)), r[:, :-1]], axis=1)) / r.max()
        eg = np.abs(wrap_pm(got.astype(np.float64) - truth, 1.0 / KF)) * rmin
        eo = np.abs(wrap_pm(orc.astype(np.float64) - truth, 1.0 / KF)) * rmin
        rg, ro = float(np.sqrt(np.mean(eg ** 2))), float(np.sqrt(np.mean(eo ** 2)))
        rms_floor, el_floor = 2e-5, 2 * REF * 1e-4
    else:
        eg = np.abs(got.astype(np.complex128) - truth)
        eo = np.abs(orc.astype(np.complex128) - truth)
        rg, ro = rel_rms(got, truth), rel_rms(orc, truth)
        rms_floor, el_floor = 1e-6, 2e-5 * float(np.abs(truth).max())
    mask = np.zeros(eg.shape, bool)
    if eg.ndim == 1:
        mask[:] = True                                  # --mix: every output sums every channel
    else:
        mask[rows, :] = True
        for s in starts:
            mask[:, s:s + 128] = True
    mg, mo = float(eg[mask].max()), float(eo[mask].max())
    print(f"{tag}: rms {rg:.3e} (oracle f32 {ro:.3e}); max near DC / call starts {mg:.3e} (oracle f32 {mo:.3e}, floor {el_floor:.1e})")
    assert rg <= 2 * ro + rms_floor, (tag, rg, ro)
    assert mg <= 4 * mo + el_floor, (tag, mg, mo)


# --------------------------------------------------------------------------- (a) dc_alpha on every route
# (id, M, Chain keywords, knobs, call sizes in frames, timed kernel of each call on the route of the defaults (None: not pinned))
R256 = [16 * 128, 16 * 64 + 5]
ROUTES = [
    ("tile256_fm", 256, dict(demod="fm"), {"CSDR_RUN_MIN_TILES": "1000000"}, [16 * 40, 16 * 9 + 5, 300], ["k_tile256<FM>"] * 3),
    ("tile256_cf32", 256, dict(demod="none"), {"CSDR_RUN_MIN_TILES": "1000000"}, [16 * 40 + 5, 16 * 9], ["k_tile256<CF32>"] * 2),
    ("run256v2_fm_nowu", 256, dict(demod="fm"), {"CSDR_RUN_MIN_TILES": "1"}, R256, ["k_run256v2<FM>", None]),
    ("run256v2_cf32_nowu", 256, dict(demod="none"), {"CSDR_RUN_MIN_TILES": "1"}, R256, ["k_run256v2<CF32>", None]),
    ("run256v2_fm_wu", 256, dict(demod="fm"), {"CSDR_RUN_MIN_TILES": "1", "CSDR_NOWU": "0"}, R256, ["k_run256v2<FM>", None]),
    ("run256v2_cf32_wu", 256, dict(demod="none"), {"CSDR_RUN_MIN_TILES": "1", "CSDR_NOWU": "0"}, R256, ["k_run256v2<CF32>", None]),
    ("run256v2_fm_g2", 256, dict(demod="fm", chan_stride=2), {"CSDR_RUN_MIN_TILES": "1"}, R256, ["k_run256v2<FM>/G2", None]),
    ("run256v2_fm_g8", 256, dict(demod="fm", chan_stride=8), {"CSDR_RUN_MIN_TILES": "1"}, R256, ["k_run256v2<FM>/G8", None]),
    # k_run64v2 takes CF32 only; k_run64 the FM output and the ragged calls
    ("run64v2_cf32", 64, dict(demod="none"), {"CSDR_RUN64_V2_ALL": "1"}, [64 * 128, 5, 64 * 96], ["k_run64v2", "k_run64<CF32>", "k_run64v2"]),
    ("run64_fm", 64, dict(demod="fm"), {}, [64 * 40, 64 * 9 + 5], ["k_run64<FM>"] * 2),
    ("run1024v3_fm_nowu", 1024, dict(demod="fm"), {"CSDR_RUN1024_V3_RUNS": "8"}, [2048, 5, 1024], ["k_run1024v3<FM>", None, "k_run1024v3<FM>"]),
    ("run1024v3_cf32_wu", 1024, dict(demod="none"), {"CSDR_RUN1024_V3_RUNS": "8", "CSDR_NOWU": "0"}, [2048, 5, 1024],
     ["k_run1024v3<CF32>", None, "k_run1024v3<CF32>"]),
    ("shard1024_fm_g8", 1024, dict(demod="fm", chan_stride=8), {"CSDR_SHARD1024_RUNS": "4"}, [1024, 5, 1024], ["k_shard1024<FM>/G8", "k_run1024<FM>", "k_shard1024<FM>/G8"]),
    ("run1024v2_fm_g2", 1024, dict(demod="fm", chan_stride=2), {"CSDR_RUN1024_RUNS": "4"}, [1024, 5, 1024], ["k_run1024v2<FM>/G2", "k_run1024<FM>", "k_run1024v2<FM>/G2"]),
    ("front4096_fm", 4096, dict(demod="fm"), {}, [40, 9], ["k_front4096+k_back4096<FM>"] * 2),
    ("front4096_cf32", 4096, dict(demod="none"), {}, [40, 9], ["k_front4096+k_back4096<CF32>"] * 2),
    ("generic_m20_fm", 20, dict(demod="fm"), {}, [400, 133], ["k_pfb_fir"] * 2),
    ("generic_256_forced_cf32", 256, dict(demod="none", flags=TIMED | _lib.FLAG_FORCE_GENERIC), {}, [16 * 40 + 5, 300], ["k_pfb_fir"] * 2),
    ("mixid_4096", 4096, dict(demod="none", mix=True), {}, [40, 9, 130], ["k_dc_fold"] * 3),
    ("mixid_shard_4096_g8", 4096, dict(demod="none", mix=True, chan_stride=8), {}, [40, 9, 130], ["k_dc_fold8"] * 3),
    ("m1_fm", 1, dict(demod="fm"), {}, [30000, 12345], ["k_dc_apply"] * 2),
]
# Dropped combinations: k_run64v2 has no FM output (k_run64 covers it); k_run1024v2<FM, 2> has no CF32 instantiation (CF32 shards of
# 1024 channels run the whole band + row gather); the mix-identity folds exist for DeNo only.


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("case", ROUTES, ids=[c[0] for c in ROUTES])
def test_dc_alpha_on_every_route(case, alpha, monkeypatch):
    tag, M, kw, knobs, frames, want_names = case
    kw = dict(kw)
    kw.setdefault("flags", TIMED)
    demod, mix, G = kw.get("demod", "none"), kw.get("mix", False), kw.get("chan_stride", 0)
    rows_dc = _dc_rows(M)
    g = int(rows_dc[0] % G) if G > 1 else 0                 # a shard that owns a channel next to DC
    if G > 1:
        kw["chan_first"] = g
    for k, v in knobs.items():
        knob(monkeypatch, k, v)
    x = _input(M, sum(frames), 900 + M)
    ch = cs.Chain(channels=M, kf=KF, dc_alpha=alpha, max_frames=max(frames), **kw)
    outs, names, pos = [], [], 0
    for f in frames:
        outs.append(ch.process(x[pos * M:(pos + f) * M]))
        names.append(ch.kernel_time()[0])
        pos += f
    got = np.concatenate(outs, axis=-1)
    path = ch.path
    ch.close()
    truth, orc, r = _references(x, M, alpha, demod, mix)
    if G > 1:
        if mix:                                              # the shard's partial mix: left fold of its rows, like Trans.hs:119-122
            t_rows = O.Chain(M, dc_block=False).process(_lfilter_c64(x, alpha))[g::G]
            o_rows = O.Chain(M, dc_alpha=alpha).process(x)[g::G]
            truth, orc = _fold(t_rows), _fold(o_rows)
        else:
            truth, orc, r = truth[g::G], orc[g::G], (r[g::G] if r is not None else None)
    rows = [i for i, c in enumerate(range(g, M, G if G > 1 else 1)) if c in set(rows_dc.tolist())]
    starts = np.cumsum([0] + frames[:-1]).tolist()
    _compare(f"{tag} alpha={alpha:g} [{path}] {names}", got, truth, orc, r, rows, starts, demod == "fm")
    _route_check(tag, path, alpha, want_names, names, M, kw)


def _route_check(tag, path, alpha, want_names, names, M, kw):
    if _scan_route(alpha):
        if M > 1:
            assert path.startswith("generic") and "+dc-scan" in path and "mix-identity" not in path, (tag, path)
        assert all(n in ("k_pfb_fir", "k_pfb1024", "k_dc_apply") for n in names), (tag, names)
    else:
        assert "+dc-scan" not in path, (tag, path)
        assert all(w is None or n == w for w, n in zip(want_names, names)), (tag, path, names, want_names)
        fused = M in (64, 256, 1024, 4096) and not kw.get("mix") and not kw["flags"] & _lib.FLAG_FORCE_GENERIC
        assert path.startswith("fused") == fused, (tag, path)


def _lfilter_c64(x, alpha):
    from scipy.signal import lfilter
    return lfilter([1.0, -1.0], [1.0, -_beta(alpha)], x.astype(np.complex128)).astype(np.complex64)


def _fold(rows):
    acc = np.zeros(rows.shape[1], np.complex64)
    for rr in rows:
        acc = (acc + rr).astype(np.complex64)
    return acc


@pytest.mark.parametrize("alpha", ALPHAS)
def test_dc_alpha_independent_launches(alpha, monkeypatch):
    """csdr_chain_submit_device (M = 256, FM): chunks of whole tiles at the run-kernel size run as independent launches whose run 0 warms
    its DC state up over the previous chunk's saved tail (WU tiles); a ragged chunk in between is serialized."""
    import torch
    knob(monkeypatch, "CSDR_RUN_MIN_TILES", "1")
    M, frames = 256, [16 * 128, 16 * 128, 16 * 8 + 5, 16 * 128]
    x = _input(M, sum(frames), 901)
    dev = torch.device("cuda", 0)
    xd = torch.from_numpy(x.view(np.float32).copy()).to(dev)
    ch = cs.Chain(channels=M, demod="fm", kf=KF, dc_alpha=alpha, max_frames=max(frames), flags=TIMED)
    outs, pos = [], 0
    for f in frames:
        o = torch.empty(M * f, dtype=torch.float32, device=dev)
        ch.submit_device(xd.data_ptr() + pos * M * 8, M * f, o.data_ptr())
        outs.append(o); pos += f
    ch.wait_device()
    torch.cuda.synchronize()
    n_indep, path, name = ch.independent_launches(), ch.path, ch.kernel_time()[0]
    ch.close()
    got = np.concatenate([o.cpu().numpy().reshape(M, -1) for o in outs], axis=1)
    truth, orc, r = _references(x, M, alpha, "fm")
    _compare(f"submit_device alpha={alpha:g} [{path}] {name}, {n_indep} independent", got, truth, orc, r, _dc_rows(M),
             np.cumsum([0] + frames[:-1]).tolist(), True)
    if _scan_route(alpha):
        assert path.startswith("generic") and "+dc-scan" in path and n_indep == 0 and name == "k_pfb_fir", (path, n_indep, name)
    else:
        assert path.startswith("fused-256") and n_indep >= 2 and name == "k_run256v2<FM>", (path, n_indep, name)


# --------------------------------------------------------------------------- (b) the standalone DC blocker and M = 1
@pytest.mark.parametrize("alpha", ALPHAS)
def test_dcblocker_alpha_against_f64_recurrence(alpha):
    x = _input(1, 300000, 902)
    cuts = [0, 1, 1000, 1024, 5000, 150000, 150000, 300000]     # test_dcblocker_matches_oracle_across_chunks
    chunks = [x[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    p = cs.dcBlocker(alpha)
    r = p._start()
    try:
        got = np.concatenate([p._process(r, c) for c in chunks])
    finally:
        p._done(r)
    from scipy.signal import lfilter
    truth = lfilter([1.0, -1.0], [1.0, -_beta(alpha)], x.astype(np.complex128))
    orc = O.DcBlock(alpha).execute(x)
    e_gpu, e_orc = rel_rms(got, truth), rel_rms(orc, truth)
    m_gpu, m_orc = float(np.abs(got - truth).max()), float(np.abs(orc - truth).max())
    print(f"dcBlocker alpha={alpha:g}: rel-rms gpu {e_gpu:.3e} oracle {e_orc:.3e}; max gpu {m_gpu:.3e} oracle {m_orc:.3e}")
    assert np.isfinite(got).all()
    assert e_gpu <= 2 * e_orc + 1e-7
    assert m_gpu <= 4 * m_orc + 1e-6
    # the chain at M = 1 over the same cuts (DC blocker + FM)
    ch = cs.Chain(channels=1, demod="fm", kf=KF, dc_alpha=alpha, max_frames=150000, flags=TIMED)
    outs, names = [], []
    for c in chunks:
        outs.append(ch.process(c))
        names.append(ch.kernel_time()[0])
    path = ch.path
    ch.close()
    got = np.concatenate(outs, axis=-1)
    tr, oc, rr = _references(x, 1, alpha, "fm")
    _compare(f"M=1 alpha={alpha:g} [{path}]", got, tr, oc, rr, [0], cuts[1:-1], True)
    assert path == "generic" and set(n for n in names if n) <= {"k_dc_apply"}, (path, names)


# --------------------------------------------------------------------------- (c) filter design
@pytest.mark.parametrize("M,m,As", [(20, 1, 60.0), (20, 3, 80.0), (64, 4, 60.0), (256, 7, 60.0), (256, 7, 100.0), (256, 12, 80.0),
                                    (1024, 7, 60.0), (1024, 16, 80.0), (4096, 7, 60.0)])
def test_chain_taps_equal_the_oracle_prototype(M, m, As):
    ch = cs.Chain(channels=M, pfb_m=m, pfb_as=As, max_frames=64)
    got = ch.taps
    ch.close()
    want = O.Pfb(M, m, As).taps
    assert got.shape == want.shape == (M * 2 * m,)
    ulp = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    print(f"taps M={M} m={m} As={As}: {int((ulp > 0).sum())} differ, max {int(ulp.max())} ulp")
    assert ulp.max() <= 1


PFB_CASES = [  # (M, m, As, knobs, frames, timed kernel)
    (256, 7, 60.0, {"CSDR_RUN_MIN_TILES": "1"}, [16 * 128, 16 * 9 + 5], "k_run256v2"),
    (64, 7, 60.0, {"CSDR_RUN64_V2_ALL": "1"}, [64 * 64, 70], "k_run64"),
    (1024, 7, 60.0, {"CSDR_RUN1024_V3_RUNS": "8"}, [2048, 1024], "k_run1024v3"),
    (4096, 7, 60.0, {}, [40, 9], "k_front4096"),
    (20, 3, 70.0, {}, [400, 133], "k_pfb_fir"),
    (256, 12, 80.0, {}, [300, 133], "k_pfb_fir"),
    (1024, 16, 80.0, {}, [200, 37], "k_pfb_fir"),
]


@pytest.mark.parametrize("demod", ["fm", "none"])
@pytest.mark.parametrize("M,m,As,knobs,frames,kname", PFB_CASES, ids=[f"M{c[0]}_m{c[1]}_As{c[2]:g}" for c in PFB_CASES])
def test_chain_with_designed_prototype_matches_extended_oracle(M, m, As, knobs, frames, kname, demod, monkeypatch):
    """m = 7, As != 80 on every fused route; m != 7 on the generic one (the fused kernels take p = 14 only).  Tolerances of
    test_chain_matches_oracle / test_chain_fm_matches_oracle."""
    for k, v in knobs.items():
        knob(monkeypatch, k, v)
    x = _input(M, sum(frames), 903, dc=(0.01, 0.01))
    ch = cs.Chain(channels=M, demod=demod, kf=KF, pfb_m=m, pfb_as=As, max_frames=max(frames), flags=TIMED)
    outs, names, pos = [], [], 0
    for f in frames:
        outs.append(ch.process(x[pos * M:(pos + f) * M]))
        names.append(ch.kernel_time()[0])
        pos += f
    path = ch.path
    ch.close()
    got = np.concatenate(outs, axis=-1)
    want = O.Chain(M, demod=demod, kf=KF, pfb_m=m, pfb_as=As).process(x)
    assert names[0].startswith(kname), (path, names)
    assert path.startswith("fused") == (m == 7), path
    if demod == "fm":
        r = np.abs(O.Chain(M, pfb_m=m, pfb_as=As).process(x))
        d = np.abs(wrap_pm(got.astype(np.float64) - want, 1.0 / KF))
        rmin = np.minimum(r, np.concatenate([np.zeros((r.shape[0], 1)), r[:, :-1]], axis=1))
        strong = rmin > 0.25 * r.max()
        print(f"M={M} m={m} As={As} FM [{path}] {names}: median {np.median(d):.2e} weighted max {(d * rmin).max() / r.max():.2e}")
        assert (d * rmin).max() / r.max() < 2 * REF * 1e-4 and np.median(d) < 2e-5
        if strong.any():
            assert d[strong].max() < 2e-5
    else:
        e, mx = rel_rms(got, want), float(np.abs(got - want).max())
        print(f"M={M} m={m} As={As} DeNo [{path}] {names}: rel-rms {e:.2e}, max {mx:.2e} of {np.abs(want).max():.2f}")
        assert e < 1e-5 and mx < 1e-4 * np.abs(want).max()


@pytest.mark.parametrize("m", [16, 17])
@pytest.mark.parametrize("G", [1, 8])
def test_mix_identity_prototype_length(m, G):
    """DeNo --mix at 4096 channels: the folds take p = 2m <= 33 (m = 16: k_dc_fold / k_dc_fold8); m = 17 runs the any-M fallbacks
    (whole band: k_dc_tile + k_branch0_fir; a shard: the pruned-DFT route), and path and timed kernel say so."""
    M, frames = 4096, [40, 9, 60]
    x = _input(M, sum(frames), 904, dc=(0.02, -0.01))
    kw = dict(channels=M, demod="none", mix=True, pfb_m=m, max_frames=max(frames), flags=TIMED)
    if G > 1:
        kw.update(chan_first=3, chan_stride=G)
    ch = cs.Chain(**kw)
    outs, names, pos = [], [], 0
    for f in frames:
        outs.append(ch.process(x[pos * M:(pos + f) * M]))
        names.append(ch.kernel_time()[0])
        pos += f
    path = ch.path
    ch.close()
    got = np.concatenate(outs)
    rows = O.Chain(M, pfb_m=m).process(x)
    want = _fold(rows[3::G] if G > 1 else rows)
    tol = max(4e-7 * float(np.abs(rows).max()) * (M // G), 1e-5 * float(np.abs(want).max()))
    print(f"mix M={M} G={G} m={m} [{path}] {names}: max {np.abs(got - want).max():.3e} (tolerance {tol:.3e})")
    assert np.abs(got - want).max() < tol
    if G == 1:
        assert path == "generic+mix-identity", path
        assert set(names) == {"k_dc_fold" if m == 16 else "k_dc_tile"}, names
    else:
        assert path == ("generic+pruned-dft+shard-mix-identity" if m == 16 else "generic+pruned-dft"), path
        assert set(names) == {"k_dc_fold8" if m == 16 else "k_pfb_fir"}, names


# --------------------------------------------------------------------------- (d) rejections
@pytest.mark.parametrize("M", [1, 256])
def test_rejected_settings(M):
    bad = [dict(dc_alpha=0.0), dict(dc_alpha=1.0), dict(dc_alpha=float("nan")), dict(dc_alpha=-0.01), dict(dc_alpha=1.5)]
    bad += [dict(pfb_m=33), dict(pfb_m=1000)] if M > 1 else []
    for kw in bad:
        with pytest.raises(cs.CsdrError) as e:
            cs.Chain(channels=M, max_frames=64, **kw)
        assert e.value.code == _lib.ERR_INVALID, kw
    # without the DC blocker alpha is not read
    cs.Chain(channels=M, max_frames=64, dc_block=False, dc_alpha=0.0).close()
    for m in (1, 32):
        cs.Chain(channels=M, max_frames=64, pfb_m=m).close()
