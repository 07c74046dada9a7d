"""The fused chain routes' CF32 planes per channel, per frame and per element: case table, fixtures and bounds.  No GPU in here; shared by
test_fused_routes_cpu.py (the table, the fixtures and the bounds against themselves) and test_fused_routes_gpu.py (the library under them).

The kernels: k_tile256, k_run256v2 and its /G shard instantiations, k_run64 / k_run64v2, k_run1024v3, k_shard1024, k_front4096 + k_back4096
and the *_dcfix kernels behind them (csrc/kernels_fused*.hip, kernels_run64_v2.hip, kernels_run1024_v3.hip, kernels_shard1024.hip,
kernels_pfb4096.hip).  They split the work by run, tile, wave and lane-to-channel mappings; what the whole-array rules of the suite
(rel-RMS < 1e-5, max < 1e-4 max|ref| against the f32 oracle) do not see is one channel scaled by a few 1e-6, one frame at a tile or run
seam off by 1e-6 across the band, or 1 % of the DC state lost at a cold run start.

Truth: chain_truth.chain_truth (numpy f64).  Yardstick: the f32 oracle O.Chain.  U = 2^-24.

Fixtures (chain_truth.noise(M, nf): white noise, every channel equally strong):
  F0  the noise, DC blocker off
  F1  the noise, DC blocker on (alpha = 0.0005): the oracle's f32 blocker state of ~16 rounds at ~1e-6
  F2  the noise + (0.3, 0.2) (test_chain_params_gpu._input's DC), DC blocker on: a state of 720 that rounds at 4e-5; what a run start,
      a tile start or a dcfix kernel loses of the state shows here
Row groups: the four channels DC lands in (chain_truth.dc_rows: the blocker's error and every DC correction sit there) and all other
rows.  Every bound is evaluated per group with the oracle's figures of the same group, over every frame, the window fill included:
  (a) every channel c:   relrms_c(got) <= 2 max_c relrms_c(oracle) + d U
  (b) every element:     |got - truth| <= 4 max |oracle - truth| + 6 d U rms(truth)
  (c) every frame t:     relrms_t(got) <= 2 max_t relrms_t(oracle) + d U band_t / group_t
      relrms_t: rms over the group's rows of |got - truth| at frame t over group_t, the rms over those rows of |truth| at frame t;
      band_t: the rms over all M rows of |truth| at frame t (never taken below group_t)
  The factor band_t / group_t is the term (c) lacked as first written (d U alone) for a group of a few rows; it is 1 for a whole band and
  within 1 +- 5e-3 for the "rest" groups.  From the operations: a butterfly stage rounds at U times the size of ITS operands, and those are
  partial sums over all branches of the frame; what a stage leaves in an output bin is therefore of the order U band_t whatever the
  bin's own value turns out to be.  A bin that is small at frame t (|r_t| is Rayleigh: over n frames the smallest |r_t| of a row is about
  band_t / sqrt(n), 0.02 band_t at 2053 frames) has the absolute error of its neighbours, not a relative one.  (a) and (b) do not need the
  factor: over all frames every channel of the noise is as strong as the band.  Measured on the MI355X with d U alone:
  k_shard1024<CF32>/G8 on F0, whose DC group is the one row 510, 1.024 at frame 637 (where |r| is 0.012 of band_t) with (a) 0.18 and (b) 0.09
  on the same row; /G4 (one row) 0.49, k_run256v2<CF32>/G2 (two rows) 0.50, every four-row group <= 0.41.  With the factor: see DESIGN.md 5.
  test_fused_routes_cpu.py asserts the derivation on the radix-2 emulation of any_m_cases.py (a 256-point transform, rows in groups of
  1, 2, 4, 256): against d U band_t the worst frame of a group is 1.01, 0.72, 0.53, 0.25; against d U group_t 45, 4.8, 1.1, 0.25.
d, from the kernel's operations (never from a measured ratio):
  whole band, contiguous shard           log2 M: radix-16 butterflies (fft16_generic.h), one rounding per radix-2 stage on every path; the
                                         value any_m_cases.py uses for k_fft_r16 and k_pfb1024
  pruned interleaved shard               log2 M: k_run256v2<.., G> runs the 256-point transform with its pass-1 butterflies pruned to the
                                         rows k1' = 0 mod G (kernels_fused_v2.hip:103-109); every output still goes through eight stages, and
                                         the shard's shift W16^(a g) rides on the pre-mix phasor table (no operation of its own)
  folding interleaved shard              log2(M / G) + sqrt(G) + 1: k_shard1024<.., G> sums the G aliasing branches behind the FIR and runs
                                         a (1024 / G)-point transform (kernels_shard1024.hip:5-11); any_m_cases.d_transform's form for k_fold
With the blocker on the oracle's terms dominate (F1: ~1e-6, F2: ~5e-5 per channel on every row), so F1 and F2 are wide by what the f32
oracle itself does; F0 is the tight one (test_fused_routes_cpu.py asserts 2 max_c relrms_c(oracle) <= d U there).

Knobs and call sizes are those of test_chain_params_gpu.ROUTES and test_fm_phase_routes_gpu.SHAPE (the smallest at which each kernel
engages; test_fused_routes_cpu.py asserts the equality), the expected path and timed kernels are read from the plans' run() and name().
k_run1024v2<FM>/G2 has no CF32 instantiation (CF32 shards of stride 2 run the whole band + row gather): no case.

split, split_timed: a second cutting of the same stream that keeps every frame on the same kernel; with the blocker off (F0) nothing in
these routes depends on where the calls are cut, and the two outputs are bitwise equal.  k_run256v2 has no such case, because its output does
depend on where its runs start, and the cutting moves them: a run start pre-mixes the 13 window samples it takes over (from the carried
history or from its halo tile) with cmul (fused_common.h: one product rounded, the other inside an fma of the compiler's choosing), the
tile loop pre-mixes with cmul2_v (v_pk_mul_f32 + v_pk_fma_f32, the other product rounded).  Both are correct to one rounding of one product,
and they differ in the last bit of some samples; the 13 frames behind every run start carry it.  Measured with the calls [272, 133] against
[128, 272, 5] (run starts at frame 272 in the first, at frame 256 in the second): the frames 256 .. 265 and 272 .. 282 differ, by at most
3.9e-7 of the rms, 3.5 % of the elements (whole band), 3.8 % (G = 2), 4.0 % (G = 8), all of them inside (a), (b), (c) by the margins of
the table.  k_run64v2, k_run1024v3, k_shard1024 and k_front4096, which also start runs inside a call, are bitwise equal."""
from collections import namedtuple

import numpy as np

import any_m_cases as A
import chain_truth as T

U = T.U
KF, ALPHA = T.KF, T.ALPHA
DC_OFFSET = 0.3 + 0.2j
# fixture: (DC blocker, offset)
FIXTURES = {"F0": (False, 0.0), "F1": (True, 0.0), "F2": (True, DC_OFFSET)}
WHOLE, CONTIG, PRUNED, FOLD = "whole", "contiguous", "pruned", "fold"

T256 = [16 * 12, 16 * 9 + 5, 64]                       # k_tile256 at chunk size, ragged, and a short call
R256 = [16 * 17, 16 * 8 + 5]                           # two runs, then one run from the carried state + 5 frames of k_tile256
PD256 = [16 * 128, 16 * 128, 16 * 8 + 5, 16 * 128]     # test_dc_alpha_independent_launches
P256, P256S = "fused-256|k_tile256<CF32>", "fused-256|k_tile256<CF32>+interleaved-shard"
P4096 = "fused-4096|k_front4096+k_back4096<CF32>"

# id; M; cs.Chain keywords (chan_stride, chan_first, chan_count, dft_backward; "dc_row": chan_first = the stride's shard that owns the first
# DC row); diagnostics knobs; calls in frames; fixtures; kind of shard (the d rule); expected path; timed kernel of every call; source: the
# ROUTES id whose knobs and the SHAPE id (or None: ROUTES') whose call sizes the case restates; entry point; split
Case = namedtuple("Case", "id M kw knobs calls fixtures kind path timed source entry split split_timed")


def _case(id, M, calls, path, timed, kw=None, knobs=None, fixtures=("F0", "F1", "F2"), kind=WHOLE, source=None, entry="process", split=None,
          split_timed=None):
    timed = [timed] * len(calls) if isinstance(timed, str) else list(timed)
    if split is not None:
        split_timed = [timed[0]] * len(split) if split_timed is None else list(split_timed)
    return Case(id, M, dict(kw or {}), dict(knobs or {}), list(calls), tuple(fixtures), kind, path, timed, source, entry, split, split_timed)


RUN1, WGS3, NOWU0 = {"CSDR_RUN_MIN_TILES": "1"}, {"CSDR_RESIDENT_WGS": "3"}, {"CSDR_NOWU": "0"}
CASES = [
    _case("run64_cf32", 64, [64 * 40, 64 * 9 + 5], "fused-k_run64<CF32>", "k_run64<CF32>", source=("run64_fm", None), split=[3141]),
    _case("run64v2_cf32", 64, [64 * 128, 5, 64 * 96], "fused-k_run64<CF32>", ["k_run64v2", "k_run64<CF32>", "k_run64v2"],
          knobs={"CSDR_RUN64_V2_ALL": "1"}, source=("run64v2_cf32", None), split=[4096, 4096, 5, 6144],
          split_timed=["k_run64v2", "k_run64v2", "k_run64<CF32>", "k_run64v2"]),
    _case("tile256_cf32", 256, T256, P256, "k_tile256<CF32>", knobs={"CSDR_RUN_MIN_TILES": "1000000"}, source=("tile256_cf32", "tile256_fm"),
          split=[405]),
    _case("run256v2_cf32_nowu", 256, R256, P256, "k_run256v2<CF32>", knobs={**RUN1, **WGS3}, source=("run256v2_cf32_nowu", "run256v2_fm_nowu")),
    # the warm-up build: with the blocker off it is the code of the no-warm-up build (no F0)
    _case("run256v2_cf32_wu", 256, R256, P256, "k_run256v2<CF32>", knobs={**RUN1, **NOWU0, **WGS3}, fixtures=("F1", "F2"),
          source=("run256v2_cf32_wu", "run256v2_fm_wu")),
    _case("run256v2_cf32_g2", 256, R256, P256S, "k_run256v2<CF32>/G2", kw=dict(chan_stride=2, chan_first="dc_row"), knobs={**RUN1, **WGS3},
          kind=PRUNED, source=("run256v2_fm_g2", "run256v2_fm_g2")),
    _case("run256v2_cf32_g8", 256, R256, P256S, "k_run256v2<CF32>/G8", kw=dict(chan_stride=8, chan_first="dc_row"), knobs={**RUN1, **WGS3},
          kind=PRUNED, source=("run256v2_fm_g8", "run256v2_fm_g8")),
    # a contiguous shard takes the tile kernel, which masks its stores, at every size: rows 101 .. 157 (unaligned at both ends, the DC rows inside)
    _case("tile256_cf32_c101_C57", 256, T256, P256, "k_tile256<CF32>", kw=dict(chan_first=101, chan_count=57), knobs=RUN1, kind=CONTIG,
          source=(None, "tile256_fm"), split=[405]),
    _case("backward256_cf32", 256, T256, P256 + "+dft-backward", "k_tile256<CF32>", kw=dict(dft_backward=True),
          knobs={"CSDR_RUN_MIN_TILES": "1000000"}, source=("tile256_cf32", "tile256_fm"), split=[405]),
    # csdr_chain_submit_device: chunks of whole tiles at the run-kernel size run as independent launches whose run 0 warms its DC state up over
    # the previous chunk's saved tail; the ragged chunk in between is serialized
    _case("submit_device256_cf32", 256, PD256, P256, "k_run256v2<CF32>", knobs=RUN1, source=("run256v2_cf32_nowu", None), entry="submit_device"),
    _case("run1024v3_cf32_nowu", 1024, [2048, 5, 1024], "fused-k_run1024v3<CF32>", ["k_run1024v3<CF32>", "k_run1024<CF32>", "k_run1024v3<CF32>"],
          knobs={"CSDR_RUN1024_V3_RUNS": "8"}, source=("run1024v3_fm_nowu", None), split=[1024, 1024, 5, 1024],
          split_timed=["k_run1024v3<CF32>", "k_run1024v3<CF32>", "k_run1024<CF32>", "k_run1024v3<CF32>"]),
    _case("run1024v3_cf32_wu", 1024, [2048, 5, 1024], "fused-k_run1024v3<CF32>", ["k_run1024v3<CF32>", "k_run1024<CF32>", "k_run1024v3<CF32>"],
          knobs={"CSDR_RUN1024_V3_RUNS": "8", **NOWU0}, fixtures=("F1", "F2"), source=("run1024v3_cf32_wu", None)),
    _case("shard1024_cf32_g8", 1024, [1024, 5, 1024], "fused-k_shard1024<CF32>/G8+interleaved-shard",
          ["k_shard1024<CF32>/G8", "k_run1024<CF32>", "k_shard1024<CF32>/G8"], kw=dict(chan_stride=8, chan_first="dc_row"),
          knobs={"CSDR_SHARD1024_RUNS": "4"}, kind=FOLD, source=("shard1024_fm_g8", None), split=[512, 512, 5, 1024],
          split_timed=["k_shard1024<CF32>/G8", "k_shard1024<CF32>/G8", "k_run1024<CF32>", "k_shard1024<CF32>/G8"]),
    _case("shard1024_cf32_g4", 1024, [1024, 5, 1024], "fused-k_shard1024<CF32>/G4+interleaved-shard",
          ["k_shard1024<CF32>/G4", "k_run1024<CF32>", "k_shard1024<CF32>/G4"], kw=dict(chan_stride=4, chan_first="dc_row"),
          knobs={"CSDR_SHARD1024_RUNS": "4"}, kind=FOLD, source=("shard1024_fm_g8", None), split=[512, 512, 5, 1024],
          split_timed=["k_shard1024<CF32>/G4", "k_shard1024<CF32>/G4", "k_run1024<CF32>", "k_shard1024<CF32>/G4"]),
    _case("front4096_cf32", 4096, [40, 9], P4096, "k_front4096+k_back4096<CF32>", source=("front4096_cf32", None), split=[49]),
]
IDS = [c.id for c in CASES]
PARAMS = [(c, f) for c in CASES for f in c.fixtures]
PARAM_IDS = [f"{c.id}-{f}" for c, f in PARAMS]


# --------------------------------------------------------------------------- rows, groups, d
_DCR = {}


def dc_rows(M):
    if M not in _DCR:
        _DCR[M] = T.dc_rows(M)
    return _DCR[M]


def chain_kw(case):
    """the case's cs.Chain keywords with the shard resolved"""
    kw = dict(case.kw)
    if kw.get("chan_first") == "dc_row":
        kw["chan_first"] = int(dc_rows(case.M)[0] % kw["chan_stride"])
    return kw


def rows_of(case):
    """band row (of the forward truth) that row i of the case's output holds"""
    kw, M = chain_kw(case), case.M
    if kw.get("dft_backward"):
        return (M - np.arange(M)) % M
    G = kw.get("chan_stride", 0)
    if G > 1:
        return np.arange(kw["chan_first"], M, G)
    c0 = kw.get("chan_first", 0)
    return np.arange(c0, c0 + (kw.get("chan_count", 0) or M - c0))


def groups_of(case):
    """{"dc": output rows that hold one of the four DC channels, "rest": the others}"""
    rows = rows_of(case)
    dc = np.isin(rows, dc_rows(case.M))
    return {"dc": np.flatnonzero(dc), "rest": np.flatnonzero(~dc)}


def d_of(case):
    """the d of the module docstring"""
    G = case.kw.get("chan_stride", 0)
    if case.kind == FOLD:
        return A.d_transform(A.POW2, case.M // G, G)
    return float(np.log2(case.M))


def d_for(M, G):
    """d of the fused route that M channels at chan_stride G take: k_shard1024 (M = 1024, G = 4, 8) folds, every other one runs log2 M stages"""
    return A.d_transform(A.POW2, M // G, G) if (M == 1024 and G in (4, 8)) else float(np.log2(M))


def element_ratio(M, rows, got, truth, orc, d):
    """worst (b) ratio of an output whose row i holds band row rows[i], over the two row groups"""
    dc = np.isin(rows, dc_rows(M))
    return max(cf32_ratios(got[m], truth[m], orc[m], d)[1][0] for m in (dc, ~dc) if m.any())


# --------------------------------------------------------------------------- references
def rms_frames(a):
    """rms over the rows, per frame"""
    return np.sqrt(np.mean(np.abs(np.atleast_2d(a)) ** 2, axis=0))


def refs(case, fixture):
    """chain_truth.refs of the case's stream on a fixture, the case's rows: dict(x, r, orc_r, ...), and band: the rms over ALL rows of
    the band of |truth|, per frame.  Nobody writes into it."""
    dc, offset = FIXTURES[fixture]
    R = T.refs(case.M, sum(case.calls), dc, offset=offset)
    rows = rows_of(case)
    out = {k: (v[rows] if isinstance(v, np.ndarray) and v.ndim == 2 else v) for k, v in R.items()}
    out["band"] = rms_frames(R["r"])
    return out


# --------------------------------------------------------------------------- the bounds
relrms_rows = A.relrms_rows


def relrms_frames(got, truth):
    got, truth = np.atleast_2d(got), np.atleast_2d(truth)
    return rms_frames(got.astype(np.complex128) - truth) / rms_frames(truth)


def cf32_ratios(got, truth, orc, d, band=None):
    """the form of any_m_cases.cf32_ratios with the per-frame bound: ((a) ratio, row), ((b) ratio, (row, frame)), ((c) ratio, frame) of one
    group (rows index the group).  band: the band's rms of |truth| per frame (None: the group's own: (c) as first written)"""
    got, truth, orc = np.atleast_2d(got), np.atleast_2d(truth), np.atleast_2d(orc)
    assert got.shape == truth.shape == orc.shape, (got.shape, truth.shape, orc.shape)
    rms = float(np.sqrt(np.mean(np.abs(truth) ** 2)))
    ba = 2.0 * float(relrms_rows(orc, truth).max()) + d * U
    bb = 4.0 * float(np.abs(orc.astype(np.complex128) - truth).max()) + 6.0 * d * U * rms
    grp = rms_frames(truth)
    bc = 2.0 * float(relrms_frames(orc, truth).max()) * grp + d * U * (grp if band is None else np.maximum(band, grp))
    pa, pc = relrms_rows(got, truth), rms_frames(got.astype(np.complex128) - truth) / bc
    pb = np.abs(got.astype(np.complex128) - truth)
    ia, ic = int(np.argmax(pa)), int(np.argmax(pc))
    ib = np.unravel_index(int(np.argmax(pb)), pb.shape)
    return (float(pa[ia]) / ba, ia), (float(pb[ib]) / bb, (int(ib[0]), int(ib[1]))), (float(pc[ic]), ic)


def check_groups(case, got, R, orc=None):
    """(a), (b), (c) per group of the case -> {group: ((a, band row), (b, (band row, frame)), (c, frame))}; the rows are the band's"""
    rows, out = rows_of(case), {}
    orc = R["orc_r"] if orc is None else orc
    for name, idx in groups_of(case).items():
        if not idx.size:
            continue
        (a, ia), (b, ib), (c, ic) = cf32_ratios(got[idx], R["r"][idx], orc[idx], d_of(case), R["band"])
        out[name] = ((a, int(rows[idx[ia]])), (b, (int(rows[idx[ib[0]]]), ib[1])), (c, ic))
    return out


def worst(res):
    """the three worst ratios over the groups"""
    return tuple(max(res[g][i][0] for g in res) for i in range(3))


def describe(res):
    return "; ".join(f"{g}: (a) {r[0][0]:.3f} row {r[0][1]}, (b) {r[1][0]:.3f} row {r[1][1][0]} frame {r[1][1][1]}, (c) {r[2][0]:.3f} frame {r[2][1]}"
                     for g, r in res.items())


def array_rule(got, ref):
    """the suite's whole-array rule (test_gpu_parity.py, test_bench_layout_*): rel-RMS < 1e-5 and max < 1e-4 max|ref|"""
    e = np.abs(got.astype(np.complex128) - ref)
    return float(np.sqrt(np.mean(e ** 2) / np.mean(np.abs(ref) ** 2))) < 1e-5 and float(e.max()) < 1e-4 * float(np.abs(ref).max())


# --------------------------------------------------------------------------- the mutation of a run start
def truth_with_state_loss(x, M, frame, factor, alpha=ALPHA):
    """the f64 chain on x with the DC blocker's state scaled by `factor` in front of `frame`: a run start that loses 1 - factor of it"""
    from scipy.signal import lfilter
    b, a = [1.0, -1.0], [1.0, -T.beta_of(alpha)]
    x = np.asarray(x, np.complex128)
    n = frame * M
    y0, z = lfilter(b, a, x[:n], zi=np.zeros(1, np.complex128))       # z = -alpha v[n - 1]: scaling it scales the state v
    y1, _ = lfilter(b, a, x[n:], zi=z * factor)
    return T.channelize(np.concatenate([y0, y1]), M)
