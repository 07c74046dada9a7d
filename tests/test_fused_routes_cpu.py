"""What test_fused_routes_gpu.py relies on, asserted without a GPU: the case table of fused_cases.py against the tables and rules it
restates, the fixture conditions, the mutations that the bounds (a), (b), (c) catch and the suite's whole-array rule passes, and the f32
oracle inside the bounds it sets."""
import inspect

import numpy as np
import pytest

import any_m_cases as A
import chain_truth as T
import fused_cases as F

U = F.U
# the largest stream of every M of the table: the shorter ones are its prefixes (the chain is causal)
LARGEST = {M: max(sum(c.calls) for c in F.CASES if c.M == M) for M in sorted({c.M for c in F.CASES})}
FIRST = {M: next(c for c in F.CASES if c.M == M and sum(c.calls) == nf and c.kind == F.WHOLE and not c.kw) for M, nf in LARGEST.items()}


def _whole(M, fixture, nf=None):
    """the whole band's refs of M on a fixture"""
    dc, offset = F.FIXTURES[fixture]
    R = dict(T.refs(M, nf or LARGEST[M], dc, offset=offset))
    R["band"] = F.rms_frames(R["r"])
    return R


# --------------------------------------------------------------------------- 1: the table against the rules it restates
def test_table_restates_the_source_tables():
    """knobs and call sizes are those of test_chain_params_gpu.ROUTES and test_fm_phase_routes_gpu.SHAPE (both modules need the built
    library to import)"""
    import test_chain_params_gpu as P
    import test_fm_phase_routes_gpu as Q
    routes = {r[0]: r for r in P.ROUTES}
    assert len(set(F.IDS)) == len(F.IDS)
    for c in F.CASES:
        rid, sid = c.source
        knobs, calls = {}, None
        if rid is not None:
            knobs, calls = dict(routes[rid][3]), list(routes[rid][4])
        if sid is not None:
            frames, extra, _ = Q.SHAPE[sid]
            knobs.update(extra)
            calls = list(frames) if frames else calls
        if c.entry == "submit_device":
            assert "frames = 256, [16 * 128, 16 * 128, 16 * 8 + 5, 16 * 128]" in inspect.getsource(P.test_dc_alpha_independent_launches)
            assert 'knob(monkeypatch, "CSDR_RUN_MIN_TILES", "1")' in inspect.getsource(P.test_dc_alpha_independent_launches)
            calls = F.PD256
        if rid is not None:
            assert c.knobs == knobs, (c.id, c.knobs, knobs)
            assert c.M == routes[rid][1], c.id
        assert c.calls == calls, (c.id, c.calls, calls)
        # the shard of a ROUTES row: the one that owns a channel next to DC
        G = c.kw.get("chan_stride", 0)
        if G > 1:
            assert F.chain_kw(c)["chan_first"] == int(P._dc_rows(c.M)[0] % G), c.id
    # every CF32 kernel the issue names has its case; k_run1024v2<FM>/G2 has no CF32 instantiation
    timed = {t for c in F.CASES for t in c.timed}
    assert timed == {"k_tile256<CF32>", "k_run256v2<CF32>", "k_run256v2<CF32>/G2", "k_run256v2<CF32>/G8", "k_run64<CF32>", "k_run64v2",
                     "k_run1024v3<CF32>", "k_run1024<CF32>", "k_shard1024<CF32>/G8", "k_shard1024<CF32>/G4", "k_front4096+k_back4096<CF32>"}
    assert not any("k_run1024v2" in t for t in timed)


def test_table_follows_its_rules():
    for c in F.CASES:
        nf = sum(c.calls)
        assert (c.M, nf) in T.SHAPES, (c.id, nf)
        assert len(c.timed) == len(c.calls), c.id
        assert c.path.startswith("fused-"), c.id
        # d: log2 M for a whole band, a contiguous shard and the pruned transform; the fold's form for k_shard1024
        G = c.kw.get("chan_stride", 0)
        if c.kind == F.FOLD:
            assert G > 1 and all("k_shard1024" in t or t == "k_run1024<CF32>" for t in c.timed), c.id
            assert F.d_of(c) == A.d_transform(A.POW2, c.M // G, G) == np.log2(c.M // G) + np.sqrt(G) + 1, c.id
        else:
            assert (c.kind == F.PRUNED) == (G > 1), c.id
            assert (c.kind == F.CONTIG) == bool(c.kw.get("chan_count")), c.id
            assert F.d_of(c) == np.log2(c.M), c.id
        assert ("+interleaved-shard" in c.path) == (G > 1) and ("+dft-backward" in c.path) == bool(c.kw.get("dft_backward")), c.id
        # every case on F0, F1, F2; the warm-up builds without F0
        assert c.fixtures == (("F1", "F2") if c.knobs.get("CSDR_NOWU") == "0" else ("F0", "F1", "F2")), c.id
        # rows and groups: every shard owns a DC row; the contiguous shard is unaligned at both ends
        rows, g = F.rows_of(c), F.groups_of(c)
        assert rows.size == len(set(rows.tolist())) and g["dc"].size >= 1 and g["rest"].size >= 1, c.id
        assert set(rows[g["dc"]].tolist()) <= set(F.dc_rows(c.M).tolist()), c.id
        if c.kind in (F.WHOLE,):
            assert g["dc"].size == 4 and rows.size == c.M, c.id
        if c.kind == F.CONTIG:
            assert rows[0] % 16 and (rows[-1] + 1) % 16 and g["dc"].size == 4, c.id
        if c.kw.get("dft_backward"):
            assert rows[0] == 0 and rows[1] == c.M - 1 and rows[-1] == 1, c.id
        # the second cutting covers the same stream and is another one
        if c.split is not None:
            assert sum(c.split) == nf and c.split != c.calls and "F0" in c.fixtures and len(c.split_timed) == len(c.split), c.id
            assert set(c.split_timed) <= set(c.timed) | {"k_tile256<CF32>"}, c.id
    assert [c.M for c in F.CASES] == sorted(c.M for c in F.CASES)       # M by M: the reference cache holds one M at a time
    assert any(c.entry == "submit_device" and "F2" in c.fixtures for c in F.CASES)


# --------------------------------------------------------------------------- 2: the fixture conditions
@pytest.mark.parametrize("M", list(LARGEST))
def test_on_f0_the_oracle_term_does_not_dominate(M):
    """2 max_c relrms_c(oracle) <= d U with the smallest d of the M's cases (measured 1.9e-7 .. 2.5e-7 against 3.6e-7 .. 7.2e-7)"""
    R = _whole(M, "F0")
    d = min(F.d_of(c) for c in F.CASES if c.M == M)
    e = 2.0 * float(F.relrms_rows(R["orc_r"], R["r"]).max())
    print(f"M={M}: 2 max_c relrms_c(oracle) {e:.3e}, d U {d * U:.3e}")
    assert e <= d * U, (M, e, d * U)


@pytest.mark.parametrize("M", list(LARGEST))
def test_on_f2_both_groups_of_the_oracle_are_finite_and_non_empty(M):
    R = _whole(M, "F2")
    for c in [c for c in F.CASES if c.M == M]:
        rows = F.rows_of(c)
        for name, idx in F.groups_of(c).items():
            assert idx.size, (c.id, name)
            pa = F.relrms_rows(R["orc_r"][rows[idx]], R["r"][rows[idx]])
            pc = F.relrms_frames(R["orc_r"][rows[idx]], R["r"][rows[idx]])
            assert np.isfinite(pa).all() and np.isfinite(pc).all() and pa.max() > 0, (c.id, name)


def test_per_frame_rounding_scales_with_the_band_and_not_with_the_group():
    """the term of (c) that fused_cases.py derives: the radix-2 emulation of a 256-point transform (any_m_cases.emu_fft_pow2, d = 8) on
    the F0 truth's FIR plane, the rows taken in groups of 1, 2, 4 and 256.  The per-frame rms of its rounding error stays inside half of
    d U band_t for the whole band (measured 0.25), inside d U band_t for every group of four (0.53: the DC group of a whole band) and
    inside half of (b)'s 6 d U band_t for a single row (1.01: one element, whose tail (b) holds with its factor 6; in (c) the oracle's
    term stands beside it).  It is no relative error of the group's own samples: against d U group_t the median one-row group reaches
    4.5 and the worst 45, the worst group of four 1.1"""
    M, nf, d = 256, 405, 8.0
    R = _whole(M, "F0", nf)
    X32 = A.fir_plane(R).astype(np.complex64)
    err = np.abs(A.emu_fft_pow2(X32).T - np.fft.fft(X32.astype(np.complex128), axis=1).T)        # [M][nf]
    vs_band, vs_group = {}, {}
    for C in (1, 2, 4, 256):
        e = np.sqrt((err ** 2).reshape(M // C, C, nf).mean(axis=1))
        g = np.sqrt((np.abs(R["r"]) ** 2).reshape(M // C, C, nf).mean(axis=1))
        vs_band[C], vs_group[C] = (e / (d * U * R["band"])).max(axis=1), (e / (d * U * g)).max(axis=1)
        print(f"groups of {C}: worst frame against d U band_t {vs_band[C].max():.3f} (median group {np.median(vs_band[C]):.3f}); "
              f"against d U group_t {vs_group[C].max():.3f} (median group {np.median(vs_group[C]):.3f})")
    assert vs_band[256].max() <= 0.5 and vs_band[4].max() <= 1.0 and vs_band[1].max() <= 3.0, {C: v.max() for C, v in vs_band.items()}
    assert np.median(vs_group[1]) > 2.0 and vs_group[1].max() > 10.0, (np.median(vs_group[1]), vs_group[1].max())


# --------------------------------------------------------------------------- 3: mutations
def _fails(res, group):
    return tuple(r[0] > 1.0 for r in res[group])


@pytest.mark.parametrize("M", list(LARGEST))
def test_mutations_of_the_truth_on_f0(M):
    """one channel times (1 + 3e-6), one frame times (1 + 2e-6) across the band, one element off by 2e-5 rms(truth): the whole-array
    rule passes each, and (a), (c), (b) fail in turn"""
    c = FIRST[M]
    R = _whole(M, "F0")
    truth, orc = R["r"], R["orc_r"]
    assert np.array_equal(F.rows_of(c), np.arange(M))
    row, frame = (5 * M) // 8 + 3, truth.shape[1] // 2 + 1
    assert row not in F.dc_rows(M)
    rms = float(np.sqrt(np.mean(np.abs(truth) ** 2)))
    muts = {"channel": truth.copy(), "frame": truth.copy(), "element": truth.copy()}
    muts["channel"][row] *= 1 + 3e-6
    muts["frame"][:, frame] *= 1 + 2e-6
    muts["element"][row, frame] += 2e-5 * rms
    base = F.check_groups(c, truth.astype(np.complex64), R)
    assert max(F.worst(base)) <= 1.0, F.describe(base)                       # the truth rounded to f32 passes
    for name, i in (("channel", 0), ("frame", 2), ("element", 1)):
        got = muts[name]
        assert F.array_rule(got, orc), name
        res = F.check_groups(c, got, R)
        print(f"M={M} {name}: {F.describe(res)}")
        assert _fails(res, "rest")[i], (name, F.describe(res))
        where = res["rest"][i][1]
        assert (where == row if i == 0 else where == (row, frame) if i == 1 else where == frame), (name, where)


@pytest.mark.parametrize("fixture", ["F1", "F2"])
def test_one_per_cent_of_the_dc_state_lost_at_a_run_boundary(fixture):
    """M = 256, 405 frames, the state times 0.99 in front of frame 272 (the second call of R256): the DC rows fail (a), (b) and (c), by
    18 / 17 / 49 on F1 and 47 / 101 / 282 on F2 (the other rows by 1.06 / 1.7 / 1.3 and 3.1 / 9.1 / 9.3: the DC rows are a group of their own).
    Against the whole-array rule, measured: on F1 the rel-RMS is 4.9e-6 (passes) and the largest element 1.39 of 1e-4 max|ref| (the
    one frame behind the boundary on row 127: fails by that); on F2 a state of 720 makes 1 % coarse enough for both parts (5.8e-4, 91x).
    So the rule is passed outright by a smaller loss: 0.2 % on F1, which the DC rows still fail on all three (3.7 / 3.4 / 10)."""
    c = next(c for c in F.CASES if c.id == "run256v2_cf32_nowu")
    M, nf = c.M, sum(c.calls)
    R = _whole(M, fixture, nf)
    got = F.truth_with_state_loss(R["x"], M, c.calls[0], 0.99)
    assert np.abs(got[:, :c.calls[0]] - R["r"][:, :c.calls[0]]).max() <= 1e-9 * np.abs(R["r"]).max()
    same = F.truth_with_state_loss(R["x"], M, c.calls[0], 1.0)
    assert np.abs(same - R["r"]).max() <= 1e-9 * np.abs(R["r"]).max()
    res = F.check_groups(c, got, R)
    print(f"{fixture} 0.99: {F.describe(res)}")
    assert _fails(res, "dc") == (True, True, True), F.describe(res)
    assert min(r[0] for r in res["dc"]) >= 10.0, F.describe(res)
    assert res["dc"][2][1] >= c.calls[0] and res["dc"][1][1][1] >= c.calls[0]      # found behind the boundary
    if fixture == "F1":
        e = got - R["orc_r"]
        assert np.sqrt(np.mean(np.abs(e) ** 2) / np.mean(np.abs(R["orc_r"]) ** 2)) < 1e-5
        small = F.truth_with_state_loss(R["x"], M, c.calls[0], 0.998)
        assert F.array_rule(small, R["orc_r"])
        res = F.check_groups(c, small, R)
        print(f"{fixture} 0.998: {F.describe(res)}")
        assert _fails(res, "dc") == (True, True, True), F.describe(res)


# --------------------------------------------------------------------------- 4: the oracle inside its own bounds
@pytest.mark.parametrize("fixture", list(F.FIXTURES))
@pytest.mark.parametrize("M", list(LARGEST))
def test_oracle_is_inside_the_bounds(M, fixture):
    R0 = _whole(M, fixture)
    for c in [c for c in F.CASES if c.M == M and fixture in c.fixtures]:
        rows, nf = F.rows_of(c), sum(c.calls)
        R = {"r": R0["r"][rows, :nf], "orc_r": R0["orc_r"][rows, :nf], "band": R0["band"][:nf]}
        res = F.check_groups(c, R["orc_r"], R)
        print(f"{c.id} {fixture}: {F.describe(res)}")
        assert max(F.worst(res)) <= 1.0, (c.id, F.describe(res))
