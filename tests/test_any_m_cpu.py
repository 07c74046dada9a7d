"""What test_any_m_gpu.py relies on, asserted without a GPU: the case table against the code's rules, the oracle inside the bounds it
sets, the f32 emulations of k_dft_direct, k_fft_pow2 and k_fold inside half of the d U terms, and three mutations that the per-channel
bound (a) catches (one of which the suite's whole-array rule passes)."""
import numpy as np
import pytest

import any_m_cases as A
import chain_truth as T
import oracle_lib as O
from util import rel_rms

U = A.U
MS = sorted({c.M for c in A.ALL_CASES})
SINCOS_M = (3, 5, 6, 7, 12, 20, 24, 48, 100, 1000)


# --------------------------------------------------------------------------- the table against the code's rules
def test_table_matches_launch_dft_rule():
    assert len({c.id for c in A.ALL_CASES}) == len(A.ALL_CASES)
    for c in A.ALL_CASES:
        G, rows = A.shard_of(c)
        assert c.M % G == 0 and rows.size and rows.max() < c.M, c.id
        N = c.M // G
        if c.dft == A.PFB1024:                         # GenericPlan::init use1024: k_pfb1024 in place of FIR + launch_dft
            assert (c.M, G) == (1024, 1) and not c.kw.get("mix") and "CSDR_NO_PFB1024" not in c.knobs, c.id
            assert (c.path, c.timed) == ("generic+pfb1024", "k_pfb1024"), c.id
        else:
            assert c.dft == A.dft_kernel(N), (c.id, N)
            assert c.timed == "k_pfb_fir", c.id
        assert c.path.startswith("generic+pruned-dft" if G > 1 else "generic"), c.id
        assert max(c.calls) <= (c.max_frames or max(c.calls)) and sum(c.calls) <= A.nf_of(c.M) - (A.SEEK if c in A.SEEK_CASES else 0), c.id


def test_table_covers_what_it_claims():
    def ragged(c, tile):
        return any(f % tile for f in c.calls if f)
    by = {}
    for c in A.A_CASES + A.B_CASES:
        by.setdefault(c.dft, []).append(c)
    # every arm of launch_dft (and k_pfb1024): ragged against its tile, and across a call boundary
    for k, tile in ((A.POW2, 1), (A.R16_4, 4), (A.R16_16, 1), (A.PFB1024, 4), (A.DIRECT, 1)):
        assert any(len([f for f in c.calls if f]) > 1 and (tile == 1 or ragged(c, tile)) for c in by[k]), k
    pow2 = {c.M // A.shard_of(c)[0] for c in by[A.POW2]}
    assert pow2 & {2, 4, 8, 16, 32, 64, 128} and 512 in pow2 and pow2 & {2048, 8192}      # 64 threads; 256 threads; strided loops
    assert max(c.M // A.shard_of(c)[0] for c in by[A.DIRECT]) >= 1000
    tab = {A.nco_table(c.M)[0] for c in A.ALL_CASES}
    assert tab == {True, False}
    assert any(c.M == 1024 and c.max_frames == 1 and c.dft == A.PFB1024 for c in A.A_CASES)          # the d_B small-plane arm
    for c0_C in [(m, c0, C) for m, c0, C, _ in A.CONTIG]:
        assert c0_C[1] % 32 and c0_C[2] % 32                                                      # unaligned contiguous shards
    ends = {(c.kw.get("demod"), bool(c.kw.get("mix"))) for c in A.B_CASES if c.kw.get("chan_count")}
    assert ends == {("none", False), ("fm", False), ("none", True), ("fm", True)}
    assert any(G & (G - 1) for _, G, _ in A.INTERLEAVED)                                          # k_fold at a G that is no power of two
    assert all(len(A.shard_of(c)[1]) <= 12 for c in A.B_CASES if c.kw.get("mix") and c.kw.get("demod") == "fm")
    # the table path with an odd tab_pos: M = 257, the second call starts on an odd frame
    odd = [c for c in A.A_CASES if c.M == 257 and A.nco_table(257)[0] and c.calls[0] % 2]
    assert odd and any(c.calls[-1] * 257 >= 2 * 4096 for c in odd)


def test_nco_period_classes():
    for M in MS:
        tab, per, w = A.nco_table(M)
        assert tab == (M not in SINCOS_M), (M, hex(w), per)
        if M & (M - 1) == 0:
            assert tab and (per % M == 0 or M % per == 0), (M, per)
    assert set(SINCOS_M) <= set(MS)
    tab, per, w = A.nco_table(257)
    assert (tab, per, w) == (True, 131072, 0x807F8000)
    assert (33 * 257) % per % 2 == 1                   # tab_pos of the call behind 33 frames


# --------------------------------------------------------------------------- the oracle inside its own bounds
def _cf32_views(c, R0):
    """(truth, oracle) of a CF32 case: rows of the band, or the one mixed row"""
    G, rows = A.shard_of(c)
    f0 = A.SEEK + 14 if c in A.SEEK_CASES else 0
    f1 = (A.SEEK if c in A.SEEK_CASES else 0) + sum(c.calls)
    R = A.sub(R0, rows, f0, f1)
    if c.kw.get("mix"):
        return R, R["r"].sum(axis=0), A.fold32(R["orc_r"])
    return R, R["r"], R["orc_r"]


@pytest.mark.parametrize("M", MS)
def test_oracle_is_inside_the_bounds(M):
    for c in [c for c in A.A_CASES + A.SPLIT_CASES + A.B_CASES + A.SEEK_CASES if c.M == M]:
        R0 = A.refs(M, c.kw.get("dc_block", True))
        R, truth, orc = _cf32_views(c, R0)
        a, b = A.cf32_ratios(orc, truth, orc, A.d_of(c), orc_factor=0.5)
        assert a <= 1.0 and b <= 1.0, (c.id, a, b)
        pc = A.relrms_rows(orc, truth)
        if sum(c.calls) >= A.NF_LARGE and not c.kw.get("mix"):         # measured: 0.4e-6 .. 2.7e-6 over the whole streams
            assert 1e-7 < pc.max() < 4e-6, (c.id, pc.max())
        if c.kw.get("demod") != "fm":
            continue
        E = T.cf32_E(R)
        if c.kw.get("mix"):
            ratio, out = A.fm_mix_ratio(A.fold32(R["orc_fm"]), R, E)
            print(f"{c.id}: oracle FM --mix worst ratio {ratio:.3f}, {100 * out:.2f} % of the samples left out")
            assert ratio <= 1.0 and out <= 0.01, (c.id, ratio, out)
        else:
            worst, bias, bb = T.check_fm(f"{c.id} oracle", R["orc_fm"], R, E, T.phi17())
            assert worst <= 1.0 and np.abs(bias).max() <= bb, (c.id, worst, bias, bb)


@pytest.mark.parametrize("M", [3, 100, 257])
def test_agc_threshold_leaves_the_squelch_open(M):
    thr = A.agc_threshold_db(M)
    R = A.refs(M)
    level = 10.0 * np.log10(np.mean(np.abs(R["r"][R["counted"]]) ** 2))
    assert thr != 0.0 and 14.0 <= level - thr <= 16.0, (M, level, thr)
    y = O.Chain(M, agc_db=thr).process(R["x"])
    assert (y != 0).mean() > 0.5, (M, thr, float((y != 0).mean()))       # what the GPU test asks of the library's output


# --------------------------------------------------------------------------- the emulations at half the d U terms
EMU = sorted({(c.dft, c.M, A.shard_of(c)[0]) for c in A.A_CASES + A.B_CASES}, key=lambda t: (t[1], t[2]))


def _emu_case(kernel, M, G, g=None, bins=None, **mut):
    """emulated transform of the truth's FIR plane rounded to f32 -> (got [rows][nf], exact transform of the same f32 plane, truth rows)"""
    R = A.refs(M)
    X32 = A.fir_plane(R).astype(np.complex64)
    N = M // G
    rows = np.arange(N) if bins is None else np.asarray(bins)
    if G > 1:
        Z = A.emu_fold(X32, G, g, **mut)
        got = A.emu_dft(Z, kernel, bins)
        band = g + G * rows
    else:
        got = A.emu_dft_direct(X32, bins, **mut) if mut else A.emu_dft(X32, kernel, bins)
        band = rows
    exact = np.fft.fft(X32.astype(np.complex128), axis=1)[:, band]
    return got.T, exact.T, R["r"][band]


@pytest.mark.parametrize("kernel,M,G", EMU, ids=[f"{k}_{M}_G{G}" for k, M, G in EMU])
def test_emulated_transforms_stay_inside_half_the_d_term(kernel, M, G):
    N = M // G
    d = A.d_transform(kernel, N, G)
    bins = np.arange(0, N, N // 64) if N >= 16384 else None
    worst_a = worst_b = 0.0
    for g in (sorted({0, 1, G - 1}) if G > 1 else [None]):
        got, exact, truth = _emu_case(kernel, M, G, g, bins)
        per_bin = np.sqrt(np.mean(np.abs(got - exact) ** 2, axis=1) / np.mean(np.abs(truth) ** 2, axis=1))
        per_el = np.abs(got - exact).max() / np.sqrt(np.mean(np.abs(truth) ** 2))
        worst_a, worst_b = max(worst_a, per_bin.max() / (d * U)), max(worst_b, per_el / (6 * d * U))
        mean_c = float(np.sqrt(np.mean(per_bin ** 2)) / (d * U))
    print(f"{kernel} N={N} G={G}: rms over bins {mean_c:.3f} d U; worst bin {worst_a:.3f} d U; worst element {worst_b:.3f} of 6 d U rms")
    assert worst_a <= 0.5, (kernel, N, G, worst_a)
    assert worst_b <= 0.5, (kernel, N, G, worst_b)


# --------------------------------------------------------------------------- mutations
def test_one_channel_off_by_2e_4_passes_the_array_rule_and_fails_a():
    M = 8192
    R = A.refs(M)
    c = next(c for c in A.A_CASES if c.M == M)
    # a channel whose largest sample is under 0.45 of the array's: 2e-4 of it then stays under the rule's 1e-4 max|ref| as well
    peak = np.abs(R["orc_r"]).max(axis=1)
    ch = 4321 + int(np.argmax(peak[4321:] < 0.45 * peak.max()))
    assert peak[ch] < 0.45 * peak.max()
    mut = R["orc_r"].copy()
    mut[ch] *= np.complex64(1 + 2e-4)
    e, mx = rel_rms(mut, R["orc_r"]), float(np.abs(mut - R["orc_r"]).max())
    assert e < 1e-5 and mx < 1e-4 * np.abs(R["orc_r"]).max(), (e, mx)           # test_chain_matches_oracle's rule: passes
    a0, b0 = A.cf32_ratios(R["orc_r"], R["r"], R["orc_r"], A.d_of(c))
    a, b = A.cf32_ratios(mut, R["r"], R["orc_r"], A.d_of(c))
    print(f"array rel-rms {e:.2e}, max {mx:.2e}; (a) ratio {a0:.3f} -> {a:.3f}, (b) ratio {b0:.3f} -> {b:.3f}")
    assert a0 <= 1.0 and b0 <= 1.0 and a > 1.0, (a0, b0, a)


@pytest.mark.parametrize("M", [100, 1000])
def test_direct_dft_with_one_twiddle_index_off_by_one_fails_a(M):
    R = A.refs(M)
    c = next(c for c in A.A_CASES if c.M == M)
    bins = np.arange(0, M, max(1, M // 50))
    k, j = int(bins[7]), M // 2 + 1
    good, _, truth = _emu_case(A.DIRECT, M, 1, bins=bins)
    bad, _, _ = _emu_case(A.DIRECT, M, 1, bins=bins, off_by_one=(k, j))
    orc = R["orc_r"][bins]
    a0, _ = A.cf32_ratios(good, truth, orc, A.d_of(c))
    a1, _ = A.cf32_ratios(bad, truth, orc, A.d_of(c))
    print(f"M={M}: (a) ratio {a0:.3f}, with twiddle {j} of bin {k} off by one {a1:.3f}")
    assert a0 <= 1.0 < a1, (a0, a1)
    assert (np.abs(bad - good).max(axis=1) > 0).sum() == 1                      # confined to the one bin


def test_fold_with_the_next_shards_phasors_fails_a():
    M, G, g = 100, 5, 1
    R = A.refs(M)
    c = next(c for c in A.B_CASES if c.M == M and c.kw.get("chan_stride") == G and c.kw["chan_first"] == g)
    good, _, truth = _emu_case(A.DIRECT, M, G, g)
    bad, _, _ = _emu_case(A.DIRECT, M, G, g, ph_g=g + 1)
    orc = R["orc_r"][g::G]
    a0, _ = A.cf32_ratios(good, truth, orc, A.d_of(c))
    a1, _ = A.cf32_ratios(bad, truth, orc, A.d_of(c))
    print(f"k_fold M={M} G={G} g={g}: (a) ratio {a0:.3f}, with ph[j2] of shard {g + 1}: {a1:.3f}")
    assert a0 <= 1.0 < a1, (a0, a1)
