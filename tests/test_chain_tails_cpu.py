"""What test_chain_tails_gpu.py relies on, asserted without a GPU: the twin decomposition is the oracle's own, the f64 truths against
direct loops, the case table against the library's rules, and six mutations of the tail that the per-row bounds of chain_tail_cases.py
catch -- one of which (a row carrying its neighbour's output) the acceptances of test_chain_wbfm_matches_oracle and
test_chain_am_matches_oracle let through."""
import numpy as np
import pytest

import chain_tail_cases as K
import chain_truth as T
import oracle_lib as O
from synth import synth_cf32

FC, DECIM = 0.025, 4
CALLS = [96, 32, 64, 8, 100]                 # 300 frames, every call a multiple of 4


def _stream(chain, x, M, calls):
    outs, pos = [], 0
    for f in calls:
        outs.append(chain.process(x[pos * M:(pos + f) * M]))
        pos += f
    return np.concatenate(outs, axis=-1)


# --------------------------------------------------------------------------- 1. the twin decomposition is the oracle's own
@pytest.mark.parametrize("M", [1, 8, 20])
@pytest.mark.parametrize("agc", [False, True])
@pytest.mark.parametrize("mix", [False, True])
def test_oracle_chain_is_its_twin_plus_the_tail_blocks(M, agc, mix):
    """O.Chain(demod="wbfm") = O.Butter2 + O.FirDecim per row behind O.Chain(demod="fm", kf=0.6); O.Chain(demod="am") = O.AmpDem per row
    behind O.Chain(demod="none"); --mix = the f32 left fold of the rows (orc_mix_f32): bit for bit, over a stream of five calls"""
    nf = sum(CALLS)
    agc = K.agc_db(M) if agc else 0.0
    x = K.keyed(M, nf, seed=11 + M) if agc else T.noise(M, nf)
    twin_fm = _stream(O.Chain(M, demod="fm", kf=K.KF_WB, agc_db=agc), x, M, CALLS).reshape(M, nf)
    twin_no = _stream(O.Chain(M, demod="none", agc_db=agc), x, M, CALLS).reshape(M, nf)
    wb = _stream(O.Chain(M, demod="wbfm", decim=DECIM, deemph_fc=FC, agc_db=agc, mix=mix), x, M, CALLS)
    am = _stream(O.Chain(M, demod="am", agc_db=agc, mix=mix), x, M, CALLS)
    want_wb, want_am = K.wbfm_tail_oracle(twin_fm, FC, DECIM), K.am_tail_oracle(twin_no)
    if mix and M > 1:
        want_wb, want_am = K.fold32(want_wb), K.fold32(want_am)
        assert wb.shape == (nf // DECIM,) and am.shape == (nf,)
    else:
        assert wb.shape == (M, nf // DECIM) and am.shape == (M, nf)
    assert wb.dtype == am.dtype == np.float32
    assert np.array_equal(wb.view(np.uint32), want_wb.reshape(wb.shape).view(np.uint32)), (M, agc, mix)
    assert np.array_equal(am.view(np.uint32), want_am.reshape(am.shape).view(np.uint32)), (M, agc, mix)
    if agc and M > 1:
        muted = float((twin_no == 0).mean())
        print(f"M={M} keyed signal behind the AGC at {agc} dB: {100 * muted:.1f} % of the plane muted")


def test_keyed_signal_opens_and_mutes_rows_behind_the_agc():
    """the AGC cases' fixture at their threshold: rows open, mute and time out inside the stream (the oracle's squelch)"""
    M, nf = 20, 4312
    z = O.Chain(M, demod="none", agc_db=K.agc_db(M)).process(K.fixture("keyed", M, nf))
    open_rows = (z != 0).mean(axis=1)
    print(f"keyed M={M}: open share per row min {open_rows.min():.2f} max {open_rows.max():.2f}, overall {float((z != 0).mean()):.2f}")
    assert 0.02 < float((z != 0).mean()) < 0.98
    # a row that is open for a while and muted for a while: both transitions happen inside the stream
    assert np.sum((open_rows > 0.1) & (open_rows < 0.9)) >= 3


# --------------------------------------------------------------------------- 2. the truths and the table
def test_truths_against_direct_loops():
    rng = np.random.default_rng(3)
    n, d = 120, 5
    z = ((rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n))) * [[1.0], [0.01]]).astype(np.complex64)
    out, q = K.am_tail_truth(z)
    al, be = float(np.float32(0.01)), float(np.float32(1) - np.float32(0.01))
    for c in range(2):
        qq = 0.0
        for t in range(n):
            m = np.hypot(float(z[c, t].real), float(z[c, t].imag))
            qq = al * m + be * qq
            assert abs(q[c, t] - qq) <= 1e-15 * max(1.0, qq) and abs(out[c, t] - 2.0 * (m - qq)) <= 1e-14, (c, t)
    f = rng.standard_normal((2, n)).astype(np.float32)
    b, a, h = (v.astype(np.float64) for v in K.design(0.0021, d))
    assert a[0] == 1.0 and h.size == 2 * d * 10 + 1
    y, bq = K.wbfm_tail_truth(f, 0.0021, d)
    assert y.shape == (2, n // d)
    for c in range(2):
        v = np.zeros(n)
        for t in range(n):
            v[t] = sum(b[i] * float(f[c, t - i]) for i in range(3) if t >= i) - sum(a[i] * v[t - i] for i in (1, 2) if t >= i)
        assert np.abs(v - bq[c]).max() <= 1e-12 * np.abs(v).max()
        for j in range(n // d):
            s = sum(h[i] * bq[c, j * d - i] for i in range(h.size) if j * d - i >= 0)
            assert abs(s - y[c, j]) <= 1e-13, (c, j)
    # the bounds' parts: a mixed row against the sum, a row of zeros reproduced exactly
    ref = K.reference("wbfm", f, 0.0021, d)
    assert K.worst(ref.orc, ref, False)[0] <= 0.5 and K.worst(K.fold32(ref.orc), ref, True)[0] <= 1.0
    zero = K.reference("am", np.zeros((1, 40), np.complex64))
    assert zero.bound[0] == 0.0 and K.worst(np.zeros((1, 40), np.float32), zero, False)[0] == 0.0
    assert K.worst(np.full((1, 40), 1e-30, np.float32), zero, False)[0] == np.inf


def test_table_against_the_librarys_rules():
    from composable_sdr_amd import _lib
    assert len({c.id for c in K.ALL_CASES}) == len(K.ALL_CASES)
    for c in K.ALL_CASES:
        d = c.kw.get("decim", 1)
        assert c.demod in ("am", "wbfm") and (d == 1 or c.demod == "wbfm"), c.id
        assert all(f > 0 and f % d == 0 for f in c.calls), (c.id, c.calls)                  # firDecim's `div`: every call a multiple of decim
        assert max(c.calls) <= c.max_frames and len(c.timed) == len(c.calls), c.id
        assert f"+{c.demod}" in c.path and all(hasattr(_lib, f) for f in c.flags), c.id     # the expected path substrings are there
        assert K.twin_kw(c).get("mix") is None and K.twin_kw(c)["demod"] in ("none", "fm"), c.id
        assert K.n_out(c, c.calls[0]) == (1 if K.mixed(c) else K.rows_of(c)) * (c.calls[0] // d), c.id
        agc = c.kw.get("agc", 0.0) != 0.0
        assert not agc or c.kw["agc"] == K.agc_db(c.M), c.id
        assert (c.fix == "keyed") == agc, c.id
        spec = agc and "FLAG_AGC_SEQUENTIAL" not in c.flags
        assert (c.tm is not None) == spec, c.id                                             # every time-parallel case states its tile-major calls
        if c.tm:
            # capi.hip chain_call / csdr_chain_create: a fused plan, max_frames >= 4096, C a multiple of 64; agc_tail_tm_supported: whole
            # 16-frame blocks, nf >= 4 W
            assert c.max_frames >= 4096 and c.M in (64, 256, 1024) and K.rows_of(c) % 64 == 0 and int(c.knobs["CSDR_AGC_W"]) * 4 == K.TM_MIN, c.id
            assert c.tm == tuple(i for i, f in enumerate(c.calls) if f % 16 == 0 and f >= K.TM_MIN), c.id
            assert any(f < K.TM_MIN for f in c.calls) and 0 in c.tm and len(c.tm) >= 2, c.id     # one short row-major call in between
        elif spec:
            assert c.max_frames < 4096 or c.M not in (64, 256, 1024, 4096), c.id
    by = lambda g: [c for c in K.ALL_CASES if c.group == g]
    for c in by("A"):
        assert len(c.calls) >= 7, c.id                                                          # every cursor flips several times
        if c.demod == "wbfm":
            d, H = c.kw["decim"], 20 * c.kw["decim"]
            assert K.design(c.kw["deemph_fc"], d)[2].size == H + 1                              # the history is H samples
            assert {d, H - d, H, H + d, 255 * d, 256 * d, 257 * d} - {0} <= set(c.calls), c.id
            assert any(4096 - d <= f < 4096 for f in c.calls) and any(4096 < f <= 4096 + d for f in c.calls), c.id
            assert (4096 in c.calls) == (4096 % d == 0), c.id
        else:
            assert c.calls[:8] == [1, 15, 16, 17, 2047, 2048, 2049, 4097] and c.calls[8:] == [1] * 6, c.id
    assert {(c.M, c.kw.get("decim"), c.kw.get("deemph_fc")) for c in by("A") if c.demod == "wbfm"} == \
        {(M, d, fc) for M in (8, 64) for d in K.WB_DECIMS for fc in K.WB_FCS}
    for c in by("B"):
        assert 4 <= len(c.calls) <= 6 and max(c.calls) <= 100 and (c.calls[-1] % 16 or c.calls[-2] % 16), c.id
    assert len(by("B")) == 4 * len(K.B_ROUTES) == 52
    am4096 = next(c for c in by("B") if c.id == "B_am_m4096_mix")
    assert any("fused-4096" in p for p in am4096.path)                                          # AM + mix stays on the fused route
    m1024 = next(c for c in by("B") if c.id == "B_am_m1024")
    assert m1024.timed[0].startswith("k_run1024v3") and any(t.startswith("k_run1024<") for t in m1024.timed)
    assert {c.M for c in by("C") if c.tm} == {64, 256, 1024} and any(K.mixed(c) for c in by("C") if c.tm)
    assert {c.M for c in by("C") if "FLAG_AGC_SEQUENTIAL" in c.flags} == {8, 256}
    assert {c.M for c in by("C") if c.tm == ()} == {20, 256}
    assert all(c.kw.get("dft_backward") and len(c.calls) == 3 and K.rows_of(c) == c.M for c in by("D")) and {c.M for c in by("D")} == {20, 256}
    assert {(c.M, c.demod) for c in by("E")} == {(M, d) for M in (20, 256) for d in ("am", "wbfm")}


# --------------------------------------------------------------------------- 3. mutations
M256 = 256
_P = {}


def _planes():
    """the oracle's planes at M = 256 over CALLS: noise (every row equally strong) and, for the AM hole, the suite's carrier fixture with
    its noise at 1e-5 (idle rows weak)"""
    if not _P:
        nf = sum(CALLS)
        x = T.noise(M256, nf)
        _P["fm"] = _stream(O.Chain(M256, demod="fm", kf=K.KF_WB), x, M256, CALLS)
        _P["none"] = _stream(O.Chain(M256, demod="none"), x, M256, CALLS)
        _P["none_back"] = _stream(O.Chain(M256, demod="none", dft_backward=True), x, M256, CALLS)
        # (faded in over 40 frames: carriers switched on at full level splatter over every row while the bank's window fills)
        n = 40 * M256
        ramp = np.ones(M256 * nf)
        ramp[:n] = np.sin(0.5 * np.pi * np.arange(n) / n) ** 2
        xs = (synth_cf32(M256 * nf, M256, seed=4242, sigma=1e-5, dc=0.0) * ramp).astype(np.complex64)
        _P["none_synth"] = _stream(O.Chain(M256, demod="none"), xs, M256, CALLS)
        _P["am_chain_synth"] = _stream(O.Chain(M256, demod="am"), xs, M256, CALLS)
    return _P


def _tail(demod, twin):
    return K.am_tail_oracle(twin) if demod == "am" else K.wbfm_tail_oracle(twin, FC, DECIM)


def _tail_with_state_from(demod, twin, k, back):
    """the oracle's tail with the state at the start of call k taken from `back` calls earlier (back = None: zeros): the calls before
    k run as they are, call k and the rest behind a state that has not seen the calls in between"""
    edges = np.concatenate([[0], np.cumsum(CALLS)])
    dec = DECIM if demod == "wbfm" else 1
    out = _tail(demod, twin).copy()
    seen = twin[:, :0] if back is None else twin[:, :edges[k - back + 1]]
    rest = _tail(demod, np.concatenate([seen, twin[:, edges[k]:]], axis=1))
    out[:, edges[k] // dec:] = rest[:, seen.shape[1] // dec:]
    return out


@pytest.mark.parametrize("demod", ["am", "wbfm"])
def test_mutations_break_the_row_bound(demod):
    P = _planes()
    twin = P["none"] if demod == "am" else P["fm"]
    ref = K.reference(demod, twin, FC, DECIM)
    good = _tail(demod, twin)
    w0, r0 = K.worst(good, ref, False)
    m0, _ = K.worst(K.fold32(good), ref, True)
    print(f"{demod} M=256: the oracle's own tail, worst row ratio {w0:.3f} (row {r0}), mixed {m0:.3f}")
    assert w0 <= 0.5 and m0 <= 1.0
    found = {}
    # (a) one row of 256 carries its neighbour's tail output
    mut = good.copy(); mut[101] = good[102]
    found["a: row 101 carries row 102's output"] = K.worst(mut, ref, False)
    # (b) the state zeroed at the third call boundary (a cursor not flipped); (c) taken from two calls back (a stale ping-pong buffer)
    found["b: state zeroed at the third call boundary"] = K.worst(_tail_with_state_from(demod, twin, 3, None), ref, False)
    found["c: state of two calls back at the third call boundary"] = K.worst(_tail_with_state_from(demod, twin, 3, 2), ref, False)
    if demod == "wbfm":
        # (d) the decimator reads x[j M - i + 1]: the oracle's decimator on its biquad output moved by one sample
        g = np.stack([O.Butter2(FC).execute_block(r) for r in twin])
        g1 = np.concatenate([g[:, 1:], np.zeros((M256, 1), np.float32)], axis=1)
        found["d: the decimator reads x[jM - i + 1]"] = K.worst(np.stack([O.FirDecim(DECIM).execute_block(r) for r in g1]), ref, False)
    # (e) the backward reversal with rows 0 and 1 swapped: the twin is the backward plane, row k against twin row k
    if demod == "am":
        tb = P["none_back"]
        refb, gb = K.reference("am", tb), _tail("am", tb)
        assert K.worst(gb, refb, False)[0] <= 0.5
        mut = gb.copy(); mut[[0, 1]] = gb[[1, 0]]
        found["e: rows 0 and 1 swapped in the backward reversal"] = K.worst(mut, refb, False)
    else:
        mut = good.copy(); mut[[0, 1]] = good[[1, 0]]
        found["e: rows 0 and 1 swapped in the backward reversal"] = K.worst(mut, ref, False)
    # (f) the mix sums C - 1 rows
    found["f: the mix sums C - 1 rows"] = K.worst(K.fold32(good[:-1]), ref, True)
    for name, (w, at) in found.items():
        print(f"{demod} M=256 mutation {name}: worst ratio {w:.3g} at {at}: FAILS the bound")
        assert w > 1.0, (demod, name, w)
    assert len(found) == (6 if demod == "wbfm" else 5)


def test_a_row_with_its_neighbours_output_passes_the_old_acceptances():
    """the hole: mutation (a) under the acceptances of test_chain_wbfm_matches_oracle (median < 2e-5, p99 < 2e-3 of the array's maximum) and
    test_chain_am_matches_oracle (whole-array max-abs < 2e-4 max(scale, 1)), with the oracle's chain as `want` as there"""
    P = _planes()
    # WBFM: any row; 1 / 256 of the samples are wrong, the 99th percentile does not see them
    want = K.wbfm_tail_oracle(P["fm"], FC, DECIM)
    mut = want.copy(); mut[101] = want[102]
    d, scale = np.abs(mut.astype(np.float64) - want), float(np.abs(want).max())
    ref = K.reference("wbfm", P["fm"], FC, DECIM)
    w, row = K.worst(mut, ref, False)
    print(f"WBFM row 101 <- row 102: old acceptance median {np.median(d):.2e} p99 {np.quantile(d, 0.99):.2e} max {d.max():.2e} of {scale:.3f}: PASSES; "
          f"per-row bound: ratio {w:.3g} at row {row}: FAILS")
    assert np.median(d) < 2e-5 * scale and np.quantile(d, 0.99) < 2e-3 * scale
    assert d.max() > 0.1 * scale and w > 1.0 and row == 101
    # AM: an idle row between the carriers (channels 4 k + 1 carry one) takes the next idle row's output
    want = P["am_chain_synth"]
    assert np.array_equal(want, K.am_tail_oracle(P["none_synth"]))
    mut = want.copy(); mut[102] = want[103]
    scale, err = float(np.abs(want).max()), float(np.abs(mut.astype(np.float64) - want).max())
    ref = K.reference("am", P["none_synth"])
    w, row = K.worst(mut, ref, False)
    print(f"AM idle row 102 <- row 103: old acceptance max abs err {err:.2e} < {2e-4 * max(scale, 1.0):.2e}: PASSES; "
          f"per-row bound: ratio {w:.3g} at row {row}: FAILS")
    assert 0 < err < 2e-4 * max(scale, 1.0)
    assert w > 1.0 and row == 102
