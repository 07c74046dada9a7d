"""The f64 references and fixtures of first_blocks_truth.py, checked where no GPU is present: every reference against the F32
oracle on the fixtures test_first_blocks_gpu.py runs, and the conditions those fixtures must meet (AGC open fraction and level
margins, the share of samples the FM mask leaves out, the resampler's stage counts at the chosen rates)."""
import numpy as np
import pytest

import first_blocks_truth as T
import oracle_lib as O
from util import wrap_pm

U24 = T.U24


# --------------------------------------------------------------------------- dcBlocker
@pytest.mark.parametrize("alpha", T.DC_ALPHAS)
def test_dc_truth_is_the_oracles_filter(alpha):
    """The sequential F32 recurrence rounds v0 = x - a1 v1 (a product and a sum at |v|) and y = v0 - v1 (exact or one rounding at
    |v|): a few ulp of the state per output, and alpha times the state error that has built up, which stays far below that.
    Granted: 4 ulp(max|v|) = 8 U24 max|v|."""
    n = T.DC_SIZES[1] + T.DC_TAIL
    x = T.dc_input(n)
    truth = T.dc_truth(x, alpha)
    v = np.cumsum(truth)                                         # v[n] = sum of y up to n
    orc = O.DcBlock(alpha).execute(x)
    err, bound = float(np.abs(orc - truth).max()), 8 * U24 * float(np.abs(v).max())
    print(f"dc alpha={alpha:g}: |oracle - f64| {err:.3e} <= {bound:.3e} (max|v| {np.abs(v).max():.1f})")
    assert err <= bound
    assert abs(O.DcBlock(alpha).a1 + float(np.float32(1) - np.float32(alpha))) < 1e-7


# --------------------------------------------------------------------------- mixDown / mixUp
def nco_freqs():
    return [0.0, 0.123, -2.9, O.pfb_offset(20), 7.0]


@pytest.mark.parametrize("fi", range(5))
def test_nco_truth_is_the_oracles_phasor(fi):
    """sinf / cosf of the host are within the 2 ulp nco_bound grants the device's sincosf; three roundings of the product"""
    f = nco_freqs()[fi]
    x = T.nco_input()[:200000]
    d = O.nco_constrain(f)
    for up in (False, True):
        o = O.Nco(f)
        assert o.dtheta == d
        orc = o.mix_up(x) if up else o.mix_down(x)
        assert o.theta == (x.size * d) & 0xFFFFFFFF
        e = np.abs(orc - T.nco_truth(x, d, up))
        b = T.nco_bound(x)
        print(f"nco f={f:g} up={up}: d_theta {d}, max |oracle - f64| {e.max():.3e}, worst ratio to the bound {np.max(e / (b + 1e-30)):.3f}")
        assert np.all(e <= b)
    if fi == 4:
        assert d == O.nco_constrain(np.float32(7.0) - 2 * np.pi) or abs(d - O.nco_constrain(7.0 - 2 * np.pi)) < 2048    # 7 > pi: wrapped


# --------------------------------------------------------------------------- automaticGainControl
@pytest.mark.parametrize("nchan,sizes", T.AGC_CASES)
def test_agc_fixture_opens_and_closes_and_keeps_clear_of_the_threshold(nchan, sizes):
    n = sum(sizes)
    z = T.agc_input(nchan, n)
    want = np.stack([O.Agc(T.AGC_THR).execute_block(z[k]) for k in range(nchan)])
    open_frac = float(np.mean(want != 0))
    margin = T.agc_level_margin_db(z)
    print(f"agc nchan={nchan} n={n}: open fraction {open_frac:.3f}, nearest level {margin:.1f} dB from the threshold")
    assert 0.2 < open_frac < 0.9
    assert margin >= 6.0
    # rows differ: no two rows share a sample
    assert nchan == 1 or not np.any(z[0] == z[1])
    # calls in pieces = one call (the oracle keeps its state)
    o = O.Agc(T.AGC_THR)
    assert np.array_equal(np.concatenate([o.execute_block(c) for c in T.split(z[0], sizes)]), want[0])


# --------------------------------------------------------------------------- fmDemodulator
@pytest.mark.parametrize("kf", T.FM_KF)
@pytest.mark.parametrize("nchan,n", T.FM_SHAPES)
def test_fm_truth_mask_and_oracle(nchan, n, kf):
    z, zeros = T.fm_input(nchan, n * T.FM_CALLS)
    truth, absp = T.fm_truth(z, kf)
    mask = T.fm_mask(z, absp)
    made = np.zeros(z.shape, bool)                               # left out by construction: r' = 0 in front, the cleared stretch
    made[:, 0] = True
    if zeros is not None:
        made[1, zeros.start:zeros.stop + 1] = True
    free = ~made
    share = float(np.mean(~mask[free])) if free.any() else 0.0
    want = np.stack([O.FreqDem(kf).demodulate_block(z[k]) for k in range(nchan)])
    d = np.abs(wrap_pm(want.astype(np.float64) - truth, 1.0 / float(np.float32(kf))))
    err = float(d[mask].max()) if mask.any() else 0.0
    print(f"fm ({nchan}, {n}) kf={kf}: mask leaves out {share:.4f} of {int(free.sum())} samples, |oracle - f64| {err:.3e} <= {T.fm_bound(kf):.3e}")
    assert share < 0.01
    assert err <= T.fm_bound(kf)
    assert T.fm_bound(0.3) <= 2e-6                               # what test_freqdem_matches_oracle grants
    if zeros is not None:
        assert np.all(want[1, zeros.start + 1:zeros.stop] == 0)


# --------------------------------------------------------------------------- iirFilter
@pytest.mark.parametrize("fc", T.IIR_FC)
def test_iir_truth_is_the_oracles_filter(fc):
    """The oracle's direct-form-II loop in F32 is the noisy side (its state is ~1 / (4 b0) times the input for a narrow low-pass):
    this shows the reference is the same filter, to 1e-3 of the output's peak, and that the published coefficients are a unit-DC-gain
    low-pass."""
    x = T.real_rows(5, sum(T.IIR_SIZES), seed=21)
    orc = O.Butter2(fc)
    b, a = orc.coeffs
    assert abs(b.astype(np.float64).sum() / a.astype(np.float64).sum() - 1.0) < 1e-2 * max(1.0, 1e-5 / fc ** 2) and a[0] == 1.0
    truth = T.iir_truth(b, a, x)
    want = np.stack([O.Butter2(fc).execute_block(r) for r in x])
    err, scale = float(np.abs(want - truth).max()), float(np.abs(truth).max())
    print(f"iir fc={fc}: |oracle - f64| {err:.3e} of {scale:.3f}")
    assert err <= 1e-3 * scale


# --------------------------------------------------------------------------- firDecimator
@pytest.mark.parametrize("m", T.FIRDECIM_M)
def test_firdecim_truth_is_the_oracles_filter(m):
    """a sequential F32 dot product of N terms: |fl(sum) - sum| <= N U24 sum |h_i x_i| (to first order)"""
    sizes = T.firdecim_sizes(m)
    x = T.real_rows(3, sum(sizes), seed=50 + m)
    orc = O.FirDecim(m)
    h = orc.taps
    assert h.size == 20 * m + 1 and sizes[5] < h.size - 1 < sizes[6]
    truth, mag = T.firdecim_truth(h, x, m)
    want = np.stack([O.FirDecim(m).execute_block(r) for r in x])
    e = np.abs(want - truth)
    print(f"firdecim m={m}: {h.size} taps, max |oracle - f64| {e.max():.3e}, worst ratio to N u sum|h x| {np.max(e / (h.size * U24 * mag + 1e-30)):.4f}")
    assert want.shape == truth.shape == (3, sum(sizes) // m)
    assert np.all(e <= h.size * U24 * mag + 1e-30)
    o = O.FirDecim(m)
    assert np.array_equal(np.concatenate([o.execute_block(c) for c in T.split(x[0], sizes)]), want[0])


# --------------------------------------------------------------------------- resampler
@pytest.mark.parametrize("rate,stages", list(zip(T.RESAMP_RATES, T.RESAMP_STAGES)) + [(r, 1) for r, _ in T.RESAMP_AS[:1]])
def test_resampler_stage_counts_at_the_chosen_rates(rate, stages):
    assert O.MsResamp(rate).num_halfband == stages
    a, b = T.resamp_splits(rate)
    assert a.count(1) == 20 and T.RESAMP_MAX in a and any(s % 2 for s in a)
    assert rate != 0.001 or b.count(100) == 300


@pytest.mark.parametrize("rate,As", [(0.001, 60.0), (0.4999, 60.0), (2.0, 60.0)] + T.RESAMP_AS)
def test_resampler_oracle_is_split_invariant_in_count(rate, As):
    """the oracle's output count and values do not depend on how the stream is cut (what the GPU test relies on when it compares
    call by call), most 100-sample calls at rate 0.001 return nothing, and every call fits 2 ceil(r n)"""
    x = T.resamp_input(rate)
    whole = O.MsResamp(rate, As).execute(x)
    assert abs(whole.size - rate * x.size) <= 2
    for sizes in T.resamp_splits(rate):
        o = O.MsResamp(rate, As)
        parts = [o.execute(c) for c in T.split(x, sizes)]
        assert np.array_equal(np.concatenate(parts), whole)
        assert all(p.size <= 2 * int(np.ceil(rate * s)) for p, s in zip(parts, sizes))
        if sizes[0] == 100:
            empty = sum(p.size == 0 for p in parts[:300])
            print(f"resampler r={rate}: {empty} of 300 calls of 100 samples return nothing")
            assert empty >= 200
    assert np.abs(whole).max() >= 1.0                            # 2e-6 max|truth| is no tighter than the existing 2e-6


# --------------------------------------------------------------------------- amDemodulator
@pytest.mark.parametrize("nchan", [1, 3])
def test_am_truth_is_the_oracles_detector_and_the_drop_sits_before_a_workgroup_boundary(nchan):
    x, dr = T.am_input(nchan)
    truth, q = T.am_truth(x)
    want = np.stack([O.AmpDem().demodulate_block(r) for r in x])
    err, scale = float(np.abs(want - truth).max()), float(np.abs(truth).max())
    seg = slice(T.AM_DROP, None)
    e_seg, s_seg = float(np.abs(want[dr, seg] - truth[dr, seg]).max()), float(np.abs(truth[dr, seg]).max())
    print(f"am nchan={nchan}: |oracle - f64| {err:.3e} of {scale:.3f}; after the drop {e_seg:.3e} of {s_seg:.3f}; "
          f"q_hat before the drop {q[dr, T.AM_DROP - 1]:.3f}, truncation term {0.99 ** 2048 * q[dr, T.AM_DROP - 1]:.2e}")
    assert err <= 2e-6 * scale and e_seg <= 2e-6 * s_seg
    # the fixture: the call of 4096 samples starts at AM_CALL0, the drop is 100 samples before its second workgroup
    starts = np.cumsum([0] + T.AM_SIZES[:-1])
    assert T.AM_SIZES[8] == 4096 and starts[8] == T.AM_CALL0 and T.AM_DROP == T.AM_CALL0 + 2048 - 100
    lev = lambda s: 10 * np.log10(np.mean(np.abs(x[dr, s].astype(np.complex128)) ** 2))
    assert 59.0 < lev(slice(T.AM_DROP - 2000, T.AM_DROP)) - lev(slice(T.AM_DROP, T.AM_DROP + 2000)) < 61.0
    assert nchan == 1 or not np.any(x[0] == x[2])
