"""The nine first-generation block Pipes (dcBlocker, mixDown / mixUp, automaticGainControl, fmDemodulator, iirFilter,
firDecimator, resampler, amDemodulator) at their kernels' seams: every size at which k_dc_carry, k_agc, k_fm, k_biquad,
k_firdecim, k_hb_decim / k_resamp_arb or k_am takes another path, more than one row, and every parameter the Pipe accepts
that moves a filter design, against the f64 references of first_blocks_truth.py (held to the oracle in
test_first_blocks_cpu.py).

Numeric bounds have the project's form  e_gpu <= 2 * e_orc + eps * max|truth|  (e_gpu: kernel against f64 truth, e_orc: the
sequential F32 oracle against the same truth; eps from the block's first test in test_gpu_parity.py).  Where a kernel's outputs
are independent dot products or a per-lane sequential recurrence (k_firdecim, k_hb_decim / k_resamp_arb, k_agc, k_fm, the NCO)
two splittings of one stream into calls must agree in every bit, and so must row r of an nchan-row handle and the same row
through an nchan = 1 handle; the blocked scans (k_biquad, k_am, the DC blocker) reorder a sum with the call boundaries, so
their splittings are held to the numeric bound and only their rows are compared bit for bit.

Every case prints its measured error beside its bound (pytest -s)."""
import ctypes as C

import numpy as np
import pytest

import first_blocks_truth as T
import oracle_lib as O
from util import max_abs_err, rel_rms, wrap_pm

pytestmark = pytest.mark.gpu

cs = pytest.importorskip("composable_sdr_amd")

U24 = T.U24


def _run(pipe, chunks, after=None):
    """the Pipe life-cycle over `chunks`; after(r) is called behind every call (r: what start returned)"""
    r = pipe._start()
    try:
        out = []
        for c in chunks:
            out.append(pipe._process(r, c))
            if after is not None:
                after(r)
        return out
    finally:
        pipe._done(r)


def _cat(parts):
    return np.concatenate(parts, axis=-1)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _rows_to_check(nchan):
    """rows compared with an nchan = 1 handle: all of a few, else the first two, both sides of the 64-row workgroup seam and the last"""
    return list(range(nchan)) if nchan <= 7 else sorted({0, 1, 63, 64, nchan - 1} & set(range(nchan)))


# --------------------------------------------------------------------------- dcBlocker
@pytest.mark.parametrize("alpha", T.DC_ALPHAS)
@pytest.mark.parametrize("n", T.DC_SIZES)
def test_dcblocker_long_single_calls(n, alpha):
    """k_dc_carry scans the carries of the 2048-sample blocks with 256 threads: up to 256 blocks (n <= 524 288) a thread owns one
    block, from block 257 on (n = 524 289) it owns K = ceil(nb / 256) > 1 consecutive blocks, decays its running carry by beta^2048
    per block and hops by beta^(2048 K d) in the scan -- the "K blocks per thread" branch.  n = 600 001 leaves the last threads
    without a block (b0 >= nb) and a ragged last block; 1 048 576 is the Pipe's default max_samples (K = 2, every thread full).
    A second call of 1000 samples shows the state the long call stored.
    Bound (test_dcblocker_alpha_against_f64_recurrence): rel-rms e_gpu <= 2 e_orc + 1e-7, max-abs <= 4 e_orc + 1e-6 max|truth|."""
    x = T.dc_input(n + T.DC_TAIL)
    got = _cat(_run(cs.dcBlocker(alpha), [x[:n], x[n:]]))
    truth = T.dc_truth(x, alpha)
    orc = O.DcBlock(alpha).execute(x)
    scale = float(np.abs(truth).max())
    e_gpu, e_orc = rel_rms(got, truth), rel_rms(orc, truth)
    m_gpu, m_orc = float(np.abs(got - truth).max()), float(np.abs(orc - truth).max())
    t_gpu, t_orc = float(np.abs(got[n:] - truth[n:]).max()), float(np.abs(orc[n:] - truth[n:]).max())
    print(f"MEASURED dcBlocker n={n} alpha={alpha:g}: rel-rms gpu {e_gpu:.3e} <= {2 * e_orc + 1e-7:.3e}; max gpu {m_gpu:.3e} <= "
          f"{4 * m_orc + 1e-6 * scale:.3e}; second call max gpu {t_gpu:.3e} <= {4 * t_orc + 1e-6 * scale:.3e}")
    assert got.shape == x.shape and np.isfinite(got.view(np.float32)).all()
    assert e_gpu <= 2 * e_orc + 1e-7
    assert m_gpu <= 4 * m_orc + 1e-6 * scale
    assert t_gpu <= 4 * t_orc + 1e-6 * scale


# --------------------------------------------------------------------------- mixDown / mixUp
def _nco_words(r):
    th, d = C.c_uint32(), C.c_uint32()
    cs._lib.check(cs._lib.lib().csdr_nco_get_words(r.h, C.byref(th), C.byref(d)))
    return th.value, d.value


_NCO_X = {}


def _nco_x():
    if "x" not in _NCO_X:
        _NCO_X["x"] = T.nco_input()
    return _NCO_X["x"]


@pytest.mark.parametrize("up", [False, True], ids=["down", "up"])
@pytest.mark.parametrize("fi", range(5))
def test_nco_words_and_values(fi, up):
    """f in {0, 0.123, -2.9, pfb_offset(20), 7.0}; 7.0 > pi goes through the constrain (the fractional part of f / 2 pi).  One call
    of 1 048 576 samples (the default max_samples: idx * d_theta wraps 2^32 many times) and a ragged split 1, 2047, 2048, 2049, rest
    around the 2048 samples of one k_dc_apply workgroup (its 8-sample vector path against its scalar tail).  After every call the
    handle's phase words equal the oracle's theta / d_theta as integers.  Values: the oracle at 1e-6 max|x|; the f64 phasor at the
    kernel's own F32 phase at first_blocks_truth.nco_bound (2 ulp of sincosf + four roundings of the product, per sample).
    The phase of sample i depends on the words and i alone: the two splittings agree in every bit."""
    f = [0.0, 0.123, -2.9, O.pfb_offset(20), 7.0][fi]
    x = _nco_x()
    mk = cs.mixUp if up else cs.mixDown
    ragged = T.NCO_RAGGED + [T.NCO_N - sum(T.NCO_RAGGED)]
    orc_nco = O.Nco(f)
    want = orc_nco.mix_up(x) if up else orc_nco.mix_down(x)
    outs = {}
    for name, sizes in (("whole", [T.NCO_N]), ("ragged", ragged)):
        o = O.Nco(f)
        chunks = T.split(x, sizes)
        it = iter(chunks)

        def words_match(r):
            c = next(it)
            o.mix_up(c) if up else o.mix_down(c)
            assert _nco_words(r) == (o.theta, o.dtheta), (name, _nco_words(r), o.theta, o.dtheta)
        outs[name] = _cat(_run(mk(f), chunks, after=words_match))
    got = outs["whole"]
    truth = T.nco_truth(x, O.nco_constrain(f), up)
    e_o, e_t, b = max_abs_err(got, want), np.abs(got - truth), T.nco_bound(x)
    print(f"MEASURED nco f={f:g} {'up' if up else 'down'}: |gpu - oracle| {e_o:.3e} <= {1e-6 * np.abs(x).max():.3e}; |gpu - f64| max {e_t.max():.3e}, "
          f"worst ratio to the per-sample bound {np.max(e_t / (b + 1e-30)):.3f} <= 1 (bound at max|x|: {b.max():.3e})")
    assert e_o <= 1e-6 * float(np.abs(x).max())
    assert np.all(e_t <= b)
    assert _same_bits(outs["ragged"], got)


# --------------------------------------------------------------------------- automaticGainControl
@pytest.mark.parametrize("nchan,sizes", T.AGC_CASES, ids=[f"{c}x{len(s)}calls" for c, s in T.AGC_CASES])
def test_agc_vector_and_scalar_rows(nchan, sizes):
    """k_agc gives a lane the 16-byte path when its row starts 16-byte aligned (c * n even) and n >= 16, the scalar path otherwise.
      (1, 1 x 20, 15, 16, 17, 31, 32, 33, 2501): n < 16 (scalar only), n = 16 / 32 (whole blocks, the prefetch of the next block
          on and off), 17 / 33 / 2501 (a scalar tail behind the blocks);
      (3, odd sizes only): c * n is odd for row 1 in every call -- the scalar path is the one under test for a whole row, beside
          vector rows 0 and 2;
      (65, [2501, 999]): a second workgroup with one row (64 channels per workgroup), odd rows scalar;
      (130, [17]): a third workgroup with two rows, one vector block and a one-sample tail.
    Acceptance as in test_agc_matches_oracle_and_squelch_decisions: squelch mismatches 0, relative error 1e-4 on open samples, open
    fraction in (0.2, 0.9).  A lane's recurrence is sequential on either path: another splitting (one call of the whole stream;
    even n where the first was odd) and an nchan = 1 handle on the row alone give the same bits."""
    n = sum(sizes)
    z = T.agc_input(nchan, n)
    got = _cat(_run(cs.automaticGainControl(T.AGC_THR, nchan=nchan, max_samples=max(sizes)), T.split(z, sizes)))
    want = np.stack([O.Agc(T.AGC_THR).execute_block(z[k]) for k in range(nchan)])
    muted_got, muted_want = got == 0, want == 0
    mism = int(np.sum(muted_got != muted_want))
    op = ~muted_want
    rel = np.abs(got[op] - want[op]) / (np.abs(want[op]) + 1e-12)
    print(f"MEASURED agc nchan={nchan} n={n}: squelch mismatches {mism} (0), open fraction {op.mean():.3f} in (0.2, 0.9), "
          f"rel err on open samples {rel.max():.3e} <= 1e-4")
    assert got.shape == want.shape
    assert mism == 0
    assert 0.2 < op.mean() < 0.9
    assert rel.max() < 1e-4
    # (i) another splitting of the same stream
    other = [n] if len(sizes) > 1 else [8, 9]
    got2 = _cat(_run(cs.automaticGainControl(T.AGC_THR, nchan=nchan, max_samples=max(other)), T.split(z, other)))
    assert _same_bits(got2, got)
    # (ii) rows alone
    for r in (_rows_to_check(nchan) if nchan > 1 else []):
        alone = _cat(_run(cs.automaticGainControl(T.AGC_THR, nchan=1, max_samples=max(sizes)), T.split(z[r], sizes)))
        assert _same_bits(alone, got[r]), r


# --------------------------------------------------------------------------- fmDemodulator
@pytest.mark.parametrize("kf", T.FM_KF)
@pytest.mark.parametrize("nchan,n", T.FM_SHAPES)
def test_fm_rows_and_carried_sample(nchan, n, kf):
    """k_fm is one thread per sample of the [nchan][n] plane, 256 per workgroup; sample 0 of a row takes r' from the handle, the last
    one stores it.  (1, 1) and (3, 1): every sample is both; (5, 255 / 256 / 257): row starts on, before and behind a workgroup
    boundary; (300, 3): more rows than samples, rows straddling workgroups.  Three calls of n samples each.
    Reference: f64 angle(conj(r') r) / (2 pi kf) of the F32 inputs, compared modulo 1 / kf on samples whose |conj(r') r| exceeds
    1e-3 of the row's mean power.  Bound: first_blocks_truth.fm_bound (fm_common.h's polynomial fit and evaluation error, the
    rounding of the two products, times ref; the F32 ref and half an ulp of the output) -- 3.2e-7 at kf = 0.3, where
    test_freqdem_matches_oracle grants 2e-6.  A cleared stretch equals the oracle exactly.  Outputs are independent given r': one
    call of 3 n samples and an nchan = 1 handle on a row alone give the same bits."""
    total = n * T.FM_CALLS
    z, zeros = T.fm_input(nchan, total)
    got = _cat(_run(cs.fmDemodulator(kf, nchan=nchan, max_samples=n), T.split(z, [n] * T.FM_CALLS)))
    truth, absp = T.fm_truth(z, kf)
    mask = T.fm_mask(z, absp)
    d = np.abs(wrap_pm(got.astype(np.float64) - truth, 1.0 / float(np.float32(kf))))
    err, bound = (float(d[mask].max()) if mask.any() else 0.0), T.fm_bound(kf)
    print(f"MEASURED fm ({nchan}, {n}) kf={kf}: |gpu - f64| {err:.3e} <= {bound:.3e}; the mask leaves out {1 - mask.mean():.4f} of {mask.size} "
          f"(each row's first sample and the cleared stretch included)")
    assert got.shape == z.shape and got.dtype == np.float32 and np.isfinite(got).all()
    assert bound <= 2e-6 * 0.3 / kf                              # what test_freqdem_matches_oracle grants at kf = 0.3, times ref(kf) / ref(0.3)
    assert err <= bound
    want = np.stack([O.FreqDem(kf).demodulate_block(z[k]) for k in range(nchan)])
    if zeros is not None:
        assert np.array_equal(got[1, zeros.start + 1:zeros.stop], want[1, zeros.start + 1:zeros.stop])
    one = _cat(_run(cs.fmDemodulator(kf, nchan=nchan, max_samples=total), [z]))
    assert _same_bits(one, got)
    for r in (_rows_to_check(nchan) if nchan > 1 else []):
        alone = _cat(_run(cs.fmDemodulator(kf, nchan=1, max_samples=n), T.split(z[r], [n] * T.FM_CALLS)))
        assert _same_bits(alone, got[r]), r


# --------------------------------------------------------------------------- iirFilter
@pytest.mark.parametrize("nchan", [1, 5])
@pytest.mark.parametrize("fc", T.IIR_FC)
def test_iirfilter_chunks_rows_and_cutoffs(fc, nchan):
    """k_biquad: one workgroup per row, 4096 samples per chunk (256 threads x 16), the state crossing chunks and calls.  Calls of
    1, 15, 16, 17 (less than, exactly and one more than a thread's 16 samples), 4095, 4096, 4097, 8191, 8193 (a chunk less one, a
    whole chunk, a second chunk of one sample, two chunks less one, a third chunk of one sample), in that order and reversed.
    fc from 0.0005 (poles at 1 - 2e-3: A^2048 matters, the f64 scan) to 0.45 (poles near -1); five rows = five workgroups.
    Reference: f64 lfilter of the oracle's F32 coefficients.  Bound (test_iirfilter_and_firdecimator_pipes_match_oracle):
    e_gpu <= 2 e_orc + 2e-6 max|truth| for both orders of the calls; rows against an nchan = 1 handle bit for bit."""
    n = sum(T.IIR_SIZES)
    x = T.real_rows(5, n, seed=21)[:nchan]
    b, a = O.Butter2(fc).coeffs
    truth = T.iir_truth(b, a, x)
    want = np.stack([O.Butter2(fc).execute_block(r) for r in x])
    scale = float(np.abs(truth).max())
    e_orc = float(np.abs(want - truth).max())
    got = {}
    for name, sizes in (("forward", T.IIR_SIZES), ("reversed", T.IIR_SIZES[::-1])):
        got[name] = _cat(_run(cs.iirFilter(2, fc, nchan=nchan, max_samples=max(sizes)), T.split(x, sizes)))
        e_gpu = float(np.abs(got[name] - truth).max())
        print(f"MEASURED iirFilter fc={fc} nchan={nchan} {name}: |gpu - f64| {e_gpu:.3e} <= {2 * e_orc + 2e-6 * scale:.3e} (oracle {e_orc:.3e}, max|truth| {scale:.3f})")
        assert got[name].shape == x.shape and np.isfinite(got[name]).all()
        assert e_gpu <= 2 * e_orc + 2e-6 * scale
    for r in (range(nchan) if nchan > 1 else []):
        alone = _cat(_run(cs.iirFilter(2, fc, nchan=1, max_samples=max(T.IIR_SIZES)), T.split(x[r], T.IIR_SIZES)))
        assert _same_bits(alone, got["forward"][r]), r


# --------------------------------------------------------------------------- firDecimator
@pytest.mark.parametrize("nchan", [1, 3])
@pytest.mark.parametrize("m", T.FIRDECIM_M)
def test_firdecimator_every_m(m, nchan):
    """k_firdecim: one thread per output, 256 outputs per workgroup, grid row per channel; the first workgroup of a row also moves
    the history (20 m samples) forward.  Calls of m and 2m (one and two outputs), 255m, 256m, 257m (a workgroup less one, whole,
    a second workgroup of one output), 3m (shorter than the history: the new history is part old history, part row) and 300m.
    m = 1 is the filter alone, m = 64 has 1281 taps.
    Reference: f64 convolution with O.FirDecim(m).taps.  Bounds: e_gpu <= 2 e_orc + 5e-6 max|truth|, and per output the standard
    bound of an F32 dot product of N terms, N 2^-24 sum |h_i x_i|.  One call of the whole stream and an nchan = 1 handle give the
    same bits (every output is its own sum in tap order).  A call that is no multiple of m raises."""
    sizes = T.firdecim_sizes(m)
    n = sum(sizes)
    x = T.real_rows(3, n, seed=50 + m)[:nchan]
    h = O.FirDecim(m).taps
    truth, mag = T.firdecim_truth(h, x, m)
    want = np.stack([O.FirDecim(m).execute_block(r) for r in x])
    scale = float(np.abs(truth).max())
    got = _cat(_run(cs.firDecimator(m, nchan=nchan, max_samples=max(sizes)), T.split(x, sizes)))
    e = np.abs(got - truth)
    e_gpu, e_orc = float(e.max()), float(np.abs(want - truth).max())
    ratio = float(np.max(e / (h.size * U24 * mag + 1e-30)))
    print(f"MEASURED firDecimator m={m} nchan={nchan}: |gpu - f64| {e_gpu:.3e} <= {2 * e_orc + 5e-6 * scale:.3e} (oracle {e_orc:.3e}); "
          f"worst ratio to N u sum|h x| {ratio:.4f} <= 1")
    assert got.shape == (nchan, n // m) and np.isfinite(got).all()
    assert e_gpu <= 2 * e_orc + 5e-6 * scale
    assert np.all(e <= h.size * U24 * mag + 1e-30)
    one = _cat(_run(cs.firDecimator(m, nchan=nchan, max_samples=n), [x]))
    assert _same_bits(one, got)
    for r in (range(nchan) if nchan > 1 else []):
        alone = _cat(_run(cs.firDecimator(m, nchan=1, max_samples=max(sizes)), T.split(x[r], sizes)))
        assert _same_bits(alone, got[r]), r
    if m > 1:
        with pytest.raises(cs.CsdrError):
            _run(cs.firDecimator(m, nchan=nchan, max_samples=max(sizes)), [np.zeros((nchan, m + 1), np.float32)])


# --------------------------------------------------------------------------- resampler
@pytest.mark.parametrize("rate,As", [(r, 60.0) for r in T.RESAMP_RATES] + T.RESAMP_AS)
def test_resampler_stage_counts_limits_and_empty_calls(rate, As, monkeypatch):
    """design_msresamp puts K half-band decimators (k_hb_decim) in front of the arbitrary stage (k_resamp_arb): K = 0 at 2.0 (the
    limit), 1.0, 0.999 and 0.5, K = 1 at 0.4999 (just across the boundary) and 0.25, 2 at 0.125, 6 at 0.01, 9 at 0.001 (the long
    cascades); As = 40 / 80 at rate 0.3 move every filter length.  Two splittings of 200 000 samples: twenty calls of one sample (a
    half-band stage then alternates between no output and one), odd sizes, one call of exactly max_samples; at rate 0.001 also 300
    calls of 100 samples, most of which return nothing (ny = 0: nothing is launched, the histories still move).
    Against the oracle: the total count is equal, every call's count is at most 2 ceil(r n), values agree to 2e-6 max|oracle|
    (test_resampler_pipe_matches_oracle_across_chunks).  Every output is its own dot product at an integer time: the two
    splittings agree in every bit."""
    monkeypatch.setenv("CSDR_QUIET", "1")
    x = T.resamp_input(rate)
    want = O.MsResamp(rate, As).execute(x)
    outs = []
    for sizes in T.resamp_splits(rate):
        parts = _run(cs.resampler(rate, As, max_samples=T.RESAMP_MAX), T.split(x, sizes))
        for s, p in zip(sizes, parts):
            assert p.size <= 2 * int(np.ceil(rate * s)), (s, p.size)
        outs.append(np.concatenate(parts))
        if sizes[0] == 100:
            assert sum(p.size == 0 for p in parts[:300]) >= 200
    got = outs[0]
    assert got.size == want.size, (got.size, want.size)
    err, scale = max_abs_err(got, want), float(np.abs(want).max())
    print(f"MEASURED resampler r={rate} As={As:g}: {got.size} out, |gpu - oracle| {err:.3e} <= {2e-6 * scale:.3e}")
    assert np.isfinite(got.view(np.float32)).all()
    assert err <= 2e-6 * scale
    assert _same_bits(outs[1], got)


# --------------------------------------------------------------------------- amDemodulator
@pytest.mark.parametrize("nchan", [1, 3])
def test_amdemodulator_chunks_rows_and_level_drop(nchan):
    """k_am: a workgroup produces 2048 samples (256 threads x 16, of 4096 staged); the first of a call starts from the stored q_hat,
    every later one from a 2048-sample warm-up that drops 0.99^2048 = 1.2e-9 of the older state.  Calls of 1, 15, 16, 17 (around
    a thread's 16 samples), 2047, 2048, 2049 and 4095, 4096, 4097 (a workgroup less one, whole, one sample into the next, at one and
    two workgroups), then fifty calls of one sample (the state through q_in / q_out alone); the same stream with the calls
    reversed.  Reference: the f64 smoother on the f64 hypot of the F32 inputs; e_gpu <= 2 e_orc + 2e-6 max|truth|
    (test_ampdem_pipe_matches_oracle_across_chunks).
    The drop row falls by 60 dB 100 samples before the second workgroup of the 4096-sample call: that workgroup restarts from a
    warm-up whose first sample still carries the full q_hat, the one input where the truncation shows.  The segment after the drop
    on its own: 2 e_orc + 2e-6 max|truth of the segment| + 0.99^2048 q_hat(before the drop) -- the documented truncation, nothing
    more.  Rows against an nchan = 1 handle bit for bit."""
    x, dr = T.am_input(nchan)
    truth, q = T.am_truth(x)
    want = np.stack([O.AmpDem().demodulate_block(r) for r in x])
    scale, seg = float(np.abs(truth).max()), slice(T.AM_DROP, None)
    s_seg, trunc = float(np.abs(truth[dr, seg]).max()), 0.99 ** 2048 * float(q[dr, T.AM_DROP - 1])
    e_orc, e_orc_seg = float(np.abs(want - truth).max()), float(np.abs(want[dr, seg] - truth[dr, seg]).max())
    got = {}
    for name, sizes in (("forward", T.AM_SIZES), ("reversed", T.AM_SIZES[::-1])):
        got[name] = _cat(_run(cs.amDemodulator(nchan=nchan, max_samples=max(sizes)), T.split(x, sizes)))
        e_gpu, e_seg = float(np.abs(got[name] - truth).max()), float(np.abs(got[name][dr, seg] - truth[dr, seg]).max())
        print(f"MEASURED amDemodulator nchan={nchan} {name}: |gpu - f64| {e_gpu:.3e} <= {2 * e_orc + 2e-6 * scale:.3e}; after the drop "
              f"{e_seg:.3e} <= {2 * e_orc_seg + 2e-6 * s_seg + trunc:.3e} (truncation term {trunc:.2e})")
        assert got[name].shape == x.shape and np.isfinite(got[name]).all()
        assert e_gpu <= 2 * e_orc + 2e-6 * scale
        assert e_seg <= 2 * e_orc_seg + 2e-6 * s_seg + trunc
    for r in (range(nchan) if nchan > 1 else []):
        alone = _cat(_run(cs.amDemodulator(nchan=1, max_samples=max(T.AM_SIZES)), T.split(x[r], T.AM_SIZES)))
        assert _same_bits(alone, got["forward"][r]), r


# --------------------------------------------------------------------------- the chain, small
def _chain(M, frames, seed, **kw):
    from synth import synth_cf32
    x = synth_cf32(M * sum(frames), M, seed=seed)
    ch = cs.Chain(channels=M, max_frames=max(frames), **kw)
    okw = {k: v for k, v in kw.items() if k in ("demod", "decim", "deemph_fc")}
    orc = O.Chain(M, **okw)
    got, want, pos = [], [], 0
    for f in frames:
        xa = x[pos * M:(pos + f) * M]
        got.append(ch.process(xa)); want.append(orc.process(xa)); pos += f
    path = ch.path
    ch.close()
    return _cat(got), _cat(want), path


@pytest.mark.parametrize("decim,frames", [(2, [4096, 1024, 2050]), (5, [4095, 1025, 2050])])
def test_chain_wbfm_other_decimations_and_narrow_deemphasis(decim, frames):
    """demod="wbfm" at M = 8 with decim 2 and 5 (k_firdecim at 41 and 101 taps, eight rows) and deemph_fc = 0.0021 (k_biquad's
    narrow low-pass, 5 kHz at 2.4 MS/s): the chain's tail beyond decim = 4 / deemph_fc = 0.025.  Acceptance of
    test_chain_wbfm_matches_oracle unchanged: median <= 2e-5, p99 <= 2e-3 of max|oracle|."""
    got, want, path = _chain(8, frames, 777, demod="wbfm", decim=decim, deemph_fc=0.0021)
    assert got.shape == want.shape == (8, sum(frames) // decim)
    d = np.abs(got.astype(np.float64) - want)
    scale = np.abs(want).max()
    print(f"MEASURED chain WBFM M=8 decim={decim} fc=0.0021 [{path}]: median {np.median(d):.2e} <= {2e-5 * scale:.2e}, p99 {np.quantile(d, 0.99):.2e} <= "
          f"{2e-3 * scale:.2e}, max {d.max():.2e}")
    assert np.median(d) < 2e-5 * scale and np.quantile(d, 0.99) < 2e-3 * scale


def test_chain_am_calls_around_one_workgroup():
    """demod="am" at M = 8 with calls of 2047 and 2049 frames: k_am's single workgroup less one sample, and one sample into a second
    workgroup, on eight rows.  Acceptance of test_chain_am_matches_oracle unchanged: max-abs <= 2e-4 max(max|oracle|, 1)."""
    got, want, path = _chain(8, [2047, 2049], 4242, demod="am")
    scale, err = np.abs(want).max(), max_abs_err(got, want)
    print(f"MEASURED chain AM M=8 [{path}]: max abs err {err:.3e} <= {2e-4 * max(scale, 1.0):.3e}")
    assert got.shape == want.shape == (8, 4096) and got.dtype == np.float32
    assert err < 2e-4 * max(scale, 1.0)
