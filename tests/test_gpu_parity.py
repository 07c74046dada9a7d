"""Parity of the HIP path (through the C ABI) against the CPU oracle on the same seeded
inputs.  Tolerances (north_star: "within a stated float tolerance"):

  PFB / chain CF32 outputs : rel-RMS <= 1e-5, max-abs <= 1e-4 * max|ref|
      (f32 FIR with fused multiply-add + f32 FFT of log2(M) stages vs. the oracle's f32
       dot products + f64 DFT: expected ~3e-7 rel-RMS)
  DC blocker               : max-abs <= 4e-6 * max|x| / alpha-normalised state (see test)
  FM outputs               : compared modulo 1/kf (the atan2 branch cut), on samples whose
                             |conj(r')r| exceeds 1e-3 of the channel's RMS power; abs <= 2e-5
  AGC                      : gain trajectory rel 1e-4; squelch decisions: mismatch count 0
  mix                      : the HIP path folds channels in the reference's left-to-right
                             order: same tolerance as the unmixed output times sqrt(M)
"""
import os

import numpy as np
import pytest

import oracle_lib as O
from host_exe import host_exe
from synth import synth_cf32
from util import knob, max_abs_err, rel_rms, wrap_pm

pytestmark = pytest.mark.gpu

cs = pytest.importorskip("composable_sdr_amd")


def _run_pipe(pipe, chunks):
    r = pipe._start()
    try:
        return [pipe._process(r, c) for c in chunks]
    finally:
        pipe._done(r)


# --------------------------------------------------------------------------- standalone Pipes
def test_dcblocker_matches_oracle_across_chunks():
    x = synth_cf32(300000, 16, seed=3)
    cuts = [0, 1, 1000, 1024, 5000, 150000, 150000, 300000]     # includes an empty chunk
    chunks = [x[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    got = np.concatenate(_run_pipe(cs.dcBlocker(), chunks))
    want = O.DcBlock(0.0005).execute(x)
    err = max_abs_err(got, want)
    print("dcblock max-abs err", err, "rel-rms", rel_rms(got, want))
    # The filter state |v| sits at ~ DC/alpha = 28, whose f32 ulp is 1.9e-6: the reference's
    # own sequential f32 recurrence carries that much rounding noise in y = v0 - v1, so
    # agreement is bounded by a few ulp(|v|), and both must be equally close to f64 truth.
    assert err < 8e-6
    assert rel_rms(got, want) < 8e-6
    v, truth = 0j, np.empty(x.size, dtype=np.complex128)
    xd, beta = x.astype(np.complex128), float(np.float32(1) - np.float32(0.0005))
    for i in range(x.size):
        v0 = xd[i] + beta * v
        truth[i] = v0 - v
        v = v0
    e_gpu, e_orc = rel_rms(got, truth), rel_rms(want, truth)
    print("vs f64 truth: gpu", e_gpu, "oracle", e_orc)
    assert e_gpu < 2 * e_orc + 1e-7


@pytest.mark.parametrize("M", [20, 256])
def test_nco_mix_matches_oracle(M):
    f = O.pfb_offset(M)
    x = synth_cf32(70000, M, seed=5)
    chunks = [x[:12345], x[12345:40000], x[40000:]]
    got = np.concatenate(_run_pipe(cs.mixDown(f), chunks))
    want = O.Nco(f).mix_down(x)
    print("nco down", M, max_abs_err(got, want))
    assert max_abs_err(got, want) < 1e-6
    got = np.concatenate(_run_pipe(cs.mixUp(0.123), chunks))
    want = O.Nco(0.123).mix_up(x)
    assert max_abs_err(got, want) < 1e-6


def test_freqdem_matches_oracle():
    nchan, n = 5, 3000
    rng = np.random.default_rng(2)
    z = (rng.standard_normal((nchan, n)) + 1j * rng.standard_normal((nchan, n))).astype(np.complex64)
    z[1, 100:200] = 0                                   # squelched stretch: arg(0) paths
    kf = 0.3
    pipe = cs.fmDemodulator(kf, nchan=nchan, max_samples=n)
    parts = _run_pipe(pipe, [z[:, :1000].copy(), z[:, 1000:].copy()])
    got = np.concatenate(parts, axis=1)
    want = np.stack([O.FreqDem(kf).demodulate_block(z[k]) for k in range(nchan)])
    d = wrap_pm(got.astype(np.float64) - want, 1.0 / kf)
    print("freqdem max err", np.abs(d).max())
    assert np.abs(d).max() < 2e-6
    assert np.array_equal(got[1, 101:200], want[1, 101:200])    # exact zeros in, exact out


def test_agc_matches_oracle_and_squelch_decisions():
    nchan, n = 6, 6000
    rng = np.random.default_rng(4)
    amp = np.array([1e-3, 3e-3, 1e-2, 3e-2, 0.1, 1.0])[:, None]
    z = amp * (rng.standard_normal((nchan, n)) + 1j * rng.standard_normal((nchan, n))) / np.sqrt(2)
    z[2, 3000:] *= 1e-3                                   # level drop: FALL/SIGNALLO/TIMEOUT path
    z = z.astype(np.complex64)
    thr = -35.0                                           # between the 3e-3 and 1e-2 channels (x sqrt2 noise)
    pipe = cs.automaticGainControl(thr, nchan=nchan, max_samples=n)
    parts = _run_pipe(pipe, [z[:, :2500].copy(), z[:, 2500:].copy()])
    got = np.concatenate(parts, axis=1)
    want = np.stack([O.Agc(thr).execute_block(z[k]) for k in range(nchan)])
    muted_got, muted_want = got == 0, want == 0
    mism = int(np.sum(muted_got != muted_want))
    print("agc squelch mismatches", mism, "open fraction", 1 - muted_want.mean())
    assert mism == 0
    assert 0.2 < 1 - muted_want.mean() < 0.9             # both regimes are exercised
    op = ~muted_want
    rel = np.abs(got[op] - want[op]) / (np.abs(want[op]) + 1e-12)
    print("agc rel err max", rel.max())
    assert rel.max() < 1e-4


# --------------------------------------------------------------------------- the chain
def _chain_case(M, nfs, **kw):
    total = sum(nfs) * M
    x = synth_cf32(total, M, seed=100 + M)
    ch = cs.Chain(channels=M, max_frames=max(max(nfs), 1), **kw)
    orc = O.Chain(M, dc_block=kw.get("dc_block", True), agc_db=kw.get("agc", 0.0),
                  demod=kw.get("demod", "none"), kf=kw.get("kf", 0.3), mix=kw.get("mix", False))
    got, want, pos = [], [], 0
    for nf in nfs:
        c = x[pos:pos + nf * M]
        pos += nf * M
        got.append(ch.process(c))
        want.append(orc.process(c))
    path = ch.path
    ch.close()
    ax = 0 if kw.get("mix", False) and M > 1 else 1
    return np.concatenate(got, axis=ax), np.concatenate(want, axis=ax), path


@pytest.mark.parametrize("M", [2, 4, 20, 64, 256])
def test_chain_deno_matches_oracle(M):
    got, want, path = _chain_case(M, [64, 1, 37, 0, 128])
    r, e = rel_rms(got, want), max_abs_err(got, want)
    print(f"chain DeNo M={M} [{path}] rel-rms {r:.3e} max-abs {e:.3e} ref max {np.abs(want).max():.3f}")
    assert r < 1e-5
    assert e < 1e-4 * np.abs(want).max()


@pytest.mark.parametrize("M", [1, 8, 20, 256])
def test_chain_fm_matches_oracle(M):
    kf = 0.3
    ref = 1.0 / (2 * np.pi * kf)
    got, want, path = _chain_case(M, [96, 32, 200], demod="fm", kf=kf)
    _, r, _ = _chain_case(M, [96, 32, 200], demod="none")        # oracle's channel samples r
    r = np.abs(r.reshape(want.shape))
    d = np.abs(wrap_pm(got.astype(np.float64) - want, 1.0 / kf))
    # The phase of r carries the channelizer's error divided by |r|: an absolute CF32 error e
    # moves m by ref*e/|r|.  With the CF32 tolerance e <= 1e-4*max|r| (test above) that is
    # |dm| * min(|r_t|,|r_t-1|) <= 2*ref*1e-4*max|r|; strong samples get a direct bound.
    rmin = np.minimum(r, np.concatenate([np.zeros((r.shape[0], 1)), r[:, :-1]], axis=1))
    weighted = d * rmin / r.max()
    strong = rmin > 0.25 * r.max()
    print(f"chain FM M={M} [{path}] median {np.median(d):.3e} weighted max {weighted.max():.3e} "
          f"strong({strong.mean():.2f}) max {d[strong].max() if strong.any() else 0:.3e}")
    assert weighted.max() < 2 * ref * 1e-4
    assert np.median(d) < 2e-5
    if strong.any():
        assert d[strong].max() < 2e-5


def _clear_threshold(M, x, skip=200):
    """Squelch threshold (dB) in the widest gap between the per-channel levels of the fixture, and the distance of
    the nearest channel from it.  Levels come from the oracle's DeNo output: the AGC's rssi settles at the channel's
    power in dB, so a channel >= 3 dB away never toggles on rounding differences."""
    y = O.Chain(M).process(x)
    lev = np.sort(10 * np.log10(np.mean(np.abs(y[:, skip:]) ** 2, axis=1) + 1e-30))
    i = int(np.argmax(np.diff(lev)))
    return float(0.5 * (lev[i] + lev[i + 1])), float(0.5 * (lev[i + 1] - lev[i]))


@pytest.mark.parametrize("M", [8, 64, 256])
def test_chain_agc_fm_matches_oracle(M):
    """Threshold >= 3 dB away from every channel's level: the mute decisions must agree EXACTLY."""
    kf = 0.3
    nfs = [512, 512, 1024]
    thr, margin = _clear_threshold(M, synth_cf32(sum(nfs) * M, M, seed=100 + M))
    assert margin >= 3.0
    got, want, path = _chain_case(M, nfs, demod="fm", kf=kf, agc=thr)
    mg, mw = got == 0, want == 0
    mism = int(np.sum(mg != mw))
    d = wrap_pm(got.astype(np.float64) - want, 1.0 / kf)
    print(f"chain AGC+FM M={M} thr={thr:.1f} dB (margin {margin:.1f} dB) [{path}] squelch mismatches {mism} open {1 - mw.mean():.3f} "
          f"p99.9 {np.quantile(np.abs(d), 0.999):.3e}")
    assert mism == 0
    assert 0.05 < 1 - mw.mean() < 0.95                   # both regimes are exercised
    # AGC normalises every open channel to |y| = 1, so a weak channel's relative CF32 error
    # (1e-5 of the strongest channel's amplitude) shows up un-attenuated in the phase
    assert np.quantile(np.abs(d), 0.999) < 5e-4
    assert np.median(np.abs(d)[~mw]) < 2e-5


def test_chain_agc_fm_near_threshold_counted_mismatches():
    """M = 8 with -a 10: the tone channels sit 1 dB BELOW the threshold (9.0 dB), so their squelch toggles on the
    rssi's own fluctuation and a 1e-5 relative difference in the gain can move an edge by a sample.  Counted bound."""
    M, kf = 8, 0.3
    got, want, path = _chain_case(M, [512, 512, 1024], demod="fm", kf=kf, agc=10.0)
    mism = int(np.sum((got == 0) != (want == 0)))
    d = wrap_pm(got.astype(np.float64) - want, 1.0 / kf)
    print(f"chain AGC+FM near threshold M={M} [{path}]: squelch mismatches {mism} of {got.size}, p99.9 {np.quantile(np.abs(d), 0.999):.3e}")
    assert mism <= 2 * M
    assert np.quantile(np.abs(d), 0.999) < 5e-4


@pytest.mark.parametrize("demod", ["none", "fm"])
def test_chain_mix_matches_oracle(demod):
    M = 16
    got, want, path = _chain_case(M, [64, 64], demod=demod, kf=0.6, mix=True)
    assert got.shape == want.shape == (128,)
    if demod == "fm":
        e = np.abs(got.astype(np.float64) - want)
        print("mix fm", np.quantile(e, 0.99), e.max())
        # a single +-1/kf branch flip in any of the M summands shifts the sum by 1/kf
        e = np.minimum(e, np.abs(wrap_pm(e, 1.0 / 0.6)))
        assert np.quantile(e, 0.99) < 1e-4
    else:
        assert rel_rms(got, want) < 4e-6


def test_chain_channel_shard_equals_slice_of_full():
    M = 32
    x = synth_cf32(M * 80, M, seed=9)
    full = cs.Chain(channels=M, demod="fm").process(x)
    part = cs.Chain(channels=M, demod="fm", chan_first=8, chan_count=12).process(x)
    assert part.shape == (12, 80)
    assert np.array_equal(part, full[8:20])


@pytest.mark.parametrize("M,G,demod,agc,mix", [(256, 8, "fm", 0.0, False), (256, 2, "none", 0.0, False), (256, 4, "fm", 0.0, False), (256, 2, "fm", 0.0, True),
                                               (256, 8, "none", 0.0, False), (256, 4, "none", 0.0, True), (256, 8, "fm", 10.0, False), (64, 4, "fm", 11.0, False),
                                               (20, 4, "none", 0.0, False), (20, 2, "fm", 0.0, True), (4096, 8, "none", 0.0, True),
                                               (1024, 8, "fm", 0.0, False), (1024, 4, "none", 0.0, False), (1024, 2, "fm", 0.0, True)])
def test_chain_interleaved_shard_pruned_dft_equals_rows_of_full(M, G, demod, agc, mix):
    """chan_stride = G: shard g produces the channels g, g + G, ... through one length-G fold + one M/G-point DFT per frame
    (SURVEY 8e(A)); every shard must equal those rows of the oracle's full output, and the mixed shards must add up to the
    full mix (what the multi-GPU all-reduce does)."""
    frames = [96, 40, 7] if M >= 1024 else [700, 300, 41]
    x = synth_cf32(M * sum(frames), M, seed=900 + M)
    want_full = O.Chain(M, demod=demod, kf=0.3, agc_db=agc, mix=False)
    wf, pos = [], 0
    for f in frames:
        wf.append(want_full.process(x[pos * M:(pos + f) * M])); pos += f
    wf = np.concatenate(wf, axis=1)
    acc = None
    for g in sorted({0, 1, G - 1}) if not mix else range(G):
        ch = cs.Chain(channels=M, demod=demod, kf=0.3, agc=agc, mix=mix, chan_first=g, chan_stride=G, max_frames=max(frames))
        # M = 256 with stride 2, 4, 8: the fused run kernel's shard variant; every other shape the any-M route
        assert ("interleaved-shard" in ch.path and "fused" in ch.path) if (M in (256, 1024) and G in (2, 4, 8)) else "pruned-dft" in ch.path
        got, pos = [], 0
        for f in frames:
            got.append(ch.process(x[pos * M:(pos + f) * M])); pos += f
        got = np.concatenate(got, axis=-1)
        ch.close()
        if mix:
            acc = got.astype(np.complex128 if demod == "none" else np.float64) if acc is None else acc + got
            continue
        want = wf[g::G]
        assert got.shape == want.shape
        if demod == "fm":
            d = np.abs(wrap_pm(got.astype(np.float64) - want, 1.0 / 0.3))
            if agc:
                assert int(np.sum((got == 0) != (want == 0))) == 0
                assert np.median(d[want != 0]) < 2e-5
            else:
                tone = (np.arange(g, M, G) % 4) == 1
                assert np.median(d) < 2e-5 and (not tone.any() or np.quantile(d[tone], 0.999) < 5e-5)
        else:
            # relative to the whole band: a shard may hold only the weak (noise-only) channels, while the f32 rounding
            # of a frame's DFT scales with its strongest bins
            e = np.sqrt(np.mean(np.abs(got.astype(np.complex128) - want) ** 2)) / np.sqrt(np.mean(np.abs(wf) ** 2))
            assert e < 1e-5, e
    if mix:
        wm = wf.astype(np.complex128 if demod == "none" else np.float64).sum(axis=0)
        scale = np.abs(wm).max() + np.abs(wf).max()
        print(f"interleaved shards M={M} G={G} {demod} mix: max |sum of shards - full mix| = {np.abs(acc - wm).max():.3e} of {scale:.2f}")
        assert np.abs(acc - wm).max() < 2e-4 * scale * (np.sqrt(M) if demod == "fm" else 1.0)


@pytest.mark.parametrize("M", [4096, 8192, 20, 64, 7])
def test_chain_deno_mix_identity_equals_full_bank(M):
    """DeNo --mix over all channels: sum_k Y_t[k] = M X_t[0] (the sum of all DFT bins is M times the first input), so the
    product path runs the DC blocker on the stream and the FIR of polyphase branch 0 only.  It must agree with the full
    bank + DFT + channel sum (CSDR_FLAG_NO_MIX_IDENTITY) and with the oracle's left fold, across calls."""
    from composable_sdr_amd import _lib
    frames = [48, 16, 5, 31] if M >= 1024 else [900, 300, 41, 1]          # 100 tiles at M = 4096: beyond the 10-tile look-back
    x = synth_cf32(M * sum(frames), M, seed=700 + M, dc=0.2 - 0.1j)
    fl = _lib.FLAG_QUIET | _lib.FLAG_FORCE_GENERIC
    a = cs.Chain(channels=M, demod="none", mix=True, max_frames=max(frames), flags=fl)
    b = cs.Chain(channels=M, demod="none", mix=True, max_frames=max(frames), flags=fl | _lib.FLAG_NO_MIX_IDENTITY)
    assert "mix-identity" in a.path and "mix-identity" not in b.path
    orc = O.Chain(M, demod="none", mix=True)
    ga, gb, wo, pos = [], [], [], 0
    for f in frames:
        xa = x[pos * M:(pos + f) * M]; pos += f
        ga.append(a.process(xa)); gb.append(b.process(xa)); wo.append(orc.process(xa))
    ga, gb, wo = np.concatenate(ga), np.concatenate(gb), np.concatenate(wo)
    # the full sum carries the rounding of M terms of size max|Y| (the identity does not): tolerance scaled by that
    ymax = float(np.abs(O.Chain(M).process(x)).max())
    tol = max(4e-7 * ymax * M, 1e-5 * float(np.abs(wo).max()))
    print(f"mix identity M={M}: vs full bank max {np.abs(ga - gb).max():.3e}, vs oracle max {np.abs(ga - wo).max():.3e} (tolerance {tol:.3e}, |out| max {np.abs(wo).max():.2f})")
    assert ga.shape == gb.shape == wo.shape
    # the oracle's f32 DC blocker adds ulp(|v|)/2 of cancellation noise per sample at |DC| = 0.22 (see test_fused256_dc_state...)
    assert np.abs(ga - gb).max() < tol and np.abs(ga - wo).max() < max(tol, 3e-4 * float(np.abs(wo).max()))
    a.close(); b.close()


def test_chain_chunk_size_invariance():
    M = 64
    x = synth_cf32(M * 300, M, seed=21)
    whole = cs.Chain(channels=M, demod="fm", max_frames=300).process(x)
    ch = cs.Chain(channels=M, demod="fm", max_frames=300)
    parts = [ch.process(x[a * M:b * M]) for a, b in ((0, 7), (7, 8), (8, 150), (150, 300))]
    got = np.concatenate(parts, axis=1)
    d = wrap_pm(got.astype(np.float64) - whole, 1.0 / 0.3)
    print("chunk invariance max diff", np.abs(d).max())
    assert np.quantile(np.abs(d), 0.999) < 2e-5


@pytest.mark.parametrize("M,demod", [(256, "fm"), (20, "none")])
def test_chain_async_submit_collect_matches_blocking(M, demod):
    """csdr_chain_submit / csdr_chain_collect (page-locked buffers, three chunks in flight, copies and kernels on separate
    streams) produce bit for bit what the blocking csdr_chain_process does, state carried across the in-flight chunks; a
    fourth submit without a collect is refused, pageable buffers are staged."""
    from composable_sdr_amd.pipes import host_array
    nfs = [512, 512, 256, 512, 128, 512, 512]
    x = synth_cf32(M * sum(nfs), M, seed=77)
    a = cs.Chain(channels=M, demod=demod, kf=0.3, max_frames=512)
    b = cs.Chain(channels=M, demod=demod, kf=0.3, max_frames=512)
    want, pos = [], 0
    for nf in nfs:
        want.append(a.process(x[pos:pos + nf * M])); pos += nf * M
    ins = [host_array((512 * M,), np.complex64) for _ in range(3)]
    outs = [host_array((M, 512), want[0].dtype) for _ in range(3)]
    got, pend, pos = [], [], 0
    for i, nf in enumerate(nfs):
        if len(pend) == 3:
            got.append(b.collect().copy()); pend.pop(0)
        k = i % 3
        ins[k].a[:nf * M] = x[pos:pos + nf * M]; pos += nf * M
        if i == 4:                                           # a pageable pair in the middle of the stream
            o = b.submit(ins[k].a[:nf * M].copy())
        else:
            o = b.submit(ins[k].a[:nf * M], outs[k].a.reshape(-1)[:M * nf].reshape(M, nf))
        pend.append(o)
        if i == 2:
            with pytest.raises(cs.CsdrError) as e:
                b.submit(ins[0].a[:M * 16])
            assert e.value.code == -6
    while pend:
        got.append(b.collect().copy()); pend.pop(0)
    b.status()
    for g, w in zip(got, want):
        assert g.shape == w.shape and np.array_equal(g.view(np.uint32), w.view(np.uint32))
    a.close(); b.close()


def test_chain_reset_restores_initial_state():
    M = 16
    x = synth_cf32(M * 50, M, seed=2)
    ch = cs.Chain(channels=M, agc=-20.0)
    a = ch.process(x)
    ch.process(x)
    ch.reset()
    b = ch.process(x)
    assert np.array_equal(a, b)


def test_chain_edge_cases_and_errors():
    M = 8
    ch = cs.Chain(channels=M, max_frames=16)
    out = ch.process(np.empty(0, dtype=np.complex64))            # empty chunk: no-op
    assert out.size == 0
    with pytest.raises(cs.CsdrError) as e:
        ch.process(np.zeros(M * 3 + 1, dtype=np.complex64))      # not a multiple of M
    assert e.value.code == -4
    with pytest.raises(cs.CsdrError) as e:
        ch.process(np.zeros(M * 17, dtype=np.complex64))         # larger than created for
    assert e.value.code == -4
    with pytest.raises(cs.CsdrError):
        cs.Chain(channels=0)
    with pytest.raises(cs.CsdrError):
        cs.Chain(channels=8, demod="fm", kf=0.0)
    with pytest.raises(cs.CsdrError):
        cs.Chain(channels=8, chan_first=6, chan_count=4)
    # the stream state survived the failed calls
    y = ch.process(np.ones(M * 4, dtype=np.complex64))
    assert y.shape == (M, 4)


def test_chain_design_matches_kat():
    ch = cs.Chain(channels=20)
    assert ch.nco[1] == 0x86666600                               # KAT2
    taps = ch.taps
    assert taps.size == 280 and abs(taps[266] - 0.00075681) < 2e-8   # KAT1
    assert np.max(np.abs(taps - O.Pfb(20).taps)) < 1e-9
    assert cs.Chain(channels=256).nco[1] == 0x80800000


def test_firpfbch_channelizer_pipe_splits_like_reference():
    M = 4
    x = synth_cf32(M * 32, M, seed=1)
    outs = _run_pipe(cs.firpfbchChannelizer(M), [x, np.empty(0, np.complex64)])
    assert len(outs[0]) == M and all(a.shape == (32,) for a in outs[0])
    assert len(outs[1]) == 1 and outs[1][0].size == 0            # Liquid.chs:856-862 on nx = 0
    want = O.Chan(M).process(x)
    assert rel_rms(np.stack(outs[0]), want) < 2e-6


# --------------------------------------------------------------------------- fused M=256 kernel
def test_fused256_ragged_chunks_and_state_carry():
    """Chunks whose frame counts are not multiples of the 16-frame tile, shorter than the
    13-frame FIR history, and longer than the look-back window, against the oracle."""
    M = 256
    nfs = [1, 5, 13, 16, 17, 3, 37, 200, 12, 400]
    got, want, path = _chain_case(M, nfs)
    assert path.startswith("fused")
    r, e = rel_rms(got, want), max_abs_err(got, want)
    print(f"fused ragged DeNo rel-rms {r:.3e} max-abs {e:.3e}")
    assert r < 1e-5 and e < 1e-4 * np.abs(want).max()
    got, want, _ = _chain_case(M, nfs, demod="fm", kf=0.3)
    d = np.abs(wrap_pm(got.astype(np.float64) - want, 1.0 / 0.3))
    print(f"fused ragged FM median {np.median(d):.3e} p99 {np.quantile(d, 0.99):.3e}")
    assert np.median(d) < 2e-5 and np.quantile(d, 0.99) < 1e-3


def test_fused256_reference_chunk_matches_oracle_and_generic():
    """One reference-sized chunk (4096 frames = 256 tiles: every workgroup role, the full
    look-back depth) and a second one for state carry; fused vs oracle vs the generic path."""
    M, nf = 256, 4096
    x = synth_cf32(2 * M * nf, M, seed=77)
    from composable_sdr_amd import _lib
    fused = cs.Chain(channels=M, demod="fm", kf=0.3, max_frames=nf)
    gen = cs.Chain(channels=M, demod="fm", kf=0.3, max_frames=nf, flags=_lib.FLAG_QUIET | _lib.FLAG_FORCE_GENERIC)
    orc = O.Chain(M, demod="fm", kf=0.3)
    assert fused.path.startswith("fused") and gen.path == "generic"
    for i in range(2):
        c = x[i * M * nf:(i + 1) * M * nf]
        a, g, w = fused.process(c), gen.process(c), orc.process(c)
        d = np.abs(wrap_pm(a.astype(np.float64) - w, 1.0 / 0.3))
        dg = np.abs(wrap_pm(a.astype(np.float64) - g, 1.0 / 0.3))
        tone = np.arange(M) % 4 == 1                         # channels that carry an FM tone
        print(f"chunk {i}: fused-vs-oracle tone-ch max {d[tone].max():.3e} all median {np.median(d):.3e}; "
              f"fused-vs-generic tone-ch max {dg[tone].max():.3e}")
        assert d[tone].max() < 2e-5 and np.median(d) < 2e-5
        assert dg[tone].max() < 2e-5


def test_fused256_no_dc_block_and_shard():
    M, nf = 256, 64
    x = synth_cf32(M * nf, M, seed=5)
    a = cs.Chain(channels=M, dc_block=False, max_frames=nf).process(x)
    w = O.Chain(M, dc_block=False).process(x)
    r = rel_rms(a, w)
    print("fused no-DC rel-rms", r)
    assert r < 1e-6                                           # without the DC blocker's f32 noise floor
    part = cs.Chain(channels=M, chan_first=100, chan_count=56, max_frames=nf).process(x)
    full = cs.Chain(channels=M, max_frames=nf).process(x)
    assert np.array_equal(part, full[100:156])


def test_fused256_output_beyond_4gib_and_contiguous_shard_at_run_size():
    """(1) k_run256v2 addresses its output with 32-bit lane offsets over 16 rows and a 64-bit base per row group, so a call whose
    [256][nf] CF32 output exceeds 4 GiB (nf > 2 097 152) stays on the run kernel: one 2 101 248-frame call against the same stream in
    two calls (state carried), rows compared at the far end of the buffer too.  (2) a contiguous channel shard (chan_first /
    chan_count) takes the look-back tile kernel at every size: run-sized call against the rows of the whole band."""
    import torch
    from composable_sdr_amd import _lib
    from synth import synth_cf32_torch
    M = 256
    dev = torch.device("cuda", 0)
    nf = 2097152 + 4096
    half = 1048576
    parts = [synth_cf32_torch(M * half, M, dev, seed=900 + i) for i in range(2)] + [synth_cf32_torch(M * 4096, M, dev, seed=902)]
    x = torch.cat([p.view(-1) for p in parts]); del parts
    assert x.numel() == 2 * M * nf
    out1 = torch.empty(M * nf * 2, dtype=torch.float32, device=dev)           # 4.3 GB
    a = cs.Chain(channels=M, max_frames=nf, flags=_lib.FLAG_QUIET | _lib.FLAG_TIME_KERNELS)
    a.process_device(x.data_ptr(), M * nf, out1.data_ptr(), 0)
    torch.cuda.synchronize()
    assert a.kernel_time()[0] == "k_run256v2<CF32>"
    a.close()
    b = cs.Chain(channels=M, max_frames=half + 4096)
    o2a = torch.empty(M * half * 2, dtype=torch.float32, device=dev)
    o2b = torch.empty(M * (nf - half) * 2, dtype=torch.float32, device=dev)
    b.process_device(x.data_ptr(), M * half, o2a.data_ptr(), 0)
    b.process_device(x.data_ptr() + M * half * 8, M * (nf - half), o2b.data_ptr(), 0)
    torch.cuda.synchronize()
    b.close()
    v1 = out1.view(M, nf, 2)
    for rows in (slice(0, 4), slice(126, 130), slice(252, 256)):
        ref = torch.cat([o2a.view(M, half, 2)[rows], o2b.view(M, nf - half, 2)[rows]], dim=1)
        got = v1[rows]
        e = float((got - ref).pow(2).sum().sqrt() / ref.pow(2).sum().sqrt())
        print(f"> 4 GiB output, rows {rows.start}..{rows.stop - 1}: one call vs two calls rel-rms {e:.2e}")
        assert e < 2e-6
    del out1, o2a, o2b, v1
    torch.cuda.empty_cache()
    # (2)
    nf2 = 40000
    xs = x[: 2 * M * nf2].view(torch.float32).cpu().numpy().view(np.complex64).reshape(-1)
    del x
    torch.cuda.empty_cache()
    full = cs.Chain(channels=M, demod="fm", max_frames=nf2).process(xs)
    sh = cs.Chain(channels=M, demod="fm", chan_first=64, chan_count=96, max_frames=nf2, flags=_lib.FLAG_QUIET | _lib.FLAG_TIME_KERNELS)
    part = sh.process(xs)
    assert sh.kernel_time()[0] == "k_tile256<FM>" and part.shape == (96, nf2)
    sh.close()
    d = np.abs(wrap_pm(part.astype(np.float64) - full[64:160], 1.0 / 0.3))
    print(f"contiguous shard at run size (tile kernel) vs whole band (run kernel): FM median {np.median(d):.2e}, tone-channel max {d[1::4].max():.2e}")
    assert np.median(d) < 5e-6 and d[1::4].max() < 5e-6


def test_fused256_dc_state_matches_long_stream():
    """A strong DC offset makes the carried DC-blocker state matter: 64 chunks of 16 frames
    must equal one chunk of 1024 frames (look-back across tiles == carry across calls)."""
    M = 256
    x = synth_cf32(M * 1024, M, seed=8, dc=0.3 + 0.2j)
    one = cs.Chain(channels=M, max_frames=1024).process(x)
    ch = cs.Chain(channels=M, max_frames=1024)
    many = np.concatenate([ch.process(x[i * 16 * M:(i + 1) * 16 * M]) for i in range(64)], axis=1)
    want = O.Chain(M).process(x)
    # With |DC| = 0.36 the reference's filter state sits at |v| ~ 720 and its y = v0 - v1 carries
    # ulp(720)/2 ~ 3e-5 of f32 cancellation noise; the HIP path evaluates y = x - alpha*v1 and is
    # closer to exact arithmetic.  So: loose bound against the f32 oracle, tight bound against the
    # oracle fed with an f64 DC blocker.
    from scipy.signal import lfilter
    beta = float(np.float32(1) - np.float32(0.0005))
    yd = lfilter([1.0, -1.0], [1.0, -beta], x.astype(np.complex128)).astype(np.complex64)
    want64 = O.Chain(M, dc_block=False).process(yd)
    print("dc state: one-vs-many", rel_rms(one, many), "one-vs-oracle(f32 dc)", rel_rms(one, want),
          "one-vs-oracle(f64 dc)", rel_rms(one, want64), "oracle f32-vs-f64", rel_rms(want, want64))
    assert rel_rms(one, many) < 2e-6
    assert rel_rms(one, want) < 2e-4
    assert rel_rms(one, want64) < 2e-6
    assert rel_rms(one, want64) < rel_rms(want, want64)


def test_fused256_run_kernel_matches_tile_kernel_and_oracle(monkeypatch):
    """Large chunks use the dependency-free run kernel (k_run256); force it on a small chunk
    (CSDR_RUN_MIN_TILES) and compare with the look-back tile kernel and the oracle, including a
    ragged tail and state carry into a second call."""
    M = 256
    nfs = [16 * 40 + 5, 16 * 9, 300]
    x = synth_cf32(M * sum(nfs), M, seed=31, dc=0.05 + 0.02j)
    for demod in ("none", "fm"):
        knob(monkeypatch, "CSDR_RUN_MIN_TILES", "1")
        run = cs.Chain(channels=M, demod=demod, kf=0.3, max_frames=max(nfs))
        knob(monkeypatch, "CSDR_RUN_MIN_TILES", "1000000")
        tile = cs.Chain(channels=M, demod=demod, kf=0.3, max_frames=max(nfs))
        orc = O.Chain(M, demod=demod, kf=0.3)
        pos = 0
        for nf in nfs:
            c = x[pos:pos + nf * M]
            pos += nf * M
            a, t, w = run.process(c), tile.process(c), orc.process(c)
            if demod == "fm":
                d = np.abs(wrap_pm(a.astype(np.float64) - t, 1.0 / 0.3))
                dw = np.abs(wrap_pm(a.astype(np.float64) - w, 1.0 / 0.3))
                tone = np.arange(M) % 4 == 1
                print(f"run-vs-tile FM nf={nf}: tone max {d[tone].max():.3e} median {np.median(d):.3e}; vs oracle tone max {dw[tone].max():.3e}")
                assert d[tone].max() < 5e-6 and np.median(d) < 5e-6
                assert dw[tone].max() < 2e-5
            else:
                print(f"run-vs-tile DeNo nf={nf}: rel-rms {rel_rms(a, t):.3e}; vs oracle {rel_rms(a, w):.3e}")
                assert rel_rms(a, t) < 1e-6
                assert rel_rms(a, w) < 1e-5


@pytest.mark.parametrize("demod", ["fm", "none"])
def test_run_kernel_without_warm_up_windows_matches_the_warm_up_build(demod, monkeypatch):
    """Round 5: whole-band k_run256v2 launches read no warm-up window in front of a run; the run starts its halo tile from DC state 0 and
    k_run256_dcfix adds what the true state contributes to the four channels around DC (126..129) over the run's first 112 frames.  Against
    the same library with the windows (CSDR_NOWU=0), a strong DC offset, 24 runs, two calls (state carried, odd first frame index inside the
    second): every channel, and the corrected ones on their own; against the oracle behind an f64 DC blocker as the strong-DC test does."""
    M, kf = 256, 0.3
    nfs = [16 * 200, 16 * 192 + 5]
    x = synth_cf32(M * sum(nfs), M, seed=55, dc=0.3 - 0.2j)
    knob(monkeypatch, "CSDR_RUN_MIN_TILES", "1")
    a = cs.Chain(channels=M, demod=demod, kf=kf, max_frames=max(nfs))
    knob(monkeypatch, "CSDR_NOWU", "0")
    b = cs.Chain(channels=M, demod=demod, kf=kf, max_frames=max(nfs))
    monkeypatch.delenv("CSDR_NOWU")
    # the oracle behind an f64 DC blocker: with |DC| = 0.36 the f32 filter state sits at |v| ~ 720 and its y = v0 - v1 carries ~3e-5 of
    # cancellation noise (test_fused256_dc_state_matches_long_stream), which is of the size this test looks for
    from scipy.signal import lfilter
    beta = float(np.float32(1) - np.float32(0.0005))
    yd = lfilter([1.0, -1.0], [1.0, -beta], x.astype(np.complex128)).astype(np.complex64)
    orc = O.Chain(M, demod=demod, kf=kf, dc_block=False)
    pos = 0
    for nf in nfs:
        c = x[pos:pos + nf * M]
        ga, gb, w = a.process(c), b.process(c), orc.process(yd[pos:pos + nf * M])
        pos += nf * M
        near = slice(126, 130)
        if demod == "none":
            e_all, e_near = rel_rms(ga, gb), rel_rms(ga[near], gb[near])
            print(f"no-warm-up vs warm-up DeNo nf={nf}: all {e_all:.2e}, channels 126..129 {e_near:.2e}; vs oracle {rel_rms(ga, w):.2e} (warm-up build {rel_rms(gb, w):.2e})")
            assert e_all < 2e-6 and e_near < 2e-5
            assert rel_rms(ga, w) < 1.2 * rel_rms(gb, w) + 1e-6 and max_abs_err(ga, w) < 1e-4 * np.abs(w).max()
        else:
            d = np.abs(wrap_pm(ga.astype(np.float64) - gb, 1.0 / kf))
            dw = np.abs(wrap_pm(ga.astype(np.float64) - w, 1.0 / kf))
            tone = np.arange(M) % 4 == 1
            print(f"no-warm-up vs warm-up FM nf={nf}: median {np.median(d):.2e}, tone max {d[tone].max():.2e}, 126..129 median {np.median(d[near]):.2e}; vs oracle tone max {dw[tone].max():.2e}")
            assert np.median(d) < 2e-6 and d[tone].max() < 1e-5 and np.median(d[near]) < 2e-5
            assert dw[tone].max() < 3e-5
    a.close(); b.close()


# --------------------------------------------------------------------------- sharding on the HIP chain
@pytest.mark.parametrize("mode", ["time", "channel"])
def test_sharded_two_ranks_on_one_gpu(mode):
    """The partitions of composable_sdr_amd.sharded driven rank by rank on one GPU (the gloo
    world-2 CPU test covers the collectives): stripes / channel shards reassemble the stream."""
    from composable_sdr_amd.pipes import ChainConfig
    from composable_sdr_amd.sharded import ShardedChain
    M, nf = 256, 1200
    x = synth_cf32(M * nf, M, seed=17)
    cfg = ChainConfig(channels=M, demod="none", max_frames=512)
    want = cs.Chain(cfg).process(x[:M * 512])
    full = np.concatenate([cs.Chain(channels=M, max_frames=nf).process(x)], axis=1)
    parts = [ShardedChain(cfg, mode=mode, rank=r, world=2).process_stream(x) for r in range(2)]
    got = np.concatenate(parts, axis=1 if mode == "time" else 0)
    if mode == "channel":
        il = [ShardedChain(cfg, mode=mode, rank=r, world=2, interleave=True).process_stream(x) for r in range(2)]
        gi = np.empty_like(got); gi[0::2], gi[1::2] = il[0], il[1]
        print("interleaved channel shards vs contiguous rel-rms", rel_rms(gi, got))
        assert rel_rms(gi, got) < 1e-6
    assert got.shape == full.shape
    print(mode, "sharded vs single rel-rms", rel_rms(got, full))
    assert rel_rms(got, full) < (2e-6 if mode == "time" else 1e-7)
    assert np.array_equal(want, full[:, :512]) or rel_rms(want, full[:, :512]) < 1e-6


def test_tail_only_chain_is_the_chain_behind_its_channelizer():
    """CSDR_FLAG_TAIL_ONLY (the per-channel tail alone: automaticGainControl -> fmDemodulator on a channel-major CF32 plane) fed with
    the DeNo chain's output must reproduce the whole chain BIT FOR BIT (same CF32 plane, same recurrence), over run-sized and small
    calls with the state carried; against the oracle on the first call."""
    import torch
    from synth import synth_cf32_torch
    M, kf = 256, 0.3
    frames = [40000, 33, 36864]
    x = synth_cf32_torch(M * sum(frames), M, torch.device("cuda", 0), seed=771).cpu().numpy().view(np.complex64).reshape(-1)
    for demod in ("fm", "none"):
        full = cs.Chain(channels=M, demod=demod, kf=kf, agc=10.0, max_frames=max(frames))
        deno = cs.Chain(channels=M, max_frames=max(frames))
        tail = cs.Chain(channels=M, demod=demod, kf=kf, agc=10.0, tail_only=True, max_frames=max(frames))
        assert "tail-only" in tail.path
        pos = 0
        for i, f in enumerate(frames):
            xa = x[pos * M:(pos + f) * M]
            a = full.process(xa)
            b = tail.process(deno.process(xa).reshape(-1))
            assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), (demod, f)
            if i == 0 and demod == "fm":
                want = O.Chain(M, demod="fm", kf=kf, agc_db=10.0).process(xa)
                assert int(np.sum((b == 0) != (want == 0))) == 0
            pos += f
        full.close(); deno.close(); tail.close()
    with pytest.raises(cs.CsdrError):
        cs.Chain(channels=M, demod="fm", tail_only=True)              # needs the AGC on


def test_hybrid_sharding_two_ranks_on_one_gpu():
    """SURVEY 8e(B) on the HIP chain, rank by rank on one GPU (the world-2 gloo test covers the all-to-all): each rank's DeNo front
    end on its time stripe behind the warm-up prefix, the [M][stripe] planes regrouped into channel blocks, each rank's tail handle
    over the whole span -- against the single-GPU chain with the AGC on."""
    import torch
    from composable_sdr_amd.pipes import ChainConfig
    from composable_sdr_amd.sharded import ShardedChain
    from synth import synth_cf32_torch
    M, nf, kf, G = 256, 81920, 0.3, 2
    x = synth_cf32_torch(M * nf, M, torch.device("cuda", 0), seed=772).cpu().numpy().view(np.complex64).reshape(-1)
    cfg = ChainConfig(channels=M, demod="fm", kf=kf, agc=10.0, max_frames=nf // G + 256)
    scs = [ShardedChain(cfg, mode="hybrid", rank=r, world=G) for r in range(G)]
    fronts = [sc.hybrid_front(x) for sc in scs]
    assert [f[0].shape for f in fronts] == [(M, nf // G)] * G and fronts[0][1] == [(0, nf // G), (nf // G, nf)]
    cn = M // G
    got = np.concatenate([scs[g].hybrid_tail([fronts[p][0][g * cn:(g + 1) * cn] for p in range(G)]) for g in range(G)], axis=0)
    one = cs.Chain(channels=M, demod="fm", kf=kf, agc=10.0, max_frames=nf)
    want = one.process(x)
    one.close()
    assert got.shape == want.shape
    mism = int(np.sum((got == 0) != (want == 0)))
    d = np.abs(wrap_pm(got.astype(np.float64) - want, 1.0 / kf))
    op = want != 0
    print(f"hybrid (2 ranks, one GPU) vs single chain: mute-mask mismatches {mism}, open {op.mean():.3f}, open median {np.median(d[op]):.2e}, p99.9 {np.quantile(d, 0.999):.2e}")
    assert mism == 0 and 0.05 < op.mean() < 0.95
    assert np.median(d[op]) < 2e-5 and np.quantile(d, 0.999) < 5e-4


@pytest.mark.parametrize("M,demod,agc", [(256, "fm", 0.0), (64, "none", 0.0), (20, "none", 0.0), (1024, "fm", 0.0), (256, "fm", 10.0), (8, "wbfm", 0.0)])
def test_dft_direction_flag_matches_a_backward_dft_oracle(M, demod, agc):
    """SURVEY section 7, hard part 1: the direction of firpfbch_crcf_analyzer_execute's transform is recalled, not pinned.  With
    CSDR_FLAG_DFT_BACKWARD the handle delivers the other convention; checked against the oracle run with an actual e^{+j} DFT
    (oracle/csdr_oracle.c orc_pfb_set_dft_backward), every route (fused 64 / 256 / 1024, any-M, AGC tail, WBFM tail), over two calls."""
    nfs = [96, 40] if M != 8 else [96, 48]
    x = synth_cf32(M * sum(nfs), M, seed=300 + M)
    ch = cs.Chain(channels=M, demod=demod, kf=0.3, agc=agc, max_frames=max(nfs), dft_backward=True)
    fw = cs.Chain(channels=M, demod=demod, kf=0.3, agc=agc, max_frames=max(nfs))
    assert "dft-backward" in ch.path
    orc = O.Chain(M, demod=demod, kf=0.3 if demod != "wbfm" else 0.6, agc_db=agc, dft_backward=True)
    pos = 0
    perm = [(M - k) % M for k in range(M)]
    for nf in nfs:
        c = x[pos:pos + nf * M]; pos += nf * M
        got, fwd, want = ch.process(c), fw.process(c), orc.process(c)
        assert np.array_equal(got.view(np.uint32), fwd[perm].view(np.uint32))       # exactly the forward handle's rows, re-labelled
        if demod == "none":
            assert rel_rms(got, want) < 1e-5
        elif agc:
            assert int(np.sum((got == 0) != (want == 0))) == 0
        else:
            kf = 0.6 if demod == "wbfm" else 0.3
            d = np.abs(wrap_pm(got.astype(np.float64) - want, 1.0 / kf)) if demod == "fm" else np.abs(got - want)
            assert np.median(d) < 2e-5, (M, demod, np.median(d))
    ch.close(); fw.close()
    with pytest.raises(cs.CsdrError):
        cs.Chain(channels=256, chan_first=1, chan_stride=2, dft_backward=True)     # shards: not built


def test_comm_collectives_under_the_c_abi_world_of_one():
    """include/csdr.h csdr_comm (RCCL loaded on demand) end to end on this box's one GPU: a communicator of one rank, then
    csdr_chain_process_device_mix (chain + ncclAllReduce on the caller's stream) against the oracle's `mix` (Trans.hs:119-122),
    csdr_comm_broadcast, and csdr_hybrid_exchange (its own block: a device copy).  N > 1 cannot be formed here (one GPU per box)."""
    import torch
    from composable_sdr_amd.pipes import ChainConfig
    from composable_sdr_amd.sharded import Comm, ShardedChain
    dev = torch.device("cuda", 0)
    comm = Comm(0, 1, Comm.unique_id())
    assert (comm.rank, comm.world) == (0, 1)
    assert cs.lib().csdr_comm_rank(comm.h) == 0 and cs.lib().csdr_comm_world(comm.h) == 1
    stream = torch.cuda.current_stream().cuda_stream
    for M, demod, agc in ((64, "fm", 0.0), (256, "none", 0.0), (20, "fm", -10.0)):
        nf = 2048
        x = synth_cf32(M * nf, M, seed=900 + M)
        sc = ShardedChain(ChainConfig(channels=M, demod=demod, kf=0.3, agc=agc, mix=True, max_frames=nf), mode="channel", rank=0, world=1, comm=comm)
        xd = torch.from_numpy(x.view(np.float32).copy()).to(dev)
        w = 1 if demod == "fm" else 2
        od = torch.zeros(nf * w, dtype=torch.float32, device=dev)
        n = sc.process_device_mix(xd, od, stream)
        torch.cuda.synchronize()
        assert n == nf
        got = od.cpu().numpy()
        got = got if demod == "fm" else got.view(np.complex64)
        want = O.Chain(M, demod=demod, kf=0.3, agc_db=agc, mix=True).process(x)
        local = cs.Chain(channels=M, demod=demod, kf=0.3, agc=agc, mix=True, max_frames=nf).process(x)
        assert np.array_equal(got.view(np.uint32), local.view(np.uint32))           # a sum over one rank changes nothing
        e = np.abs(got - want).max() / max(np.abs(want).max(), 1e-9)
        print(f"csdr_chain_process_device_mix M={M} {demod} agc={agc}: max err / max = {e:.2e}")
        assert e < 2e-5 * np.sqrt(M)
        # a chain without mix is refused
        plain = cs.Chain(channels=M, demod=demod, kf=0.3, max_frames=nf)
        rc = cs.lib().csdr_chain_process_device_mix(plain.h, comm.h, xd.data_ptr(), M * nf, od.data_ptr(), None, stream)
        assert rc == -1 and b"mix" in cs.lib().csdr_last_error()
        plain.close(); sc.chain.close()
    # broadcast from the only rank: the buffer is untouched; the hybrid exchange of a one-rank world is a copy of the plane
    buf = torch.arange(1 << 16, dtype=torch.float32, device=dev)
    keep = buf.clone()
    comm.broadcast(buf.data_ptr(), buf.numel() * 4, 0, stream)
    recv = torch.zeros_like(buf)
    comm.hybrid_exchange(buf.data_ptr(), recv.data_ptr(), 32, [buf.numel() // 2 // 32], 8, stream)
    torch.cuda.synchronize()
    assert torch.equal(buf, keep) and torch.equal(recv, keep)
    comm.close()


def test_hybrid_step_overlapped_is_bit_identical_to_serial():
    """The overlapped hybrid step (ShardedChain.process_device_hybrid(substripes=2, overlap=True): exchanges on a second stream, under
    the next round's front end and the previous round's tail) against the same rounds with everything in line on one stream: bit for
    bit, over several steps with the state carried; and against the single chain with the AGC on (a one-rank world: the stripes ARE the
    stream).  The exchange goes through the C ABI (csdr_hybrid_exchange on a one-rank RCCL communicator)."""
    import torch
    from composable_sdr_amd.pipes import ChainConfig
    from composable_sdr_amd.sharded import Comm, ShardedChain
    from synth import synth_cf32_torch
    dev = torch.device("cuda", 0)
    M, nf, kf, steps = 256, 32768, 0.3, 3
    comm = Comm(0, 1, Comm.unique_id())
    cfg = ChainConfig(channels=M, demod="fm", kf=kf, agc=10.0, max_frames=nf)
    xs = [synth_cf32_torch(M * nf, M, dev, seed=880 + i).view(-1) for i in range(steps)]
    outs = {}
    for ov in (False, True):
        sc = ShardedChain(cfg, mode="hybrid", rank=0, world=1, comm=comm)
        plane = torch.empty(M * nf * 2, dtype=torch.float32, device=dev); recv = torch.empty_like(plane)
        side = torch.cuda.Stream(device=dev)                     # not the default stream: the caller's stream is honoured
        res = []
        for i in range(steps):
            out = torch.zeros(M * nf, dtype=torch.float32, device=dev)
            n = sc.process_device_hybrid(xs[i], plane, recv, out, side.cuda_stream, substripes=2, overlap=ov)
            assert n == M * nf
            res.append(out)
        torch.cuda.synchronize()
        outs[ov] = [o.cpu().numpy().reshape(2, M, nf // 2) for o in res]
        sc.chain.close(); sc.tail.close()
    for a, b in zip(outs[False], outs[True]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    one = cs.Chain(channels=M, demod="fm", kf=kf, agc=10.0, max_frames=nf)
    for i in range(steps):
        xh = xs[i].cpu().numpy().view(np.complex64)
        for r in range(2):                                       # the single chain in the same calls: same kernels on the same samples
            want = one.process(xh[r * M * nf // 2:(r + 1) * M * nf // 2])
            assert np.array_equal(outs[True][i][r].view(np.uint32), want.view(np.uint32)), (i, r)
    one.close(); comm.close()
    from composable_sdr_amd.pipes import ChainConfig as CC
    with pytest.raises(ValueError):
        ShardedChain(CC(channels=M, demod="fm", kf=kf, agc=10.0, mix=True, max_frames=nf), mode="hybrid", rank=0, world=1)


@pytest.mark.parametrize("shard,mix", [("channel", True), ("channel", False), ("time", False)])
def test_bench_channel_shard_two_ranks_one_gpu(shard, mix):
    """bench.py's N > 1 paths end to end under torch.distributed.run with two ranks (both on this box's only GPU, gloo
    instead of RCCL: CSDR_BENCH_ONE_GPU): the JSON line names the partition, the collective and the rank count."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CSDR_BENCH_ONE_GPU="1", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29571", os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--frames", "8192",
           "--shard", shard, "--demod", "none", "--no-cpu-baseline", "--no-agc-variant", "--preheat-ms", "300", "--full"] + (["--mix"] if mix else [])
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=root)
    lines = [l for l in p.stdout.splitlines() if l.startswith('{"metric"')]
    assert p.returncode == 0 and len(lines) == 1, p.stderr[-2000:]
    r = json.loads(lines[0])
    assert r["n_gpus"] == 2 and r["config"]["rccl_ranks"] == 2 and r["value"] > 0
    assert r["cold_window"]["value"] > 0 and r["sustained_long"]["seconds"] >= 0.25 and r["sustained_long"]["value"] > 0
    # the roofline figure is the sustained run's launch cadence (hipEvents around that run), the K-step window and the event pairs sit beside it
    rf = r["roofline"]
    assert rf["launches_event_pairs"] == 3 and rf["launch_ms"] > 0 and rf["launches"] == r["sustained_long"]["launches"] >= 10
    assert "sustained_long" in rf["launch_ms_source"] and rf["frac_k_step_window"] > 0 and rf["frac_event_pairs"] > 0
    assert abs(rf["launch_ms"] - r["sustained_long"]["launch_ms_events"]) < 1e-9
    assert r["value_sustained"] == r["sustained_long"]["value"]
    # which partition `value` is: the FIRST key of config, inside the first 120 characters of its text
    assert list(r["config"])[0] == "sharding"
    if shard == "channel":
        assert r["scaling"] == "strong" and r["config"]["sharding"].startswith("channel shards (north_star's partition)") and "interleaved-shard" in r["config"]["route"]
        assert ("all-reduce" in r["config"]["collective"]) == mix and ("all-reduce" in r["config"]["sharding"]) == mix
    else:
        assert r["scaling"] == "weak" and r["config"]["sharding"].startswith("independent time stripes, no collective") and r["config"]["collective"] == "none"
        assert "value_channel_shard" in r["config"]["sharding"]
        # the default partition's line also carries north_star's partition, measured in the same run
        cs2 = r["channel_shard"]
        assert cs2["value"] > 0 and cs2["scaling"] == "strong" and "channel-interleaved" in cs2["sharding"] and cs2["rccl_ranks"] == 2
        assert ("all-reduce" in cs2["collective"]) == mix
    if not mix:
        # the AGC configuration through time-sharded front ends, one all-to-all and channel-sharded tails, same run
        hy = r["hybrid"]
        assert hy["value"] > 0 and hy["scaling"] == "weak" and "all_to_all" in hy["path"] and "tail-only" in hy["path"] and hy["rccl_ranks"] == 2
        assert hy["overlap"]["substripes"] == 2 and hy["overlap"]["ms_per_step_serial"] > 0 and r["value_hybrid"] == hy["value"]
    if shard == "time":
        assert r["value_channel_shard"] == r["channel_shard"]["value"]
    # the label names the kernel that was timed, not a create-time string
    assert r["config"]["path"].endswith("|" + r["roofline"]["kernel"])


def test_bench_side_measurements_cannot_cost_the_line():
    """The N > 1 side measurements (channel_shard / hybrid: the only data-path collectives of a default run, never run on N > 1 hardware)
    sit behind the contract's numbers under a watchdog: with a limit they cannot meet the line is still printed -- without them, with
    `side_error` -- and both ranks leave with status 0."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CSDR_BENCH_ONE_GPU="1", MASTER_ADDR="127.0.0.1", CSDR_BENCH_SIDE_TIMEOUT="0.001")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29573", os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--frames", "8192",
           "--demod", "none", "--no-cpu-baseline", "--no-agc-variant", "--preheat-ms", "300", "--full"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=root)
    lines = [l for l in p.stdout.splitlines() if l.startswith('{"metric"')]
    assert p.returncode == 0 and len(lines) == 1, p.stderr[-2000:]
    r = json.loads(lines[0])
    assert r["n_gpus"] == 2 and r["value"] > 0 and r["roofline"]["launches_event_pairs"] == 3 and r["sustained_long"]["value"] > 0
    assert "did not finish" in r["side_error"] and "channel_shard" not in r and "hybrid" not in r
    assert "side measurements failed" in p.stderr
    # a CI that wants a hung side path to fail the job asks for it: the line is still printed, the status is 3
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(env, CSDR_BENCH_SIDE_STRICT="1"), cwd=root)
    lines = [l for l in p.stdout.splitlines() if l.startswith('{"metric"')]
    assert p.returncode != 0 and len(lines) == 1 and "side_error" in json.loads(lines[0]), p.stderr[-2000:]


def test_bench_plain_run_dumps_the_last_timed_step(tmp_path):
    """A plain bench.py run (no --full) prints the headline fields of exactly K timed steps and none of the side measurements;
    --dump-outputs writes what the last timed step computed: the same array in two runs, equal to the output of a fresh handle
    taken through the same W + K steps on the same inputs."""
    import json
    import subprocess
    import sys
    import torch
    from synth import synth_cf32_torch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    M, nf, K, W = 256, 8192, 5, 2
    runs = []
    for d in ("a", "b"):
        cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", str(W), "--frames", str(nf),
               "--preheat-ms", "200", "--dump-outputs", str(tmp_path / d)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root)
        lines = [l for l in p.stdout.splitlines() if l.startswith('{"metric"')]
        assert p.returncode == 0 and len(lines) == 1, p.stderr[-2000:]
        runs.append(json.loads(lines[0]))
    r = runs[0]
    assert r["steps"] == K and r["warmup"] == W and r["value"] > 0 and r["ms_per_step"] > 0
    assert r["unit"] == "MS/s" and r["higher_is_better"] is True and r["dtype"] == "f32" and r["metric"].startswith("MS/s")
    assert abs(r["value"] - M * nf / r["ms_per_step"] / 1e3) <= 0.02 * r["value"]
    for k in ("roofline", "cold_window", "sustained", "agc_variant", "other_configs", "cpu_baseline"):
        assert k not in r, k
    a, b = (np.load(tmp_path / d / "output.npy") for d in ("a", "b"))
    assert a.dtype == np.float32 and a.shape == (M, nf)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    dev = torch.device("cuda", 0)
    xs = [synth_cf32_torch(M * nf, M, dev, seed=20260101 + 7919 * i) for i in range(2)]
    out = torch.empty(M * nf, dtype=torch.float32, device=dev)
    from composable_sdr_amd import _lib
    ch = cs.Chain(channels=M, demod="fm", kf=0.3, max_frames=nf, device=0, flags=_lib.FLAG_QUIET | _lib.FLAG_TIME_KERNELS | _lib.FLAG_TIME_REGION)
    stream = torch.cuda.current_stream().cuda_stream
    for i in list(range(W)) + list(range(K)):
        ch.process_device(xs[i & 1].data_ptr(), M * nf, out.data_ptr(), stream)
    torch.cuda.synchronize()
    ch.close()
    assert np.array_equal(out.cpu().numpy().reshape(M, nf).view(np.uint32), a.view(np.uint32))


def test_seek_frames_sets_premix_phase():
    M = 256
    x = synth_cf32(M * 80, M, seed=23)
    ref = cs.Chain(channels=M, dc_block=False, max_frames=80).process(x)
    ch = cs.Chain(channels=M, dc_block=False, max_frames=80)
    ch.seek_frames(33)                                  # odd frame: the pre-mix phasor row flips
    got = ch.process(x[33 * M:])
    # after the 13-frame FIR transient the outputs coincide with the un-seeked stream
    assert rel_rms(got[:, 14:], ref[:, 33 + 14:]) < 1e-6
    gen = cs.Chain(channels=20, dc_block=False, max_frames=80)   # generic path, non-periodic NCO
    x20 = synth_cf32(20 * 80, 20, seed=24)
    ref20 = cs.Chain(channels=20, dc_block=False, max_frames=80).process(x20)
    gen.seek_frames(33)
    assert rel_rms(gen.process(x20[33 * 20:])[:, 14:], ref20[:, 33 + 14:]) < 1e-6


# --------------------------------------------------------------------------- file-in / file-out replay
def test_sdr_process_example3_shape(tmp_path):
    """README Example 3 scaled by 1/25: -n 640000 -c 20 --demod DeNo -> 20 files of n/20 samples
    x 8 bytes, 'no samples are lost' (KAT4), contents equal to the oracle's."""
    from composable_sdr_amd.app import sdr_process
    M, n = 20, 640000
    x = synth_cf32(n + 777, M, seed=3)                       # file longer than -n: takeNArr trims
    src = tmp_path / "input.cf32"
    x.tofile(src)
    names = sdr_process(str(src), channels=M, demod="none", numsamples=n, outname=str(tmp_path / "output"), chunksize=1000)
    assert len(names) == M and names[0].endswith("output_ch1.cf32") and names[-1].endswith("output_ch20.cf32")
    want = O.Chain(M).process(x[:n])
    for k, nm in enumerate(names):
        got = np.fromfile(nm, dtype=np.complex64)
        assert got.nbytes == n // M * 8 == 256000
        # per-file error against the stream-wide scale (noise-only channels are 20 dB below the tones)
        assert max_abs_err(got, want[k]) < 1e-4 * np.abs(want).max()
        assert np.sqrt(np.mean(np.abs(got - want[k]) ** 2)) < 1e-5 * np.sqrt(np.mean(np.abs(want) ** 2))


def test_sdr_process_fm_mix_single_output(tmp_path):
    from composable_sdr_amd.app import sdr_process
    M, n = 256, 256 * 4096 + 256 * 100
    x = synth_cf32(n, M, seed=4)
    src = tmp_path / "in.cf32"
    x.tofile(src)
    names = sdr_process(str(src), channels=M, demod="fm", kf=0.3, mix=True, numsamples=n, outname=str(tmp_path / "o"))
    assert names == [str(tmp_path / "o.f32")]
    got = np.fromfile(names[0], dtype=np.float32)
    assert got.size == n // M                                 # one mixed stream of n/M samples


# --------------------------------------------------------------------------- BASELINE.json configs 4 and 5 shapes
def test_config4_shape_1024ch_fm_matches_oracle():
    M = 1024
    got, want, path = _chain_case(M, [24, 9], demod="fm", kf=0.3)
    _, r, _ = _chain_case(M, [24, 9], demod="none")
    r = np.abs(r.reshape(want.shape))
    d = np.abs(wrap_pm(got.astype(np.float64) - want, 1.0 / 0.3))
    rmin = np.minimum(r, np.concatenate([np.zeros((M, 1)), r[:, :-1]], axis=1))
    print(f"cfg4 shape M=1024 FM [{path}] median {np.median(d):.3e} weighted max {(d * rmin / r.max()).max():.3e}")
    assert (d * rmin / r.max()).max() < 2 * (1 / (2 * np.pi * 0.3)) * 1e-4 and np.median(d) < 5e-5


def test_config5_shape_4096ch_mix_matches_oracle():
    M = 4096
    got, want, path = _chain_case(M, [10, 6], mix=True)
    assert got.shape == want.shape == (16,)
    full, wfull, _ = _chain_case(M, [10, 6])
    print(f"cfg5 shape M=4096 [{path}] DeNo rel-rms {rel_rms(full, wfull):.3e}; mix abs err {np.abs(got - want).max():.3e} of {np.abs(want).max():.3f}")
    assert rel_rms(full, wfull) < 1e-5
    # 4096-term left fold of values up to ~70: bounded by the unmixed tolerance times sqrt(M)
    assert np.abs(got - want).max() < 1e-4 * np.abs(wfull).max() * np.sqrt(M)


def test_freqdem_of_a_collapsed_agc_gain_stays_finite():
    """Round 5 find: with the reference's g0 = 1000 start transient a strong channel drives the AGC gain down to ~1e-21, the
    products conj(r') r of the open samples behind it are ~1e-41 -- denormal -- and v_rcp_f32 takes a denormal for zero: freqdem came out
    NaN where liquid's cargf gives an angle.  fm_sample_rn / fm_quad_rn now scale such products by 2^90 first."""
    rng = np.random.default_rng(7)
    n = 4096
    base = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    for scale, tol in ((1.0, 2e-6), (1e-12, 2e-6), (3e-21, None), (1e-23, None)):
        x = (base * np.float32(scale)).astype(np.complex64)
        got = _run_pipe(cs.fmDemodulator(0.3), [x])[0]
        want = O.FreqDem(0.3).demodulate_block(x)
        assert np.isfinite(got).all(), scale
        d = np.abs(wrap_pm(got.astype(np.float64) - want, 1.0 / 0.3))
        print(f"freqdem at |r| ~ {scale:g}: max |err| {d.max():.2e} median {np.median(d):.2e}")
        if tol is not None:
            assert d.max() < tol
        else:
            # the oracle's (and liquid's) own products are denormal here: a few significant bits; the GPU's scaled ones are exact
            assert np.median(d) < 0.05
    # and through the chain: AGC + FM on a signal whose start transient collapses the gain
    M = 64
    x = (synth_cf32(M * 600, M, seed=77) * np.float32(40.0)).astype(np.complex64)
    got = cs.Chain(channels=M, demod="fm", kf=0.3, agc=-40.0, max_frames=600).process(x)
    assert np.isfinite(got).all()


@pytest.mark.parametrize("demod,agc,mix", [("none", 0.0, False), ("fm", 0.0, False), ("fm", 0.0, True), ("fm", 23.0, False), ("none", -10.0, True)])
def test_fused4096_chain_matches_oracle_and_any_m_route(demod, agc, mix):
    """The fused 4096-channel route (k_front4096: branch-tiled DC blocker + pre-mix + FIR + radix-4 split; k_back4096: four 1024-point DFTs
    per frame + tails; kernels_pfb4096.hip) against the oracle and against the any-M route (CSDR_FLAG_FORCE_GENERIC), every call on its
    own.  Calls: 40 frames (one run; run 0 from the zero state), 9 (odd, fewer frames than the 21-frame cold-start window: the saved raw tail
    is shifted, the NCO parity turns odd), 250 (two runs: a cold start inside the call; ends inside a 16-frame block), 1024 (eight runs:
    the XCD-aware workgroup map).  (-a 23: at 4096 channels the noise-only channels of the synthetic signal sit at rssi ~ +10 dB -- sigma^2 x
    0.93 M -- and the carriers at +36 dB; the squelch threshold goes between the two populations, as SURVEY 8d prescribes.)"""
    from composable_sdr_amd import _lib
    M, kf = 4096, 0.3
    nfs = [40, 9, 250, 1024]
    x = synth_cf32(M * sum(nfs), M, seed=4096)
    x = (x + np.complex64(0.02 - 0.01j)).astype(np.complex64)        # a DC offset the blocker has to carry across runs and calls
    kw = dict(channels=M, demod=demod, kf=kf, agc=agc, mix=mix, max_frames=max(nfs))
    ch = cs.Chain(**kw)
    gen = cs.Chain(flags=_lib.FLAG_QUIET | _lib.FLAG_FORCE_GENERIC, **kw)
    assert "fused-4096" in ch.path and "k_front4096" in ch.path and "fused" not in gen.path
    orc = O.Chain(M, demod=demod, kf=kf, agc_db=agc, mix=mix)
    pos = 0
    for nf in nfs:
        c = x[pos:pos + nf * M]; pos += nf * M
        got, alt, want = ch.process(c), gen.process(c), orc.process(c)
        assert got.shape == want.shape
        if agc:
            if mix:
                e = np.abs(got - want).max() / max(np.abs(want).max(), 1e-9)
                print(f"fused-4096 DeNo+AGC mix nf={nf}: {e:.2e}")
                assert e < 2e-5 * np.sqrt(M)
            else:
                assert int(np.sum((got == 0) != (want == 0))) == 0, nf
                op = want != 0
                d = np.abs(wrap_pm(got.astype(np.float64) - want, 1.0 / kf))
                assert not op.any() or np.median(d[op]) < 2e-5
        elif demod == "none":
            print(f"fused-4096 DeNo nf={nf}: vs oracle {rel_rms(got, want):.2e}, vs any-M {rel_rms(got, alt):.2e}")
            assert rel_rms(got, want) < 1e-5 and max_abs_err(got, want) < 1e-4 * np.abs(want).max()
            assert rel_rms(got, alt) < 2e-6
        elif mix:
            # a sum of 4096 freqdem outputs, most of them from noise-only channels: a sample next to the branch cut of arg() lands on the
            # other side of it under any rounding difference and moves the sum by exactly 1 / kf -- compared modulo 1 / kf
            d, da = np.abs(wrap_pm(got.astype(np.float64) - want, 1.0 / kf)), np.abs(wrap_pm(got.astype(np.float64) - alt, 1.0 / kf))
            print(f"fused-4096 FM mix nf={nf}: mod 1/kf max err vs oracle {d.max():.2e} median {np.median(d):.2e}, vs any-M {da.max():.2e} (sum of {M} values <= {1 / (2 * kf):.2f})")
            # (3072 of the 4096 summands are noise-only channels whose phase error is the CF32 error over a small |r|: the f32 routes agree
            # with each other to < 5e-3, with the oracle's f64 DFT to the sum of those ill-conditioned terms)
            assert np.median(d) < 1e-2 and np.quantile(d, 0.99) < 0.15 and da.max() < 5e-3
        else:
            d = np.abs(wrap_pm(got.astype(np.float64) - want, 1.0 / kf))
            da = np.abs(wrap_pm(got.astype(np.float64) - alt, 1.0 / kf))
            tone = np.arange(M) % 4 == 1
            print(f"fused-4096 FM nf={nf}: median {np.median(d):.2e}, tone p99.9 {np.quantile(d[tone], 0.999):.2e}; vs any-M median {np.median(da):.2e}")
            assert np.median(d) < 2e-5 and np.quantile(d[tone], 0.999) < 2e-5 and np.median(da) < 2e-6
    ch.close(); gen.close()


def test_cpp_soapy_sdr_file_matches_python_replay(tmp_path):
    """The C++ host (soapy_sdr_file) and the Python replay drive the same C ABI: identical bytes."""
    import os
    import subprocess
    from composable_sdr_amd.app import sdr_process
    exe = host_exe("soapy_sdr_file")
    M, n = 64, 64 * 4096 + 64 * 37
    x = synth_cf32(n + 100, M, seed=6)
    src = tmp_path / "in.cf32"
    x.tofile(src)
    py = sdr_process(str(src), channels=M, demod="fm", kf=0.3, numsamples=n, outname=str(tmp_path / "py"), chunksize=1024)
    r = subprocess.run([exe, "--filename", str(src), "-n", str(n), "-c", str(M), "--demod", "DeNBFM", "0.3", "-o", str(tmp_path / "cc")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for k in (1, 17, 64):
        a = np.fromfile(tmp_path / f"py_ch{k}.f32", dtype=np.float32)
        b = np.fromfile(tmp_path / f"cc_ch{k}.f32", dtype=np.float32)
        assert a.size == n // M and np.array_equal(a, b)


def test_cpp_soapy_sdr_file_channel_shards_and_mix_through_the_c_collectives(tmp_path):
    """host/soapy_sdr_file --world / --rank / --id-file (one process per GPU; here the two processes of a world of two run one after the
    other on this box's GPU, which per-channel sinks allow: no exchange step): process R writes exactly the files _ch<R+1>, _ch<R+1+W>, ...
    (SoapySDR.hs:209-212) with the contents of the unsharded run; `--mix` in a world of one goes through csdr_chain_process_mix
    (RCCL all-reduce under the C ABI) and leaves the unsharded run's bytes."""
    import os
    import subprocess
    exe = host_exe("soapy_sdr_file")
    M, n, W = 64, 64 * 4096 * 2 + 64 * 37, 2
    x = synth_cf32(n + 100, M, seed=61)
    src = tmp_path / "in.cf32"
    x.tofile(src)
    base = [exe, "--filename", str(src), "-n", str(n), "-c", str(M), "--demod", "DeNBFM", "0.3"]
    r = subprocess.run(base + ["-o", str(tmp_path / "one")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for g in range(W):
        r = subprocess.run(base + ["-o", str(tmp_path / "sh"), "--world", str(W), "--rank", str(g)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        mine = sorted(f for f in os.listdir(tmp_path) if f.startswith("sh_ch"))
        assert len(mine) == (g + 1) * M // W                  # only the owned channels' files appear
    for k in range(1, M + 1):
        a = np.fromfile(tmp_path / f"one_ch{k}.f32", dtype=np.float32)
        b = np.fromfile(tmp_path / f"sh_ch{k}.f32", dtype=np.float32)
        assert a.size == b.size == n // M
        d = np.abs(wrap_pm(a.astype(np.float64) - b, 1.0 / 0.3))
        assert np.median(d) < 2e-5, k                         # pruned DFT of the shard vs the whole band: chain tolerance
    # --mix: a world of one through the communicator (id file bootstrap) == no communicator at all
    r = subprocess.run(base + ["-m", "-o", str(tmp_path / "mix0")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run(base + ["-m", "-o", str(tmp_path / "mix1"), "--world", "1", "--rank", "0", "--id-file", str(tmp_path / "id.bin")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert not os.path.exists(tmp_path / "id.bin")          # rank 0 removes the id once every rank has joined: nothing stale for the next run
    # a stale id of an earlier (crashed) run under the same path is replaced, not read: the run still succeeds
    (tmp_path / "id.bin").write_bytes(b"CSDRID01" + (12345).to_bytes(8, "little") + bytes(128))
    r = subprocess.run(base + ["-m", "-o", str(tmp_path / "mix2"), "--world", "1", "--rank", "0", "--id-file", str(tmp_path / "id.bin"), "--id-nonce", "777"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert not os.path.exists(tmp_path / "id.bin")
    a, b = np.fromfile(tmp_path / "mix0.f32", dtype=np.float32), np.fromfile(tmp_path / "mix1.f32", dtype=np.float32)
    assert a.size == n // M and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # a sharded --mix without its bootstrap is refused
    r = subprocess.run(base + ["-m", "--world", "2", "--rank", "0"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--id-file" in r.stderr


def test_sdr_process_offset_front_end(tmp_path):
    """--offset = mixDown/mixUp per source chunk in front of takeNArr (SoapySDR.hs:200-207)."""
    from composable_sdr_amd.app import sdr_process
    n, fs, off = 40000, 2.56e6, 100e3
    x = synth_cf32(n, 1, seed=9)
    src = tmp_path / "i.cf32"
    x.tofile(src)
    names = sdr_process(str(src), channels=1, demod="none", numsamples=n, outname=str(tmp_path / "o"), offset=off, samplerate=fs)
    got = np.fromfile(names[0], dtype=np.complex64)
    f = np.float32(2 * np.pi * off / fs)
    want = O.DcBlock().execute(O.Nco(f).mix_down(x))
    assert got.size == n and rel_rms(got, want) < 1e-5


# --------------------------------------------------------------------------- BASELINE.json full sizes: size-independent properties
def _torch_chain(M, nf, demod, **kw):
    import torch
    ch = cs.Chain(channels=M, demod=demod, max_frames=nf, **kw)
    return ch, torch


def test_full_size_cfg3_linearity_and_kernel_agreement(monkeypatch):
    """configs[2] size (256 ch, 262 144 frames = 67 M samples per chunk), device-resident:
    (1) the two fused kernels (dependency-free runs vs look-back tiles) agree on the whole chunk,
    (2) DeNo is linear: chain(x1 + 2 x2) = chain(x1) + 2 chain(x2),
    (3) a tone at a channel centre lands in that channel only (>= 75 dB), gain ~ M."""
    import torch
    from synth import channel_centre, synth_cf32_torch
    M, nf = 256, 262144
    dev = torch.device("cuda", 0)
    x1 = synth_cf32_torch(M * nf, M, dev, seed=1)
    x2 = synth_cf32_torch(M * nf, M, dev, seed=2)

    def run(x, demod, run_min):
        knob(monkeypatch, "CSDR_RUN_MIN_TILES", str(run_min))
        ch = cs.Chain(channels=M, demod=demod, max_frames=nf)
        out = torch.empty(M * nf * (1 if demod == "fm" else 2), dtype=torch.float32, device=dev)
        ch.process_device(x.data_ptr(), M * nf, out.data_ptr(), 0)
        torch.cuda.synchronize()
        ch.close()
        return out

    a = run(x1, "fm", 1)                    # k_run256
    b = run(x1, "fm", 10 ** 9)              # k_tile256
    d = torch.remainder(a - b + 0.5 / 0.3, 1 / 0.3) - 0.5 / 0.3
    dd = d.abs().view(M, nf)
    tone = torch.arange(M, device=dev) % 4 == 1
    print("full-size run-vs-tile FM: tone-channel max", float(dd[tone].max()), "median all", float(dd.median()))
    assert float(dd[tone].max()) < 5e-6 and float(dd.median()) < 5e-6
    del a, b, d, dd

    y1 = run(x1, "none", 1)
    y2 = run(x2, "none", 1)
    y12 = run(x1 + 2 * x2, "none", 1)
    err = (y12 - (y1 + 2 * y2)).abs().max()
    scale = y12.abs().max()
    print("full-size linearity: max err", float(err), "of", float(scale))
    assert float(err) < 2e-5 * float(scale)
    del y1, y2, y12

    k = 37
    n = torch.arange(M * nf, device=dev, dtype=torch.float64)
    ph = torch.remainder(channel_centre(k, M) * n, 2 * np.pi).to(torch.float32)
    tone_x = torch.stack([torch.cos(ph), torch.sin(ph)], dim=1).contiguous()
    del n, ph
    yt = run(tone_x, "none", 1).view(M, nf, 2)
    p = torch.sqrt((yt[:, 100:, :] ** 2).sum(-1)).mean(1)
    others = torch.cat([p[:k], p[k + 1:]])
    iso = 20 * torch.log10(p[k] / (others.max() + 1e-30))
    print("full-size tone: channel", int(p.argmax()), "isolation dB", float(iso), "gain/M", float(p[k]) / M)
    assert int(p.argmax()) == k and float(iso) > 75 and abs(float(p[k]) / M - 1) < 0.02


def test_run64_v2_matches_first_generation_kernel_and_oracle(monkeypatch):
    """k_run64v2 (CF32, whole band, nf % 64 == 0: DMA'd tiles, in-place passes, wave-local DFT) against k_run64
    (CSDR_RUN64_V1) and the oracle: an odd call first (first-generation kernel: odd NCO parity, non-trivial DC state and window),
    then 8192 frames (8 runs with warm-up and halo), a ragged call (first generation again), and 2048 more."""
    M = 64
    frames = [5, 8192, 70, 2048]
    knob(monkeypatch, "CSDR_RUN64_V2_ALL", "1")                  # (by default k_run64v2 takes calls of >= 3072 tiles only: below that k_run64 is faster)
    x = synth_cf32(M * sum(frames), M, seed=64)
    x = (x + np.complex64(0.05 - 0.02j)).astype(np.complex64)
    kw = dict(channels=M, demod="none", max_frames=max(frames))
    a = cs.Chain(**kw)
    knob(monkeypatch, "CSDR_RUN64_V1", "1")
    b = cs.Chain(**kw)
    monkeypatch.delenv("CSDR_RUN64_V1")
    orc = O.Chain(M, demod="none")
    ga, gb, wo, pos, names = [], [], [], 0, []
    for f in frames:
        xa = x[pos * M:(pos + f) * M]; pos += f
        ga.append(a.process(xa)); gb.append(b.process(xa)); wo.append(orc.process(xa))
        names.append((a.kernel_time()[0], b.kernel_time()[0]))
    print("kernels:", names)
    assert names[0][0] == "k_run64<CF32>" and names[1][0] == "k_run64v2" and names[2][0] == "k_run64<CF32>" and names[3][0] == "k_run64v2"
    assert all(n[1] == "k_run64<CF32>" for n in names)
    ga, gb, wo = [np.concatenate(v, axis=1) for v in (ga, gb, wo)]
    print(f"run64v2: vs v1 {rel_rms(ga, gb):.2e}, vs oracle {rel_rms(ga, wo):.2e}; last call vs oracle {rel_rms(ga[:, -2048:], wo[:, -2048:]):.2e}")
    assert rel_rms(ga, gb) < 2e-6 and rel_rms(ga, wo) < 1e-5
    assert rel_rms(ga[:, 5:5 + 64], wo[:, 5:5 + 64]) < 1e-5 and rel_rms(ga[:, -64:], wo[:, -64:]) < 1e-5
    a.close(); b.close()


def test_run64_v2_without_warm_up_windows_matches_the_warm_up_build(monkeypatch):
    """Round 5: k_run64v2's runs read no warm-up window either (as k_run256v2): a run starts its halo tile from DC state 0 and
    k_run64_dcfix adds what the true state contributes to the channels 30..33 over the run's first 448 frames.  Against the same library
    with the windows (CSDR_NOWU=0) on a strong DC offset, 16 + 14 runs in two calls (odd frame parity in the second through a 5-frame
    call between them), every channel and the corrected ones on their own; against the oracle behind an f64 DC blocker."""
    from scipy.signal import lfilter
    M = 64
    frames = [64 * 256, 5, 64 * 224]
    x = synth_cf32(M * sum(frames), M, seed=164, dc=0.3 - 0.2j)
    knob(monkeypatch, "CSDR_RUN64_V2_ALL", "1")
    a = cs.Chain(channels=M, demod="none", max_frames=max(frames))
    knob(monkeypatch, "CSDR_NOWU", "0")
    b = cs.Chain(channels=M, demod="none", max_frames=max(frames))
    monkeypatch.delenv("CSDR_NOWU")
    beta = float(np.float32(1) - np.float32(0.0005))
    yd = lfilter([1.0, -1.0], [1.0, -beta], x.astype(np.complex128)).astype(np.complex64)
    orc = O.Chain(M, demod="none", dc_block=False)
    pos, near = 0, slice(30, 34)
    for nf in frames:
        c = x[pos:pos + nf * M]
        ga, gb, w = a.process(c), b.process(c), orc.process(yd[pos:pos + nf * M])
        pos += nf * M
        kn = a.kernel_time()[0]
        e_all, e_near = rel_rms(ga, gb), rel_rms(ga[near], gb[near])
        print(f"M=64 no-warm-up vs warm-up nf={nf} [{kn}]: all {e_all:.2e}, channels 30..33 {e_near:.2e}; vs oracle (f64 dc) {rel_rms(ga, w):.2e} (warm-up build {rel_rms(gb, w):.2e})")
        assert kn == ("k_run64v2" if nf % 64 == 0 else "k_run64<CF32>")
        assert e_all < 2e-6 and e_near < 2e-5
        assert rel_rms(ga, w) < 1.2 * rel_rms(gb, w) + 1e-6 and max_abs_err(ga, w) < 1e-4 * np.abs(w).max()
    a.close(); b.close()


@pytest.mark.parametrize("demod,agc", [("fm", 0.0), ("none", 0.0), ("fm", 10.0)])
def test_run1024_v3_without_warm_up_windows_matches_the_warm_up_build(demod, agc, monkeypatch):
    """Round 5: k_run1024v3's runs start cold from DC state 0 as well (no read-only warm-up tiles); k_run1024_dcfix adds what the true state
    contributes to the channels 510..513 over a run's first 32 frames (FM: freqdem of the corrected side copies; CF32: in place, row-major
    or on the tile-major plane of the AGC route).  Against the same library with the windows (CSDR_NOWU=0) on a strong DC offset, 8 runs of
    128 / 32 tiles, a 5-frame call in between (other kernel, odd parity behind it); FM / DeNo also against the oracle behind an f64 blocker."""
    from scipy.signal import lfilter
    M, kf = 1024, 0.3
    frames = [4096, 5, 1024]
    x = synth_cf32(M * sum(frames), M, seed=1024, dc=0.3 - 0.2j)
    knob(monkeypatch, "CSDR_RUN1024_V3_RUNS", "8")
    kw = dict(channels=M, demod=demod, kf=kf, agc=agc, max_frames=max(frames))
    a = cs.Chain(**kw)
    knob(monkeypatch, "CSDR_NOWU", "0")
    b = cs.Chain(**kw)
    monkeypatch.delenv("CSDR_NOWU")
    beta = float(np.float32(1) - np.float32(0.0005))
    yd = lfilter([1.0, -1.0], [1.0, -beta], x.astype(np.complex128)).astype(np.complex64)
    orc = O.Chain(M, demod=demod, kf=kf, dc_block=False) if agc == 0.0 else None
    pos, near = 0, slice(510, 514)
    for nf in frames:
        c = x[pos:pos + nf * M]
        ga, gb = a.process(c), b.process(c)
        w = orc.process(yd[pos:pos + nf * M]) if orc else None
        pos += nf * M
        kn = a.kernel_time()[0]
        if nf % 4 == 0:
            assert kn.startswith("k_run1024v3"), kn
        if agc:
            assert np.array_equal(ga == 0, gb == 0)                         # the same squelch decisions
            d = np.abs(wrap_pm(ga.astype(np.float64) - gb, 1.0 / kf))
            print(f"M=1024 AGC+FM no-warm-up vs warm-up nf={nf} [{kn}]: median {np.median(d):.2e}, p99.9 {np.quantile(d, 0.999):.2e}, 510..513 median {np.median(d[near]):.2e}")
            assert np.median(d) < 2e-6 and np.quantile(d, 0.999) < 1e-3 and np.median(d[near]) < 2e-5
        elif demod == "none":
            e_all, e_near = rel_rms(ga, gb), rel_rms(ga[near], gb[near])
            print(f"M=1024 DeNo no-warm-up vs warm-up nf={nf} [{kn}]: all {e_all:.2e}, 510..513 {e_near:.2e}; vs oracle (f64 dc) {rel_rms(ga, w):.2e} (warm-up build {rel_rms(gb, w):.2e})")
            assert e_all < 2e-6 and e_near < 2e-5
            assert rel_rms(ga, w) < 1.2 * rel_rms(gb, w) + 1e-6
        else:
            d = np.abs(wrap_pm(ga.astype(np.float64) - gb, 1.0 / kf))
            dw = np.abs(wrap_pm(ga.astype(np.float64) - w, 1.0 / kf))
            tone = np.arange(M) % 4 == 1
            print(f"M=1024 FM no-warm-up vs warm-up nf={nf} [{kn}]: median {np.median(d):.2e}, tone max {d[tone].max():.2e}, 510..513 median {np.median(d[near]):.2e}; vs oracle tone max {dw[tone].max():.2e}")
            assert np.median(d) < 2e-6 and d[tone].max() < 1e-5 and np.median(d[near]) < 2e-5
            assert dw[tone].max() < 3e-5
    a.close(); b.close()


@pytest.mark.parametrize("M,demod,env,frames,extra", [
    (64, "none", "CSDR_RUN64_V1", [8192, 2048], {}),
    (64, "none", "CSDR_RUN64_V1", [8192], {"mix": True}),
    (1024, "fm", "CSDR_RUN1024_V1", [4096], {}),
    (1024, "fm", "CSDR_RUN1024_V1", [4096, 96], {"mix": True}),
    (256, "fm", "CSDR_RUN_MIN_TILES", [40000], {}),
])
def test_second_generation_run_kernels_without_dc_blocker(M, demod, env, frames, extra, monkeypatch):
    """dc_block = False (alpha = 0, beta = 0 inside the kernels) and DeNo --mix through k_run64v2 / k_run1024v3 / k_run256v2
    against the first-generation kernels: without the DC scan's approximated run-start state the CF32 results are bitwise
    those of k_run64 (same FIR order, same DFT butterflies)."""
    x = synth_cf32(M * sum(frames), M, seed=3)
    if M == 64:
        knob(monkeypatch, "CSDR_RUN64_V2_ALL", "1")              # (k_run64v2 for calls of every size)
    kw = dict(channels=M, demod=demod, kf=0.3, max_frames=max(frames), dc_block=False, **extra)
    a = cs.Chain(**kw)
    knob(monkeypatch, env, "1000000" if env == "CSDR_RUN_MIN_TILES" else "1")     # M = 256: the look-back tile kernel is the other implementation
    b = cs.Chain(**kw)
    monkeypatch.delenv(env)
    pos = 0
    for f in frames:
        xa = x[pos * M:(pos + f) * M]; pos += f
        ga, gb = a.process(xa), b.process(xa)
        ka, kb = a.kernel_time()[0], b.kernel_time()[0]
        assert ("v2" in ka or "v3" in ka) and "v2" not in kb and "v3" not in kb, (ka, kb)      # (M = 1024 FM: k_run1024v3)
        if demod == "fm":
            d = np.abs(ga.astype(np.float64) - gb); d = np.minimum(d, np.abs(d - 1 / 0.3))
            sc = np.sqrt(M) if extra.get("mix") else 1.0          # (--mix: a sample is the sum of M channels' differences)
            assert np.median(d) < 1e-6 * sc and np.quantile(d, 0.999) < 5e-5 * sc, (np.median(d), np.quantile(d, 0.999))
        else:
            assert rel_rms(ga, gb) < 1e-6
    a.close(); b.close()


def test_full_size_cfg2_64ch_chunk_invariance():
    """configs[1] size (64 ch, 1 048 576 frames): one chunk == 16 chunks (state carry), DeNo."""
    import torch
    from synth import synth_cf32_torch
    M, nf = 64, 1048576
    dev = torch.device("cuda", 0)
    x = synth_cf32_torch(M * nf, M, dev, seed=3)
    one = torch.empty(M * nf * 2, dtype=torch.float32, device=dev)
    ch = cs.Chain(channels=M, max_frames=nf)
    assert "k_run64" in ch.path
    ch.process_device(x.data_ptr(), M * nf, one.data_ptr(), 0)
    torch.cuda.synchronize()
    ch.close()
    parts = torch.empty(16, M, nf // 16, 2, dtype=torch.float32, device=dev)
    ch = cs.Chain(channels=M, max_frames=nf // 16)
    for i in range(16):
        ch.process_device(x.data_ptr() + i * (M * nf // 16) * 8, M * nf // 16, parts[i].data_ptr(), 0)
    torch.cuda.synchronize()
    ch.close()
    many = parts.permute(1, 0, 2, 3).reshape(M, nf, 2)
    err = (many - one.view(M, nf, 2)).abs().max()
    scale = one.abs().max()
    print("cfg2 full size one-vs-16 chunks: max err", float(err), "of", float(scale))
    assert float(err) < 1e-5 * float(scale)


# --------------------------------------------------------------------------- time-parallel AGC tail


def _bursty(M, nf, seed, kind):
    """channel-rich inputs that exercise the squelch state machine: tones switching on and off with gaps
    around the 1000-sample timeout, level steps, silence"""
    rng = np.random.default_rng(seed)
    n = M * nf
    t = np.arange(n)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.02
    if kind == "zeros":
        x[: n // 3] = 0
        x[2 * n // 3:] = 0
    from synth import channel_centre
    for k in range(1, M, 3):
        w = channel_centre(k, M)
        gate = np.ones(nf)
        if kind in ("bursts", "zeros"):
            # on/off pattern in frames (= per-channel samples): gaps of 200..1500
            pos, on = 0, bool(k & 1)
            while pos < nf:
                ln = int(rng.integers(200, 1500))
                gate[pos:pos + ln] = 1.0 if on else 0.0
                pos += ln; on = not on
        elif kind == "steps":
            pos = 0
            while pos < nf:
                ln = int(rng.integers(300, 2500))
                gate[pos:pos + ln] = 10.0 ** rng.uniform(-2.5, 0.0)
                pos += ln
        amp = np.repeat(gate, M) * (0.4 / np.sqrt(M / 3))
        x += amp * np.exp(1j * (w * t + 0.3 * np.sin(2 * np.pi * t / (M * 50.0))))
    return x.astype(np.complex64)


@pytest.mark.parametrize("M,demod,mix", [(256, "fm", False), (256, "none", False), (64, "fm", False), (20, "none", False),
                                         (16, "fm", True), (1, "fm", False)])
@pytest.mark.parametrize("kind", ["bursts", "steps", "zeros"])
def test_agc_tail_is_bit_identical_to_sequential(M, demod, mix, kind, monkeypatch):
    """the segmented, verified AGC tail must reproduce the one-lane-per-channel kernels bit for bit, for any
    signal (speculation only decides how much is recomputed), across calls and ragged chunk lengths"""
    from composable_sdr_amd import _lib
    knob(monkeypatch, "CSDR_AGC_L", "256")          # many segments even at test sizes
    knob(monkeypatch, "CSDR_AGC_W", "512")
    frames = [4096, 1000, 2056 + 3, 16, 7, 3000] if M > 1 else [40000, 1000, 20563, 16, 7]
    nf = sum(frames)
    x = _bursty(M, nf, 1234 + M, kind)
    kw = dict(channels=M, demod=demod, kf=0.3, agc=8.0, mix=mix, max_frames=max(frames))
    a = cs.Chain(flags=_lib.FLAG_QUIET, **kw)
    b = cs.Chain(flags=_lib.FLAG_QUIET | _lib.FLAG_AGC_SEQUENTIAL, **kw)
    assert "agc-spec" in a.path and "agc-spec" not in b.path
    pos = 0
    for f in frames:
        xa = x[pos * M:(pos + f) * M]
        ya, yb = a.process(xa), b.process(xa)
        assert ya.shape == yb.shape
        assert np.array_equal(ya.view(np.uint32), yb.view(np.uint32)), (M, demod, kind, f, pos)
        pos += f
    checked, redone = a.agc_stats()
    opened = float(np.mean(yb != 0))
    print(f"agc tail M={M} {demod} {kind}: segments checked {checked}, recomputed {redone}; last chunk non-zero {opened:.2f}")
    assert checked > 0
    a.close(); b.close()


@pytest.mark.parametrize("M,demod", [(64, "fm"), (16, "none")])
def test_agc_tail_default_segment_rule_bit_identical(M, demod):
    """the same with the segment length the plan picks on its own (no CSDR_AGC_L / _W): several 64-segment groups
    per channel, the last one partly filled, ragged and odd chunk lengths"""
    from composable_sdr_amd import _lib
    frames = [30000, 28111, 4096, 27001]
    nf = sum(frames)
    x = _bursty(M, nf, 99 + M, "bursts")
    kw = dict(channels=M, demod=demod, kf=0.3, agc=8.0, max_frames=max(frames))
    a = cs.Chain(flags=_lib.FLAG_QUIET, **kw)
    b = cs.Chain(flags=_lib.FLAG_QUIET | _lib.FLAG_AGC_SEQUENTIAL, **kw)
    pos = 0
    for f in frames:
        xa = x[pos * M:(pos + f) * M]
        ya, yb = a.process(xa), b.process(xa)
        assert np.array_equal(ya.view(np.uint32), yb.view(np.uint32)), (M, demod, f, pos)
        pos += f
    checked, redone = a.agc_stats()
    print(f"agc tail default rule M={M} {demod}: segments checked {checked}, recomputed {redone}")
    assert checked > 4 * M
    a.close(); b.close()


def _bursty_torch(M, nf, seed, dev):
    """_bursty's "bursts" signal at run-kernel sizes, generated on the GPU: noise + every third channel keyed on and off with gaps
    of 200 .. 1500 channel samples (around the 1000-sample squelch timeout)"""
    import torch
    from synth import channel_centre
    g = torch.Generator(device=dev); g.manual_seed(seed)
    n = M * nf
    x = torch.randn(n, 2, generator=g, device=dev, dtype=torch.float32) * 0.02
    t = torch.arange(n, device=dev, dtype=torch.float64)
    rng = np.random.default_rng(seed)
    for k in range(1, M, 3):
        gate = np.ones(nf, dtype=np.float32)
        pos, on = 0, bool(k & 1)
        while pos < nf:
            ln = int(rng.integers(200, 1500))
            gate[pos:pos + ln] = 1.0 if on else 0.0
            pos += ln; on = not on
        amp = torch.from_numpy(gate).to(dev).repeat_interleave(M) * (0.4 / np.sqrt(M / 3))
        ph = channel_centre(k, M) * t + 0.3 * torch.sin(2 * np.pi * t / (M * 50.0))
        x[:, 0] += (amp * torch.cos(ph)).float(); x[:, 1] += (amp * torch.sin(ph)).float()
    return x.reshape(-1)


@pytest.mark.parametrize("demod,G", [("fm", 1), ("none", 1), ("fm", 8), ("fm", 2)])
def test_agc_tail_tile_major_route_is_bit_identical_to_sequential(demod, G, monkeypatch):
    """k_agc_spec_tm (round 4: the fused 256-channel chains write the CF32 plane tile-major, a workgroup's 64 streams are 64 channels
    at one segment, contiguous 8 KiB per block by LDS-DMA, packed freqdem) against the one-lane-per-channel kernels, BIT FOR BIT, on
    a keyed signal that makes segment boundaries fail (short warm-up, short segments), over run-sized calls with the state carried;
    whole band and interleaved shards (C = 32: two segments per workgroup; C = 128)."""
    import torch
    from composable_sdr_amd import _lib
    M, kf = 256, 0.3
    knob(monkeypatch, "CSDR_AGC_W", "512")
    knob(monkeypatch, "CSDR_AGC_L_TM", "688")
    frames = [36864, 40000, 33, 32768 + 48]
    dev = torch.device("cuda", 0)
    xd = _bursty_torch(M, sum(frames), 4321 + G, dev)
    kw = dict(channels=M, demod=demod, kf=kf, agc=8.0, max_frames=max(frames))
    if G > 1:
        kw.update(chan_first=G - 1, chan_stride=G)
    a = cs.Chain(flags=_lib.FLAG_QUIET, **kw)
    b = cs.Chain(flags=_lib.FLAG_QUIET | _lib.FLAG_AGC_SEQUENTIAL, **kw)
    C, w = M // G, (1 if demod == "fm" else 2)
    pos = 0
    for f in frames:
        oa = torch.zeros(C * f * w, dtype=torch.float32, device=dev); ob = torch.zeros_like(oa)
        ptr = xd.data_ptr() + pos * M * 8
        a.process_device(ptr, M * f, oa.data_ptr(), 0)
        b.process_device(ptr, M * f, ob.data_ptr(), 0)
        torch.cuda.synchronize()
        assert torch.equal(oa.view(torch.int32), ob.view(torch.int32)), (demod, G, f, pos)
        opened = float((ob != 0).float().mean())
        assert 0.02 < opened < 0.98 or f < 100, opened
        pos += f
    checked, redone = a.agc_stats()
    tmc = a.agc_tile_major_calls()
    print(f"tile-major AGC tail {demod} G={G}: {tmc} of {len(frames)} calls on k_agc_spec_tm; segments checked {checked}, recomputed {redone}")
    assert tmc == 3                                      # the 33-frame call is not whole tiles: row-major route
    assert redone > 0                                    # the keyed signal does make speculation fail: the repair path ran
    a.status(); b.status()
    a.close(); b.close()


@pytest.mark.parametrize("demod", ["fm", "none"])
def test_agc_tail_tile_major_route_at_1024_channels_is_bit_identical_to_sequential(demod, monkeypatch):
    """The same at M = 1024: k_run1024v3<CF32> writes the plane tile-major (the 128-byte lines of a 16-frame block back to back) for
    k_agc_spec_tm; against the one-lane-per-channel kernels behind the row-major plane, BIT FOR BIT, keyed signal, state carried over
    run-sized, ragged and short calls."""
    import torch
    from composable_sdr_amd import _lib
    M, kf = 1024, 0.3
    knob(monkeypatch, "CSDR_AGC_W", "512")
    knob(monkeypatch, "CSDR_AGC_L_TM", "688")
    frames = [8192, 8192 + 16, 33, 4096 + 32]
    dev = torch.device("cuda", 0)
    xd = _bursty_torch(M, sum(frames), 977, dev)
    kw = dict(channels=M, demod=demod, kf=kf, agc=8.0, max_frames=max(frames))
    a = cs.Chain(flags=_lib.FLAG_QUIET, **kw)
    b = cs.Chain(flags=_lib.FLAG_QUIET | _lib.FLAG_AGC_SEQUENTIAL, **kw)
    w = 1 if demod == "fm" else 2
    pos, names = 0, []
    for f in frames:
        oa = torch.zeros(M * f * w, dtype=torch.float32, device=dev); ob = torch.zeros_like(oa)
        ptr = xd.data_ptr() + pos * M * 8
        a.process_device(ptr, M * f, oa.data_ptr(), 0)
        b.process_device(ptr, M * f, ob.data_ptr(), 0)
        torch.cuda.synchronize()
        names.append(a.kernel_time()[0])
        assert torch.equal(oa.view(torch.int32), ob.view(torch.int32)), (demod, f, pos)
        opened = float((ob != 0).float().mean())
        assert 0.02 < opened < 0.98 or f < 100, opened
        pos += f
    checked, redone = a.agc_stats()
    tmc = a.agc_tile_major_calls()
    print(f"tile-major AGC tail at 1024 channels, {demod}: {tmc} of {len(frames)} calls on k_agc_spec_tm ({names}); segments checked {checked}, recomputed {redone}")
    assert tmc == 3 and redone > 0
    a.status(); b.status()
    a.close(); b.close()


@pytest.mark.parametrize("demod", ["fm", "none"])
def test_agc_tail_tile_major_route_at_64_channels_is_bit_identical_to_sequential(demod, monkeypatch):
    """The same at M = 64 (round 6): k_run64v2 writes the plane tile-major -- a 16-lane row of its stores is one 128-byte line either
    way -- for k_agc_spec_tm (64 channels = exactly one wave per time position); against the one-lane-per-channel kernels behind the
    row-major plane, BIT FOR BIT, keyed signal, state carried over run-sized, ragged and short calls, with and without the cold-start
    correction of the four channels around DC (k_run64_dcfix on the tile-major plane)."""
    import torch
    from composable_sdr_amd import _lib
    M, kf = 64, 0.3
    knob(monkeypatch, "CSDR_AGC_W", "512")
    knob(monkeypatch, "CSDR_AGC_L_TM", "688")
    knob(monkeypatch, "CSDR_RUN64_V2_ALL", "1")          # k_run64v2 below its size threshold (3072 tiles), so that the test stays small
    frames = [16384, 16384 + 64, 33, 8192 + 128]
    dev = torch.device("cuda", 0)
    xd = _bursty_torch(M, sum(frames), 978, dev)
    kw = dict(channels=M, demod=demod, kf=kf, agc=8.0, max_frames=max(frames))
    a = cs.Chain(flags=_lib.FLAG_QUIET, **kw)
    b = cs.Chain(flags=_lib.FLAG_QUIET | _lib.FLAG_AGC_SEQUENTIAL, **kw)
    w = 1 if demod == "fm" else 2
    pos, names = 0, []
    for f in frames:
        oa = torch.zeros(M * f * w, dtype=torch.float32, device=dev); ob = torch.zeros_like(oa)
        ptr = xd.data_ptr() + pos * M * 8
        a.process_device(ptr, M * f, oa.data_ptr(), 0)
        b.process_device(ptr, M * f, ob.data_ptr(), 0)
        torch.cuda.synchronize()
        names.append(a.kernel_time()[0])
        assert torch.equal(oa.view(torch.int32), ob.view(torch.int32)), (demod, f, pos)
        opened = float((ob != 0).float().mean())
        assert 0.02 < opened < 0.98 or f < 100, opened
        pos += f
    checked, redone = a.agc_stats()
    tmc = a.agc_tile_major_calls()
    print(f"tile-major AGC tail at 64 channels, {demod}: {tmc} of {len(frames)} calls on k_agc_spec_tm ({names}); segments checked {checked}, recomputed {redone}")
    assert tmc == 3 and names[0] == names[1] == names[3] == "k_run64v2"
    a.status(); b.status()
    a.close(); b.close()


def test_agc_tile_major_knob_is_the_handles_own(monkeypatch):
    """CSDR_AGC_TM=0 is read when a handle is created, with the tail's other knobs: a handle made while it is set keeps the row-major
    route, a handle made after it is removed takes k_agc_spec_tm, whichever of them asked first -- and both routes give the same bits.
    64 channels, DeNo, one call of TM_MIN = 2048 frames, the shortest the tile-major route takes under TM_KNOBS.  max_frames is 4096,
    not the call's 2048: a handle has the guards a tile-major plane needs only from max_frames = 4096 on (AgcTail::setup), so a
    2048-frame handle takes the row-major route whatever the knob says."""
    import torch
    from chain_tail_cases import TM_KNOBS, TM_MIN
    from composable_sdr_amd import _lib
    M, nf = 64, TM_MIN
    for k, v in TM_KNOBS.items():
        knob(monkeypatch, k, v)
    dev = torch.device("cuda", 0)
    xd = _bursty_torch(M, nf, 980, dev)
    kw = dict(channels=M, demod="none", agc=8.0, max_frames=4096, flags=_lib.FLAG_QUIET)
    knob(monkeypatch, "CSDR_AGC_TM", "0")
    a = cs.Chain(**kw)
    monkeypatch.delenv("CSDR_AGC_TM")
    b = cs.Chain(**kw)
    oa = torch.zeros(M * nf * 2, dtype=torch.float32, device=dev); ob = torch.zeros_like(oa)
    a.process_device(xd.data_ptr(), M * nf, oa.data_ptr(), 0)
    b.process_device(xd.data_ptr(), M * nf, ob.data_ptr(), 0)
    torch.cuda.synchronize()
    print(f"CSDR_AGC_TM=0 at create: {a.agc_tile_major_calls()} tile-major calls [{a.path}]; removed: {b.agc_tile_major_calls()} [{b.path}]")
    assert a.agc_tile_major_calls() == 0 and b.agc_tile_major_calls() == 1
    assert torch.equal(oa.view(torch.int32), ob.view(torch.int32)) and bool((oa != 0).any())
    a.status(); b.status()
    a.close(); b.close()


def test_agc_tail_tile_major_route_at_4096_channels_is_bit_identical_to_sequential(monkeypatch):
    """The same at M = 4096 (round 6): k_back4096<CF32> stores its 16-frame blocks' lines back to back for k_agc_spec_tm (64 channel groups
    of 64); FM output against the one-lane-per-channel kernels behind the row-major plane, BIT FOR BIT, over a tile-major, a second
    tile-major and a short row-major call with the state carried."""
    import torch
    from composable_sdr_amd import _lib
    M, kf = 4096, 0.3
    knob(monkeypatch, "CSDR_AGC_W", "512")
    knob(monkeypatch, "CSDR_AGC_L_TM", "688")
    frames = [4096, 2048 + 16, 33]
    dev = torch.device("cuda", 0)
    xd = _bursty_torch(M, sum(frames), 979, dev)
    kw = dict(channels=M, demod="fm", kf=kf, agc=8.0, max_frames=max(frames))
    a = cs.Chain(flags=_lib.FLAG_QUIET, **kw)
    b = cs.Chain(flags=_lib.FLAG_QUIET | _lib.FLAG_AGC_SEQUENTIAL, **kw)
    assert "fused-4096" in a.path
    pos = 0
    for f in frames:
        oa = torch.zeros(M * f, dtype=torch.float32, device=dev); ob = torch.zeros_like(oa)
        ptr = xd.data_ptr() + pos * M * 8
        a.process_device(ptr, M * f, oa.data_ptr(), 0)
        b.process_device(ptr, M * f, ob.data_ptr(), 0)
        torch.cuda.synchronize()
        assert torch.equal(oa.view(torch.int32), ob.view(torch.int32)), (f, pos)
        pos += f
    tmc = a.agc_tile_major_calls()
    print(f"tile-major AGC tail at 4096 channels: {tmc} of {len(frames)} calls on k_agc_spec_tm; segments {a.agc_stats()}")
    assert tmc == 2
    a.status(); b.status()
    a.close(); b.close()


def test_agc_tail_steady_state_needs_no_recompute():
    """on a stationary signal (the bench's) the speculation always verifies after the first call"""
    from composable_sdr_amd import _lib
    M, nf = 256, 16384
    x = synth_cf32(M * nf * 3, M, seed=77)
    a = cs.Chain(channels=M, demod="fm", kf=0.3, agc=10.0, max_frames=nf, flags=_lib.FLAG_QUIET)
    a.process(x[:M * nf])
    c0, r0 = a.agc_stats()
    a.process(x[M * nf:2 * M * nf]); a.process(x[2 * M * nf:])
    c1, r1 = a.agc_stats()
    print(f"agc tail steady state: first call {r0}/{c0} recomputed, next two {r1 - r0}/{c1 - c0}")
    assert c1 > c0 and (r1 - r0) <= (c1 - c0) // 100
    # the first call of a stream pilots the create-time transient (k_agc_pilot): its speculation verifies like any other call's
    assert r0 <= c0 // 50, (r0, c0)
    a.close()


def test_agc_tail_full_size_bit_identical_and_oracle_prefix():
    """The benchmarked AGC shape: 256 ch x 262 144 frames, -a 10, the segment length / warm-up the plan picks itself
    (L = 1040, W = 1024).  (1) the time-parallel tail equals the one-lane-per-channel kernels bit for bit over the whole
    chunk and a second one (state carry); (2) the first 8192 frames agree with the oracle, squelch decisions exactly
    (the threshold is >= 8 dB away from every channel level)."""
    import torch
    from composable_sdr_amd import _lib
    from synth import synth_cf32_torch
    M, nf, kf = 256, 262144, 0.3
    dev = torch.device("cuda", 0)
    xs = [synth_cf32_torch(M * nf, M, dev, seed=11 + i) for i in range(2)]
    kw = dict(channels=M, demod="fm", kf=kf, agc=10.0, max_frames=nf)
    a = cs.Chain(flags=_lib.FLAG_QUIET, **kw)
    b = cs.Chain(flags=_lib.FLAG_QUIET | _lib.FLAG_AGC_SEQUENTIAL, **kw)
    assert "agc-spec" in a.path and "agc-spec" not in b.path
    oa = torch.empty(M * nf, dtype=torch.float32, device=dev)
    ob = torch.empty_like(oa)
    first = None
    for i, x in enumerate(xs):
        a.process_device(x.data_ptr(), M * nf, oa.data_ptr(), 0)
        b.process_device(x.data_ptr(), M * nf, ob.data_ptr(), 0)
        torch.cuda.synchronize()
        same = bool(torch.equal(oa.view(torch.int32), ob.view(torch.int32)))
        print(f"full-size AGC tail, chunk {i}: bit-identical {same}, open fraction {float((ob != 0).float().mean()):.3f}")
        assert same
        if i == 0:
            first = oa.view(M, nf)[:, :8192].cpu().numpy()
    checked, redone = a.agc_stats()
    print(f"full-size AGC tail: segments checked {checked}, recomputed {redone}")
    assert checked >= 2 * 256 * 150                     # (tile-major route: ~168 segments per channel and chunk)
    a.close(); b.close()
    x0 = xs[0][: M * 8192].cpu().numpy().view(np.complex64).reshape(-1)
    want = O.Chain(M, demod="fm", kf=kf, agc_db=10.0).process(x0)
    mism = int(np.sum((first == 0) != (want == 0)))
    d = np.abs(wrap_pm(first.astype(np.float64) - want, 1.0 / kf))
    op = want != 0
    print(f"full-size AGC prefix vs oracle: squelch mismatches {mism}, open {op.mean():.3f}, median {np.median(d[op]):.3e}, p99.9 {np.quantile(d, 0.999):.3e}")
    assert mism == 0
    assert np.median(d[op]) < 2e-5 and np.quantile(d, 0.999) < 5e-4


def test_fused256_run_kernel_strong_dc_warm_up(monkeypatch):
    """|DC| = 0.36 through the RUN kernel (CSDR_RUN_MIN_TILES = 1, 128 tiles = 16 runs): every run but the first gets
    its DC-blocker state from the read-only warm-up over the 6 tiles in front of its halo tile (beta^24576 = 4.6e-6 of
    |v| ~ 720 is left out).  Against the oracle behind an f64 DC blocker, and against the look-back tile kernel."""
    from scipy.signal import lfilter
    M, nf = 256, 16 * 128
    x = synth_cf32(M * nf, M, seed=8, dc=0.3 + 0.2j)
    from composable_sdr_amd import _lib
    fl = _lib.FLAG_QUIET | _lib.FLAG_TIME_KERNELS
    knob(monkeypatch, "CSDR_RUN_MIN_TILES", "1")
    run = cs.Chain(channels=M, max_frames=nf, flags=fl)
    knob(monkeypatch, "CSDR_RUN_MIN_TILES", "1000000")
    tile = cs.Chain(channels=M, max_frames=nf, flags=fl)
    a, t = run.process(x), tile.process(x)
    krun, ktile = run.kernel_time()[0], tile.kernel_time()[0]
    assert "k_run256" in krun and "k_tile256" in ktile
    beta = float(np.float32(1) - np.float32(0.0005))
    yd = lfilter([1.0, -1.0], [1.0, -beta], x.astype(np.complex128)).astype(np.complex64)
    want64 = O.Chain(M, dc_block=False).process(yd)
    want32 = O.Chain(M).process(x)
    # the left-out tail of the state is a slowly decaying offset: it lands in the two channels next to DC only
    e = np.abs(a.astype(np.complex128) - want64)
    print(f"strong-DC run kernel [{krun}]: vs tile kernel {rel_rms(a, t):.3e}; vs f64-DC oracle {rel_rms(a, want64):.3e} "
          f"(oracle f32 vs f64: {rel_rms(want32, want64):.3e}); worst channel {int(e.max(axis=1).argmax())} max abs err {e.max():.3e} of {np.abs(want64).max():.1f}")
    assert rel_rms(a, t) < 2e-6
    assert rel_rms(a, want64) < 2e-6
    assert rel_rms(a, want64) < rel_rms(want32, want64)      # closer to exact arithmetic than the f32 reference recurrence
    assert e.max() < 2e-4 * np.abs(want64).max()
    run.close(); tile.close()


# --------------------------------------------------------------------------- AM demodulator (a15)


def _am_signal(n, seed=5):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    env = 1.0 + 0.6 * np.sin(2 * np.pi * t / 97.0) + 0.2 * np.sin(2 * np.pi * t / 23.0)
    x = 0.4 * env * np.exp(1j * (0.21 * t + 0.5)) + 0.01 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return x.astype(np.complex64)


def test_ampdem_pipe_matches_oracle_across_chunks():
    """amDemodulator Pipe (ampmodem DSB peak detector as recalled -- unpinned): chunked stream against the oracle.
    Tolerance: the smoother runs as a blocked scan, so q_hat differs from the sequential f32 recurrence by
    rounding only: abs <= 2e-6 on outputs of magnitude ~1."""
    x = _am_signal(30000)
    want = O.AmpDem().demodulate_block(x)
    sizes = [1, 15, 2048, 2049, 4096, 5000, 16791]
    assert sum(sizes) == x.size
    chunks, pos = [], 0
    for s in sizes:
        chunks.append(x[pos:pos + s]); pos += s
    got = np.concatenate(_run_pipe(cs.amDemodulator(max_samples=20000), chunks))
    err = max_abs_err(got, want)
    print(f"ampdem pipe: max abs err {err:.3e} (max |want| {np.abs(want).max():.3f})")
    assert err < 2e-6
    # the modulation comes back (after the smoother has settled)
    assert np.corrcoef(got[5000:], np.sin(2 * np.pi * np.arange(5000, x.size) / 97.0))[0, 1] > 0.9


@pytest.mark.parametrize("M,agc,mix", [(8, 0.0, False), (256, 0.0, False), (64, 8.0, False), (16, 0.0, True), (1, 0.0, False)])
def test_chain_am_matches_oracle(M, agc, mix):
    frames = [3000, 1096, 2048 + 5] if M > 1 else [30000, 10960, 20485]
    nf = sum(frames)
    x = synth_cf32(M * nf, M, seed=4242)
    ch = cs.Chain(channels=M, demod="am", agc=agc, mix=mix, max_frames=max(frames))
    orc = O.Chain(M, demod="am", agc_db=agc, mix=mix)
    got, want, pos = [], [], 0
    for f in frames:
        xa = x[pos * M:(pos + f) * M]
        got.append(ch.process(xa)); want.append(orc.process(xa)); pos += f
    got, want = np.concatenate(got, axis=-1), np.concatenate(want, axis=-1)
    scale = np.abs(want).max()
    err = max_abs_err(got, want)
    print(f"chain AM M={M} agc={agc} mix={mix} [{ch.path}]: max abs err {err:.3e} of {scale:.3f}")
    assert got.shape == want.shape and got.dtype == np.float32
    if agc:
        # the AGC's gain trajectory differs by ~1e-5 relative between the two f32 implementations (see the AGC tests)
        # (a muted sample demodulates to 2 (0 - q_hat) != 0, so zeros of the AM output are NOT the squelch decisions;
        # those are compared exactly on the CF32 output of the same chain below)
        thr, margin = _clear_threshold(M, x)
        assert abs(thr - agc) < margin - 3.0              # -a 8 lies >= 3 dB from every channel level of this fixture
        assert np.quantile(np.abs(got - want), 0.999) < 2e-3 * scale
        cd = cs.Chain(channels=M, demod="none", agc=agc, max_frames=nf)
        zd, zo = cd.process(x), O.Chain(M, demod="none", agc_db=agc).process(x)
        cd.close()
        mism = int(np.sum((zd == 0) != (zo == 0)))
        print(f"same fixture, DeNo + AGC: squelch mismatches {mism}, open {float(np.mean(zo != 0)):.3f}")
        assert mism == 0
    else:
        # the peak detector doubles the chain's CF32 error (tolerance 1e-4 max|ref|, dominated by the reference's own
        # f32 DC-blocker noise, see test_chain_deno_matches_oracle); the detector itself agrees to 2e-6 (pipe test)
        assert err < 2e-4 * max(scale, 1.0) * (np.sqrt(M) if mix else 1.0)
    ch.close()


# --------------------------------------------------------------------------- resampler (a14)


@pytest.mark.parametrize("rate", [0.078125, 0.3, 0.625, 1.0, 1.7])
def test_resampler_pipe_matches_oracle_across_chunks(rate, monkeypatch):
    """resampler r 60 (Liquid.chs:115-117; msresamp structure, parameters fixed by this repo -- unpinned): the
    chunked GPU stream equals the restatement sample for sample in count and to f32 rounding in value (the
    Q32.32 output timing is integer arithmetic on both sides)."""
    monkeypatch.setenv("CSDR_QUIET", "1")
    rng = np.random.default_rng(11)
    n = 200000
    t = np.arange(n)
    x = (0.5 * np.exp(2j * np.pi * 0.11 * rate * t) + 0.2 * np.exp(-2j * np.pi * 0.31 * rate * t)
         + 0.05 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    want = O.MsResamp(rate).execute(x)
    sizes = [1, 2, 1024, 1023, 4096, 50001, 65536]
    sizes.append(n - sum(sizes))
    chunks, pos = [], 0
    for s in sizes:
        chunks.append(x[pos:pos + s]); pos += s
    parts = _run_pipe(cs.resampler(rate, 60.0, max_samples=max(sizes)), chunks)
    got = np.concatenate(parts)
    assert got.size == want.size, (got.size, want.size)
    assert abs(got.size - rate * n) <= 2
    err = max_abs_err(got, want)
    print(f"resampler r={rate}: {got.size} samples out, max abs err {err:.3e}")
    assert err < 2e-6
    # every chunk's count stays inside the buffer the reference allocates: 2*ceil(r*nx) (Liquid.chs:81)
    for s, p in zip(sizes, parts):
        assert p.size <= 2 * int(np.ceil(rate * s))


def test_resampler_rate_zero_is_identity_and_bad_rates_are_rejected(monkeypatch):
    monkeypatch.setenv("CSDR_QUIET", "1")
    x = (np.arange(100) + 1j).astype(np.complex64)
    (y,) = _run_pipe(cs.resampler(0.0), [x])
    assert np.array_equal(x, y)
    with pytest.raises(cs.CsdrError):
        _run_pipe(cs.resampler(2.5), [x])


def test_sdr_process_config1_shape(tmp_path, monkeypatch):
    """BASELINE configs[0]: -s 2.56e6 -b 200e3 -c 1 --demod FM -n 2e6: resampler (r = 0.078125) -> takeNArr -> dcBlocker
    -> freqdem, one .f32 of exactly n samples; equals the oracle replay of the same composition."""
    monkeypatch.setenv("CSDR_QUIET", "1")
    from composable_sdr_amd.app import sdr_process
    n_in, n_out = 700000, 50000
    x = synth_cf32(n_in, 1, seed=99)
    src = tmp_path / "in.cf32"
    x.tofile(src)
    (name,) = sdr_process(str(src), channels=1, demod="fm", kf=0.3, numsamples=n_out, outname=str(tmp_path / "o"),
                          chunksize=1024, samplerate=2.56e6, bandwidth=200e3)
    got = np.fromfile(name, dtype=np.float32)
    assert got.size == n_out
    rs = O.MsResamp(np.float32(200e3 / 2.56e6))
    y = np.concatenate([rs.execute(x[i:i + 1024]) for i in range(0, n_in, 1024)])[:n_out]
    want = O.Chain(1, demod="fm", kf=0.3).process(y)
    d = wrap_pm(got.astype(np.float64) - want.ravel(), 1.0 / 0.3)
    print(f"config-1 shape: {got.size} samples, p99.9 |d| {np.quantile(np.abs(d), 0.999):.3e}")
    assert np.quantile(np.abs(d), 0.999) < 2e-4


def test_cpp_soapy_sdr_file_front_end_matches_python_replay(tmp_path, monkeypatch):
    """-s / -b / --offset of the C++ CLI (resampler . offset in front of takeNArr) and DeAM: identical bytes to
    the Python replay of the same composition."""
    import os
    import subprocess
    monkeypatch.setenv("CSDR_QUIET", "1")
    from composable_sdr_amd.app import sdr_process
    exe = host_exe("soapy_sdr_file")
    x = synth_cf32(400000, 1, seed=8)
    src = tmp_path / "in.cf32"
    x.tofile(src)
    for demod, cli in (("fm", ["DeNBFM", "0.3"]), ("am", ["DeAM"])):
        py = sdr_process(str(src), channels=1, demod=demod, kf=0.3, numsamples=20000, outname=str(tmp_path / f"py_{demod}"),
                         chunksize=1024, samplerate=2.56e6, bandwidth=200e3, offset=-30e3)
        r = subprocess.run([exe, "--filename", str(src), "-n", "20000", "-c", "1", "--demod", *cli, "-s", "2.56e6", "-b", "200e3",
                            "--offset", "-30e3", "-o", str(tmp_path / f"cc_{demod}")], capture_output=True, text=True, timeout=120,
                           env=dict(os.environ, CSDR_QUIET="1"))
        assert r.returncode == 0, r.stderr
        a = np.fromfile(py[0], dtype=np.float32)
        b = np.fromfile(tmp_path / f"cc_{demod}.f32", dtype=np.float32)
        assert a.size == 20000 and np.array_equal(a, b), demod


# --------------------------------------------------------------------------- WBFM audio tail (f3)


def test_iirfilter_and_firdecimator_pipes_match_oracle():
    """iirFilter 2 fc 0 10 10 and firDecimator m (Liquid.chs:629-638, 485-501; arithmetic recalled, unpinned) as
    chunked Pipes against the restatement.  The biquad runs as a blocked scan: f32 rounding-order differences only."""
    rng = np.random.default_rng(21)
    n = 40000
    x = (np.sin(2 * np.pi * 0.01 * np.arange(n)) + 0.3 * rng.standard_normal(n)).astype(np.float32)
    sizes = [4, 1000, 4096, 4100, 8192, 22608]
    assert sum(sizes) == n
    chunks, pos = [], 0
    for s in sizes:
        chunks.append(x[pos:pos + s]); pos += s
    for fc in (0.025, 0.0021):                      # 5 kHz at 200 kS/s and at 2.4 MS/s
        orc = O.Butter2(fc)
        want = orc.execute_block(x)
        got = np.concatenate(_run_pipe(cs.iirFilter(2, fc, max_samples=30000), chunks))
        # a narrow low-pass in direct form II keeps a large internal state, so the sequential f32 loop is itself
        # noisy: both are measured against the same coefficients run in f64
        from scipy.signal import lfilter
        b, a = orc.coeffs
        truth = lfilter(b.astype(np.float64), a.astype(np.float64), x.astype(np.float64))
        e_gpu, e_orc = np.abs(got - truth).max(), np.abs(want - truth).max()
        print(f"iirFilter fc={fc}: |gpu - f64| {e_gpu:.3e}, |oracle - f64| {e_orc:.3e}, |gpu - oracle| {max_abs_err(got, want):.3e}")
        assert e_gpu < 2 * e_orc + 2e-6
    want = O.FirDecim(4).execute_block(x)
    got = np.concatenate(_run_pipe(cs.firDecimator(4, max_samples=30000), chunks))
    err = max_abs_err(got, want)
    print(f"firDecimator 4: {got.size} out, max abs err {err:.3e} of {np.abs(want).max():.3f}")
    assert got.size == n // 4 and err < 5e-6
    with pytest.raises(cs.CsdrError):
        _run_pipe(cs.firDecimator(4), [x[:1001]])
    with pytest.raises(cs.CsdrError):
        _run_pipe(cs.iirFilter(4, 0.1), [x[:16]])


@pytest.mark.parametrize("M,agc,mix", [(1, 0.0, False), (8, 0.0, False), (256, 0.0, False), (64, 8.0, False), (16, 0.0, True)])
def test_chain_wbfm_matches_oracle(M, agc, mix):
    """DeWBFM 4 = firDecimator 4 . iirDeemph . fmDemodulator 0.6 . agc per channel (SoapySDR.hs:252-259)."""
    frames = [4096, 1024, 2048] if M > 1 else [40000, 10960, 20480]
    nf = sum(frames)
    x = synth_cf32(M * nf, M, seed=777)
    fc = 5000.0 / 200e3
    ch = cs.Chain(channels=M, demod="wbfm", decim=4, deemph_fc=fc, agc=agc, mix=mix, max_frames=max(frames))
    orc = O.Chain(M, demod="wbfm", decim=4, deemph_fc=fc, agc_db=agc, mix=mix)
    got, want, pos = [], [], 0
    for f in frames:
        xa = x[pos * M:(pos + f) * M]
        got.append(ch.process(xa)); want.append(orc.process(xa)); pos += f
    got, want = np.concatenate(got, axis=-1), np.concatenate(want, axis=-1)
    assert got.shape == want.shape == ((nf // 4,) if (mix and M > 1) else (M, nf // 4))
    # freqdem outputs are compared modulo 1/kf before the linear tail in the FM tests; after a low-pass and a
    # decimator a branch-cut flip is smeared over ~80 output samples, so compare robustly: the bulk must agree
    d = np.abs(got.astype(np.float64) - want)
    scale = np.abs(want).max()
    print(f"chain WBFM M={M} agc={agc} mix={mix} [{ch.path}]: median {np.median(d):.2e} p99 {np.quantile(d, 0.99):.2e} max {d.max():.2e} of {scale:.3f}")
    assert np.median(d) < 2e-5 * scale and np.quantile(d, 0.99) < 2e-3 * scale
    with pytest.raises(cs.CsdrError):
        ch.process(x[:M * 1023])
    ch.close()


def test_cpp_soapy_sdr_file_wbfm_audio_matches_python_replay(tmp_path, monkeypatch):
    """README's most used mode, offline: -b 200e3 --demod "DeWBFM 4 AU": C++ CLI and Python replay write the same
    .au bytes (24-byte header with rate round(outBW) div decim div nch = 50000, big-endian floats)."""
    import os
    import struct
    import subprocess
    monkeypatch.setenv("CSDR_QUIET", "1")
    from composable_sdr_amd.app import sdr_process
    exe = host_exe("soapy_sdr_file")
    x = synth_cf32(600000, 1, seed=18)
    src = tmp_path / "in.cf32"
    x.tofile(src)
    n = 4096 * 8
    py = sdr_process(str(src), channels=1, demod="wbfm", decim=4, numsamples=n, outname=str(tmp_path / "py"), chunksize=1024,
                     samplerate=2.56e6, bandwidth=200e3, audio="AU")
    r = subprocess.run([exe, "--filename", str(src), "-n", str(n), "-c", "1", "--demod", "DeWBFM", "4", "-s", "2.56e6", "-b", "200e3",
                        "--audio", "AU", "-o", str(tmp_path / "cc")], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, CSDR_QUIET="1"))
    assert r.returncode == 0, r.stderr
    a, b = open(py[0], "rb").read(), open(tmp_path / "cc.au", "rb").read()
    assert a == b and len(a) == 24 + 4 * (n // 4)
    assert struct.unpack(">4sIIIII", a[:24]) == (b".snd", 24, 4 * (n // 4), 6, 50000, 1)


def test_graft_entry_smoke_passes():
    """the driver's smoke(): one small invocation of the hot path on cuda:0 checked against the oracle"""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import __graft_entry__ as g
    g.smoke()


# --------------------------------------------------------------------------- fused FIR + DFT kernel for M = 1024


@pytest.mark.parametrize("demod,agc,shard", [("fm", 0.0, None), ("none", 0.0, None), ("fm", 17.0, None), ("fm", 0.0, (300, 200)), ("am", 0.0, None)])
def test_pfb1024_fused_kernel_matches_three_kernel_route_and_oracle(demod, agc, shard, monkeypatch):
    """M = 1024: k_pfb1024 (FIR + DFT + transpose + freqdem in one kernel) against the k_pfb_fir / k_fft_r16 / k_transpose_fm
    route (CSDR_NO_PFB1024) on ragged chunks, and against the oracle.  Same arithmetic per output sample (FIR tap order,
    DFT index scheme, freqdem routine): CF32 agrees to rounding of the FMA grouping, FM modulo 1/kf."""
    M = 1024
    frames = [64, 8, 37, 200, 3, 128, 1000]              # the last one is long enough for runs with warm-up and halo tiles
    nf = sum(frames)
    x = synth_cf32(M * nf, M, seed=31)
    kw = dict(channels=M, demod=demod, kf=0.3, agc=agc, max_frames=max(frames))
    if shard:
        kw.update(chan_first=shard[0], chan_count=shard[1])
    a = cs.Chain(**kw)                                   # k_run1024: DC blocker + pre-mix + FIR + DFT + tail in one kernel
    knob(monkeypatch, "CSDR_NO_RUN1024", "1")
    a2 = cs.Chain(**kw)                                  # k_dc_tile + k_pfb1024
    knob(monkeypatch, "CSDR_NO_PFB1024", "1")
    b = cs.Chain(**kw)                                   # k_dc_tile + k_pfb_fir + k_fft_r16 + k_transpose(_fm)
    monkeypatch.delenv("CSDR_NO_PFB1024")
    monkeypatch.delenv("CSDR_NO_RUN1024")
    assert "k_run1024" in a.path and "pfb1024" in a2.path and "pfb1024" not in b.path and "run1024" not in b.path
    orc = O.Chain(M, demod=demod, kf=0.3, agc_db=agc) if not shard else O.Chain(M, demod=demod, kf=0.3)
    ga, ga2, gb, wo, pos = [], [], [], [], 0
    for f in frames:
        xa = x[pos * M:(pos + f) * M]
        ga.append(a.process(xa)); ga2.append(a2.process(xa)); gb.append(b.process(xa)); wo.append(orc.process(xa)); pos += f
    ga, ga2, gb, wo = [np.concatenate(v, axis=1) for v in (ga, ga2, gb, wo)]
    # the back half alone (same DC kernel in front) reproduces the three-kernel route bit for bit
    if not agc:
        assert np.array_equal(ga2.view(np.uint32), gb.view(np.uint32))
    if shard:
        wo = wo[shard[0]:shard[0] + shard[1]]
    assert ga.shape == gb.shape == wo.shape
    if demod == "none":
        assert rel_rms(ga, gb) < 1e-6 and rel_rms(ga, wo) < 1e-5
    elif demod == "am":
        assert max_abs_err(ga, gb) < 1e-4 * np.abs(gb).max() and max_abs_err(ga, wo) < 2e-4 * max(1.0, np.abs(wo).max())
    else:
        d1 = np.abs(wrap_pm(ga.astype(np.float64) - gb, 1.0 / 0.3))
        d2 = np.abs(wrap_pm(ga.astype(np.float64) - wo, 1.0 / 0.3))
        print(f"pfb1024 {demod} agc={agc} shard={shard}: vs 3-kernel median {np.median(d1):.2e} p99.9 {np.quantile(d1, 0.999):.2e}; vs oracle median {np.median(d2):.2e}")
        if agc:
            # -a 17 sits in the 26 dB gap between the noise-only (<= 4 dB) and the tone channels (30 dB) of this fixture
            mk, mo = int(np.sum((ga == 0) != (gb == 0))), int(np.sum((ga == 0) != (wo == 0)))
            print(f"pfb1024 squelch mismatches: vs 3-kernel route {mk}, vs oracle {mo}")
            assert mk == 0 and mo == 0
            assert np.median(d1) < 2e-5 and np.median(d2) < 2e-5
        else:
            assert np.median(d1) < 2e-6 and np.quantile(d1[1::4], 0.999) < 2e-5 and np.median(d2) < 2e-5
    a.close(); a2.close(); b.close()


@pytest.mark.parametrize("demod", ["fm", "none"])
def test_run1024_v3_matches_first_generation_kernel_and_oracle(demod, monkeypatch):
    """k_run1024v3 (one 512-thread workgroup per CU, front / back wave roles, a row's 128-byte line staged in registers: whole band,
    calls of whole 4-frame tiles) against k_run1024 (CSDR_RUN1024_V3=0) and the oracle.  Calls: 5 frames (odd: first-generation kernel,
    leaves the NCO parity odd and a non-trivial DC state, window and r'), 4096 (v3: one run per block, with warm-up, halo and muted tile),
    517 (ragged: k_run1024 picks up v3's state), 2048 (v3 again, picks up its state), 1204 (v3: the call ends inside a line -- its last
    block stores the front 80 / 32 bytes of every row's line), 36 (v3: a single partial block F32, two blocks + a partial one CF32)."""
    M = 1024
    frames = [5, 4096, 517, 2048, 1204, 36]
    nf = sum(frames)
    x = synth_cf32(M * nf, M, seed=79)
    x = (x + np.complex64(0.01 - 0.005j)).astype(np.complex64)    # a DC offset the blocker has to remove across run starts
    kw = dict(channels=M, demod=demod, kf=0.3, max_frames=max(frames))
    a = cs.Chain(**kw)                                            # default: k_run1024v3 where it applies
    knob(monkeypatch, "CSDR_RUN1024_V3", "0")
    b = cs.Chain(**kw)
    monkeypatch.delenv("CSDR_RUN1024_V3")
    orc = O.Chain(M, demod=demod, kf=0.3)
    ga, gb, wo, pos, names = [], [], [], 0, []
    for f in frames:
        xa = x[pos * M:(pos + f) * M]
        ga.append(a.process(xa)); gb.append(b.process(xa)); wo.append(orc.process(xa)); pos += f
        names.append((a.kernel_time()[0], b.kernel_time()[0]))
    print("kernels:", names)
    t = "FM" if demod == "fm" else "CF32"
    assert [n[0] for n in names] == [f"k_run1024<{t}>", f"k_run1024v3<{t}>", f"k_run1024<{t}>", f"k_run1024v3<{t}>", f"k_run1024v3<{t}>", f"k_run1024v3<{t}>"]
    assert all(n[1] == f"k_run1024<{t}>" for n in names)
    ga, gb, wo = [np.concatenate(v, axis=1) for v in (ga, gb, wo)]
    if demod == "none":
        print(f"run1024v3 DeNo: vs v1 {rel_rms(ga, gb):.2e}, vs oracle {rel_rms(ga, wo):.2e}")
        assert rel_rms(ga, gb) < 2e-6 and rel_rms(ga, wo) < 1e-5
        pos = 0
        for f in frames:                                          # every call on its own (a wrong hand-over shows in the call behind it)
            assert rel_rms(ga[:, pos:pos + f], wo[:, pos:pos + f]) < 1e-5, f
            pos += f
        blk = np.abs(ga - wo)[:, 5:5 + 4096].reshape(M // 64, 64, -1, 16)          # every row block and every 16-frame line of the first v3 call
        assert blk.max(axis=(1, 3)).max() < 1e-4 * np.abs(wo).max()
        a.close(); b.close()
        return
    d1 = np.abs(wrap_pm(ga.astype(np.float64) - gb, 1.0 / 0.3))
    d2 = np.abs(wrap_pm(ga.astype(np.float64) - wo, 1.0 / 0.3))
    print(f"run1024v3 FM: vs v1 median {np.median(d1):.2e} p99.9 {np.quantile(d1, 0.999):.2e} max {d1.max():.2e}; "
          f"vs oracle median {np.median(d2):.2e} p99.9 {np.quantile(d2, 0.999):.2e}")
    assert np.median(d1) < 2e-6 and np.median(d2) < 2e-5
    assert np.quantile(d1, 0.999) < 5e-5
    starts = d1[:, 5:5 + 4096:32]                                 # 4096 frames / 128 runs: every run start of the first v3 call
    assert np.quantile(starts, 0.999) < 5e-5
    for lo, hi in ((5, 5 + 4096), (5 + 4096 + 517, 5 + 4096 + 517 + 2048)):      # every row block and every 32-frame line of the v3 calls
        blk = d2[:, lo:hi].reshape(M // 64, 64, -1, 32)
        assert np.median(blk, axis=(1, 3)).max() < 2e-5
    tail1, tail2 = d1[:, -(1204 + 36):], d2[:, -(1204 + 36):]     # the calls that end inside a line: every 4-frame piece of every row
    # (a whole call's own figures: piece medians up to 5e-4 on noise-only channels behind a run start, p99.9 1.3e-5)
    assert np.median(tail1.reshape(M, -1, 4), axis=2).max() < 1e-3 and np.quantile(tail1, 0.999) < 5e-5 and np.median(tail1) < 2e-6 and np.median(tail2) < 2e-5
    a.close(); b.close()


def test_full_size_cfg4_shape_1024ch_fm_properties(monkeypatch):
    """configs[3] shape on one GPU (1024 ch, 65 536 frames = 67 M samples per chunk, k_run1024):
    (1) one chunk == 8 chunks (DC state, FIR window, freqdem r' and the run splits carry over),
    (2) the fused kernel agrees with the four-kernel any-M route on the whole chunk,
    (3) a tone at a channel centre lands in that channel only (>= 75 dB), gain ~ M."""
    import torch
    from synth import channel_centre, synth_cf32_torch
    M, nf = 1024, 65536
    dev = torch.device("cuda", 0)
    x = synth_cf32_torch(M * nf, M, dev, seed=5)

    def run(xx, demod, parts=1):
        ch = cs.Chain(channels=M, demod=demod, max_frames=nf // parts)
        width = 1 if demod == "fm" else 2
        outs = []
        for i in range(parts):
            o = torch.empty(M * (nf // parts) * width, dtype=torch.float32, device=dev)
            ch.process_device(xx.data_ptr() + i * (M * nf // parts) * 8, M * nf // parts, o.data_ptr(), 0)
            outs.append(o.view(M, nf // parts, width))
        torch.cuda.synchronize()
        path = ch.path
        ch.close()
        return torch.cat(outs, dim=1), path

    one, path = run(x, "fm")
    assert "k_run1024" in path
    many, _ = run(x, "fm", parts=8)
    d = (torch.remainder(one - many + 0.5 / 0.3, 1 / 0.3) - 0.5 / 0.3).abs().view(M, nf)
    tone = torch.arange(M, device=dev) % 4 == 1
    print("cfg4 shape one-vs-8 chunks FM: tone-channel max", float(d[tone].max()), "median all", float(d.median()))
    assert float(d[tone].max()) < 1e-5 and float(d.median()) < 5e-6
    knob(monkeypatch, "CSDR_NO_RUN1024", "1")
    knob(monkeypatch, "CSDR_NO_PFB1024", "1")
    gen, gpath = run(x, "fm")
    monkeypatch.delenv("CSDR_NO_RUN1024"); monkeypatch.delenv("CSDR_NO_PFB1024")
    assert "generic" in gpath and "pfb1024" not in gpath
    d = (torch.remainder(one - gen + 0.5 / 0.3, 1 / 0.3) - 0.5 / 0.3).abs().view(M, nf)
    print("cfg4 shape fused-vs-generic FM: tone-channel max", float(d[tone].max()), "median all", float(d.median()))
    assert float(d[tone].max()) < 1e-5 and float(d.median()) < 5e-6
    del one, many, gen, d

    k = 531
    n = torch.arange(M * nf, device=dev, dtype=torch.float64)
    ph = torch.remainder(channel_centre(k, M) * n, 2 * np.pi).to(torch.float32)
    tone_x = torch.stack([torch.cos(ph), torch.sin(ph)], dim=1).contiguous()
    del n, ph
    yt, _ = run(tone_x, "none")
    p = torch.sqrt((yt[:, 100:, :] ** 2).sum(-1)).mean(1)
    others = torch.cat([p[:k], p[k + 1:]])
    iso = 20 * torch.log10(p[k] / (others.max() + 1e-30))
    print("cfg4 shape tone: channel", int(p.argmax()), "isolation dB", float(iso), "gain/M", float(p[k]) / M)
    assert int(p.argmax()) == k and float(iso) > 75 and abs(float(p[k]) / M - 1) < 0.02


def test_full_size_cfg5_shape_4096ch_mix_linearity():
    """configs[4] shape on one GPU (4096 ch, 16 384 frames, DeNo --mix, sum inside the DFT kernel): the mixed output is
    linear in the input and chunk-invariant."""
    import torch
    from synth import synth_cf32_torch
    M, nf = 4096, 16384
    dev = torch.device("cuda", 0)
    x1 = synth_cf32_torch(M * nf, M, dev, seed=7)
    x2 = synth_cf32_torch(M * nf, M, dev, seed=8)

    def run(xx, parts=1):
        ch = cs.Chain(channels=M, demod="none", mix=True, max_frames=nf // parts)
        outs = []
        for i in range(parts):
            o = torch.empty((nf // parts) * 2, dtype=torch.float32, device=dev)
            ch.process_device(xx.data_ptr() + i * (M * nf // parts) * 8, M * nf // parts, o.data_ptr(), 0)
            outs.append(o)
        torch.cuda.synchronize()
        ch.close()
        return torch.cat(outs)

    y1, y2, y12 = run(x1), run(x2), run(x1 + 2 * x2)
    scale = float(y12.abs().max())
    err = float((y12 - (y1 + 2 * y2)).abs().max())
    inv = float((run(x1, parts=4) - y1).abs().max())
    print("cfg5 shape mix: linearity err", err, "chunk-invariance err", inv, "of", scale)
    assert err < 1e-4 * scale and inv < 1e-4 * scale


# --------------------------------------------------------------------------- the oracle at the BENCHMARKED layouts
# One whole bench-sized chunk (67 M samples: 512 runs with warm-up, halo and run-start frames; the 1.2 : 0.8 tile shares)
# through the product path, device-resident like bench.py, against the oracle on the same samples.  The oracle runs at
# ~20 MS/s on the GPU box: 3-10 s per call.


def _bench_layout(M, nf, seed, **kw):
    import torch
    from synth import synth_cf32_torch
    dev = torch.device("cuda", 0)
    x = synth_cf32_torch(M * nf, M, dev, seed=seed)
    ch = cs.Chain(channels=M, max_frames=nf, flags=kw.pop("flags", 4) | 1, **kw)
    fm, mix = kw.get("demod", "none") == "fm", kw.get("mix", False)
    n_out = (nf if mix else M * nf) * (1 if fm else 2)
    out = torch.empty(n_out, dtype=torch.float32, device=dev)
    ch.process_device(x.data_ptr(), M * nf, out.data_ptr(), 0)
    torch.cuda.synchronize()
    kname, path = ch.kernel_time()[0], ch.path
    ch.close()
    got = out.cpu().numpy()
    got = got if fm else got.view(np.complex64)
    got = got.reshape(-1) if mix else got.reshape(M, nf)
    xh = x.cpu().numpy().view(np.complex64).reshape(-1)
    del x, out
    torch.cuda.empty_cache()
    return got, xh, kname, path


def _fm_against_oracle(got, xh, M, kf, label, r):
    """The tolerances of test_chain_fm_matches_oracle on a whole bench-sized chunk.  r: |channel samples| (only weights the
    phase errors: taken from the product's own DeNo run of the same chunk, which the cfg2 / DeNo tests pin to the oracle, to
    save a second 67 M-sample oracle pass)."""
    ref = 1.0 / (2 * np.pi * kf)
    want = O.Chain(M, demod="fm", kf=kf).process(xh)
    assert got.shape == want.shape == r.shape
    rmax = float(r.max())
    worst_w, worst_s, med = 0.0, 0.0, []
    for k0 in range(0, M, 32):                           # by blocks of rows: the f64 temporaries of a whole chunk would be 2 GiB
        sl = slice(k0, k0 + 32)
        d = np.abs(wrap_pm(got[sl].astype(np.float64) - want[sl], 1.0 / kf))
        rr = r[sl]
        rmin = np.minimum(rr, np.concatenate([np.zeros((rr.shape[0], 1), rr.dtype), rr[:, :-1]], axis=1))
        worst_w = max(worst_w, float((d * rmin).max()) / rmax)
        strong = rmin > 0.25 * rmax
        if strong.any():
            worst_s = max(worst_s, float(d[strong].max()))
        med.append(float(np.median(d)))
    print(f"{label}: whole chunk vs oracle: median {np.median(med):.3e}, weighted max {worst_w:.3e} (tol {2 * ref * 1e-4:.3e}), strong-sample max {worst_s:.3e}")
    assert worst_w < 2 * ref * 1e-4
    assert max(med) < 2e-5
    assert worst_s < 2e-5


def test_bench_layout_cfg3_256ch_fm_whole_chunk_matches_oracle():
    """k_run256v2<FM> at 256 x 262 144 (BASELINE configs[2] shape as bench.py runs it) against O.Chain, every sample."""
    M, nf, kf = 256, 262144, 0.3
    got, xh, kname, path = _bench_layout(M, nf, 31, demod="fm", kf=kf)
    assert kname == "k_run256v2<FM>", (kname, path)
    r = np.abs(_bench_layout(M, nf, 31)[0])
    _fm_against_oracle(got, xh, M, kf, f"cfg3 {kname}", r)


def test_bench_layout_cfg3_256ch_fm_agc_whole_chunk_matches_oracle():
    """BASELINE configs[2] as literally written (256-ch PFB + AGC `-a 10` + FM) at the bench size, 256 x 262 144: k_run256v2<CF32>
    + the time-parallel AGC tail against O.Chain(agc_db=10), EVERY sample: mute decisions exactly, open samples within the FM
    tolerance of test_chain_agc_fm_matches_oracle."""
    M, nf, kf = 256, 262144, 0.3
    got, xh, kname, path = _bench_layout(M, nf, 35, demod="fm", kf=kf, agc=10.0)
    assert kname == "k_run256v2<CF32>" and "agc-spec" in path, (kname, path)
    want = O.Chain(M, demod="fm", kf=kf, agc_db=10.0).process(xh)
    assert got.shape == want.shape
    mism, nopen, med, q = 0, 0, [], []
    for k0 in range(0, M, 32):
        sl = slice(k0, k0 + 32)
        mg, mw = got[sl] == 0, want[sl] == 0
        mism += int(np.sum(mg != mw)); nopen += int(np.sum(~mw))
        d = np.abs(wrap_pm(got[sl].astype(np.float64) - want[sl], 1.0 / kf))
        if (~mw).any():
            med.append(float(np.median(d[~mw])))
        q.append(float(np.quantile(d, 0.999)))
    print(f"cfg3 + AGC [{path}]: whole chunk vs oracle: squelch mismatches {mism}, open fraction {nopen / want.size:.3f}, open-sample median {max(med):.3e}, p99.9 {max(q):.3e}")
    assert mism == 0
    assert 0.05 < nopen / want.size < 0.95
    assert max(med) < 2e-5 and max(q) < 5e-4


def test_bench_layout_cfg2_64ch_deno_whole_chunk_matches_oracle():
    """k_run64v2 at 64 x 1 048 576 (BASELINE configs[1]) against O.Chain, every sample."""
    M, nf = 64, 1048576
    got, xh, kname, path = _bench_layout(M, nf, 32)
    assert kname == "k_run64v2", (kname, path)
    want = O.Chain(M).process(xh)
    r, e = rel_rms(got, want), max_abs_err(got, want)
    print(f"cfg2 {kname}: whole chunk vs oracle: rel-rms {r:.3e}, max-abs {e:.3e} of {np.abs(want).max():.2f}")
    assert r < 1e-5 and e < 1e-4 * np.abs(want).max()


def test_bench_layout_cfg4_shape_1024ch_fm_whole_chunk_matches_oracle():
    """k_run1024v3 at 1024 x 65 536 (BASELINE configs[3] shape on one GPU) against O.Chain, every sample."""
    M, nf, kf = 1024, 65536, 0.3
    got, xh, kname, path = _bench_layout(M, nf, 33, demod="fm", kf=kf)
    assert kname == "k_run1024v3<FM>", (kname, path)
    r = np.abs(_bench_layout(M, nf, 33)[0])
    _fm_against_oracle(got, xh, M, kf, f"cfg4 shape {kname}", r)


def test_bench_layout_cfg5_shape_4096ch_mix_identity_whole_chunk_matches_oracle_and_full_bank():
    """The DeNo --mix identity (k_dc_fold + k_mixid_finish) at 4096 x 16 384 (BASELINE configs[4] shape on one GPU) against
    the oracle's full bank + DFT + left fold, every sample, and against the product's own full computation
    (CSDR_FLAG_NO_MIX_IDENTITY) at that size."""
    from composable_sdr_amd import _lib
    M, nf = 4096, 16384
    got, xh, kname, path = _bench_layout(M, nf, 34, demod="none", mix=True)
    assert "mix-identity" in path and kname == "k_dc_fold", (kname, path)
    full, _, kname2, path2 = _bench_layout(M, nf, 34, demod="none", mix=True, flags=_lib.FLAG_QUIET | _lib.FLAG_NO_MIX_IDENTITY)
    assert "mix-identity" not in path2
    want = O.Chain(M, demod="none", mix=True).process(xh)
    assert got.shape == full.shape == want.shape == (nf,)
    ymax = float(np.abs(O.Chain(M).process(xh[: M * 256])).max())      # size of the M terms the full sums add up
    tol = max(4e-7 * ymax * M, 1e-5 * float(np.abs(want).max()))
    print(f"cfg5 shape [{path}]: identity vs full bank [{path2}] max {np.abs(got - full).max():.3e}, vs oracle max {np.abs(got - want).max():.3e}, "
          f"full bank vs oracle {np.abs(full - want).max():.3e} (tolerance {tol:.3e}, |out| max {np.abs(want).max():.2f})")
    assert np.abs(got - full).max() < tol
    assert np.abs(got - want).max() < tol


@pytest.mark.parametrize("M,G", [(4096, 8), (4096, 4), (4096, 2), (8192, 8)])
def test_shard_mix_identity_matches_oracle_rows_and_the_pruned_dft_route(M, G):
    """BASELINE configs[4] per rank (4096 channels, DeNo --mix, channels split over the GPUs, one all-reduce): the channel sum of the
    interleaved shard g of G is (M / G) x the phasor sum of the G surviving polyphase branches' FIRs (k_dc_fold8 + k_mixid_shard_finish,
    round 6).  Against the oracle -- the left fold of the rows g, g + G, ... of O.Chain(M) -- and against the product's own bank + pruned
    DFT + channel sum (CSDR_FLAG_NO_MIX_IDENTITY), over calls that carry the DC state, the branch histories and an odd NCO parity; and
    the ranks' partial mixes add up to the whole-band mix (what the all-reduce returns)."""
    from composable_sdr_amd import _lib
    nfs = [40, 9, 130]
    x = synth_cf32(M * sum(nfs), 256, seed=4100 + G)
    x = (x + np.complex64(0.02 - 0.01j)).astype(np.complex64)        # a DC offset the blocker has to carry through the eighths of a tile
    orc = O.Chain(M)
    rows = [orc.process(x[sum(nfs[:i]) * M: sum(nfs[:i + 1]) * M]) for i in range(len(nfs))]
    ymax = float(max(np.abs(r).max() for r in rows))
    total = [np.zeros(nf, np.complex128) for nf in nfs]
    for g in sorted({0, 1, G - 1} if G > 2 else {0, 1}):
        kw = dict(channels=M, demod="none", mix=True, chan_first=g, chan_stride=G, max_frames=max(nfs))
        ch = cs.Chain(flags=_lib.FLAG_QUIET | _lib.FLAG_TIME_KERNELS, **kw)
        alt = cs.Chain(flags=_lib.FLAG_QUIET | _lib.FLAG_NO_MIX_IDENTITY, **kw)
        assert "shard-mix-identity" in ch.path and "shard-mix-identity" not in alt.path
        pos = 0
        for i, nf in enumerate(nfs):
            c = x[pos:pos + nf * M]; pos += nf * M
            got, ref = ch.process(c), alt.process(c)
            assert ch.kernel_time()[0] == "k_dc_fold8"
            want = np.zeros(nf, np.complex64)
            for r in rows[i][g::G]:                                  # strict left fold in f32, like Trans.hs:119-122
                want = (want + r).astype(np.complex64)
            tol = max(4e-7 * ymax * (M // G), 1e-5 * float(np.abs(want).max()))
            print(f"shard mix identity M={M} G={G} g={g} nf={nf}: vs oracle rows {np.abs(got - want).max():.3e}, vs pruned-DFT route {np.abs(got - ref).max():.3e} "
                  f"(tolerance {tol:.3e}, |out| max {np.abs(want).max():.2f})")
            assert got.shape == want.shape == (nf,)
            assert np.abs(got - want).max() < tol and np.abs(got - ref).max() < tol
        ch.close(); alt.close()
    if G == 2:                                                       # both ranks ran: their partial mixes add up to the whole-band mix
        pos = 0
        whole = cs.Chain(channels=M, demod="none", mix=True, max_frames=max(nfs))
        parts = [cs.Chain(channels=M, demod="none", mix=True, chan_first=g, chan_stride=G, max_frames=max(nfs)) for g in range(G)]
        for nf in nfs:
            c = x[pos:pos + nf * M]; pos += nf * M
            w = whole.process(c)
            ssum = sum(pc.process(c).astype(np.complex128) for pc in parts)
            assert np.abs(ssum - w).max() < max(4e-7 * ymax * M, 1e-5 * float(np.abs(w).max()))
        whole.close()
        for pc in parts:
            pc.close()


# --------------------------------------------------------------------------- pipelined device entry point
@pytest.mark.parametrize("demod", ["fm", "none"])
def test_submit_device_independent_launches_match_serial_calls(demod):
    """csdr_chain_submit_device: run-kernel-sized chunks of whole tiles run as INDEPENDENT launches on two alternating
    streams (run 0 starts cold from the previous chunk's saved tail); small and ragged chunks, and csdr_chain_process_device
    calls in between, are serialized behind them.  Against the same stream through csdr_chain_process_device only (exact
    state carry) and against the oracle: the run-start tolerance of the run kernels (run vs tile kernel test)."""
    import torch
    M, kf = 256, 0.3
    frames = [40000, 40000, 33, 40000, 40016, 40001, 40000, 40000, 48000]
    serial_call = {3}                                     # this chunk goes through process_device on a caller stream in between
    from synth import synth_cf32_torch
    dev = torch.device("cuda", 0)
    xd = synth_cf32_torch(M * sum(frames), M, dev, seed=77, dc=(0.09, -0.04)).view(-1)     # (on the GPU: numpy takes over a minute for 84 M samples)
    x = xd.cpu().numpy().view(np.complex64).reshape(-1)
    width = 1 if demod == "fm" else 2
    kw = dict(channels=M, demod=demod, kf=kf, max_frames=max(frames))
    a, b = cs.Chain(**kw), cs.Chain(**kw)
    st = torch.cuda.Stream()
    outs_a, outs_b, pos = [], [], 0
    for i, f in enumerate(frames):
        oa = torch.empty(M * f * width, dtype=torch.float32, device=dev)
        ob = torch.empty(M * f * width, dtype=torch.float32, device=dev)
        ptr = xd.data_ptr() + pos * M * 8
        if i in serial_call:
            a.process_device(ptr, M * f, oa.data_ptr(), st.cuda_stream)
        else:
            a.submit_device(ptr, M * f, oa.data_ptr())
        b.process_device(ptr, M * f, ob.data_ptr(), 0)
        outs_a.append(oa); outs_b.append(ob); pos += f
    a.wait_device()
    torch.cuda.synchronize()
    n_indep = a.independent_launches()
    print("independent launches:", n_indep, "of", len(frames))
    assert n_indep == 5                                   # chunks 0 (fresh stream: zero history), 1, 4, 7, 8; 2 is small, 3 the serial call, 5 ragged, 6 follows the ragged one
    ga = np.concatenate([o.cpu().numpy().reshape(M, -1) for o in outs_a], axis=1)
    gb = np.concatenate([o.cpu().numpy().reshape(M, -1) for o in outs_b], axis=1)
    a.close(); b.close()
    n_or = sum(frames[:3])                                 # the oracle on the first three calls (two independent launches and a small one)
    want = O.Chain(M, demod=demod, kf=kf).process(x[: M * n_or])
    if demod == "fm":
        d = np.abs(wrap_pm(ga.astype(np.float64) - gb, 1.0 / kf))
        do = np.abs(wrap_pm(ga[:, :n_or].astype(np.float64) - want, 1.0 / kf))
        print(f"pipelined vs serial FM: tone channels max {d[1::4].max():.3e}, median {np.median(d):.3e}; vs oracle tone p99.9 {np.quantile(do[1::4], 0.999):.3e}")
        assert d[1::4].max() < 5e-6 and np.median(d) < 5e-6
        # the fixture's |DC| = 0.094 puts the oracle's own f32 DC-blocker noise (ulp(|v|) / 2 at |v| = 190) into the weak
        # channels' phases: the all-channel median is bounded by what the serial path shows against the same oracle
        ds = np.abs(wrap_pm(gb[:, :n_or].astype(np.float64) - want, 1.0 / kf))
        assert np.quantile(do[1::4], 0.999) < 2e-5 and np.median(do) < 1.05 * np.median(ds) + 1e-7
    else:
        ga, gb = ga.view(np.complex64), gb.view(np.complex64)
        print(f"pipelined vs serial CF32: rel-rms {rel_rms(ga, gb):.3e}; vs oracle {rel_rms(ga[:, :n_or], want):.3e}")
        assert rel_rms(ga, gb) < 1e-6
        # |DC| = 0.094: the oracle's own f32 DC-blocker noise sets the floor (1.3e-5); the pipelined path must sit where the serial one does
        assert rel_rms(ga[:, :n_or], want) < 1.05 * rel_rms(gb[:, :n_or], want) + 1e-7 and rel_rms(ga[:, :n_or], want) < 3e-5
        assert max_abs_err(ga[:, :n_or], want) < 1e-4 * np.abs(want).max()


@pytest.mark.parametrize("M,G,demod,agc", [(256, 2, "fm", 0.0), (256, 4, "none", 0.0), (256, 8, "fm", 0.0), (256, 8, "none", 0.0), (1024, 8, "fm", 0.0), (1024, 2, "fm", 0.0),
                                           (1024, 4, "none", 0.0), (1024, 4, "fm", 0.0), (1024, 8, "none", 0.0), (1024, 8, "fm", 10.0),
                                           (256, 8, "fm", 10.0), (256, 2, "fm", 10.0)])
def test_fused_interleaved_shard_run_sized_calls_match_whole_band(M, G, demod, agc):
    """k_run256v2<.., G> at run-kernel sizes (many runs with cold starts, paired F32 stores, ragged and tiny calls in between,
    state carried from call to call): every shard g must reproduce the rows g, g + G, ... of the whole-band fused chain on the
    same calls (same kernels upstream of pass 1, so FM agrees to the rounding of a differently pruned butterfly).
    With the AGC on (k_run256v2<CF32, G> into the shard's [M / G][nf] plane + k_agc_spec on it: the configuration behind the
    per-rank AGC figures of DESIGN 4.1 / 6) the mute mask must equal the whole band's bit for bit, and the first run-sized call is
    also compared with rows g::G of the oracle directly."""
    kf = 0.3
    from composable_sdr_amd import _lib
    # M = 1024: k_run1024v2<FM, G> on the run-sized calls of whole 4-frame tiles, the whole-band kernel + row gather on the others (and for CF32)
    import torch
    from synth import synth_cf32_torch
    frames = [40000, 5, 33, 40016, 16, 40001, 36864] if M == 256 else [12288, 5, 33, 12292, 16, 12289, 8192]
    # (generated on the GPU: numpy takes minutes for 46 M samples of 256 carriers)
    x = synth_cf32_torch(M * sum(frames), M, torch.device("cuda", 0), seed=500 + G, dc=(0.04, 0.03)).cpu().numpy().view(np.complex64).reshape(-1)
    full = cs.Chain(channels=M, demod=demod, kf=kf, agc=agc, max_frames=max(frames))
    wf, pos = [], 0
    for f in frames:
        wf.append(full.process(x[pos * M:(pos + f) * M])); pos += f
    wf = np.concatenate(wf, axis=1)
    full.close()
    want_or = O.Chain(M, demod=demod, kf=kf, agc_db=agc).process(x[: M * frames[0]]) if agc else None     # 10 M samples: ~1 s of oracle
    for g in sorted({0, 1, G - 1}):
        ch = cs.Chain(channels=M, demod=demod, kf=kf, agc=agc, chan_first=g, chan_stride=G, max_frames=max(frames),
                      flags=_lib.FLAG_QUIET | _lib.FLAG_TIME_KERNELS)
        assert "interleaved-shard" in ch.path
        got, pos, knames = [], 0, []
        for f in frames:
            got.append(ch.process(x[pos * M:(pos + f) * M])); pos += f
            knames.append(ch.kernel_time()[0])
        got = np.concatenate(got, axis=1)
        ch.close()
        if M == 256:                                     # the run-sized calls went through the fused shard kernel itself
            kwant = f"k_run256v2<{'FM' if (demod == 'fm' and not agc) else 'CF32'}>/G{G}"
            assert [knames[i] for i in (0, 3, 5, 6)] == [kwant] * 4, (knames, kwant)
        elif not agc:                                    # M = 1024: the run-sized calls of whole 4-frame tiles (12288, 12292, 8192 frames)
            kwant = f"k_shard1024<{'FM' if demod == 'fm' else 'CF32'}>/G{G}" if G >= 4 else ("k_run1024v2<FM>/G2" if demod == "fm" else "k_run1024<CF32>")
            assert [knames[i] for i in (0, 3, 6)] == [kwant] * 3, knames
            assert knames[5] == f"k_run1024<{'FM' if demod == 'fm' else 'CF32'}>", knames   # 12289 frames: ragged -> whole band + row gather
        want = wf[g::G]
        assert got.shape == want.shape
        if agc:
            mism = int(np.sum((got == 0) != (want == 0)))
            d = np.abs(wrap_pm(got.astype(np.float64) - want, 1.0 / kf))
            op = want != 0
            print(f"fused shard G={G} g={g} FM + AGC: mute-mask mismatches vs whole band {mism}, open {op.mean():.3f}, p99.9 {np.quantile(d, 0.999):.2e}")
            assert mism == 0
            tones = ((np.arange(g, M, G) % 4) == 1).any()          # the fixture's carriers sit on channels k = 1 (mod 4)
            assert op.mean() > 0.05 or not tones                 # (a shard may hold carriers only, or none)
            assert (not tones or np.median(d[op]) < 2e-5) and np.quantile(d, 0.999) < 5e-4      # (noise-only shards open for the create-time transient only)
            wo, go = want_or[g::G], got[:, : frames[0]]
            mo = int(np.sum((go == 0) != (wo == 0)))
            do = np.abs(wrap_pm(go.astype(np.float64) - wo, 1.0 / kf))
            print(f"    first call vs oracle rows {g}::{G}: mute-mask mismatches {mo}, p99.9 {np.quantile(do, 0.999):.2e}")
            assert mo == 0
            assert (not tones or np.median(do[wo != 0]) < 2e-5) and np.quantile(do, 0.999) < 5e-4
        elif demod == "fm":
            d = np.abs(wrap_pm(got.astype(np.float64) - want, 1.0 / kf))
            tone = (np.arange(g, M, G) % 4) == 1
            print(f"fused shard G={G} g={g} FM: median {np.median(d):.2e}, tone-channel max {d[tone].max() if tone.any() else 0:.2e}")
            assert np.median(d) < 2e-6 and (not tone.any() or d[tone].max() < 1e-5)
        else:
            e = np.sqrt(np.mean(np.abs(got.astype(np.complex128) - want) ** 2)) / np.sqrt(np.mean(np.abs(wf) ** 2))
            print(f"fused shard G={G} g={g} CF32: rel-rms (of the whole band) {e:.2e}")
            assert e < 2e-6, e


@pytest.mark.parametrize("M,nf,cases", [
    (256, 40000, [(8, 3, "fm"), (2, 1, "none"), (4, 2, "fm")]),
    # BASELINE configs[3] per rank: 1024 channels split over 8 GPUs, rank g owns g, g + 8, ... (Trans.hs:124-129, SoapySDR.hs:223-225)
    (1024, 12288, [(8, 0, "fm"), (8, 3, "fm"), (8, 7, "fm"), (2, 1, "fm"), (4, 2, "fm"), (8, 5, "none"), (4, 1, "none")]),
])
def test_fused_interleaved_shard_run_sized_call_matches_oracle_rows(M, nf, cases):
    """One run-sized call of the fused shard kernels compared DIRECTLY with the oracle (not with the whole-band kernel):
    k_run256v2<FM, 8> / k_run256v2<CF32, 2> on 40 000 frames x 256 channels, and k_run1024v2<FM, G> -- the kernel a rank of
    BASELINE configs[3] runs -- on 12 288 frames x 1024 channels, against O.Chain(...)[g::G] with the tolerances of the
    whole-band bench-layout tests (_fm_against_oracle); the kernel name is taken from the launch timer, so a silent change
    of route fails the test."""
    import torch
    from composable_sdr_amd import _lib
    from synth import synth_cf32_torch
    kf = 0.3
    x = synth_cf32_torch(M * nf, M, torch.device("cuda", 0), seed=611).cpu().numpy().view(np.complex64).reshape(-1)
    w_fm = O.Chain(M, demod="fm", kf=kf).process(x)
    w_cf = O.Chain(M).process(x)
    r = np.abs(w_cf)
    for G, g, demod in cases:
        # M = 1024: strides 4 and 8 run k_shard1024 (round 6: fold behind the FIR + short DFT across the lanes), stride 2 keeps k_run1024v2
        fam = "k_run256v2" if M == 256 else ("k_shard1024" if G >= 4 else "k_run1024v2")
        ch = cs.Chain(channels=M, demod=demod, kf=kf, chan_first=g, chan_stride=G, max_frames=nf, flags=_lib.FLAG_QUIET | _lib.FLAG_TIME_KERNELS)
        assert "interleaved-shard" in ch.path
        got = ch.process(x)
        kname = ch.kernel_time()[0]
        ch.close()
        assert kname == f"{fam}<{'FM' if demod == 'fm' else 'CF32'}>/G{G}", kname
        if demod == "fm":
            want, rr = w_fm[g::G], r[g::G]
            assert got.shape == want.shape == (M // G, nf)
            d = np.abs(wrap_pm(got.astype(np.float64) - want, 1.0 / kf))
            rmin = np.minimum(rr, np.concatenate([np.zeros((rr.shape[0], 1), rr.dtype), rr[:, :-1]], axis=1))
            ref = 1.0 / (2 * np.pi * kf)
            strong = rmin > 0.25 * r.max()
            smax = float(d[strong].max()) if strong.any() else 0.0      # (a shard may hold no carrier at all)
            print(f"{kname} g={g} vs oracle rows: median {np.median(d):.2e}, weighted max {(d * rmin).max() / r.max():.2e}, strong max {smax:.2e}")
            assert (d * rmin).max() / r.max() < 2 * ref * 1e-4 and np.median(d) < 2e-5 and smax < 2e-5
        else:
            want = w_cf[g::G]
            e = np.sqrt(np.mean(np.abs(got.astype(np.complex128) - want) ** 2)) / np.sqrt(np.mean(np.abs(w_cf) ** 2))
            print(f"{kname} g={g} vs oracle rows: rel-rms (of the whole band) {e:.2e}, max-abs {np.abs(got - want).max():.2e}")
            assert e < 1e-5 and np.abs(got - want).max() < 1e-4 * np.abs(w_cf).max()


def test_run1024v2_shard_kernels_behind_the_knob_match_oracle_rows(monkeypatch):
    """k_run1024v2<FM, 4 | 8> stay built behind CSDR_NO_SHARD1024=1 (the A/B of profiles/r06_shard1024_call_sizes.txt; stride 2 is their
    default route): the same direct comparison with the oracle's rows, so that the round-6 removal of the kernel's whole-band code
    paths is pinned for every instantiation that is still compiled."""
    import torch
    from composable_sdr_amd import _lib
    from synth import synth_cf32_torch
    knob(monkeypatch, "CSDR_NO_SHARD1024", "1")
    M, nf, kf = 1024, 12288, 0.3
    x = synth_cf32_torch(M * nf, M, torch.device("cuda", 0), seed=612).cpu().numpy().view(np.complex64).reshape(-1)
    w_fm = O.Chain(M, demod="fm", kf=kf).process(x)
    r = np.abs(O.Chain(M).process(x))
    ref = 1.0 / (2 * np.pi * kf)
    for G, g in [(8, 6), (4, 3), (2, 0)]:
        ch = cs.Chain(channels=M, demod="fm", kf=kf, chan_first=g, chan_stride=G, max_frames=nf, flags=_lib.FLAG_QUIET | _lib.FLAG_TIME_KERNELS)
        got = ch.process(x)
        kname = ch.kernel_time()[0]
        ch.close()
        assert kname == f"k_run1024v2<FM>/G{G}", kname
        want, rr = w_fm[g::G], r[g::G]
        d = np.abs(wrap_pm(got.astype(np.float64) - want, 1.0 / kf))
        rmin = np.minimum(rr, np.concatenate([np.zeros((rr.shape[0], 1), rr.dtype), rr[:, :-1]], axis=1))
        strong = rmin > 0.25 * r.max()
        smax = float(d[strong].max()) if strong.any() else 0.0
        print(f"{kname} g={g} vs oracle rows: median {np.median(d):.2e}, weighted max {(d * rmin).max() / r.max():.2e}, strong max {smax:.2e}")
        assert (d * rmin).max() / r.max() < 2 * ref * 1e-4 and np.median(d) < 2e-5 and smax < 2e-5


def test_submit_device_on_interleaved_shard_with_short_chunks():
    """csdr_chain_submit_device on a chan_stride = 2 chain with chunks of 1 .. 6 whole tiles.  Shards never
    run as independent launches and must not save a tail (the copy of the last WU + 1 tiles would read in front of the chunk):
    same result as csdr_chain_process_device."""
    import torch
    from synth import synth_cf32_torch
    M, kf = 256, 0.3
    dev = torch.device("cuda", 0)
    frames = [32, 16, 96, 40000, 48, 7]
    xd = synth_cf32_torch(M * sum(frames), M, dev, seed=88).view(-1)
    kw = dict(channels=M, demod="fm", kf=kf, chan_first=1, chan_stride=2, max_frames=max(frames))
    a, b = cs.Chain(**kw), cs.Chain(**kw)
    # (outputs allocated and cleared up front: a fill queued on torch's stream would race with the handle's own streams)
    oa = [torch.zeros(M // 2 * f, dtype=torch.float32, device=dev) for f in frames]
    ob = [torch.zeros(M // 2 * f, dtype=torch.float32, device=dev) for f in frames]
    torch.cuda.synchronize()
    pos = 0
    for f, ya, yb in zip(frames, oa, ob):
        ptr = xd.data_ptr() + pos * M * 8
        a.submit_device(ptr, M * f, ya.data_ptr())
        b.process_device(ptr, M * f, yb.data_ptr(), 0)
        pos += f
    a.wait_device()
    torch.cuda.synchronize()
    assert a.independent_launches() == 0
    for f, ya, yb in zip(frames, oa, ob):
        assert torch.equal(ya, yb), f
    a.status(); b.status()
    a.close(); b.close()


def test_round3_entry_points_reset_seek_and_fallbacks():
    """Housekeeping of the round-3 paths: reset / seek_frames on a fused interleaved shard and on a handle with pipelined chunks
    restore the initial state; strides the fused shard kernels do not take (16) use the any-M route; bad sizes are rejected."""
    import torch
    from synth import synth_cf32_torch
    M, kf, nf = 256, 0.3, 36864
    dev = torch.device("cuda", 0)
    xd = synth_cf32_torch(M * nf * 2, M, dev, seed=91).view(-1)
    x = xd.cpu().numpy().view(np.complex64).reshape(-1)
    # (1) fused shard: reset and seek
    ch = cs.Chain(channels=M, demod="fm", kf=kf, chan_first=1, chan_stride=4, max_frames=nf)
    assert "interleaved-shard" in ch.path
    a1 = ch.process(x[: M * nf]); a2 = ch.process(x[M * nf:])
    ch.reset()
    b1 = ch.process(x[: M * nf])
    assert np.array_equal(a1, b1)
    ch.seek_frames(nf)                                    # the second chunk alone, from a fresh state at its stream position
    c2 = ch.process(x[M * nf:])
    d = np.abs(wrap_pm(c2[:, 64:].astype(np.float64) - a2[:, 64:], 1.0 / kf))      # behind the FIR / DC transient of the fresh start
    assert np.median(d) < 1e-3
    ch.close()
    # (2) pipelined chunks, reset, pipelined chunks again
    ch = cs.Chain(channels=M, demod="fm", kf=kf, max_frames=nf)
    outs = [torch.empty(M * nf, dtype=torch.float32, device=dev) for _ in range(4)]
    for i in range(2):
        ch.submit_device(xd.data_ptr() + i * M * nf * 8, M * nf, outs[i].data_ptr())
    ch.wait_device()
    ch.reset()
    for i in range(2):
        ch.submit_device(xd.data_ptr() + i * M * nf * 8, M * nf, outs[2 + i].data_ptr())
    ch.wait_device()
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[3])
    with pytest.raises(cs.CsdrError):
        ch.submit_device(xd.data_ptr(), M * 16 + 3, outs[0].data_ptr())
    ch.close()
    # (3) a stride without a fused shard kernel
    g16 = cs.Chain(channels=M, demod="none", chan_first=5, chan_stride=16, max_frames=512)
    assert "pruned-dft" in g16.path
    y = g16.process(x[: M * 512])
    w = O.Chain(M).process(x[: M * 512])[5::16]
    assert rel_rms(y, w) < 1e-5 * np.sqrt(np.mean(np.abs(O.Chain(M).process(x[: M * 512])) ** 2)) / np.sqrt(np.mean(np.abs(w) ** 2)) + 1e-5
    g16.close()
