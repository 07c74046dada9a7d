"""Stereo FM decoding (csdr_fmstereo_*) on the GPU against the CPU restatement in tests/fms_restatement.py.

Tolerances: the decoder parity bound is rel-RMS 1e-5 on L and R.  The GPU evaluates sinf / cosf / atanf with the device
library (a few ulp from libm's) and its FIRs in f32 with FMA (the restatement: f64, rounded once), so the PLL's uint32 words
drift from the restatement's by a few LSBs of the f32-quantised phase; that moves u by ~1e-7 of its scale.  With an offset
pilot the acquisition itself is where such LSB differences are amplified (the loop pulls in over the first ~0.2 s), so that
case is compared after 0.5 s, once both loops are locked, at 1e-4."""
import os
import struct
import subprocess

import numpy as np
import pytest

import fms_restatement as F
import oracle_lib as O
from host_exe import host_exe
from synth import synth_cf32

pytestmark = pytest.mark.gpu

cs = pytest.importorskip("composable_sdr_amd")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = 192e3


def _rel_rms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2) / np.mean(b ** 2)))


def _report(tag, got, want):
    d = np.abs(np.asarray(got, np.float64) - want)
    s = np.abs(want).max()
    print(f"{tag}: |err| median {np.median(d) / s:.2e} p99 {np.quantile(d, 0.99) / s:.2e} max {d.max() / s:.2e} (of max |ref|)")


def _words_diff(a, b):
    return [((int(x) - int(y) + 2 ** 31) % 2 ** 32) - 2 ** 31 for x, y in zip(a, b)]


@pytest.mark.parametrize("offset_hz,n,skip_s,tol", [(0.0, 96000, 0.0, 1e-5), (20.0, 144000, 0.5, 1e-4)])
def test_decoder_matches_restatement(offset_hz, n, skip_s, tol):
    x = F.stereo_mpx(n, Q, pilot_offset_hz=offset_hz, seed=11)
    want, st = F.decode(x, Q, 4)
    dec = cs.FmStereo(Q, 4, max_samples=n)
    assert (dec.delay, dec.taps_len) == (st["P"]["d"], st["P"]["N"]) == (71, 142)
    got = dec.process(x)
    th, dth = dec.pll()
    dec.close()
    k = 2 * int(skip_s * Q / 4)
    dw = _words_diff((th, dth), (st["theta"], st["dtheta"]))
    _report(f"DeFMS offset {offset_hz} Hz", got[k:], want[k:])
    print(f"  end state: theta {th} vs {st['theta']} ({dw[0]:+d} LSB), d_theta {dth} vs {st['dtheta']} ({dw[1]:+d} LSB)")
    for ch in (0, 1):
        r = _rel_rms(got[k + ch::2], want[k + ch::2])
        print(f"  {'LR'[ch]}: rel-RMS {r:.2e}")
        assert r <= tol
    # the loop tracks the same pilot: the end frequency words agree to far below 0.01 Hz
    assert abs(dw[1]) / 2 ** 32 * Q < 0.01


def test_chunking_is_bit_identical():
    n = 96000
    x = F.stereo_mpx(n, Q, pilot_offset_hz=5.0, seed=12)
    ref = cs.FmStereo(Q, 4, max_samples=n)
    one = ref.process(x)
    w_one = ref.pll()
    ref.close()
    rng = np.random.default_rng(5)
    ragged, pos = [], 0
    while pos < n:
        c = min(int(rng.integers(1, 3000)) * 4, n - pos)
        ragged.append(c)
        pos += c
    for calls in ([1024] * (n // 1024) + ([n % 1024] if n % 1024 else []), ragged):
        dec = cs.FmStereo(Q, 4, max_samples=12000)
        outs, pos = [], 0
        for c in calls:
            outs.append(dec.process(x[pos:pos + c]))
            pos += c
        got = np.concatenate(outs)
        assert got.shape == one.shape and np.array_equal(got, one)
        assert dec.pll() == w_one
        dec.close()


def test_multi_stream_handle_equals_single_stream_handles():
    C, n = 64, 20000
    X = np.stack([F.stereo_mpx(n, Q, pilot_offset_hz=float(c % 9) * 3 - 12, seed=100 + c, fl=500 + 50 * c) for c in range(C)])
    multi = cs.FmStereo(Q, 4, nchan=C, max_samples=n)
    got = multi.process(X)
    assert got.shape == (C, 2 * (n // 4))
    for c in range(C):
        one = cs.FmStereo(Q, 4, max_samples=n)
        assert np.array_equal(one.process(X[c]), got[c]), c
        assert one.pll() == multi.pll(c)
        one.close()
    multi.close()


def test_mono_broadcast_has_no_difference_signal():
    n = 57600
    x = F.stereo_mpx(n, Q, pilot=False, seed=13)
    dec = cs.FmStereo(Q, 4, max_samples=n)
    lr = dec.process(x)
    dec.close()
    assert np.all(np.isfinite(lr))
    k = 2 * int(0.05 * Q / 4)
    L, R = lr[k::2].astype(np.float64), lr[k + 1::2].astype(np.float64)
    db = 10 * np.log10(np.sum((L - R) ** 2) / np.sum((L + R) ** 2))
    print(f"mono: |L-R| / |L+R| = {db:.1f} dB")
    assert db <= -30


def _replay(src, n, chunksize, samplerate, bandwidth, decim=4):
    """the restatement's DeFMS decim: per source chunk [-> O.MsResamp] (takeNArr n trims the prepared stream to n samples) ->
    O.FreqDem(0.8), then the decoder over the calls' lengths"""
    x = np.fromfile(src, dtype=np.complex64)
    rs = O.MsResamp(np.float32(bandwidth / samplerate)) if bandwidth else None
    fd = O.FreqDem(0.8)
    mpx, calls, seen = [], [], 0
    for i in range(0, x.size, chunksize):
        a = x[i:i + chunksize]
        if rs is not None:
            a = rs.execute(a)
        a = a[: n - seen]
        seen += a.size
        mpx.append(fd.demodulate_block(a))
        calls.append(a.size)
        if seen == n:
            break
    q = bandwidth or samplerate
    return F.decode(np.concatenate(mpx), q, decim, calls=calls)[0]


@pytest.mark.parametrize("bandwidth,q,decim", [pytest.param(0.0, Q, 4, id="0.0"), pytest.param(192e3, Q, 4, id="192000.0"),
                                               pytest.param(0.0, 240e3, 5, id="240k-decim5")])
def test_sdr_process_fms_matches_replay_and_cpp_host(tmp_path, monkeypatch, bandwidth, q, decim):
    """q: the decoder's rate, behind the resampler where there is one.  240 kHz with decim 5 (N = 178, d = 88): 1024-sample calls
    are no multiple of 5, and the sink's rate is still 48 kHz"""
    monkeypatch.setenv("CSDR_QUIET", "1")
    from composable_sdr_amd.app import sdr_process
    fs = 2 * q if bandwidth else q
    n = 65536                                                  # samples after the resampler (takeNArr follows it)
    x, _ = F.stereo_broadcast((2 if bandwidth else 1) * n + 5000, fs, kf=0.8, seed=21)
    src = tmp_path / "in.cf32"
    x.tofile(src)
    py = sdr_process(str(src), channels=1, demod="fms", decim=decim, numsamples=n, outname=str(tmp_path / "py"), chunksize=1024,
                     samplerate=fs, bandwidth=bandwidth, audio="AU")
    a = open(py[0], "rb").read()
    hdr = struct.unpack(">4sIIIII", a[:24])
    got = np.frombuffer(a[24:], dtype=">f4").astype(np.float32)
    assert hdr == (b".snd", 24, 4 * got.size, 6, 48000, 2)
    want = _replay(src, n, 1024, fs, bandwidth, decim)
    assert got.shape == want.shape
    # freqdem branch cuts land differently on the two sides (a flip is smeared over ~N samples by the FIRs): robust comparison
    d = np.abs(got.astype(np.float64) - want)
    scale = np.abs(want).max()
    _report(f"sdr_process DeFMS {decim} -s {fs:g} -b {bandwidth}", got, want)
    assert np.median(d) < 2e-5 * scale and np.quantile(d, 0.99) < 2e-3 * scale
    exe = host_exe("soapy_sdr_file")
    args = [exe, "--filename", str(src), "-n", str(n), "-c", "1", "--demod", "DeFMS", str(decim), "-s", str(fs), "--audio", "AU",
            "-o", str(tmp_path / "cc")]
    if bandwidth:
        args += ["-b", str(bandwidth)]
    r = subprocess.run(args, capture_output=True, text=True, timeout=300, env=dict(os.environ, CSDR_QUIET="1"))
    assert r.returncode == 0, r.stderr
    assert open(tmp_path / "cc.au", "rb").read() == a


def test_multi_station_from_the_channelizer():
    """Chain(channels=128, demod="fm", kf=0.8) -> fmstereo(nchan=128), device to device.  Every row of the decoder's output
    against the restatement on the MPX row the device chain handed it; and the tone-bearing rows (k = 1 mod 4 of the synthetic
    band) end to end against the restatement on O.Chain's row (on the noise-only rows the chains' freqdem outputs part where a
    weak sample's phase sits on the branch cut, which tests/test_gpu_parity.py covers on its own terms)"""
    import torch
    M, nf = 128, 8192
    x = synth_cf32(M * nf, M, seed=31)
    ch = cs.Chain(channels=M, demod="fm", kf=0.8, max_frames=nf)
    dec = cs.FmStereo(Q, 4, nchan=M, max_samples=nf)
    d_in = torch.from_numpy(x.view(np.float32).copy()).cuda()
    d_mid = torch.empty(M * nf, dtype=torch.float32, device="cuda")
    d_out = torch.empty(M * 2 * (nf // 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert ch.process_device(d_in.data_ptr(), M * nf, d_mid.data_ptr(), 0) == M * nf
    assert dec.process_device(d_mid.data_ptr(), nf, d_out.data_ptr(), 0) == M * 2 * (nf // 4)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy().reshape(M, -1)
    mid = d_mid.cpu().numpy().reshape(M, nf)
    ch.close()
    dec.close()
    want_dev, _, _ = F.decode_rows(mid, Q, 4)
    worst = 0.0
    for r in range(M):
        rr = _rel_rms(got[r], want_dev[r])
        worst = max(worst, rr)
        assert rr <= 1e-4, (r, rr)
    print(f"128 stations, restatement on the device MPX: worst per-row rel-RMS {worst:.2e}")
    tones = np.arange(1, M, 4)
    want, _, _ = F.decode_rows(O.Chain(M, demod="fm", kf=0.8).process(x)[tones], Q, 4)
    worst = 0.0
    for i, r in enumerate(tones):
        d = np.abs(got[r].astype(np.float64) - want[i])
        scale = np.abs(want[i]).max()
        worst = max(worst, np.median(d) / scale)
        assert np.median(d) < 2e-5 * scale and np.quantile(d, 0.99) < 2e-3 * scale, r
    print(f"128 stations, tone rows vs O.Chain: worst per-row median |err| {worst:.2e} of the row's max")
