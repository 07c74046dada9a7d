"""Symbol timing recovery (csdr_symsync_*) on the GPU against the CPU restatement in tests/symsync_restatement.py.

The kernel and the restatement perform the same f32 operations in the same order (no contraction, one summation order, roundf,
a correctly rounded / k), so every comparison here is bit for bit.  The restatement takes the handle's banks (get_taps); the
design itself is compared separately."""
import os
import subprocess

import numpy as np
import pytest

import symsync_restatement as S
from host_exe import host_exe
from synth import synth_cf32

pytestmark = pytest.mark.gpu

cs = pytest.importorskip("composable_sdr_amd")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _bits(a):
    return np.asarray(a, f32).view(np.uint32)


def _fsk(nsym, offset=0.37, ppm=200.0, seed=1):
    x, bits = S.nrz_fsk_iq(nsym, k=4, offset=offset, ppm=ppm, seed=seed)
    return S.freqdem(x, f32(0.08)), bits


def _noise_fm(n, seed=2):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    return S.freqdem(x, f32(0.08))


def _gpu_calls(h, X, calls):
    """X [nchan][N] through handle h in calls of the given sizes: (per-stream outputs, counts [ncalls][nchan])"""
    outs = [[] for _ in range(h.nchan)]
    counts, pos = [], 0
    for c in calls:
        y, ny = h.process_rows(X[:, pos:pos + c])
        pos += c
        counts.append(ny.astype(np.int64))
        for r in range(h.nchan):
            outs[r].append(y[r, :ny[r]])
    return [np.concatenate(o) for o in outs], np.array(counts)


def test_design_matches_the_restatement():
    h = cs.SymSync(4, 4, 0.0, 64)
    mf, dmf = h.taps()
    h.close()
    P = S.design()
    assert mf.shape == (32, 64)
    print(f"banks: {np.mean(mf == P['mf']):.4f} / {np.mean(dmf == P['dmf']):.4f} of the taps bitwise equal")
    np.testing.assert_allclose(mf, P["mf"], rtol=0, atol=2e-7 * np.abs(P["mf"]).max())
    np.testing.assert_allclose(dmf, P["dmf"], rtol=0, atol=2e-7 * np.abs(P["dmf"]).max())


@pytest.mark.parametrize("signal", ["fsk", "noise"])
def test_one_stream_matches_restatement(signal):
    x = _fsk(6000)[0] if signal == "fsk" else _noise_fm(24000)
    calls = [4096] * (x.size // 4096) + [x.size % 4096]
    h = cs.SymSync(4, 4, 0.0, 64, max_samples=4096)
    got, gc = _gpu_calls(h, x.reshape(1, -1), calls)
    st = h.state(0)
    want, wc, _, s = S.run_calls(x, calls, banks=h.taps())
    h.close()
    assert np.array_equal(gc, wc)
    assert np.array_equal(_bits(got[0]), _bits(want[0])), signal
    assert _bits(st).tolist() == _bits([s.tau[0], s.rate[0], s.dl[0], s.q_hat[0]]).tolist()
    print(f"{signal}: {got[0].size} outputs bit-identical, state tau {st[0]:.6f} rate {st[1]:.6f} del {st[2]:.6f}")


def test_random_call_sizes_equal_one_call():
    x, _ = _fsk(5000, seed=3)
    one = cs.SymSync(4, 4, 0.0, 64, max_samples=x.size)
    ref = one.process(x)
    one.close()
    rng = np.random.default_rng(7)
    calls, pos = [], 0
    while pos < x.size:
        c = min(int(rng.choice([1, 2, 3, 5, 7, 13, 63, 64, 65, 1000, 2047])), x.size - pos)
        calls.append(c)
        pos += c
    h = cs.SymSync(4, 4, 0.0, 64, max_samples=4096)
    got, _ = _gpu_calls(h, x.reshape(1, -1), calls)
    h.close()
    assert np.array_equal(_bits(got[0]), _bits(ref))


def test_256_streams_match_restatement_and_single_handles():
    C, nsym = 256, 1500
    rows = []
    for r in range(C):
        m, _ = _fsk(nsym, offset=(r * 0.137) % 4.0, ppm=-300.0 + 600.0 * r / (C - 1), seed=100 + r)
        rows.append(m[:5800])
    X = np.stack(rows)
    calls = [2048, 2048, 1704]
    h = cs.SymSync(4, 4, 0.0, 64, nchan=C, max_samples=2048)
    got, gc = _gpu_calls(h, X, calls)
    banks = h.taps()
    h.close()
    want, wc, _, _ = S.run_calls(X, calls, banks=banks)
    assert np.array_equal(gc, wc)
    for r in range(C):
        assert np.array_equal(_bits(got[r]), _bits(want[r])), r
    for r in (0, 77, 255):
        one = cs.SymSync(4, 4, 0.0, 64, max_samples=2048)
        g1, _ = _gpu_calls(one, X[r:r + 1], calls)
        one.close()
        assert np.array_equal(_bits(g1[0]), _bits(got[r])), r


def test_chain_rows_device_to_device():
    """Chain(channels=8, demod="fm", kf=0.08) rows -> process_device (device to device) equals the host path on the same rows"""
    import torch
    M, nf = 8, 4096
    x = synth_cf32(M * nf, M, seed=41)
    ch = cs.Chain(channels=M, demod="fm", kf=float(f32(0.08)), max_frames=nf)
    dev = cs.SymSync(4, 4, 0.0, 64, nchan=M, max_samples=nf)
    d_in = torch.from_numpy(x.view(np.float32).copy()).cuda()
    d_mid = torch.empty(M * nf, dtype=torch.float32, device="cuda")
    d_y = torch.empty(M * nf, dtype=torch.float32, device="cuda")
    d_ny = torch.zeros(M, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert ch.process_device(d_in.data_ptr(), M * nf, d_mid.data_ptr(), 0) == M * nf
    dev.process_device(d_mid.data_ptr(), nf, d_y.data_ptr(), d_ny.data_ptr(), 0)
    torch.cuda.synchronize()
    ny = d_ny.cpu().numpy()
    y = d_y.cpu().numpy().reshape(M, nf)
    mid = d_mid.cpu().numpy().reshape(M, nf)
    ch.close()
    dev.close()
    host = cs.SymSync(4, 4, 0.0, 64, nchan=M, max_samples=nf)
    hy, hny = host.process_rows(mid)
    host.close()
    assert np.array_equal(ny, hny.astype(np.int32))
    for r in range(M):
        assert np.array_equal(_bits(y[r, :ny[r]]), _bits(hy[r, :hny[r]])), r


def _replay_sync(src, n, chunksize, nch, k, mixed, samplerate, bandwidth, offset, banks):
    """the Python app's DeNBFMSync path restated: prep (the library's mixer / resampler) -> takeNArr n -> compact (4 k nch 1024)
    -> Chain(fm, kf = 0.02 k) per compacted chunk -> the restatement over the chunk's rows -> per-channel files or the mix"""
    from composable_sdr_amd.app import _prep, readFromFile
    from composable_sdr_amd.pipes import unPipe
    from composable_sdr_amd.trans import takeNArr
    process, cleanup = unPipe(_prep(offset, samplerate, bandwidth, chunksize))
    x = np.concatenate(list(takeNArr(n, process(readFromFile(chunksize, str(src))))))
    cleanup()
    K = 4 * k * nch * 1024
    ch = cs.Chain(channels=nch, demod="fm", kf=float(f32(0.02) * f32(k)), max_frames=4 * k * 1024)
    ss = S.SymSync(nch, k=k, banks=banks)
    outs = [[] for _ in range(nch)]
    mix = []
    for i in range(0, x.size, K):
        a = x[i:i + K]
        u = a.size // nch * nch
        if u == 0:
            continue
        rows = ch.process(a[:u]).reshape(nch, -1)
        y, ny = ss.process(rows)
        rs = [y[r, :ny[r]] for r in range(nch)]
        for r in range(nch):
            outs[r].append(rs[r])
        acc = rs[0]
        for r in rs[1:]:
            m = min(acc.size, r.size)
            acc = (acc[:m] + r[:m]).astype(f32)
        mix.append(acc)
    ch.close()
    if mixed:
        return [np.concatenate(mix)]
    return [np.concatenate(o) for o in outs]


@pytest.mark.parametrize("nch,mixed", [(1, False), (8, False), (8, True)])
def test_sdr_process_nbfmsync_matches_replay_and_cpp_host(tmp_path, monkeypatch, nch, mixed):
    monkeypatch.setenv("CSDR_QUIET", "1")
    from composable_sdr_amd.app import sdr_process
    k, n = 4, 40000 * nch
    x = synth_cf32(n + 3000, nch, seed=51)
    src = tmp_path / "in.cf32"
    x.tofile(src)
    h = cs.SymSync(k, 4, 0.0, 64)
    banks = h.taps()
    h.close()
    py = sdr_process(str(src), channels=nch, demod="nbfmsync", k=k, mix=mixed, numsamples=n, outname=str(tmp_path / "py"),
                     chunksize=1024, samplerate=2.56e6)
    want = _replay_sync(src, n, 1024, nch, k, mixed, 2.56e6, 0.0, 0.0, banks)
    assert len(py) == len(want) == (1 if (mixed or nch == 1) else nch)
    for p, w in zip(py, want):
        got = np.fromfile(p, dtype=f32)
        assert got.size == w.size and got.size > 0, p
        assert np.array_equal(_bits(got), _bits(w)), p
    exe = host_exe("soapy_sdr_file")
    args = [exe, "--filename", str(src), "-n", str(n), "-c", str(nch), "--demod", "DeNBFMSync", str(k), "-s", "2.56e6",
            "-o", str(tmp_path / "cc")] + (["-m"] if mixed else [])
    r = subprocess.run(args, capture_output=True, text=True, timeout=300, env=dict(os.environ, CSDR_QUIET="1"))
    assert r.returncode == 0, r.stderr
    for p in py:
        q = str(tmp_path / "cc") + os.path.basename(p)[2:]
        assert open(q, "rb").read() == open(p, "rb").read(), q


def test_readme_example_6_recovers_fsk_bits(tmp_path, monkeypatch):
    """soapy-sdr --offset 1.8e3 -b 4.8e3 --demod "DeNBFMSync 4" on a 24 kHz recording: a 1200-baud FSK signal 1.8 kHz above
    the tuned frequency is mixed down, resampled to 4.8 kHz (k = 4 samples per symbol), FM-demodulated and synchronised; the
    decisions at the loop's instants give the transmitted bits after lock"""
    monkeypatch.setenv("CSDR_QUIET", "1")
    from composable_sdr_amd.app import sdr_process
    fs, baud, nsym = 24000.0, 1200.0, 4000
    bb, bits = S.nrz_fsk_iq(nsym, k=int(fs / baud), offset=3.3, ppm=100.0, dev=600.0 / fs, seed=61)
    t = np.arange(bb.size)
    x = (bb * np.exp(2j * np.pi * 1800.0 / fs * t)).astype(np.complex64)
    src = tmp_path / "in.cf32"
    x.tofile(src)
    n = int(x.size * 4800.0 / fs) - 64
    out = sdr_process(str(src), channels=1, demod="nbfmsync", k=4, numsamples=n, outname=str(tmp_path / "ex6"), chunksize=1024,
                      samplerate=fs, bandwidth=4800.0, offset=1800.0)
    y = np.fromfile(out[0], dtype=f32)
    marks = np.zeros(y.size, bool)
    marks[2::2] = True                                        # decim_counter reaches k_out = 2 at outputs 2, 4, 6, ...
    e, m, lag, _ = S.decide(y, marks, bits, 800)
    print(f"example 6: {y.size} outputs, {e} errors in {m} symbols after lock (lag {lag})")
    assert m > 2000 and e == 0
