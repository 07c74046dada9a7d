"""Complex symbol timing recovery (csdr_symsync_set_* / csdr_symsync_process_c*) on the GPU against the CPU
restatement in tests/symsyncc_restatement.py.

k_symsyncc and the restatement perform the same f32 operations in the same order, so every comparison of streams here is bit
for bit.  The restatement takes the handle's banks (get_taps); the design is compared separately, within the bound
tests/test_symsync_gpu.py uses for its banks."""
import faulthandler
import os
import subprocess

import numpy as np
import pytest

import symsync_restatement as S
import symsyncc_restatement as R
from host_exe import host_exe
from synth import synth_cf32

pytestmark = pytest.mark.gpu

cs = pytest.importorskip("composable_sdr_amd")
from composable_sdr_amd import _lib                           # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, c64 = np.float32, np.complex64
ARK, RRC = R.ARKAISER, R.RRC


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(120, exit=True)          # a GPU call that does not come back ends the process
    yield
    faulthandler.cancel_dump_traceback_later()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _make(k, m, npfb, k_out=1, nchan=1, max_samples=4096, ftype=ARK, beta=0.5, lf_bw=0.01):
    h = cs.SymSync(k, m, 0.0, npfb, nchan=nchan, max_samples=max_samples, lf_bw=lf_bw, k_out=k_out)
    h.set_rnyquist(ftype, beta)
    return h


def _gpu_calls(h, X, calls):
    """X [nchan][N] complex through handle h in calls of the given sizes: (per-stream outputs, counts [ncalls][nchan])"""
    outs = [[] for _ in range(h.nchan)]
    counts, pos = [], 0
    for c in calls:
        y, ny = h.process_c(X[:, pos:pos + c])
        pos += c
        counts.append(ny.astype(np.int64))
        for r in range(h.nchan):
            outs[r].append(y[r, :ny[r]])
    return [np.concatenate(o) for o in outs], np.array(counts)


@pytest.fixture(scope="module")
def qpsk():
    """one QPSK stream per k, shared and never written to"""
    out = {k: R.psk(4096 // k + 40, k, seed=10 + k)[0] for k in (2, 4)}
    for v in out.values():
        v.setflags(write=False)
    return out


@pytest.mark.parametrize("k,m,npfb,ftype,beta", [(2, 3, 32, ARK, 0.5), (4, 4, 64, RRC, 0.35)])
def test_banks_after_set_rnyquist_match_the_restatement(k, m, npfb, ftype, beta):
    h = _make(k, m, npfb, ftype=ftype, beta=beta)
    mf, dmf = h.taps()
    h.close()
    P = R.design(k, m, npfb, 0.01, 1, ftype, float(f32(beta)))
    assert mf.shape == (2 * k * m, npfb)
    print(f"banks: {np.mean(mf == P['mf']):.4f} / {np.mean(dmf == P['dmf']):.4f} of the taps bitwise equal")
    np.testing.assert_allclose(mf, P["mf"], rtol=0, atol=2e-7 * np.abs(P["mf"]).max())
    np.testing.assert_allclose(dmf, P["dmf"], rtol=0, atol=2e-7 * np.abs(P["dmf"]).max())


@pytest.mark.parametrize("k,m,npfb,k_out,n", [(2, 3, 32, 1, 4096), (4, 4, 64, 1, 2048), (4, 4, 64, 2, 2048)])
def test_one_stream_matches_restatement(qpsk, k, m, npfb, k_out, n):
    x = qpsk[k][:n]
    h = _make(k, m, npfb, k_out, max_samples=n)
    got, gc = _gpu_calls(h, x.reshape(1, -1), [n])
    st = h.state(0)
    want, wc, _, s = R.run_calls(x, [n], k=k, m=m, M=npfb, k_out=k_out, banks=h.taps())
    h.close()
    assert np.array_equal(gc, wc) and got[0].size > n * k_out // k - 8
    assert np.array_equal(_bits(got[0]), _bits(want[0]))
    assert _bits(np.array(st, f32)).tolist() == _bits(np.array([s.tau[0], s.rate[0], s.dl[0], s.q_hat[0]], f32)).tolist()
    print(f"({k},{m},{npfb},k_out {k_out}): {got[0].size} outputs bit-identical, tau {st[0]:.6f} rate {st[1]:.6f} del {st[2]:.6f}")


def test_random_call_sizes_and_an_empty_call_equal_one_call(qpsk):
    x = qpsk[2][:4001]
    one = _make(2, 3, 32, max_samples=x.size)
    ref, _ = _gpu_calls(one, x.reshape(1, -1), [x.size])
    one.close()
    rng = np.random.default_rng(7)
    calls, pos = [], 0
    while pos < x.size:
        c = min(int(rng.integers(1, 701)), x.size - pos)
        calls.append(c)
        pos += c
    calls.insert(3, 0)
    assert any(c % 2 for c in calls) and max(calls) > 64
    h = _make(2, 3, 32, max_samples=700)
    got, gc = _gpu_calls(h, x.reshape(1, -1), calls)
    h.close()
    assert gc[3, 0] == 0
    assert np.array_equal(_bits(got[0]), _bits(ref[0]))


def test_67_streams_match_restatement_and_single_handles():
    """a second workgroup with three live lanes; offsets, drifts and amplitudes differ per stream"""
    C, n = 67, 1200
    rows = []
    for r in range(C):
        x, _ = R.psk(n // 2 + 40, 2, offset=(r * 0.137) % 2.0, ppm=-300.0 + 600.0 * r / (C - 1), seed=100 + r, amp=0.25 + 0.05 * r)
        rows.append(x[:n])
    X = np.stack(rows)
    calls = [500, 700]
    h = _make(2, 3, 32, nchan=C, max_samples=700)
    got, gc = _gpu_calls(h, X, calls)
    banks = h.taps()
    h.close()
    want, wc, _, _ = R.run_calls(X, calls, k=2, m=3, M=32, banks=banks)
    assert np.array_equal(gc, wc)
    for r in range(C):
        assert np.array_equal(_bits(got[r]), _bits(want[r])), r
    for r in (0, 63, 64, 66):
        one = _make(2, 3, 32, max_samples=700)
        g1, _ = _gpu_calls(one, X[r:r + 1], calls)
        one.close()
        assert np.array_equal(_bits(g1[0]), _bits(got[r])), r


def test_chain_rows_device_to_device():
    """Chain(channels=8, demod="none") CF32 rows -> process_c_device (device to device) equals the host path on the same rows"""
    import torch
    M, nf = 8, 2048
    x = synth_cf32(M * nf, M, seed=41)
    ch = cs.Chain(channels=M, demod="none", max_frames=nf)
    dev = _make(2, 3, 32, nchan=M, max_samples=nf)
    d_in = torch.from_numpy(x.view(np.float32).copy()).cuda()
    d_mid = torch.empty(2 * M * nf, dtype=torch.float32, device="cuda")
    d_y = torch.zeros(2 * M * nf, dtype=torch.float32, device="cuda")
    d_ny = torch.zeros(M, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert ch.process_device(d_in.data_ptr(), M * nf, d_mid.data_ptr(), 0) == M * nf
    dev.process_c_device(d_mid.data_ptr(), nf, d_y.data_ptr(), d_ny.data_ptr(), 0)
    torch.cuda.synchronize()
    ny = d_ny.cpu().numpy()
    y = d_y.cpu().numpy().view(c64).reshape(M, nf)
    mid = d_mid.cpu().numpy().view(c64).reshape(M, nf)
    ch.close()
    dev.close()
    host = _make(2, 3, 32, nchan=M, max_samples=nf)
    hy, hny = host.process_c(mid)
    host.close()
    assert np.array_equal(ny, hny.astype(np.int32)) and ny.min() > nf // 2 - 8
    for r in range(M):
        assert np.array_equal(_bits(y[r, :ny[r]]), _bits(hy[r, :hny[r]])), r


def test_real_rows_after_set_rnyquist_match_the_real_restatement(qpsk):
    """symsync_rrrf_create_rnyquist for free: the old process on F32 rows with the new banks"""
    x = np.ascontiguousarray(qpsk[4].real[:2048] * f32(1.3), f32)
    h = _make(4, 3, 32, k_out=2, ftype=RRC, beta=0.35, lf_bw=0.05, max_samples=1024)
    y1, n1 = h.process_rows(x[:1024])
    y2, n2 = h.process_rows(x[1024:])
    banks = h.taps()
    h.close()
    want, wc, _, _ = S.run_calls(x, [1024, 1024], k=4, m=3, M=32, lf_bw=0.05, k_out=2, banks=banks)
    assert [int(n1[0]), int(n2[0])] == wc[:, 0].tolist()
    got = np.concatenate([y1[0, :n1[0]], y2[0, :n2[0]]])
    assert got.size > 1000 and np.array_equal(_bits(got), _bits(want[0]))


def test_set_taps_with_the_kaiser_prototype_reproduces_creates_banks():
    """the prototype is read back from create's matched-filter bank; its last tap, which no bank holds, is the first one (the
    Kaiser prototype is symmetric bit for bit)"""
    h = cs.SymSync(4, 4, 0.0, 64)
    mf, dmf = h.taps()
    L, M = mf.shape
    H = np.empty(L * M + 1, f32)
    H[:L * M] = mf[::-1].reshape(-1)                          # mf[j][p] = H[p + (L - 1 - j) M]
    H[L * M] = H[0]
    assert np.array_equal(H[:L * M], H[1:][::-1])
    h.set_taps(H * f32(0.5))                                  # other banks in between
    assert not np.array_equal(h.taps()[0], mf)
    h.set_taps(H)
    mf2, dmf2 = h.taps()
    h.close()
    assert np.array_equal(_bits(mf2), _bits(mf)) and np.array_equal(_bits(dmf2), _bits(dmf))


def test_after_a_setter_or_reset_the_handle_equals_a_fresh_one(qpsk):
    x = qpsk[2][:1500].reshape(1, -1)
    fresh = _make(2, 3, 32, max_samples=1500)
    ref, rc = _gpu_calls(fresh, x, [1500])
    banks = fresh.taps()
    fresh.close()
    h = _make(2, 3, 32, ftype=RRC, beta=0.35, max_samples=1500)
    h.process_c(x[:, :700])                                   # other banks, a state in mid-stream
    proto = cs.firdes_rnyquist(ARK, 2 * 32, 3, 0.5)           # what set_rnyquist hands to set_taps
    for what, redo in [("set_rnyquist", lambda: h.set_rnyquist(ARK, 0.5)), ("reset", h.reset), ("set_taps", lambda: h.set_taps(proto))]:
        redo()
        assert all(np.array_equal(_bits(g), _bits(w)) for g, w in zip(h.taps(), banks)), what
        assert h.state(0) == (f32(0), f32(2), f32(2), f32(0)), what
        got, gc = _gpu_calls(h, x, [1500])
        assert np.array_equal(gc, rc) and np.array_equal(_bits(got[0]), _bits(ref[0])), what
    h.close()


def test_mixed_real_and_complex_calls_are_refused_and_change_nothing(qpsk):
    x = qpsk[2][:2000].reshape(1, -1)
    ref = _make(2, 3, 32, max_samples=1000)
    want, _ = _gpu_calls(ref, x, [1000, 1000])
    ref.close()
    h = _make(2, 3, 32, max_samples=1000)
    y1, n1 = h.process_c(x[:, :1000])
    with pytest.raises(cs.CsdrError) as e:
        h.process_rows(np.ones(100, f32))
    assert e.value.code == _lib.ERR_INVALID and "CF32" in str(e.value)
    y2, n2 = h.process_c(x[:, 1000:])
    got = np.concatenate([y1[0, :n1[0]], y2[0, :n2[0]]])
    assert np.array_equal(_bits(got), _bits(want[0]))
    # the other way round, after reset has reopened the choice
    h.reset()
    r = np.ascontiguousarray(x.real[0, :1000])
    a, na = h.process_rows(r)
    with pytest.raises(cs.CsdrError) as e:
        h.process_c(x[:, :100])
    assert e.value.code == _lib.ERR_INVALID and "F32" in str(e.value)
    b, nb = h.process_rows(r)
    banks = h.taps()
    h.close()
    w, wc, _, _ = S.run_calls(np.concatenate([r, r]), [1000, 1000], k=2, m=3, M=32, lf_bw=0.01, k_out=1, banks=banks)
    assert np.array_equal(_bits(np.concatenate([a[0, :na[0]], b[0, :nb[0]]])), _bits(w[0]))


def test_a_handle_beyond_the_complex_lds_rule_still_serves_real_rows(qpsk):
    """(k, m, npfb) = (4, 8, 64): 8 * 64 * 64 + 512 * 95 = 81408 bytes > 65536"""
    h = cs.SymSync(4, 8, 0.0, 64, max_samples=512)
    with pytest.raises(cs.CsdrError) as e:
        h.process_c(qpsk[4][:512])
    assert e.value.code == _lib.ERR_INVALID and "65536" in str(e.value)
    r = np.ascontiguousarray(qpsk[4].real[:512])
    y, ny = h.process_rows(r)
    banks = h.taps()
    h.close()
    w, wc, _, _ = S.run_calls(r, [512], k=4, m=8, M=64, banks=banks)
    assert ny[0] == wc[0, 0] and np.array_equal(_bits(y[0, :ny[0]]), _bits(w[0]))
    # the largest handles the rule promises
    for k, m, npfb in [(4, 8, 32), (4, 4, 64)]:
        g = _make(k, m, npfb, max_samples=512)
        y, ny = g.process_c(qpsk[4][:512])
        g.close()
        assert 100 < ny[0] <= 512


def test_pipe_over_three_chunks_equals_the_object_and_the_cpp_host(tmp_path):
    C, n = 3, 1500
    X = np.stack([R.psk(n // 2 + 40, 2, offset=0.3 * r, ppm=100.0 * r, seed=70 + r)[0][:n] for r in range(C)])
    calls = [500, 500, 500]
    pipe = cs.symSyncC(3, 2, nchan=C, max_samples=500)
    r = pipe._start()
    chunks = [pipe._process(r, X[:, i:i + 500]) for i in range(0, n, 500)]
    pipe._done(r)
    obj = _make(2, 3, 32, nchan=C, max_samples=500)
    got, gc = _gpu_calls(obj, X, calls)
    obj.close()
    for c in range(C):
        assert np.array_equal(_bits(np.concatenate([ch[c] for ch in chunks])), _bits(got[c])), c
    exe = host_exe("symsyncc_host")
    src, dst = tmp_path / "in.cf32", tmp_path / "out.cf32"
    X.astype(c64).tofile(src)
    p = subprocess.run([exe, "3", "2", str(C), "500", str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    want = b"".join(np.ascontiguousarray(ch[c]).tobytes() for ch in chunks for c in range(C))
    assert len(want) > 8 * 700 * C and open(dst, "rb").read() == want


def test_life_cycle_of_a_complex_handle(qpsk):
    """tests/test_block_lifecycle_gpu.py's shape for a complex SymSync: two handles are independent, close is idempotent and a
    closed object refuses"""
    x = qpsk[2]
    x1, x2 = np.stack([x[:1500], x[100:1600], x[200:1700]]), np.stack([x[1500:2000], x[1600:2100], x[1700:2200]])
    run = lambda h, v: h.process_c(v)                          # noqa: E731

    def same(g, w, what):
        assert g[1].tolist() == w[1].tolist() and g[1].min() > 0, what
        for r in range(3):
            assert np.array_equal(_bits(g[0][r, :g[1][r]]), _bits(w[0][r, :w[1][r]])), what
    make = lambda: _make(2, 3, 32, nchan=3, max_samples=1500)  # noqa: E731
    a, b = make(), make()
    same(run(a, x1), run(b, x1), "two fresh handles, the same input")
    b.close()
    got = run(a, x2)
    c = make()
    run(c, x1)
    same(got, run(c, x2), "the survivor of a destroy against a third fresh handle")
    for h in (a, b, c):
        h.close()
        h.close()
    for h in (a, b, c):
        for use in (lambda: h.h, lambda: run(h, x1), lambda: h.set_rnyquist(ARK, 0.5)):
            with pytest.raises(cs.CsdrError) as e:
                use()
            assert e.value.code == _lib.ERR_INVALID and "already destroyed" in str(e.value)
    for _ in range(3):
        make().close()
