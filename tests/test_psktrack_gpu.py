"""pskTracker and symTracker (csdr_psktrack_*) on the GPU against the CPU restatement in
tests/psktrack_restatement.py.  k_psktrack and the restatement perform the same f32 operations in the same order, so every
comparison of streams here is bit for bit.  The GPU is not driven into any fault path; bad arguments are exercised on the host
side only (tests/test_psktrack_cpu.py)."""
import faulthandler
import subprocess

import numpy as np
import pytest

import psktrack_cases as K
import psktrack_restatement as R
import symsyncc_restatement as SC
from host_exe import host_exe

pytestmark = pytest.mark.gpu

cs = pytest.importorskip("composable_sdr_amd")
from composable_sdr_amd import _lib                           # noqa: E402

f32, c64 = np.float32, np.complex64
DD, CM = R.DD, R.CM
SB = 16                                                        # the kernel's LDS staging block (psktrack_common.h)


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(120, exit=True)          # a GPU call that does not come back ends the process
    yield
    faulthandler.cancel_dump_traceback_later()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_rows(got, want, what):
    assert len(got) == len(want), what
    for r, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(_bits(g), _bits(w)), (what, r)


def _gpu_calls(h, X, calls, nxs=None):
    """X [nchan][N] through handle h in calls of the given sizes (nxs: each call's per-row counts): (y per row, symbols per row,
    counts [ncalls][nchan])"""
    ys, ks, counts, pos = [[] for _ in range(h.nchan)], [[] for _ in range(h.nchan)], [], 0
    for i, c in enumerate(calls):
        x = X[:, pos:pos + c]
        y, k, ny = h.process_rows(x if nxs is None else [x[r, :nxs[i][r]] for r in range(h.nchan)], symbols=True)
        pos += c
        counts.append(ny.astype(np.int64))
        for r in range(h.nchan):
            ys[r].append(y[r, :ny[r]])
            ks[r].append(k[r, :ny[r]])
    return [np.concatenate(v) for v in ys], [np.concatenate(v) for v in ks], np.array(counts)


def _state_equal(h, s, rows):
    for r in rows:
        th, fr, p, nsym, w = h.state(r)
        assert (th, fr, nsym) == (int(s.theta[r]), int(s.freq[r]), int(s.nsym[r])), r
        assert _bits(np.array([p], f32))[0] == _bits(s.p[r:r + 1])[0], r
        assert np.array_equal(_bits(w), _bits(s.w[r])), r


@pytest.fixture(scope="module")
def signals():
    """(bits, sps) -> one impaired row through the two-path channel, shared and never written to"""
    out = {}
    for bits in (1, 2):
        for sps in (1, 2):
            X, _, _ = K.rows(4200 if sps == 1 else 2100, bits, sps, seed=20 + bits, channel=K.CHANNELS[0], conditions=[(0.002, 2.0, 0.05)])
            out[bits, sps] = X[0, :4096].copy()
            out[bits, sps].setflags(write=False)
    return out


CASES = [(2, 1, 0, DD), (1, 1, 0, DD), (2, 2, 9, DD), (1, 2, 9, CM), (2, 2, 17, CM), (1, 2, 17, DD)]


@pytest.mark.parametrize("bits,sps,eq_len,mode", CASES)
def test_one_row_equals_the_restatement(signals, bits, sps, eq_len, mode):
    x = signals[bits, sps]
    kw = dict(bits=bits, sps=sps, eq_len=eq_len, eq_mode=mode, eq_delay=100)
    h = cs.PskTrack(nchan=1, max_samples=4096, **kw)
    y, k, ny = h.process_rows(x, symbols=True)
    wy, wk, wc, s = R.run_calls(x, [x.size], **kw)
    assert int(ny[0]) == int(wc[0, 0]) == x.size // sps
    assert np.array_equal(_bits(y[0, :ny[0]]), _bits(wy[0])) and np.array_equal(k[0, :ny[0]], wk[0])
    _state_equal(h, s, [0])
    h.close()
    assert np.abs(s.w[0]).sum() > 1.0 if eq_len else True       # the equaliser has adapted: more than the unit centre tap


@pytest.mark.parametrize("bits,sps,eq_len,mode", [(2, 2, 9, DD), (1, 1, 0, DD)])
def test_chunking_is_bit_identical(signals, bits, sps, eq_len, mode):
    """call sizes from 1 .. 700, odd ones and the staging block +-1 among them, and an empty call, against one call"""
    x = signals[bits, sps]
    rng = np.random.default_rng(5)
    calls = [SB - 1, 333, 0, SB + 1, 1, SB] + rng.integers(1, 701, 64).tolist()
    calls = calls[:int(np.searchsorted(np.cumsum(calls), x.size))]
    calls.append(x.size - sum(calls))
    assert sum(c % 2 for c in calls) >= 4 and 0 in calls and max(calls) <= 700
    kw = dict(bits=bits, sps=sps, eq_len=eq_len, eq_mode=mode, eq_delay=50)
    one = cs.PskTrack(nchan=1, max_samples=4096, **kw)
    y, k, ny = one.process_rows(x, symbols=True)
    want = one.state()
    one.close()
    h = cs.PskTrack(nchan=1, max_samples=700, **kw)
    gy, gk, gc = _gpu_calls(h, x.reshape(1, -1), calls)
    got = h.state()
    h.close()
    assert gc.sum() == ny[0] and gc[2, 0] == 0
    assert np.array_equal(_bits(gy[0]), _bits(y[0, :ny[0]])) and np.array_equal(gk[0], k[0, :ny[0]])
    assert got[:2] == want[:2] and got[3] == want[3] and np.array_equal(_bits(got[4]), _bits(want[4]))


def test_sixty_seven_rows_of_their_own_lengths():
    """a second workgroup with three live lanes; every row its own offset, phase, amplitude and sample counts (0 and n among
    them, odd ones too) over two calls; rows 0, 63, 64, 66 also against one-row handles"""
    C, n = 67, 600
    pts, _ = K.symbols(700, 2, seed=31)
    x2 = K.matched(pts, K.CHANNELS[1])
    X = np.stack([K.impaired(x2, 0.003 * np.sin(r), 0.7 * r, 0.05 * (1 + r % 9) ** 2)[:2 * n] for r in range(C)]).astype(c64)
    rng = np.random.default_rng(8)
    nxs = [rng.integers(0, n + 1, C) for _ in range(2)]
    nxs[0][[0, 1, 2, 66]] = [n, 0, 333, 599]
    nxs[1][[0, 1, 2, 66]] = [n, n, 0, 1]
    kw = dict(bits=2, sps=2, eq_len=9, eq_mode=DD, eq_delay=20)
    h = cs.PskTrack(nchan=C, max_samples=n, **kw)
    gy, gk, gc = _gpu_calls(h, X, [n, n], nxs)
    s = R.PskTrack(C, **kw)
    wy, wk = [[] for _ in range(C)], [[] for _ in range(C)]
    for i in range(2):
        y, k, ny = s.process(X[:, i * n:(i + 1) * n], nxs[i])
        assert gc[i].tolist() == ny.tolist()
        for r in range(C):
            wy[r].append(y[r, :ny[r]])
            wk[r].append(k[r, :ny[r]])
    _same_rows(gy, [np.concatenate(v) for v in wy], "y")
    _same_rows(gk, [np.concatenate(v) for v in wk], "sym")
    _state_equal(h, s, range(C))
    h.close()
    for r in (0, 63, 64, 66):
        one = cs.PskTrack(nchan=1, max_samples=n, **kw)
        y1 = np.concatenate([one.process(X[r, i * n:i * n + nxs[i][r]]) for i in range(2)])
        one.close()
        assert np.array_equal(_bits(y1), _bits(gy[r])), r


def test_device_entry_restart_and_life_cycle(signals):
    import torch
    x = signals[2, 2]
    n = 1024
    kw = dict(bits=2, sps=2, eq_len=9, eq_mode=CM, eq_delay=50)
    host = cs.PskTrack(nchan=1, max_samples=n, **kw)
    first = host.process_rows(x[:n], symbols=True)
    second = host.process_rows(x[n:2 * n], symbols=True)
    dev = cs.PskTrack(nchan=1, max_samples=n, **kw)
    d_x = torch.from_numpy(x[:n].copy().view(f32)).cuda()
    d_y = torch.zeros(2 * n, dtype=torch.float32, device="cuda")
    d_k = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_ny = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dev.process_device(d_x.data_ptr(), n, 0, d_y.data_ptr(), d_k.data_ptr(), d_ny.data_ptr(), 0)
    torch.cuda.synchronize()
    dev.close()
    assert int(d_ny.cpu()[0]) == int(first[2][0]) == n // 2
    assert np.array_equal(_bits(d_y.cpu().numpy().view(c64)[:n // 2]), _bits(first[0][0, :n // 2]))
    assert np.array_equal(d_k.cpu().numpy().astype(np.uint32)[:n // 2], first[1][0, :n // 2])
    for calls_before in (1, 2):                                 # the state sits on either side of the handle's ping-pong
        host.restart()
        assert host.state()[:4] == (0, 0, f32(1), 0) and host.state()[4][4] == 1
        for want in (first, second)[:calls_before]:
            got = host.process_rows(x[:n] if want is first else x[n:2 * n], symbols=True)
            for g, w in zip(got, want):
                assert np.array_equal(_bits(g[..., :n // 2] if g.ndim > 1 else g), _bits(w[..., :n // 2] if w.ndim > 1 else w))
    host.close()
    host.close()
    with pytest.raises(cs.CsdrError) as e:
        host.process(x[:n])
    assert e.value.code == _lib.ERR_INVALID and "already destroyed" in str(e.value)
    for _ in range(3):
        cs.PskTrack(nchan=3, max_samples=64, **kw).close()


def test_host_refuses_a_row_count_above_n():
    h = cs.PskTrack(1, nchan=2, max_samples=64)
    x, y, ny = np.zeros((2, 8), c64), np.zeros((2, 8), c64), np.zeros(2, np.uint32)
    nx = np.array([8, 9], np.uint32)
    rc = h._get("process", x.ctypes.data, 8, nx.ctypes.data, y.ctypes.data, None, ny.ctypes.data)
    assert rc == _lib.ERR_SIZE
    assert h._get("process", x.ctypes.data, 65, None, y.ctypes.data, None, ny.ctypes.data) == _lib.ERR_SIZE
    assert h.state()[3] == 0                                    # a refused call leaves the rows untouched
    h.close()


M_, K_, NSYM = 4, 4, 2048


@pytest.fixture(scope="module")
def composite():
    """the composite case of tests/test_psktrack_cpu.py, truncated to 2048 symbols, three rows of different timing offsets"""
    rows = []
    for r in range(3):
        x, _ = SC.psk(NSYM + 2 * M_ + 2, K_, M_, SC.RRC, 0.25, 1.6 + 0.5 * r, 100.0, bits_per_symbol=1, seed=7 + r)
        rows.append(x * np.exp(2j * np.pi * 0.001 * np.arange(x.size) / K_))
    X = np.stack(rows).astype(c64)
    X.setflags(write=False)
    return X


def _by_hand(X, calls):
    """SymSync then PskTrack through their device entries on one stream, nothing read between: per-row outputs"""
    import torch
    C = X.shape[0]
    nmax = max(calls)
    sync = cs.SymSync(K_, M_, 0.0, 16, nchan=C, max_samples=nmax, lf_bw=0.01, k_out=2)
    sync.set_rnyquist(cs.CSDR_FIRFILT_RRC, 0.25)
    banks = sync.taps()
    track = cs.PskTrack(1, 2, cs.pipes.SYMTRACK_PHASE, 9, eq_mode=CM, nchan=C, max_samples=nmax)
    outs, pos = [[] for _ in range(C)], 0
    stream = torch.cuda.current_stream().cuda_stream
    for n in calls:
        d_x = torch.from_numpy(X[:, pos:pos + n].copy().view(f32)).cuda()
        d_mid = torch.zeros(2 * C * n, dtype=torch.float32, device="cuda")
        d_y = torch.zeros(2 * C * n, dtype=torch.float32, device="cuda")
        d_cnt = torch.zeros(2 * C, dtype=torch.int32, device="cuda")
        sync.process_c_device(d_x.data_ptr(), n, d_mid.data_ptr(), d_cnt[:C].data_ptr(), stream)
        track.process_device(d_mid.data_ptr(), n, d_cnt[:C].data_ptr(), d_y.data_ptr(), 0, d_cnt[C:].data_ptr(), stream)
        torch.cuda.synchronize()
        ny = d_cnt[C:].cpu().numpy()
        y = d_y.cpu().numpy().view(c64).reshape(C, n)
        for r in range(C):
            outs[r].append(y[r, :ny[r]])
        pos += n
    sync.close()
    track.close()
    return [np.concatenate(o) for o in outs], banks


def test_behind_the_synchroniser_equals_the_composed_restatements(composite):
    X = composite
    n = X.shape[1]
    got, banks = _by_hand(X, [n])
    mid, _, _, s = SC.run_calls(X, [n], k=K_, m=M_, M=16, lf_bw=0.01, k_out=2, banks=banks)
    assert not s.fault.any()
    t = R.PskTrack(3, bits=1, sps=2, phase=cs.pipes.SYMTRACK_PHASE, eq_len=9, eq_mode=CM)
    nx = np.array([m.size for m in mid])
    P = np.zeros((3, n), c64)
    for r in range(3):
        P[r, :nx[r]] = mid[r]
    y, _, ny = t.process(P, nx)
    assert ny.min() > NSYM - 40
    _same_rows(got, [y[r, :ny[r]] for r in range(3)], "symsync -> psktrack")


def test_symtracker_pipe_equals_the_objects_and_the_cpp_host(composite, tmp_path):
    X = composite[:, :6000]
    calls = [2000, 2000, 2000]
    want, _ = _by_hand(X, calls)
    pipe = cs.symTracker(M_, K_, nchan=3, max_samples=2000)
    r = pipe._start()
    chunks = [pipe._process(r, X[:, i:i + 2000]) for i in range(0, 6000, 2000)]
    pipe._done(r)
    _same_rows([np.concatenate([ch[c] for ch in chunks]) for c in range(3)], want, "symTracker")
    exe = host_exe("psktrack_host")
    src, dst = tmp_path / "in.cf32", tmp_path / "out.cf32"
    X.astype(c64).tofile(src)
    p = subprocess.run([exe, f"{M_}:{K_}", "3", "2000", str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    blob = b"".join(np.ascontiguousarray(ch[c]).tobytes() for ch in chunks for c in range(3))
    assert len(blob) > 8 * 1300 * 3 and open(dst, "rb").read() == blob
    # the block alone: the pskTracker Pipe on a raw file
    Y = X[:, :3000]
    pipe = cs.pskTracker(2, 2, 0, 9, nchan=3, max_samples=1000)
    r = pipe._start()
    chunks = [pipe._process(r, Y[:, i:i + 1000]) for i in range(0, 3000, 1000)]
    pipe._done(r)
    Y.astype(c64).tofile(src)
    p = subprocess.run([exe, "2:2:0:9:0", "3", "1000", str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    blob = b"".join(np.ascontiguousarray(ch[c]).tobytes() for ch in chunks for c in range(3))
    assert len(blob) == 8 * 500 * 3 * 3 and open(dst, "rb").read() == blob
