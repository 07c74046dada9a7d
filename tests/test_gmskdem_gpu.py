"""gmskDemodulator / firFilterRNyquist (csdr_gmskdem_*) on the GPU: against the f64 restatement in
tests/gmsk_restatement.py within a derived bound, and bit for bit against itself under every cut of a stream, every row count and
both entries.  Every test runs under a time limit of its own: a watchdog thread ends the process if a GPU call does not come back."""
import faulthandler
import os
import subprocess

import numpy as np
import pytest

import gmsk_restatement as G
from host_exe import host_exe
from synth import channel_centre

pytestmark = pytest.mark.gpu

cs = pytest.importorskip("composable_sdr_amd")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
LIMIT_S = 300
S = 256                                      # symbols per workgroup of k_gmskdem for k <= 32 (kernels_gmskdem.hip)
CASES = [(2, 1, 0.3), (4, 3, 0.3), (5, 3, 0.4), (7, 2, 0.5), (64, 8, 0.3)]


@pytest.fixture(autouse=True)
def _time_limit(monkeypatch):
    monkeypatch.setenv("CSDR_QUIET", "1")
    faulthandler.dump_traceback_later(LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _gmsk(kmb, nsym, seed, offset=0.01, snr_db=20.0, amp=1.0, phase0=0.0):
    k, m, bt = kmb
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, nsym)
    return G.gmskmod(bits, k, m, bt, offset=offset, snr_db=snr_db, amp=amp, rng=rng, phase0=phase0), bits


def _one_call(x, kmb, nchan=1):
    """(sym, soft) of one call from fresh state through the host entry"""
    k, m, bt = kmb
    x = np.asarray(x, np.complex64).reshape(nchan, -1)
    h = cs.GmskDem(k, m, bt, nchan=nchan, max_samples=x.shape[1])
    out = h.process_rows(x, soft=True)
    h.close()
    return out


def _in_calls(x, kmb, sizes, nchan=1):
    """(sym, soft) of the stream cut into calls of `sizes` symbols"""
    k, m, bt = kmb
    x = np.asarray(x, np.complex64).reshape(nchan, -1)
    assert sum(sizes) * k == x.shape[1]
    h = cs.GmskDem(k, m, bt, nchan=nchan, max_samples=max(sizes) * k)
    syms, softs, pos = [], [], 0
    for c in sizes:
        s, d = h.process_rows(x[:, pos:pos + c * k], soft=True)
        syms.append(s)
        softs.append(d)
        pos += c * k
    h.close()
    return np.concatenate(syms, axis=1), np.concatenate(softs, axis=1)


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))


@pytest.mark.parametrize("kmb", CASES + [(64, 1, 1.0)], ids=str)
def test_get_design_equals_firdes_gmskrx(kmb):
    k, m, bt = kmb
    h = cs.GmskDem(k, m, bt)
    t = h.design()
    h.close()
    assert t.shape == (2 * k * m + 1,) and np.array_equal(_bits(t), _bits(cs.firdes_gmskrx(k, m, bt)))


@pytest.mark.parametrize("kmb", CASES, ids=str)
def test_one_stream_against_the_restatement(kmb):
    """Measured on an MI355X: the largest |soft - d64| is 0.135 of the bound at (2, 1, .3), 0.055 at (4, 3, .3), 0.053 at
    (5, 3, .4) and (7, 2, .5), 0.003 at (64, 8, .3)"""
    k, m, bt = kmb
    nsym = 700 if k < 64 else 300                                        # three workgroups, the last one partly filled
    # the stream starts in the third quadrant: out of the zero history phi[0] = arg(conj(0) x[0]) = atan2(+0, -0) = pi there (0 in
    # the other three), so that the first symbol d[0] = r[0] phi[0] is a decision too
    x, bits = _gmsk(kmb, nsym, seed=10 * k + m, phase0=-0.75 * np.pi)
    assert x[0].real < 0 and x[0].imag < 0
    r = cs.firdes_gmskrx(k, m, bt)
    G.assert_usable(x, r.size)
    sym, soft = _one_call(x, kmb)
    d64, mag = G.demod(x, r, k)
    tol = G.tolerance(r, mag)
    ratio = float((np.abs(soft.astype(np.float64) - d64) / tol).max())
    print(f"{kmb}: max |soft - d64| / bound = {ratio:.3f}, bound <= {tol.max():.3e}, smallest |d64| = {np.abs(d64).min():.3f}")
    assert ratio <= 1.0
    assert (np.abs(d64) > tol).all()                                     # no symbol is left undecided on these inputs
    assert np.array_equal(sym, (d64 > 0).astype(np.uint32))
    assert np.array_equal(sym, (soft > 0).astype(np.uint32))
    assert np.array_equal(sym[0, 2 * m:], bits[:nsym - 2 * m].astype(np.uint32))   # 20 dB: no bit errors either


@pytest.mark.parametrize("ns", [1, S - 1, S, S + 1, 2 * S + 3])
def test_tile_edges(ns):
    kmb = (4, 3, 0.3)
    total = 2 * S + 3 + ns
    x, _ = _gmsk(kmb, total, seed=ns)
    ref = _one_call(x, kmb)
    assert _same(_in_calls(x, kmb, [ns, total - ns]), ref)               # a call of ns symbols from fresh state, then with a history
    assert _same(_in_calls(x, kmb, [total - ns, ns]), ref)


def test_calls_shorter_than_the_history():
    kmb = (4, 3, 0.3)
    n = 2 * 3 + 3
    x, _ = _gmsk(kmb, n, seed=77)
    assert _same(_in_calls(x, kmb, [1] * n), _one_call(x, kmb))


@pytest.mark.parametrize("kmb", [(5, 3, 0.4), (8, 2, 0.3)], ids=str)
def test_random_call_sizes_equal_one_call(kmb):
    rng = np.random.default_rng(kmb[0])
    sizes = [int(v) for v in rng.integers(1, 2048, 5)] + [1, 2047]
    x, _ = _gmsk(kmb, sum(sizes), seed=3)
    X = np.stack([x, np.roll(x, 17) * f32(0.3)])                         # two rows: the second starts unaligned when n is odd
    assert _same(_in_calls(X, kmb, sizes, nchan=2), _one_call(X, kmb, nchan=2))


def _rows(kmb, C, nsym):
    rng = np.random.default_rng(C)
    X = np.stack([_gmsk(kmb, nsym, seed=500 + c, offset=float(rng.uniform(-0.05, 0.05)), amp=float(10.0 ** rng.uniform(-3, 1)))[0]
                  for c in range(C)])
    X[C // 2] = 0
    return X


def _device_entry(X, kmb, soft=True):
    import torch
    k, m, bt = kmb
    C, n = X.shape
    h = cs.GmskDem(k, m, bt, nchan=C, max_samples=n)
    d_x = torch.from_numpy(X.view(f32).copy()).cuda()
    d_sym = torch.zeros(C * (n // k), dtype=torch.int32, device="cuda")
    d_soft = torch.zeros(C * (n // k), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    h.process_device(d_x.data_ptr(), n, d_sym.data_ptr(), d_soft.data_ptr() if soft else 0, 0)
    torch.cuda.synchronize()
    h.close()
    return d_sym.cpu().numpy().view(np.uint32).reshape(C, n // k), d_soft.cpu().numpy().reshape(C, n // k)


@pytest.mark.parametrize("C", [256, 3])
def test_rows_are_independent_and_both_entries_agree(C):
    kmb = (4, 3, 0.3)
    X = _rows(kmb, C, 300)
    dev = _device_entry(X, kmb)
    assert _same(dev, _one_call(X, kmb, nchan=C))
    assert not dev[0][C // 2].any() and not dev[1][C // 2].any()         # the all-zero row: phi = +0, d = +0, bit 0
    k, m, bt = kmb
    one = cs.GmskDem(k, m, bt, max_samples=X.shape[1])
    for c in range(C):
        s, d = one.process_rows(X[c], soft=True)
        assert np.array_equal(s[0], dev[0][c]) and np.array_equal(_bits(d[0]), _bits(dev[1][c])), c
        one.reset()
    one.close()


def test_symbols_are_the_same_bits_without_soft_values():
    kmb = (5, 3, 0.4)
    X = _rows(kmb, 4, 600)
    k, m, bt = kmb
    h = cs.GmskDem(k, m, bt, nchan=4, max_samples=X.shape[1])
    a = h.process_rows(X)
    h.reset()
    b, _ = h.process_rows(X, soft=True)
    h.close()
    assert np.array_equal(a, b)
    assert np.array_equal(_device_entry(X, kmb, soft=False)[0], a)


def test_reset_gives_the_fresh_state_output_again():
    kmb = (4, 3, 0.3)
    x, _ = _gmsk(kmb, 300, seed=8)
    k, m, bt = kmb
    h = cs.GmskDem(k, m, bt, max_samples=x.size)
    a = h.process_rows(x, soft=True)
    b = h.process_rows(x, soft=True)                                     # with the first pass as history
    h.reset()
    c = h.process_rows(x, soft=True)
    h.close()
    assert _same(a, c) and not np.array_equal(_bits(a[1][0, :6]), _bits(b[1][0, :6]))


def test_errors():
    import ctypes as C
    from composable_sdr_amd import _lib
    kmb = (4, 3, 0.3)
    x, _ = _gmsk(kmb, 40, seed=1)
    ref = _one_call(x, kmb)
    h = cs.GmskDem(4, 3, 0.3, max_samples=96)
    a = h.process_rows(x[:64], soft=True)
    for bad in (x[64:64 + 6], np.zeros(100, np.complex64)):             # not a multiple of k; more than max_samples
        with pytest.raises(cs.CsdrError) as e:
            h.process_rows(bad)
        assert e.value.code == _lib.ERR_SIZE
    with pytest.raises(cs.CsdrError) as e:
        h.process_device(0, 97, 0)                                       # checked before the buffers
    assert e.value.code == _lib.ERR_SIZE
    b = h.process_rows(x[64:], soft=True)                                # the state is what the last good call left
    assert _same((np.concatenate([a[0], b[0]], axis=1), np.concatenate([a[1], b[1]], axis=1)), ref)
    assert h.process_rows(np.zeros(0, np.complex64)).shape == (1, 0)
    n_out, sym = C.c_uint32(), np.zeros(16, np.uint32)
    lib, p = _lib.lib(), lambda v: v.ctypes.data_as(C.c_void_p)            # noqa: E731
    assert lib.csdr_gmskdem_process(h.h, None, 64, p(sym), None, C.byref(n_out)) == _lib.ERR_INVALID
    assert lib.csdr_gmskdem_process(h.h, p(x), 64, None, None, C.byref(n_out)) == _lib.ERR_INVALID
    assert lib.csdr_gmskdem_process(h.h, p(x), 64, p(sym), None, None) == _lib.ERR_INVALID
    assert lib.csdr_gmskdem_process(None, p(x), 64, p(sym), None, C.byref(n_out)) == _lib.ERR_INVALID
    assert lib.csdr_gmskdem_process_device(h.h, None, 64, None, None, None) == _lib.ERR_INVALID
    assert lib.csdr_gmskdem_get_design(None, None, None) == _lib.ERR_INVALID
    assert lib.csdr_gmskdem_reset(None) == _lib.ERR_INVALID
    h.reset()
    assert _same(h.process_rows(x[:64], soft=True), a)                   # none of the refused calls touched the state
    h.close()


def _gmsk_band(M, kmb, nsym, occupied, pad_frames, seed):
    """a wideband stream of M (nsym + 2) k samples whose channels `occupied` carry GMSK at their centres (each modulated at the
    wideband rate: k M samples per symbol), starting pad_frames channel samples into the stream"""
    k, m, bt = kmb
    rng = np.random.default_rng(seed)
    nf = (nsym + 2) * k
    n = M * nf
    t = np.arange(n, dtype=np.float64)
    x = (0.01 / np.sqrt(2.0)) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    sent = {}
    for c in occupied:
        sent[c] = rng.integers(0, 2, nsym).astype(np.uint32)
        bb = G.gmskmod(sent[c], k * M, m, bt).astype(np.complex128)
        sig = np.zeros(n, np.complex128)
        sig[pad_frames * M:pad_frames * M + bb.size] = bb
        x += sig * np.exp(1j * channel_centre(c, M) * t) / len(occupied)
    return x.astype(np.complex64), sent, nf


def test_chain_plane_device_to_device():
    """DeNo Chain -> process_device on the chain's device plane, no host copy in between.  With the signals 2 channel samples into
    the stream the analysis bank's delay puts symbol i at the output of symbol i + 2 m + 1"""
    import torch
    M, kmb, nsym = 16, (8, 3, 0.3), 120
    k, m, bt = kmb
    occupied = [3, 10]
    x, sent, nf = _gmsk_band(M, kmb, nsym, occupied, pad_frames=2, seed=5)
    ch = cs.Chain(channels=M, demod="none", max_frames=nf)
    dem = cs.GmskDem(k, m, bt, nchan=M, max_samples=nf)
    d_in = torch.from_numpy(x.view(np.float32).copy()).cuda()
    d_mid = torch.empty(2 * M * nf, dtype=torch.float32, device="cuda")
    d_sym = torch.zeros(M * (nf // k), dtype=torch.int32, device="cuda")
    d_soft = torch.zeros(M * (nf // k), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert ch.process_device(d_in.data_ptr(), M * nf, d_mid.data_ptr(), 0) == M * nf
    dem.process_device(d_mid.data_ptr(), nf, d_sym.data_ptr(), d_soft.data_ptr(), 0)
    torch.cuda.synchronize()
    sym = d_sym.cpu().numpy().view(np.uint32).reshape(M, nf // k)
    soft = d_soft.cpu().numpy().reshape(M, nf // k)
    ch.close()
    dem.close()
    ch = cs.Chain(channels=M, demod="none", max_frames=nf)               # the host-path composition
    rows = ch.process(x)
    ch.close()
    assert _same((sym, soft), _one_call(rows, kmb, nchan=M))
    dl = 2 * m + 1
    nc = nf // k - dl
    errors = sum(int((sym[c, dl:] != sent[c][:nc]).sum()) for c in occupied)
    print(f"{errors} bit errors in {len(occupied)} x {nc} symbols")
    assert errors == 0


def test_fir_filter_r_nyquist_and_the_argument_order():
    rng = np.random.default_rng(6)
    x = rng.standard_normal((2, 3000)).astype(f32)
    outs = []
    for pipe in (cs.firFilterRNyquist(4, 3, 0.3, nchan=2), cs.firFilterR(cs.firdes_gmskrx(4, 3, 0.3), 0.25, nchan=2)):
        r = pipe._start()
        outs.append(np.concatenate([pipe._process(r, x[:, :1001]), pipe._process(r, x[:, 1001:])], axis=1))
        pipe._done(r)
    assert outs[0].shape == x.shape and np.array_equal(_bits(outs[0]), _bits(outs[1]))
    pipe = cs.gmskDemodulator(3, 8, 0.3)                                 # m, k: 64 samples are 8 symbols
    r = pipe._start()
    y = pipe._process(r, _gmsk((8, 3, 0.3), 8, seed=2)[0])
    pipe._done(r)
    assert y.shape == (8,) and y.dtype == np.uint32


def test_cpp_pipe_writes_the_same_bytes_as_the_python_pipe(tmp_path):
    m, k, bw, C, chunk = 3, 4, 0.3, 5, 1000
    n = 4 * chunk
    x = _rows((k, m, bw), C, n // k)
    src, dst = tmp_path / "in.cf32", tmp_path / "out.u32"
    x.tofile(src)
    exe = host_exe("gmskdem_host")
    r = subprocess.run([exe, str(m), str(k), str(bw), str(C), str(chunk), str(src), str(dst)], capture_output=True, text=True,
                       timeout=120, env=dict(os.environ, CSDR_QUIET="1"))
    assert r.returncode == 0, r.stderr
    pipe = cs.gmskDemodulator(m, k, bw, nchan=C, max_samples=chunk)
    rr = pipe._start()
    want = b"".join(pipe._process(rr, x[:, p:p + chunk]).tobytes() for p in range(0, n, chunk))
    pipe._done(rr)
    assert len(want) == 4 * C * 4 * (chunk // k) and open(dst, "rb").read() == want
