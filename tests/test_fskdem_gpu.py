"""fskDemodulator (csdr_fskdem_*) on the GPU against the CPU restatement in tests/fsk_restatement.py.

k_fskdem and demod_f32 perform the same f32 operations in the same order (no contraction, one summation order, a table built the
same way, a correctly rounded sqrt), so symbols and energies are compared bit for bit.  Every test runs under a time limit of its
own: a watchdog thread ends the process if a GPU call does not come back."""
import faulthandler
import os
import subprocess

import numpy as np
import pytest

import fsk_restatement as F
from host_exe import host_exe
from synth import channel_centre

pytestmark = pytest.mark.gpu

cs = pytest.importorskip("composable_sdr_amd")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
LIMIT_S = 300

# (m, k, bw) -> K, demod_map: the table of known answers (computed on the CPU from the text of the design)
DESIGNS = [
    ((1, 8, 0.25), 8, [6, 2]),
    ((1, 4, 0.25), 4, [3, 1]),
    ((2, 8, 0.25), 12, [9, 11, 1, 3]),
    ((2, 10, 0.45), 20, [11, 17, 3, 9]),
    ((2, 16, 0.3), 20, [14, 18, 2, 6]),
    ((3, 32, 0.2), 35, [28, 30, 32, 34, 1, 3, 5, 7]),
    ((4, 64, 0.25), 120, list(range(90, 119, 4)) + list(range(2, 31, 4))),
    ((1, 2048, 0.25), 2048, [1536, 512]),
]
# beyond the table: an odd k (8-byte loads), 32 and 256 tones (several passes of 16 tones; the second with repeated bins), a table
# too long for LDS (K = 5000), and a tone that wraps to bin K = bin 0
EXTRA = [(2, 7, 0.3), (5, 64, 0.3), (8, 64, 0.45), (1, 2048, 0.1234), (1, 3, 0.01)]


@pytest.fixture(autouse=True)
def _time_limit(monkeypatch):
    monkeypatch.setenv("CSDR_QUIET", "1")
    faulthandler.dump_traceback_later(LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _noise(shape, seed):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)).astype(np.complex64)


def _fsk(m, k, bw, nsym, snr_db, seed):
    rng = np.random.default_rng(seed)
    sym = rng.integers(0, 1 << m, nsym).astype(np.uint32)
    return F.fskmod(sym, m, k, bw) + F.awgn(nsym * k, snr_db, rng), sym


def _ties(k, nsym, seed):
    """symbols (a, 0, .., b at k / 2, 0, ..): for (1, 4, .25) and (1, 8, .25) (K = k, bins [3, 1] and [6, 2]) sample k / 2 meets the
    same table entry in both bins, so the two sums are the same operations on the same numbers"""
    rng = np.random.default_rng(seed)
    x = np.zeros((nsym, k), np.complex64)
    x[:, 0] = rng.standard_normal(nsym) + 1j * rng.standard_normal(nsym)
    x[:, k // 2] = rng.standard_normal(nsym) + 1j * rng.standard_normal(nsym)
    return x.reshape(-1)


def _check(x, mkb, nchan=1, energy=True):
    m, k, bw = mkb
    x = np.asarray(x, np.complex64)
    n = x.size // nchan
    h = cs.FskDem(m, k, bw, nchan=nchan, max_samples=n)
    got = h.process_rows(x, energy=energy)
    h.close()
    ws, wE = F.demod_f32(x.reshape(nchan, n), m, k, bw)
    gs, gE = got if energy else (got, None)
    assert gs.shape == (nchan, n // k) and gs.dtype == np.uint32
    assert np.array_equal(gs, ws), (mkb, int((gs != ws).sum()))
    if energy:
        assert np.array_equal(_bits(gE), _bits(wE)), (mkb, int((_bits(gE) != _bits(wE)).sum()))
    return gs


@pytest.mark.parametrize("mkb,K,dmap", DESIGNS, ids=[str(d[0]) for d in DESIGNS])
def test_get_design_equals_the_restatement(mkb, K, dmap):
    h = cs.FskDem(*mkb)
    gK, gmap = h.design()
    h.close()
    rK, rmap = F.design(*mkb)
    assert gK == rK == K and gmap.tolist() == rmap.tolist() == dmap


@pytest.mark.parametrize("mkb", [d[0] for d in DESIGNS] + EXTRA, ids=str)
def test_one_stream_bit_identical(mkb):
    m, k, bw = mkb
    nsym = 1500 if k < 1024 else 300                         # not a multiple of the 256 symbols a workgroup takes
    _check(_noise(nsym * k + k // 2, seed=k + m), mkb)       # a tail of k / 2 samples is dropped
    x, sent = _fsk(m, k, bw, nsym, 10.0, seed=3 * k + m)
    got = _check(x, mkb)
    if mkb in [d[0] for d in DESIGNS]:
        assert np.array_equal(got[0], sent)
    _check(np.zeros(3 * k, np.complex64), mkb)


def test_zeros_and_exact_ties_give_the_lower_index():
    s = _check(np.zeros(700 * 8, np.complex64), (1, 8, 0.25))
    assert not s.any()
    for mkb in ((1, 4, 0.25), (1, 8, 0.25)):
        m, k, bw = mkb
        x = _ties(k, 600, seed=k)
        h = cs.FskDem(m, k, bw, max_samples=x.size)
        s, E = h.process_rows(x, energy=True)
        h.close()
        assert np.array_equal(_bits(E[0, :, 0]), _bits(E[0, :, 1])) and E.all()
        assert not s.any()
        _check(x, mkb)


@pytest.mark.parametrize("mkb", [(1, 8, 0.25), (2, 16, 0.3), (4, 64, 0.25), (2, 7, 0.3)], ids=str)
def test_256_streams_bit_identical(mkb):
    m, k, bw = mkb
    C, nsym = 256, 300
    rows = [_fsk(m, k, bw, nsym, 3.0, seed=1000 + r)[0] for r in range(0, C, 2)]
    noise = _noise((C // 2, nsym * k), seed=77)
    tail = 3 if k in (7, 16) else 2                          # an odd row length: every second row starts unaligned (8-byte loads)
    X = np.empty((C, nsym * k + tail), np.complex64)
    X[0::2, :nsym * k] = rows
    X[1::2, :nsym * k] = noise
    X[:, nsym * k:] = 1.0
    got = _check(X, mkb, nchan=C)
    for r in (0, 101, 255):
        one = cs.FskDem(m, k, bw, max_samples=X.shape[1])
        assert np.array_equal(one.process(X[r]), got[r]), r
        one.close()


@pytest.mark.parametrize("mkb", [(1, 8, 0.25), (4, 64, 0.25), (5, 64, 0.3)], ids=str)
def test_symbols_are_the_same_bits_with_and_without_energies(mkb):
    m, k, bw = mkb
    x = _noise((8, 999 * k), seed=5)
    h = cs.FskDem(m, k, bw, nchan=8, max_samples=x.shape[1])
    a = h.process_rows(x)
    b, _ = h.process_rows(x, energy=True)
    c = h.process_rows(x)
    h.close()
    assert np.array_equal(a, b) and np.array_equal(a, c)
    _check(x, mkb, nchan=8, energy=False)


def test_chunking_at_symbol_boundaries_equals_one_call():
    m, k, bw = 2, 16, 0.3
    x = _noise((4, 2000 * k), seed=9)
    one = cs.FskDem(m, k, bw, nchan=4, max_samples=x.shape[1])
    ref, refE = one.process_rows(x, energy=True)
    one.close()
    rng = np.random.default_rng(2)
    h = cs.FskDem(m, k, bw, nchan=4, max_samples=600 * k)
    outs, outE, pos = [], [], 0
    while pos < x.shape[1]:
        c = min(int(rng.choice([1, 2, 3, 17, 255, 256, 257, 600])) * k, x.shape[1] - pos)
        s, E = h.process_rows(x[:, pos:pos + c], energy=True)
        outs.append(s)
        outE.append(E)
        pos += c
    h.close()
    assert np.array_equal(np.concatenate(outs, axis=1), ref)
    assert np.array_equal(_bits(np.concatenate(outE, axis=1)), _bits(refE))


def test_a_tail_shorter_than_a_symbol_is_dropped_not_carried():
    m, k, bw = 2, 16, 0.3
    x = _noise((3, 5000), seed=13)
    h = cs.FskDem(m, k, bw, nchan=3, max_samples=1024)
    pos = 0
    for c in (1000, 15, 16, 17, 1023, 1, 999, 929):
        a = x[:, pos:pos + c]
        got = h.process_rows(a)
        want, _ = F.demod_f32(a, m, k, bw)
        assert got.shape == (3, c // k) and np.array_equal(got, want), c
        pos += c
    h.close()


def _fsk_band(M, m, k, bw, nsym, occupied, pad_frames, seed):
    """a wideband stream of M nsym' k samples whose channels `occupied` carry fskmod signals at their centres (each modulated at
    the wideband rate: k M samples per symbol, tones at +- bw / M), starting pad_frames channel samples into the stream"""
    rng = np.random.default_rng(seed)
    nf = (nsym + 2) * k
    n = M * nf
    t = np.arange(n, dtype=np.float64)
    x = (0.01 / np.sqrt(2.0)) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    sent = {}
    for c in occupied:
        sent[c] = rng.integers(0, 1 << m, nsym).astype(np.uint32)
        bb = F.fskmod(sent[c], m, k * M, bw / M).astype(np.complex128)
        sig = np.zeros(n, np.complex128)
        sig[pad_frames * M:pad_frames * M + bb.size] = bb
        x += sig * np.exp(1j * channel_centre(c, M) * t) / len(occupied)
    return x.astype(np.complex64), sent, nf


@pytest.mark.parametrize("M", [16, 256])
def test_chain_plane_device_to_device(M):
    """DeNo Chain -> process_device on the chain's device plane, no host copy in between.  The analysis bank delays a channel by
    7.5 channel samples (the prototype's 2 x 7 M taps); the signals start k - 7 = 1 channel sample into the stream, so symbol i
    is demodulated as symbol i + 1, half a sample off its window"""
    import torch
    m, k, bw, nsym = 1, 8, 0.25, 254
    occupied = list(range(1, M, 4))
    x, sent, nf = _fsk_band(M, m, k, bw, nsym, occupied, pad_frames=1, seed=M)
    ch = cs.Chain(channels=M, demod="none", max_frames=nf)
    dem = cs.FskDem(m, k, bw, nchan=M, max_samples=nf)
    d_in = torch.from_numpy(x.view(np.float32).copy()).cuda()
    d_mid = torch.empty(2 * M * nf, dtype=torch.float32, device="cuda")
    d_sym = torch.zeros(M * (nf // k), dtype=torch.int32, device="cuda")
    d_e = torch.zeros(M * (nf // k) * 2, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert ch.process_device(d_in.data_ptr(), M * nf, d_mid.data_ptr(), 0) == M * nf
    dem.process_device(d_mid.data_ptr(), nf, d_sym.data_ptr(), d_e.data_ptr(), 0)
    torch.cuda.synchronize()
    rows = d_mid.cpu().numpy().view(np.complex64).reshape(M, nf)
    sym = d_sym.cpu().numpy().view(np.uint32).reshape(M, nf // k)
    E = d_e.cpu().numpy().reshape(M, nf // k, 2)
    ch.close()
    dem.close()
    ws, wE = F.demod_f32(rows, m, k, bw)
    assert np.array_equal(sym, ws) and np.array_equal(_bits(E), _bits(wE))
    errors = sum(int((sym[c, 1:nsym + 1] != sent[c]).sum()) for c in occupied)
    print(f"M = {M}: {errors} symbol errors in {len(occupied)} x {nsym} symbols")
    assert errors == 0


def test_pipe_behind_the_channelizer_equals_the_nchan_handle():
    """mux (replicate nch (fskDemodulator m k bw)) . firpfbchChannelizer nch against one handle of nch streams"""
    M, m, k, bw = 16, 2, 16, 0.3
    x, _, nf = _fsk_band(M, m, k, bw, 60, [1, 5, 9, 13], pad_frames=9, seed=4)
    pipe = cs.compose(cs.mux([cs.fskDemodulator(m, k, bw, max_samples=nf)] * M), cs.firpfbchChannelizer(M, max_frames=nf))
    r = pipe._start()
    a = pipe._process(r, x[:M * (nf // 2)])
    b = pipe._process(r, x[M * (nf // 2):])
    pipe._done(r)
    ch = cs.Chain(channels=M, dc_block=False, max_frames=nf)
    dem = cs.fskDemodulator(m, k, bw, nchan=M, max_samples=nf)
    rd = dem._start()
    wa = dem._process(rd, ch.process(x[:M * (nf // 2)]))
    wb = dem._process(rd, ch.process(x[M * (nf // 2):]))
    dem._done(rd)
    ch.close()
    assert len(a) == len(b) == M and wa.shape == (M, nf // 2 // k)
    for c in range(M):
        assert a[c].dtype == np.uint32 and np.array_equal(a[c], wa[c]) and np.array_equal(b[c], wb[c]), c
    one = cs.fskDemodulator(m, k, bw)
    r1 = one._start()
    assert one._process(r1, _noise(100, 1)).shape == (6,)    # [n] -> [n div k]
    one._done(r1)


def test_errors():
    from composable_sdr_amd import _lib
    for bad in ((0, 8, 0.25), (9, 8, 0.25), (1, 1, 0.25), (1, 2049, 0.25), (1, 8, 0.0), (1, 8, -0.1), (1, 8, 0.5), (1, 8, 0.7)):
        with pytest.raises(cs.CsdrError) as e:
            cs.FskDem(*bad)
        assert e.value.code == _lib.ERR_INVALID, bad
    h = cs.FskDem(1, 8, 0.25, nchan=2, max_samples=64)
    with pytest.raises(cs.CsdrError) as e:
        h.process_rows(np.zeros((2, 65), np.complex64))
    assert e.value.code == _lib.ERR_SIZE
    assert h.process_rows(np.zeros((2, 7), np.complex64)).shape == (2, 0)
    assert h.process_rows(np.zeros((2, 64), np.complex64)).shape == (2, 8)
    h.close()


def test_cpp_pipe_writes_the_same_bytes_as_the_python_pipe(tmp_path):
    m, k, bw, C, n, chunk = 2, 16, 0.3, 5, 4000, 1000
    x = _noise((C, n), seed=21)
    src, dst = tmp_path / "in.cf32", tmp_path / "out.u32"
    x.tofile(src)
    exe = host_exe("fskdem_host")
    r = subprocess.run([exe, str(m), str(k), str(bw), str(C), str(chunk), str(src), str(dst)], capture_output=True, text=True,
                       timeout=120, env=dict(os.environ, CSDR_QUIET="1"))
    assert r.returncode == 0, r.stderr
    pipe = cs.fskDemodulator(m, k, bw, nchan=C, max_samples=chunk)
    rr = pipe._start()
    want = b"".join(pipe._process(rr, x[:, p:p + chunk]).tobytes() for p in range(0, n, chunk))
    pipe._done(rr)
    assert len(want) == 4 * C * 4 * (chunk // k) and open(dst, "rb").read() == want
