"""The FIR filter (csdr_firfilt_*) on the GPU against the CPU restatement in tests/fir_restatement.py.

k_firfilt and filter_f32 perform the same f32 operations in the same order (no contraction, acc = +0 and the taps in the order
0 .. L - 1, the scale last), so outputs are compared bit for bit.  Every test runs under a time limit of its own: a watchdog
thread ends the process if a GPU call does not come back."""
import faulthandler
import os
import subprocess

import numpy as np
import pytest

import fir_restatement as R
from host_exe import host_exe
from synth import channel_centre

pytestmark = pytest.mark.gpu

cs = pytest.importorskip("composable_sdr_amd")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
LIMIT_S = 300


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype in (np.float32, np.complex64), a.dtype
    return a.view(np.uint32)


def _same(got, want, what=""):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    g, w = _bits(got), _bits(want)
    assert np.array_equal(g, w), (what, int((g != w).sum()), g.size)


def _noise(shape, cplx, seed):
    rng = np.random.default_rng(seed)
    if cplx:
        return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)).astype(np.complex64)
    return rng.standard_normal(shape).astype(f32)


def _make(L, cplx, nchan, max_samples):
    """the Kaiser creator where the design exists (L >= 2 and not degenerate), noise taps through the taps creator otherwise"""
    if L >= 8:
        return cs.FirFilt.kaiser(L, 0.1, 60.0, is_complex=cplx, nchan=nchan, max_samples=max_samples)
    taps = np.random.default_rng(L).standard_normal(L).astype(f32)
    return cs.FirFilt(taps, 0.75, is_complex=cplx, nchan=nchan, max_samples=max_samples)


def test_taps_are_what_the_design_function_returns_and_what_was_given():
    for n, fc, As in ((21, 0.25, 60.0), (65, 0.05, 60.0), (889, 800.0 / 1.2e6, 60.0), (2048, 0.1, 80.0)):
        h = cs.FirFilt.kaiser(n, fc, As, is_complex=False)
        taps, scale = h.taps()
        assert h.taps_len == n
        h.close()
        _same(taps, cs.firdes_kaiser(n, fc, As))
        assert scale == f32(2) * f32(fc) and scale.dtype == np.float32
    given = np.random.default_rng(0).standard_normal(77).astype(f32)
    for cplx in (False, True):
        h = cs.FirFilt(given, -1.25, is_complex=cplx, nchan=3)
        taps, scale = h.taps()
        h.close()
        _same(taps, given)
        assert scale == f32(-1.25)


@pytest.mark.parametrize("nchan", [1, 3, 256])
@pytest.mark.parametrize("L", [1, 2, 21, 64, 65, 255, 889, 2048])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_outputs_bit_identical_to_the_restatement(cplx, L, nchan):
    """noise (a call whose rows take 16-byte accesses and end inside a tile, then an odd-sized one that continues it), after a reset
    an impulse per row and a call of zeros behind it"""
    n1, n2 = 5096, 2333 if nchan < 256 else 1111
    h = _make(L, cplx, nchan, n1)
    taps, scale = h.taps()
    x = _noise((nchan, n1 + n2), cplx, seed=1000 * L + nchan + cplx)
    want, _ = R.filter_f32(taps, scale, x)
    _same(h.process(x[:, :n1]), want[:, :n1], "noise, first call")
    _same(h.process(x[:, n1:]), want[:, n1:], "noise, second call")
    h.reset()
    ni = L + 9
    imp = np.zeros((nchan, ni), x.dtype)
    pos = np.arange(nchan) % 3
    imp[np.arange(nchan), pos] = 1.0
    y = h.process(imp)
    w, hist = R.filter_f32(taps, scale, imp)
    _same(y, w, "impulse")
    resp = f32(scale) * (f32(0) + taps)                      # exactly s * (0 + h[i])
    for c in (0, 1 % nchan, nchan - 1):
        _same(np.ascontiguousarray(y[c, pos[c]:pos[c] + L].real), resp, "impulse response")
        assert not y[c, :pos[c]].any() and not y[c, pos[c] + L:].any()
        if cplx:
            assert not y[c].imag.any()
    z = h.process(np.zeros((nchan, 37), x.dtype))
    _same(z, R.filter_f32(taps, scale, np.zeros((nchan, 37), x.dtype), hist)[0], "zeros")
    zz = h.process(np.zeros((nchan, L + 3), x.dtype))
    assert not zz[:, L:].any()
    h.close()
    if nchan == 1:
        one = _make(L, cplx, 1, n1)
        got = one.process(x[0, :n1])                          # a 1-D array in gives a 1-D array out
        one.close()
        _same(got, want[0, :n1], "1-D")


@pytest.mark.parametrize("cplx,L,nchan", [(True, 65, 3), (False, 255, 2), (True, 2048, 1), (False, 2, 5)])
def test_one_call_equals_many_and_reset_gives_the_create_state(cplx, L, nchan):
    cuts = [0, 1, 7, 333, 20, 30, 10, 64, 4096, 2049, 1, 0, 5, 100, 101, 33, 4096, 777]     # max_samples itself; 20, 30, 10 (and
    if L > 200:                                                                             # more for long filters) below L - 1,
        cuts = cuts[:4] + [150, 199, 3, 180] + cuts[4:]                                     # back to back
    total = sum(cuts)
    x = _noise((nchan, total), cplx, seed=L)
    one = _make(L, cplx, nchan, total)
    taps, scale = one.taps()
    ref = one.process(x)
    one.close()
    _same(ref, R.filter_f32(taps, scale, x)[0], "one call")
    h = _make(L, cplx, nchan, 4096)
    outs, pos = [], 0
    for c in cuts:
        y = h.process(x[:, pos:pos + c])
        assert y.shape == (nchan, c)
        outs.append(y)
        pos += c
    _same(np.concatenate(outs, axis=1), ref, "many calls")
    h.reset()
    pos = 0
    for c, first in zip(cuts[:6], outs[:6]):
        _same(h.process(x[:, pos:pos + c]), first, "after reset")
        pos += c
    h.close()


def _tone_band(M, nf, chan, f, seed):
    """M nf wideband samples: one tone of amplitude 1 that channel `chan` sees at f cycles per channel sample, over white noise of
    1e-5 (so that every row holds something)"""
    rng = np.random.default_rng(seed)
    n = M * nf
    t = np.arange(n, dtype=np.float64)
    x = (1e-5 / np.sqrt(2.0)) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    x += np.exp(1j * (channel_centre(chan, M) + 2.0 * np.pi * f / M) * t)
    return x.astype(np.complex64)


@pytest.mark.parametrize("M", [16, 256])
def test_chain_plane_device_to_device(M):
    """DeNo Chain -> process_device on the chain's device plane, no host copy in between: bit-identical to the restatement of the
    chain's own rows, and the tone of one channel leaves with |H(f)| times its amplitude.

    The amplitude of a tone at f is taken as |mean(row[t] e^{-2 pi j f t})| over a window of W samples.  f = 1 / 32 and W = 1024
    make f W an integer, so the window holds whole periods and a steady tone projects onto itself without leakage; it starts at
    t0 = 256, behind the analysis bank's start-up (14 channel samples) plus the filter's 64 samples of history, so both rows are
    in steady state.  What is left is the 1e-5 noise floor, 1e-5 / sqrt(W) after the projection, and the f32 rounding of the
    filter (4e-6 sum |h| |x| for L = 65): far inside the 1e-4 asked."""
    import torch
    L, fc, f, chan = 65, 0.05, 1.0 / 32.0, 5
    t0, W = 256, 1024
    nf = 2048
    x = _tone_band(M, nf, chan, f, seed=M)
    ch = cs.Chain(channels=M, demod="none", max_frames=nf)
    fir = cs.FirFilt.kaiser(L, fc, 60.0, is_complex=True, nchan=M, max_samples=nf)
    taps, scale = fir.taps()
    d_in = torch.from_numpy(x.view(np.float32).copy()).cuda()
    d_mid = torch.empty(2 * M * nf, dtype=torch.float32, device="cuda")
    d_out = torch.zeros(2 * M * nf, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert ch.process_device(d_in.data_ptr(), M * nf, d_mid.data_ptr(), 0) == M * nf
    fir.process_device(d_mid.data_ptr(), nf, d_out.data_ptr(), 0)
    torch.cuda.synchronize()
    rows = d_mid.cpu().numpy().view(np.complex64).reshape(M, nf)
    got = d_out.cpu().numpy().view(np.complex64).reshape(M, nf)
    ch.close()
    fir.close()
    _same(got, R.filter_f32(taps, scale, rows)[0], f"M = {M}")
    ph = np.exp(-2j * np.pi * f * np.arange(t0, t0 + W))
    a_in = abs(np.mean(rows[chan, t0:t0 + W].astype(np.complex128) * ph))
    a_out = abs(np.mean(got[chan, t0:t0 + W].astype(np.complex128) * ph))
    rms_in = np.sqrt(np.mean(np.abs(rows[chan, t0:t0 + W].astype(np.complex128)) ** 2))
    Hf = abs(R.response(taps, scale, f))
    print(f"M = {M}: tone amplitude in {a_in:.6f} (row rms {rms_in:.6f}), out {a_out:.6f}, ratio {a_out / a_in:.7f}, |H(f)| {Hf:.7f}, "
          f"relative difference {abs(a_out / a_in - Hf) / Hf:.2e}")
    assert a_in > 0.5 * rms_in and a_in > 1e-3               # the row is that tone
    assert abs(a_out / a_in - Hf) <= 1e-4 * Hf


def test_pipe_behind_the_channelizer_equals_the_nchan_handle():
    """mux (replicate nch (firFilterC ..)) . firpfbchChannelizer nch against one handle of nch rows"""
    M, nf, L = 16, 600, 33
    taps = cs.firdes_kaiser(L, 0.2, 60.0)
    x = _tone_band(M, nf, 3, 0.05, seed=4) + 0.1 * _noise(M * nf, True, seed=5)
    pipe = cs.compose(cs.mux([cs.firFilterC(taps, 0.4, max_samples=nf)] * M), cs.firpfbchChannelizer(M, max_frames=nf))
    r = pipe._start()
    a = pipe._process(r, x[:M * 250])
    b = pipe._process(r, x[M * 250:])
    pipe._done(r)
    ch = cs.Chain(channels=M, dc_block=False, max_frames=nf)
    fir = cs.firFilterC(taps, 0.4, nchan=M, max_samples=nf)
    rf = fir._start()
    wa = fir._process(rf, np.asarray(ch.process(x[:M * 250])).reshape(M, -1))
    wb = fir._process(rf, np.asarray(ch.process(x[M * 250:])).reshape(M, -1))
    fir._done(rf)
    ch.close()
    assert len(a) == len(b) == M and wa.shape == (M, 250) and wb.shape == (M, nf - 250)
    for c in range(M):
        _same(np.asarray(a[c]), wa[c], c)
        _same(np.asarray(b[c]), wb[c], c)
    k = cs.firFilterCKaiser(21, 0.1)
    rk = k._start()
    assert k._process(rk, _noise(100, True, 1)).shape == (100,)
    k._done(rk)


def test_firFilterR_against_firDecimator_1():
    """existing product code: firDecimator 1 is the 21 taps of firdes_kaiser(21, 0.5, 60) at decimation 1, summed with fma.  Both
    round the same exact sum, in different ways: |a - b| <= 2 (L + 2) 2^-24 sum |h| max |x|"""
    L = 21
    taps = cs.firdes_kaiser(L, 0.5, 60.0)
    x = _noise((4, 9209), False, seed=8)
    a, b = cs.firFilterR(taps, 1.0, nchan=4, max_samples=4096), cs.firDecimator(1, nchan=4, max_samples=4096)
    ra, rb = a._start(), b._start()
    bound = 2.0 * (L + 2) * 2.0 ** -24 * float(np.abs(taps.astype(np.float64)).sum()) * float(np.abs(x).max())
    worst, pos = 0.0, 0
    for c in (1000, 4096, 17, 4096):
        ya, yb = a._process(ra, x[:, pos:pos + c]), b._process(rb, x[:, pos:pos + c])
        assert ya.shape == yb.shape == (4, c)
        worst = max(worst, float(np.abs(ya.astype(np.float64) - yb.astype(np.float64)).max()))
        pos += c
    a._done(ra)
    b._done(rb)
    print(f"firFilterR against firDecimator 1: worst |a - b| = {worst:.3e}, bound {bound:.3e}")
    assert worst <= bound


def test_errors():
    from composable_sdr_amd import _lib
    h = cs.FirFilt(np.ones(5, f32), 1.0, is_complex=False, nchan=2, max_samples=64)
    with pytest.raises(cs.CsdrError) as e:
        h.process(np.zeros((2, 65), f32))
    assert e.value.code == _lib.ERR_SIZE
    assert h.process(np.zeros((2, 0), f32)).shape == (2, 0)
    assert h.process(np.ones((2, 64), f32)).shape == (2, 64)
    h.close()
    with pytest.raises(cs.CsdrError):
        h.process(np.zeros((2, 8), f32))                     # a destroyed handle
    with pytest.raises(cs.CsdrError):
        h.taps()
    for make in (lambda: cs.FirFilt(np.zeros(0, f32)), lambda: cs.FirFilt(np.ones(2049, f32)), lambda: cs.FirFilt(np.ones(5, f32), nchan=0),
                 lambda: cs.FirFilt.kaiser(1, 0.1), lambda: cs.FirFilt.kaiser(2049, 0.1), lambda: cs.FirFilt.kaiser(21, 0.0),
                 lambda: cs.FirFilt.kaiser(21, 0.1, mu=0.1), lambda: cs.FirFilt.kaiser(21, 0.1, nchan=0)):
        with pytest.raises(cs.CsdrError) as e:
            make()
        assert e.value.code == _lib.ERR_INVALID
    ok = cs.FirFilt(np.ones(2048, f32), max_samples=16)
    assert ok.taps_len == 2048
    ok.close()


@pytest.mark.parametrize("kind", ["r", "c", "k"])
def test_cpp_pipes_write_the_same_bytes_as_the_python_pipes(tmp_path, kind):
    C, n, chunks = 5, 9000, [1000, 3, 4096, 77, 20]
    cplx = kind != "r"
    x = _noise((C, n), cplx, seed=21)
    taps = cs.firdes_kaiser(51, 0.1, 60.0)
    src, dst, tp = tmp_path / "in.raw", tmp_path / "out.raw", tmp_path / "taps.f32"
    x.tofile(src)
    taps.tofile(tp)
    exe = host_exe("firfilt_host")
    design = "65:0.05:60" if kind == "k" else f"{tp}:0.25"
    r = subprocess.run([exe, kind, design, str(C), ",".join(map(str, chunks)), str(src), str(dst)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    pipe = {"r": lambda: cs.firFilterR(taps, 0.25, nchan=C, max_samples=4096), "c": lambda: cs.firFilterC(taps, 0.25, nchan=C, max_samples=4096),
            "k": lambda: cs.firFilterCKaiser(65, 0.05, 60.0, nchan=C, max_samples=4096)}[kind]()
    rr = pipe._start()
    want, pos, k = [], 0, 0
    while pos < n:
        c = min(chunks[k % len(chunks)], n - pos)
        want.append(pipe._process(rr, x[:, pos:pos + c]).tobytes())
        pos += c
        k += 1
    pipe._done(rr)
    want = b"".join(want)
    assert len(want) == x.nbytes and open(dst, "rb").read() == want
