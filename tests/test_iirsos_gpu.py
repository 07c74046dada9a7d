"""The order-n IIR filter (csdr_iirsos_*) on the GPU.

The form is the project's existing one for the biquad (test_iirfilter_and_firdecimator_pipes_match_oracle): truth is the
handle's own f32 coefficients run in f64 by scipy.signal.lfilter, section by section, and the kernel is held to
    |gpu - truth|max <= 2 |filter_f32 - truth|max + 2e-6 max |truth|
with filter_f32 the sequential f32 cascade of tests/iir_restatement.py: a narrow low-pass in direct form II keeps a large
internal state, so the sequential f32 loop is itself noisy, and the kernel (a blocked scan: the f32 summation order differs, the
block states are combined in f64) may be as noisy as that loop, not noisier.  All three figures are printed.

k_iirsos is NOT bit-identical between two ways of cutting one stream into calls: how a sample's sum is grouped depends on its
position in the 4096-sample block, and a call starts a new block.  The same calls on the same state give the same bits.
Every test runs under a time limit of its own: a watchdog thread ends the process if a GPU call does not come back."""
import faulthandler
import os
import subprocess

import numpy as np
import pytest

import iir_restatement as R
from host_exe import host_exe
from synth import channel_centre

pytestmark = pytest.mark.gpu

cs = pytest.importorskip("composable_sdr_amd")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
LIMIT_S = 300

NCHANS = (1, 3, 64)
LENGTHS = (1, 15, 16, 17, 4095, 4096, 4097, 3 * 4096 + 5)
CONT = 333                                                    # the continuation call: odd
DESIGNS = [(n, fc) for n in (1, 2, 3, 8, 16) for fc in (0.1, 0.02)] + [(3, 0.0021)]


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _signal(C, n, cplx, seed):
    """sine + 0.3 noise per row (the existing biquad test's signal), the rows at different frequencies"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    f = 0.01 * (1.0 + 0.07 * np.arange(C))[:, None]
    x = np.sin(2 * np.pi * f * t) + 0.3 * rng.standard_normal((C, n))
    if cplx:
        x = x + 1j * (np.cos(2 * np.pi * 1.3 * f * t) + 0.3 * rng.standard_normal((C, n)))
    return x.astype(np.complex64 if cplx else f32)


def _bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype in (np.float32, np.complex64), a.dtype
    return a.view(np.uint32)


def _check(got, ref32, truth, what):
    """the bound of the module docstring on one region; prints the three figures"""
    assert got.shape == truth.shape and got.dtype == ref32.dtype, (what, got.shape, truth.shape, got.dtype)
    e_gpu = float(np.abs(got - truth).max())
    e_ref = float(np.abs(ref32 - truth).max())
    top = float(np.abs(truth).max())
    print(f"{what}: |gpu - f64| {e_gpu:.3e}, |filter_f32 - f64| {e_ref:.3e}, max |f64| {top:.3e}, bound {2 * e_ref + 2e-6 * top:.3e}")
    assert np.isfinite(got).all(), what
    assert e_gpu <= 2.0 * e_ref + 2e-6 * top, what
    return e_gpu


@pytest.mark.parametrize("n,fc", DESIGNS, ids=[f"{n}-{fc}" for n, fc in DESIGNS])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_accuracy_against_f64_truth(cplx, n, fc):
    """every nchan and row length, then a continuation call of odd size on the carried state.  A causal filter's first L outputs
    do not depend on what follows, so one reference stream per design serves every length"""
    N = max(LENGTHS) + CONT
    x = _signal(max(NCHANS), N, cplx, seed=100 * n + cplx)
    probe = cs.IirSos.prototype(n, fc, is_complex=cplx)
    b, a = probe.sos()
    assert probe.nsec == (n + 1) // 2 == b.shape[0]
    probe.close()
    wb, wa = cs.iirdes_butter_lowpass(n, fc)
    assert np.array_equal(b, wb) and np.array_equal(a, wa)    # the handle runs what the design function returns
    ref32, _ = R.filter_f32(b, a, x)
    truth = R.filter_f64(b, a, x)
    worst = 0.0
    for C in NCHANS:
        for L in LENGTHS:
            h = cs.IirSos.prototype(n, fc, 0.0, 10.0, 10.0, cplx, C, max(L, CONT))
            y = np.concatenate([h.process(x[:C, :L]), h.process(x[:C, L:L + CONT])], axis=1)
            h.close()
            worst = max(worst, _check(y, ref32[:C, :L + CONT], truth[:C, :L + CONT], f"order {n} fc {fc} nchan {C} n {L} + {CONT}"))
    print(f"order {n}, fc {fc}, {'complex' if cplx else 'real'}: worst |gpu - f64| = {worst:.3e}")
    one = cs.IirSos.prototype(n, fc, is_complex=cplx, max_samples=64)
    got = one.process(x[0, :64])                              # a 1-D array in gives a 1-D array out
    one.close()
    assert got.shape == (64,)
    _check(got, ref32[0, :64], truth[0, :64], "1-D")


@pytest.mark.parametrize("cplx,n,fc,nchan", [(False, 3, 0.02, 2), (True, 8, 0.02, 3), (True, 16, 0.1, 1), (False, 3, 0.0021, 5)])
def test_one_call_against_many_and_reset_gives_the_create_state(cplx, n, fc, nchan):
    """the cut list of the biquad test plus single-sample and empty calls, against one call, both under the bound (not bit for
    bit: see the module docstring; the difference is printed).  reset: the same calls again give the same bits as a fresh handle"""
    cuts = [4, 1, 1000, 4096, 4100, 0, 8192, 3001]
    total = sum(cuts)
    x = _signal(nchan, total, cplx, seed=n)
    one = cs.IirSos.prototype(n, fc, is_complex=cplx, nchan=nchan, max_samples=total)
    b, a = one.sos()
    ref = one.process(x)
    one.close()
    ref32, _ = R.filter_f32(b, a, x)
    truth = R.filter_f64(b, a, x)
    _check(ref, ref32, truth, "one call")
    h = cs.IirSos.prototype(n, fc, is_complex=cplx, nchan=nchan, max_samples=max(cuts))
    outs, pos = [], 0
    for c in cuts:
        y = h.process(x[:, pos:pos + c])
        assert y.shape == (nchan, c)
        outs.append(y)
        pos += c
    many = np.concatenate(outs, axis=1)
    _check(many, ref32, truth, "many calls")
    print(f"|many - one|max = {float(np.abs(many - ref).max()):.3e}, {int((_bits(many) != _bits(ref)).sum())} of {_bits(ref).size} words differ")
    h.reset()
    pos = 0
    for c, first in zip(cuts, outs):
        assert np.array_equal(_bits(h.process(x[:, pos:pos + c])), _bits(first)), ("after reset", pos)
        pos += c
    h.close()


@pytest.mark.parametrize("fc", [0.025, 0.0021])
def test_iirFilterN_2_against_the_existing_iirFilter_2(fc):
    """the same design through the new object and through csdr_iirfilt (k_biquad), same chunking: each within the bound of the
    f64 truth of the new handle's coefficients, and within that same bound of each other"""
    n = 20000
    x = _signal(1, n, False, seed=21)[0]
    sizes = [4, 1000, 4096, 4100, 8192, 2608]
    assert sum(sizes) == n
    b, a = cs.iirdes_butter_lowpass(2, fc)
    new, old = cs.iirFilterN(2, fc, max_samples=8192), cs.iirFilter(2, fc, max_samples=8192)
    rn, ro = new._start(), old._start()
    yn, yo, pos = [], [], 0
    for s in sizes:
        yn.append(new._process(rn, x[pos:pos + s]))
        yo.append(old._process(ro, x[pos:pos + s]))
        pos += s
    new._done(rn)
    old._done(ro)
    yn, yo = np.concatenate(yn), np.concatenate(yo)
    ref32, _ = R.filter_f32(b, a, x)
    truth = R.filter_f64(b, a, x)
    _check(yn, ref32, truth, f"iirFilterN 2 {fc}")
    e_ref, top = float(np.abs(ref32 - truth).max()), float(np.abs(truth).max())
    bound = 2.0 * e_ref + 2e-6 * top
    e_old, d = float(np.abs(yo - truth).max()), float(np.abs(yn - yo).max())
    print(f"fc = {fc}: |iirFilter 2 - f64| {e_old:.3e}, |iirFilterN 2 - iirFilter 2| {d:.3e}, bound {bound:.3e}")
    assert e_old <= bound
    assert d <= bound


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_create_sos_with_a_chebyshev_design_from_scipy(cplx):
    """cheby1(4, 1, 0.2) as scipy hands it over (a0 = 1), and the same with every section scaled by an a0 of its own: the handle
    divides it out again (iirfiltsos)"""
    from scipy.signal import cheby1
    sos = cheby1(4, 1, 0.2, output="sos")
    b, a = sos[:, :3].astype(f32), sos[:, 3:].astype(f32)
    x = _signal(3, 9000, cplx, seed=4)
    ref32, _ = R.filter_f32(b, a, x)
    truth = R.filter_f64(b, a, x)
    for scale in (np.ones(2, f32), np.array([2.0, -0.5], f32)):
        h = cs.IirSos(b * scale[:, None], a * scale[:, None], is_complex=cplx, nchan=3, max_samples=5000)
        hb, ha = h.sos()
        assert h.nsec == 2 and np.array_equal(hb, b) and np.array_equal(ha, a)      # powers of two divide out exactly
        y = np.concatenate([h.process(x[:, :5000]), h.process(x[:, 5000:])], axis=1)
        h.close()
        _check(y, ref32, truth, f"cheby1(4, 1, 0.2) scaled by {scale}")
    pipe = cs.iirFilterSOS(b, a, complex=cplx, nchan=3, max_samples=9000)
    r = pipe._start()
    _check(pipe._process(r, x), ref32, truth, "iirFilterSOS")
    pipe._done(r)


def _tone_band(M, nf, chan, f, seed):
    """M nf wideband samples: one tone of amplitude 1 that channel `chan` sees at f cycles per channel sample, over white noise"""
    rng = np.random.default_rng(seed)
    n = M * nf
    t = np.arange(n, dtype=np.float64)
    x = (0.05 / np.sqrt(2.0)) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    x += np.exp(1j * (channel_centre(chan, M) + 2.0 * np.pi * f / M) * t)
    return x.astype(np.complex64)


def test_pipe_behind_the_channelizer_equals_the_nchan_handle():
    """mux (replicate nch (iirCFilter ..)) . firpfbchChannelizer nch against one handle of nch rows: the same calls on the same
    rows, so the same bits"""
    M, nf = 16, 600
    x = _tone_band(M, nf, 3, 0.05, seed=4)
    pipe = cs.compose(cs.mux([cs.iirCFilter(3, 0.1, 0.0, 10.0, 10.0, max_samples=nf)] * M), cs.firpfbchChannelizer(M, max_frames=nf))
    r = pipe._start()
    p1 = pipe._process(r, x[:M * 250])
    p2 = pipe._process(r, x[M * 250:])
    pipe._done(r)
    ch = cs.Chain(channels=M, dc_block=False, max_frames=nf)
    iir = cs.iirCFilter(3, 0.1, nchan=M, max_samples=nf)
    ri = iir._start()
    w1 = iir._process(ri, np.asarray(ch.process(x[:M * 250])).reshape(M, -1))
    w2 = iir._process(ri, np.asarray(ch.process(x[M * 250:])).reshape(M, -1))
    iir._done(ri)
    ch.close()
    assert len(p1) == len(p2) == M and w1.shape == (M, 250) and w2.shape == (M, nf - 250)
    for c in range(M):
        assert np.array_equal(_bits(np.asarray(p1[c])), _bits(w1[c])), c
        assert np.array_equal(_bits(np.asarray(p2[c])), _bits(w2[c])), c


def test_chain_plane_device_to_device():
    """DeNo Chain (16 channels) -> process_device on the chain's CF32 plane, no host copy in between, out of place and then in
    place on a second handle: within the bound of the f64 truth of the chain's own rows, and both the same bits"""
    import torch
    M, nf = 16, 5000
    x = _tone_band(M, nf, 5, 1.0 / 32.0, seed=M)
    ch = cs.Chain(channels=M, demod="none", max_frames=nf)
    h1 = cs.IirSos.prototype(3, 0.1, is_complex=True, nchan=M, max_samples=nf)
    h2 = cs.IirSos.prototype(3, 0.1, is_complex=True, nchan=M, max_samples=nf)
    b, a = h1.sos()
    d_in = torch.from_numpy(x.view(np.float32).copy()).cuda()
    d_mid = torch.empty(2 * M * nf, dtype=torch.float32, device="cuda")
    d_out = torch.zeros(2 * M * nf, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert ch.process_device(d_in.data_ptr(), M * nf, d_mid.data_ptr(), 0) == M * nf
    h1.process_device(d_mid.data_ptr(), nf, d_out.data_ptr(), 0)
    torch.cuda.synchronize()
    rows = d_mid.cpu().numpy().view(np.complex64).reshape(M, nf)
    got = d_out.cpu().numpy().view(np.complex64).reshape(M, nf)
    h2.process_device(d_mid.data_ptr(), nf, d_mid.data_ptr(), 0)
    torch.cuda.synchronize()
    inplace = d_mid.cpu().numpy().view(np.complex64).reshape(M, nf)
    ch.close()
    h1.close()
    h2.close()
    assert float(np.abs(rows).max()) > 0.1                    # the chain wrote the plane
    _check(got, R.filter_f32(b, a, rows)[0], R.filter_f64(b, a, rows), "chain plane")
    assert np.array_equal(_bits(inplace), _bits(got))


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_impulse_per_row_after_reset(cplx):
    """after noise and a reset, an impulse at a position of its own in every row (across a block boundary too): the f64 impulse
    response of the handle's coefficients, within the bound; nothing before the impulse"""
    C, n = 5, 4200
    h = cs.IirSos.prototype(5, 0.05, is_complex=cplx, nchan=C, max_samples=n)
    b, a = h.sos()
    h.process(_signal(C, 1000, cplx, seed=3))
    h.reset()
    imp = np.zeros((C, n), np.complex64 if cplx else f32)
    pos = np.array([0, 1, 15, 4095, 4096])
    imp[np.arange(C), pos] = (1.0 - 0.5j) if cplx else 1.0
    y = h.process(imp)
    h.close()
    _check(y, R.filter_f32(b, a, imp)[0], R.filter_f64(b, a, imp), "impulse")
    for c in range(C):
        assert not y[c, :pos[c]].any(), c


def test_errors():
    from composable_sdr_amd import _lib
    h = cs.IirSos.prototype(3, 0.1, is_complex=False, nchan=2, max_samples=64)
    with pytest.raises(cs.CsdrError) as e:
        h.process(np.zeros((2, 65), f32))
    assert e.value.code == _lib.ERR_SIZE
    assert h.process(np.zeros((2, 0), f32)).shape == (2, 0)
    assert h.process(np.ones((2, 64), f32)).shape == (2, 64)
    with pytest.raises(cs.CsdrError) as e:
        h.process_device(0, 8, 0)
    assert e.value.code == _lib.ERR_INVALID
    h.close()
    with pytest.raises(cs.CsdrError):
        h.process(np.zeros((2, 8), f32))                     # a destroyed handle
    with pytest.raises(cs.CsdrError):
        h.sos()
    with pytest.raises(cs.CsdrError):
        h.reset()
    b, a = cs.iirdes_butter_lowpass(4, 0.1)
    for make in (lambda: cs.IirSos.prototype(0, 0.1), lambda: cs.IirSos.prototype(17, 0.1), lambda: cs.IirSos.prototype(3, 0.0),
                 lambda: cs.IirSos.prototype(3, 0.5), lambda: cs.IirSos.prototype(3, 0.1, nchan=0), lambda: cs.IirSos(b, a, nchan=0),
                 lambda: cs.IirSos(np.tile(b[0], 9), np.tile(a[0], 9)), lambda: cs.IirSos(np.zeros(0, f32), np.zeros(0, f32)),
                 lambda: cs.IirSos(b, a * np.array([1.0, 0.0], f32)[:, None]), lambda: cs.IirSos(b[:1], np.array([1.0, 0.0, 1.0], f32)),
                 lambda: cs.IirSos(b[:1], np.array([1.0, 2.0, 1.0], f32))):
        with pytest.raises(cs.CsdrError) as e:
            make()
        assert e.value.code == _lib.ERR_INVALID
    ok = cs.IirSos.prototype(16, 0.25, max_samples=16)
    assert ok.nsec == 8
    ok.close()
    with pytest.raises(cs.CsdrError):
        cs.iirFilter(4, 0.1)._start()                         # the existing object is unchanged: order 2 only


@pytest.mark.parametrize("kind", ["p", "r", "c"])
def test_cpp_pipes_write_the_same_bytes_as_the_python_pipes(tmp_path, kind):
    from scipy.signal import cheby1
    C, n, chunks = 5, 9000, [1000, 3, 4096, 77, 20]
    cplx = kind != "r"
    x = _signal(C, n, cplx, seed=21)
    sos = cheby1(4, 1, 0.2, output="sos").astype(f32)
    src, dst, sp = tmp_path / "in.raw", tmp_path / "out.raw", tmp_path / "sos.f32"
    x.tofile(src)
    sos.tofile(sp)
    exe = host_exe("iirsos_host")
    design = "5:0.05" if kind == "p" else str(sp)
    r = subprocess.run([exe, kind, design, str(C), ",".join(map(str, chunks)), str(src), str(dst)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    pipe = (cs.iirCFilter(5, 0.05, 0.0, 10.0, 10.0, nchan=C, max_samples=4096) if kind == "p" else
            cs.iirFilterSOS(sos[:, :3], sos[:, 3:], complex=cplx, nchan=C, max_samples=4096))
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
