"""realToComplex / complexToReal (csdr_firhilb_*) on the GPU against the CPU restatement in
tests/firhilb_restatement.py.

The kernel and the restatement perform the same f32 operations in the same order (no contraction, one summation order), so every
comparison of outputs here is bit for bit; the restatement takes the handle's taps (get_taps), and the taps are compared with the
float64 design separately, at the bound tests/test_symsync_gpu.py uses for its banks."""
import numpy as np
import pytest

import firhilb_restatement as F

pytestmark = pytest.mark.gpu

cs = pytest.importorskip("composable_sdr_amd")

f32 = np.float32
MAXN = 4096


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _signal(kind, nfloats, seed=1):
    if kind == "noise":
        return np.random.default_rng(seed).standard_normal(nfloats).astype(f32)
    return np.cos(2 * np.pi * 0.2875 * np.arange(nfloats) + 0.3).astype(f32)


def _ragged(total, seed):
    """seeded call sizes summing to `total`: 0, 1, odd ones, tile edges and MAXN among them"""
    rng = np.random.default_rng(seed)
    calls = [0, 1, MAXN, 3, 0, 511, 512, 513, 9]
    while sum(calls) < total:
        calls.append(int(rng.choice([0, 1, 2, 5, 19, 20, 21, 333, 1025, MAXN])))
    over = sum(calls) - total
    while over > 0:
        c = calls.pop()
        over -= c
    calls.append(-over)
    assert sum(calls) == total and max(calls) <= MAXN
    return calls


def _gpu_calls(h, x, calls, interp):
    step = 1 if interp else 2
    out, pos = [], 0
    for c in calls:
        a = x[pos:pos + step * c]
        pos += step * c
        out.append(h.interp(a) if interp else h.decim(a))
    return np.concatenate(out)


def test_taps_match_the_float64_design():
    h = cs.FirHilb()
    hq = h.taps()
    assert h.taps_len == 10 and hq.dtype == f32
    h.close()
    want = F.design(5, 60.0)
    print(f"taps: {np.mean(hq == want.astype(f32)):.2f} bitwise equal to the rounded f64 design; max |diff| {np.abs(hq - want).max():.3e}")
    np.testing.assert_allclose(hq, want, rtol=0, atol=2e-7 * np.abs(want).max())
    h = cs.FirHilb(m=7, as_db=80.0)
    np.testing.assert_allclose(h.taps(), F.design(7, 80.0), rtol=0, atol=2e-7 * np.abs(F.design(7, 80.0)).max())
    h.close()


@pytest.mark.parametrize("signal", ["noise", "tone"])
@pytest.mark.parametrize("interp", [False, True], ids=["decim", "interp"])
def test_bit_identical_to_the_restatement_for_every_chunking(signal, interp):
    n = 3 * MAXN + 777
    x = _signal(signal, 2 * n)
    if interp:
        x = x.view(np.complex64)
    h = cs.FirHilb(max_samples=MAXN)
    taps = h.taps()
    whole = cs.FirHilb(max_samples=n)
    one = whole.interp(x) if interp else whole.decim(x)
    whole.close()
    want = F.run_calls(F.FirHilb(taps=taps), x, [n], interp)
    assert one.size == want.size == (2 * n if interp else n)
    assert np.array_equal(_bits(one), _bits(want))
    calls = _ragged(n, seed=5)
    got = _gpu_calls(h, x, calls, interp)
    assert np.array_equal(_bits(got), _bits(one))
    # reset reproduces the first run
    h.reset()
    again = _gpu_calls(h, x, [MAXN, MAXN, MAXN, 777], interp)
    h.close()
    assert np.array_equal(_bits(again), _bits(one))
    print(f"{signal} {'interp' if interp else 'decim'}: {one.size} outputs bit-identical in 1, 4 and {len(calls)} calls")


def test_odd_length_drops_the_last_float_and_empty_calls_are_valid():
    x = _signal("noise", 2001, seed=9)
    h = cs.FirHilb(max_samples=MAXN)
    a = h.decim(x[:0])
    b = h.decim(x)
    c = h.interp(np.empty(0, np.complex64))
    taps = h.taps()
    h.close()
    assert a.size == 0 and c.size == 0 and b.size == 1000
    assert np.array_equal(_bits(b), _bits(F.FirHilb(taps=taps).decim(x[:2000])))
    p = cs.realToComplex(max_samples=MAXN)
    r = p._start()
    assert np.array_equal(_bits(p._process(r, x)), _bits(b))
    p._done(r)


def test_one_handle_driven_in_both_directions_shares_the_windows():
    rng = np.random.default_rng(12)
    x = rng.standard_normal(2 * 600).astype(f32)
    z = (rng.standard_normal(500) + 1j * rng.standard_normal(500)).astype(np.complex64)
    h = cs.FirHilb(max_samples=MAXN)
    r = F.FirHilb(taps=h.taps())
    got = [h.decim(x[:400]), h.interp(z[:123]), h.decim(x[400:]), h.interp(z[123:])]
    h.close()
    want = [r.decim(x[:400]), r.interp(z[:123]), r.decim(x[400:]), r.interp(z[123:])]
    for g, w in zip(got, want):
        assert np.array_equal(_bits(g), _bits(w))


@pytest.mark.parametrize("misalign", [0, 1])
def test_device_entry_points_equal_the_host_ones(misalign):
    """device to device on the caller's stream, in ragged calls; misalign = 1 shifts both buffers by one float off their
    16-byte alignment (the kernel then takes its scalar loads and stores)"""
    import torch
    n = 2 * MAXN + 301
    x = _signal("noise", 2 * n, seed=21)
    host = cs.FirHilb(max_samples=n)
    want_d = host.decim(x)
    host.reset()
    want_i = host.interp(x.view(np.complex64))
    host.close()
    d_x = torch.zeros(2 * n + 4, dtype=torch.float32, device="cuda")
    d_x[misalign:misalign + 2 * n] = torch.from_numpy(x).cuda()
    d_y = torch.zeros(2 * n + 4, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for interp, want in ((False, want_d), (True, want_i)):
        h = cs.FirHilb(max_samples=MAXN)
        d_y.zero_()
        pos = 0
        for c in _ragged(n, seed=6):
            fn = h.interp_device if interp else h.decim_device
            fn(d_x.data_ptr() + 4 * (misalign + 2 * pos), c, d_y.data_ptr() + 4 * (misalign + 2 * pos), stream)
            pos += c
        torch.cuda.synchronize()
        y = d_y.cpu().numpy()
        h.close()
        assert np.array_equal(_bits(y[misalign:misalign + 2 * n]), _bits(want)), interp
        assert not y[:misalign].any() and not y[misalign + 2 * n:].any()       # nothing written outside the call's 2 n floats


def test_round_trip_is_the_delayed_quadrature():
    """as tests/test_firhilb_cpu.py states it: interp(decim(x)) is the quadrature of x (cos -> sin) delayed by 4 m - 1 real
    samples, to the image level of the tone test (-58 dB rms over the band 0.1 .. 0.4)"""
    m, N = 5, 16384
    x, xq = F.band_limited(N)
    a, b = cs.FirHilb(max_samples=N), cs.FirHilb(max_samples=N)
    y = b.interp(a.decim(x.astype(f32))).astype(np.float64)
    a.close()
    b.close()
    d = 4 * m - 1
    err = y[d + 200:] - xq[200:-d]
    rel_db = 20 * np.log10(np.sqrt(np.mean(err ** 2)) / np.sqrt(np.mean(x ** 2)))
    print(f"round trip on the GPU: delay {d}, error {rel_db:.2f} dB")
    assert rel_db <= -58.0
