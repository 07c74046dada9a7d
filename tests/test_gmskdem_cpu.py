"""gmskDemodulator / firFilterRNyquist without a GPU: the two host-only designs against their restatement in
tests/gmsk_restatement.py, the zero-ISI property of the f32 taps, the limits, and the receiver's quality on noiseless GMSK
(restatement only)."""
import ctypes as C
import math

import numpy as np
import pytest

import gmsk_restatement as G

cs = pytest.importorskip("composable_sdr_amd")
from composable_sdr_amd import _lib  # noqa: E402

f32 = np.float32
CASES = [(2, 1, 0.2), (4, 3, 0.3), (5, 3, 0.4), (8, 4, 0.5), (3, 3, 0.3), (64, 8, 0.3), (64, 1, 1.0)]
GRID = [(k, m, bt) for k in (2, 4, 5, 8) for m in (2, 3, 4) for bt in (0.3, 0.5)]


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("kmb", CASES, ids=str)
def test_designs_equal_the_restatement(kmb):
    k, m, bt = kmb
    for got, want in ((cs.firdes_gmsktx(k, m, bt), G.firdes_gmsktx(k, m, float(f32(bt)))), (cs.firdes_gmskrx(k, m, bt), G.firdes_gmskrx(k, m, float(f32(bt))))):
        assert got.dtype == f32 and got.shape == want.shape == (2 * k * m + 1,)
        err = float(np.abs(got.astype(np.float64) - want).max())
        bound = 2.0 ** -22 * float(np.abs(want).max())
        print(f"{kmb}: max |tap - restatement| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound
    g, r = cs.firdes_gmsktx(k, m, bt), cs.firdes_gmskrx(k, m, bt)
    assert abs(float(g.astype(np.float64).sum()) - 1.0) < 1e-6
    assert np.array_equal(r.view(np.uint32), r[::-1].view(np.uint32))          # exactly symmetric in f32


@pytest.mark.parametrize("kmb", CASES, ids=str)
def test_f32_taps_have_no_isi_over_their_span(kmb):
    k, m, bt = kmb
    g, r = cs.firdes_gmsktx(k, m, bt).astype(np.float64), cs.firdes_gmskrx(k, m, bt).astype(np.float64)
    L = g.size
    c = np.convolve(g, r)
    worst = max(abs(c[L - 1] - 1.0), max(abs(c[L - 1 + j * k]) for j in range(-m, m + 1) if j))
    print(f"{kmb}: worst zero-ISI residual {worst:.3e}, condition {G.condition(k, m, bt):.1f}")
    assert worst <= 1e-5


@pytest.mark.parametrize("bad", [(1, 3, 0.3), (65, 3, 0.3), (4, 0, 0.3), (4, 9, 0.3), (4, 3, 0.19), (4, 3, 1.01)], ids=str)
def test_limits(bad):
    k, m, bt = bad
    h = np.zeros(2 * 65 * 9 + 1, f32)
    for fn in (_lib.lib().csdr_firdes_gmsktx, _lib.lib().csdr_firdes_gmskrx):
        assert fn(k, m, bt, _ptr(h)) == _lib.ERR_INVALID
    assert not h.any()
    out = C.c_void_p()
    assert _lib.lib().csdr_gmskdem_create(k, m, bt, 1, 64, C.byref(out)) == _lib.ERR_INVALID and not out.value
    for fn in (cs.firdes_gmsktx, cs.firdes_gmskrx):
        with pytest.raises(cs.CsdrError) as e:
            fn(k, m, bt)
        assert e.value.code == _lib.ERR_INVALID


def test_null_pointers_and_mu():
    assert _lib.lib().csdr_firdes_gmsktx(4, 3, 0.3, None) == _lib.ERR_INVALID
    assert _lib.lib().csdr_firdes_gmskrx(4, 3, 0.3, None) == _lib.ERR_INVALID
    assert _lib.lib().csdr_gmskdem_create(4, 3, 0.3, 1, 64, None) == _lib.ERR_INVALID
    with pytest.raises(cs.CsdrError) as e:
        cs.firFilterRNyquist(4, 3, 0.3, mu=0.1)
    assert e.value.code == _lib.ERR_INVALID


@pytest.mark.parametrize("kmb", GRID, ids=str)
def test_the_receiver_decodes_noiseless_gmsk_with_an_open_eye(kmb):
    """restatement only: 4000 random symbols from a transmitter with the same m; symbol s comes out at s + 2 m"""
    k, m, bt = kmb
    nsym = 4000
    bits = np.random.default_rng(100 * k + 10 * m + int(10 * bt)).integers(0, 2, nsym)
    x = G.gmskmod(bits, k, m, bt)
    d, _ = G.demod(x, G.firdes_gmskrx(k, m, bt), k)
    d = d[0]
    assert np.array_equal(d[2 * m:] > 0, bits[:nsym - 2 * m] == 1)
    eye = float(np.abs(d[2 * m + 5:]).min()) / (0.5 * math.pi)
    print(f"{kmb}: smallest |d| = {eye:.3f} of pi / 2")
    assert eye >= 0.9


def test_no_gpu_means_loud_failure_not_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    for make in (lambda: cs.GmskDem(4, 3, 0.3), lambda: cs.gmskDemodulator(3, 4, 0.3)._start(), lambda: cs.firFilterRNyquist(4, 3, 0.3)._start()):
        with pytest.raises(cs.CsdrError) as e:
            make()
        assert e.value.code == -3 and "no CPU fallback" in str(e.value)
