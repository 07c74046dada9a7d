"""The FIR filter (csdr_firfilt_*) without a GPU: the design functions of the C ABI against the known answers
and the existing restatement, the design's frequency-domain properties, the refusals, and the f32 arithmetic the kernel uses
(fir_restatement.filter_f32) against the same sum in f64.

Error model: an output is scale times a sum of L products, each product and each accumulation rounded once in f32, then the
scale's rounding, so |y32 - y64| <= (L + 2) 2^-24 |scale| sum_i |h_i| |x_{t-i}| per output (the standard bound for L rounded
products summed in order, plus the scale; valid for L <= 2048)."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fir_restatement as R
import fms_restatement as S

cs = pytest.importorskip("composable_sdr_amd")
from composable_sdr_amd import _lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32

# (n, fc, As): the last is the stereo decoder's pilot filter at q = 1.2e6
DESIGNS = [(21, 0.25, 60.0), (51, 0.1, 60.0), (65, 0.05, 60.0), (101, 0.2, 80.0), (889, 800.0 / 1.2e6, 60.0)]


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_firdes_kaiser_meets_the_known_answers_of_ex1_5_gif():
    with open(os.path.join(ROOT, "tests", "golden", "kat_ex1_5_gif.json")) as f:
        kat = json.load(f)["kat1_taps_M20_m7_As80"]
    h = cs.firdes_kaiser(281, 0.025, 80.0)
    assert h.dtype == np.float32 and h.shape == (281,)
    worst = max(abs(float(h[int(i)]) - v) for i, v in kat.items())
    print(f"KAT1: worst |h - printed| = {worst:.2e} over indices {min(map(int, kat))}..{max(map(int, kat))}")
    assert sorted(map(int, kat)) == list(range(249, 280))
    for i, v in kat.items():
        assert abs(float(h[int(i)]) - v) < 2e-8, (i, h[int(i)], v)


@pytest.mark.parametrize("n,fc,As", DESIGNS, ids=[f"{d[0]}" for d in DESIGNS])
def test_firdes_kaiser_equals_the_restatement_within_one_ulp(n, fc, As):
    fc = f32(fc)                                              # the C ABI takes fc as a float
    h = cs.firdes_kaiser(n, fc, As)
    want = S.firdes_kaiser(n, fc, As)
    ulps = np.abs(h.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
    print(f"({n}, {float(fc):.6g}, {As}): {int((h != want).sum())} taps differ, worst {ulps.max():.1f} ulp")
    assert np.all(ulps <= 1.0)
    assert np.array_equal(h, h[::-1])                         # linear phase: the taps are symmetric, bit for bit


@pytest.mark.parametrize("n,fc,As", DESIGNS[:4], ids=[f"{d[0]}" for d in DESIGNS[:4]])
def test_scaled_design_has_unit_dc_gain_and_its_stop_band(n, fc, As):
    """the scaled taps 2 fc h from a 65536-point FFT: |DC gain - 1| <= 1e-3, and from fc + df / 2 on (df = (As - 7.95) /
    (14.36 (n - 1)), Kaiser's transition width) nothing above -(As - 2) dB.  The 889-tap pilot design is left out on purpose:
    its DC gain is 0.56, n fc is too small for the window"""
    h = cs.firdes_kaiser(n, fc, As).astype(np.float64) * float(f32(2) * f32(fc))
    N = 65536
    Hf = np.abs(np.fft.rfft(h, N))
    dc = Hf[0]
    df = (As - 7.95) / (14.36 * (n - 1))
    k0 = int(np.ceil((fc + 0.5 * df) * N))
    stop = 20.0 * np.log10(Hf[k0:].max())
    print(f"({n}, {fc}, {As}): DC gain error {abs(dc - 1.0):.1e}, stop band from {fc + 0.5 * df:.4f}: {stop:.1f} dB")
    assert abs(dc - 1.0) <= 1e-3
    assert stop <= -(As - 2.0)


def test_fir_groupdelay():
    for n, fc, As in DESIGNS[:4]:
        h = cs.firdes_kaiser(n, fc, As)
        for f in (0.0, 0.01):
            gd = cs.fir_groupdelay(h, f)
            assert abs(gd - 0.5 * (n - 1)) <= 1e-3, (n, f, gd)
            assert abs(gd - float(S.fir_group_delay(h, f))) <= 1e-5, (n, f, gd)
    rng = np.random.default_rng(1)
    h = rng.standard_normal(33).astype(f32)                   # not symmetric: only the two implementations agree
    for f in (0.0, 0.05, 0.3):
        assert abs(cs.fir_groupdelay(h, f) - float(S.fir_group_delay(h, f))) <= 1e-5 * max(1.0, abs(float(S.fir_group_delay(h, f))))


BAD = [(1, 0.25, 60.0, 0.0), (2049, 0.25, 60.0, 0.0), (21, 0.0, 60.0, 0.0), (21, 0.51, 60.0, 0.0), (21, 0.25, 0.0, 0.0),
       (21, 0.25, 60.0, 0.1)]


@pytest.mark.parametrize("n,fc,As,mu", BAD, ids=["n=1", "n=2049", "fc=0", "fc=0.51", "as=0", "mu=0.1"])
def test_design_refusals_need_no_gpu(n, fc, As, mu):
    h = np.zeros(4096, f32)
    assert _lib.lib().csdr_firdes_kaiser(n, fc, As, mu, _ptr(h)) == _lib.ERR_INVALID
    assert not h.any()
    assert _lib.lib().csdr_firdes_kaiser(21, 0.25, 60.0, 0.0, _ptr(h)) == 0 and h[:21].all() and not h[21:].any()


def test_design_refuses_null_pointers():
    assert _lib.lib().csdr_firdes_kaiser(21, 0.25, 60.0, 0.0, None) == _lib.ERR_INVALID
    h, gd = np.ones(5, f32), C.c_float()
    assert _lib.lib().csdr_fir_groupdelay(None, 5, 0.0, C.byref(gd)) == _lib.ERR_INVALID
    assert _lib.lib().csdr_fir_groupdelay(_ptr(h), 5, 0.0, None) == _lib.ERR_INVALID
    assert _lib.lib().csdr_fir_groupdelay(_ptr(h), 0, 0.0, C.byref(gd)) == _lib.ERR_INVALID
    with pytest.raises(cs.CsdrError) as e:
        cs.firdes_kaiser(1, 0.25)
    assert e.value.code == _lib.ERR_INVALID


def test_no_gpu_means_loud_failure_not_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    for make in (lambda: cs.FirFilt(np.ones(5, f32)), lambda: cs.FirFilt.kaiser(21, 0.25), lambda: cs.firFilterR(np.ones(3, f32))._start(),
                 lambda: cs.firFilterC(np.ones(3, f32))._start(), lambda: cs.firFilterCKaiser(21, 0.1)._start()):
        with pytest.raises(cs.CsdrError) as e:
            make()
        assert e.value.code == -3 and "no CPU fallback" in str(e.value)


def _noise(shape, cplx, seed):
    rng = np.random.default_rng(seed)
    if cplx:
        return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)).astype(np.complex64)
    return rng.standard_normal(shape).astype(f32)


def _taps(L, seed):
    """a Kaiser low-pass where the design exists, noise taps for the lengths it does not make interesting"""
    if L >= 8:
        return S.firdes_kaiser(L, 0.1, 60.0), f32(0.2)
    return np.random.default_rng(seed).standard_normal(L).astype(f32), f32(0.75)


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("L", [21, 65, 889, 2048])
def test_f32_sum_against_the_f64_sum_within_the_error_model(L, cplx):
    taps, scale = _taps(L, L)
    n = 20000 if L < 500 else 6000
    x = _noise((2, n), cplx, seed=L + cplx)
    y32, _ = R.filter_f32(taps, scale, x)
    y64, _ = R.filter_f64(taps, scale, x)
    worst = 0.0
    for a, b, B in zip(R.components(y32), R.components(y64), R.bound(taps, scale, x)):
        err = np.abs(a.astype(np.float64) - b)
        ok = B > 0
        worst = max(worst, float((err[ok] / B[ok]).max()))
        assert np.all(err <= B)
    print(f"L = {L}, {'complex' if cplx else 'real'}: worst |y32 - y64| / bound = {worst:.3f}")
    # noise taps too: no structure in the signs of the products
    t2 = np.random.default_rng(L).standard_normal(L).astype(f32)
    a32, _ = R.filter_f32(t2, 1.0, x[:, :2000])
    a64, _ = R.filter_f64(t2, 1.0, x[:, :2000])
    for a, b, B in zip(R.components(a32), R.components(a64), R.bound(t2, 1.0, x[:, :2000])):
        assert np.all(np.abs(a.astype(np.float64) - b) <= B)


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("L", [1, 2, 21, 255])
def test_restatement_is_chunk_invariant_bit_for_bit(L, cplx):
    taps, scale = _taps(L, 7 * L)
    n = 5000
    x = _noise((3, n), cplx, seed=3 * L + cplx)
    ref, ref_hist = R.filter_f32(taps, scale, x)
    rng = np.random.default_rng(L)
    sizes = [0, 1, 2, 3, 7, max(L - 2, 0), max(L - 2, 0), L - 1, L, 64, 333, 1000]      # several below L - 1, back to back
    outs, hist, pos = [], None, 0
    while pos < n:
        c = min(int(rng.choice(sizes)), n - pos)
        y, hist = R.filter_f32(taps, scale, x[:, pos:pos + c], hist)
        outs.append(y)
        pos += c
    got = np.concatenate(outs, axis=1)
    assert got.dtype == ref.dtype
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(hist, ref_hist)
    # impulse: exactly scale * (0 + h[i])
    imp = np.zeros(L + 5, x.dtype)
    imp[0] = 1.0
    y, _ = R.filter_f32(taps, scale, imp)
    assert np.array_equal(y[:L].real.astype(f32), f32(scale) * (f32(0) + taps)) and not y[L:].any()


HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_k_firfilt_keeps_its_window_and_sums_in_registers(tmp_path):
    """both instantiations (real, complex): the sliding window and the 8 sums are register arrays indexed by unrolled loops; in
    scratch memory they would cost a round trip per tap.  LDS is dynamic (tile + halo, skewed): none of it static, and the
    largest request (complex, 2048 taps) stays below 64 KiB"""
    src = os.path.join(ROOT, "composable_sdr_amd", "csrc", "kernels_firfilt.hip")
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-c", src, "-o", str(tmp_path / "fir.o"),
                          "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    blocks = [b for b in re.split(r"remark: Function Name: ", out.stderr)[1:] if "k_firfilt" in b.splitlines()[0]]
    assert len(blocks) == 2
    for b in blocks:
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, b[:400]
        assert int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) == 0, b[:400]
        assert int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1)) <= 64 * 1024, b[:400]
    text = open(src).read()
    tile = int(re.search(r"FF_T = (\d+)", text).group(1)) * int(re.search(r"FF_R = (\d+)", text).group(1))
    slots = tile + 2048 - 1
    assert 8 * (slots + (slots >> 3) + 1) <= 64 * 1024
