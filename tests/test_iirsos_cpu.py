"""The order-n IIR filter (csdr_iirsos_*) without a GPU: the design function of the C ABI against the numpy
restatement, against scipy's Butterworth design and against the analytic magnitude, the unit DC gain of every section, the
refusals that need no GPU, and the restatement's own f32 cascade against f64.

The design is pinned by mathematics: an order-n Butterworth low-pass through the bilinear transform has one answer, and
scipy.signal.butter computes it independently of tests/iir_restatement.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import iir_restatement as R

cs = pytest.importorskip("composable_sdr_amd")
from composable_sdr_amd import _lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32

DESIGNS = [(1, .1), (2, .025), (3, .1), (4, .05), (7, .02), (8, .01), (16, .1), (16, .25), (3, .0021), (6, .45)]
IDS = [f"{n}-{fc}" for n, fc in DESIGNS]


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("n,fc", DESIGNS, ids=IDS)
def test_design_equals_the_restatement_within_one_ulp(n, fc):
    fc = f32(fc)                                              # the C ABI takes fc as a float
    b, a = cs.iirdes_butter_lowpass(n, fc)
    wb, wa = R.butter_lowpass_sos(n, fc)
    S = (n + 1) // 2
    assert b.shape == a.shape == wb.shape == wa.shape == (S, 3) and b.dtype == a.dtype == np.float32
    worst = 0.0
    for got, want in ((b, wb), (a, wa)):
        ulps = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
        worst = max(worst, float(ulps.max()))
        assert np.all(ulps <= 1.0), (got, want)
    print(f"({n}, {float(fc):.6g}): worst {worst:.1f} ulp")
    assert np.all(a[:, 0] == 1.0)
    if n & 1:                                                 # the first-order section comes last
        assert a[-1, 2] == 0.0 and b[-1, 2] == 0.0 and b[-1, 0] == b[-1, 1]
    # highest Q first: the pole radius |p_d|^2 = a2 falls from section to section
    pairs = a[:n // 2, 2]
    assert np.all(np.diff(pairs) < 0)


@pytest.mark.parametrize("n,fc", DESIGNS, ids=IDS)
def test_design_against_scipy_butter_and_the_analytic_magnitude(n, fc):
    """513 frequencies on [0, pi): the cascade of the f32 coefficients against scipy's f64 design and against
    1 / sqrt(1 + (tan(w / 2) / tan(pi fc))^(2 n)).  In f64 the two designs agree to about 1e-13 (asserted at 1e-11).  The f32
    coefficients are held to 1e-6, which leaves room for their rounding, except where the rounding itself needs more: a narrow
    section has 1 + a1 + a2 of the order (2 pi fc)^2 next to a1 near -2, and half an ulp of a1 moves its gain by 6e-8 / (1 + a1 +
    a2).  There the bound is R.rounding_bound (every coefficient off by at most half an ulp, first order) with 5 % for the
    second order; it comes from the number format, not from what the library returns.  The cases that use it, with the figures:
    DESIGN.md 4.14"""
    from scipy.signal import butter, sosfreqz
    fc32 = f32(fc)
    b, a = cs.iirdes_butter_lowpass(n, fc32)
    w = np.pi * np.arange(513) / 513.0
    H = R.response(b, a, w)
    sos = butter(n, 2.0 * float(fc32), output="sos")
    _, Hs = sosfreqz(sos, worN=w)
    e_sp = float(np.abs(H - Hs).max())
    e_an = float(np.abs(np.abs(H) - R.butter_magnitude(n, fc32, w)).max())
    # the f64 restatement alone, as the design check of the issue has it
    b64, a64 = R.butter_lowpass_sos64(n, float(fc32))
    e64 = float(np.abs(R.response(b64, a64, w) - Hs).max())
    e64_an = float(np.abs(np.abs(R.response(b64, a64, w)) - R.butter_magnitude(n, fc32, w)).max())
    rb = 1.05 * float(R.rounding_bound(b64, a64, w).max())
    tol = max(1e-6, rb)
    print(f"({n}, {fc}): |H - scipy|max = {e_sp:.2e}, ||H| - analytic|max = {e_an:.2e}, bound used {tol:.2e} (rounding bound {rb:.2e}); "
          f"f64 restatement against scipy {e64:.2e}, against the analytic magnitude {e64_an:.2e}")
    assert e64 <= 1e-11 and e64_an <= 1e-11
    assert e_sp <= tol
    assert e_an <= tol


def test_order_2_is_the_existing_biquad_design():
    """csdr_iirfilt's five coefficients (design_butter2_lowpass: K = tan(pi fc), norm = 1 / (1 + sqrt(2) K + K^2)) within 1 ulp.
    fc = 0.25 is left out: there a1 is zero in mathematics and rounding noise of the order 1e-16 in either form"""
    for fc in (0.025, 0.0021, 0.1, 0.2, 0.4):
        fc32 = f32(fc)
        b, a = cs.iirdes_butter_lowpass(2, fc32)
        K = np.tan(np.pi * float(fc32))
        nrm = 1.0 / (1.0 + np.sqrt(2.0) * K + K * K)
        want = np.array([K * K * nrm, 2.0 * K * K * nrm, K * K * nrm, 2.0 * (K * K - 1.0) * nrm, (1.0 - np.sqrt(2.0) * K + K * K) * nrm]).astype(f32)
        got = np.array([b[0, 0], b[0, 1], b[0, 2], a[0, 1], a[0, 2]], f32)
        ulps = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
        print(f"fc = {fc}: {got} worst {ulps.max():.1f} ulp")
        assert np.all(ulps <= 1.0), (fc, got, want)


@pytest.mark.parametrize("n,fc", DESIGNS, ids=IDS)
def test_every_section_has_unit_dc_gain(n, fc):
    """The DC gain of a section is (b0 + b1 + b2) / (1 + a1 + a2).  Each of the five f32 coefficients is off its f64 value by
    at most half an ulp of itself, and none is larger than 2 in magnitude, so the two sums of the rounded coefficients, taken
    in f64, differ by less than 4 ulp of the largest coefficient of the section (2.5 would do: 0.5 each for a1, a2 and the
    three b).  Stated on the sums, not on their quotient: for a narrow filter 1 + a1 + a2 is itself only a few thousand ulp of
    a1, so the quotient of the f32 coefficients cannot be one within 4 ulp of one.  The unrounded design has the gain exactly.
    The quotient itself is held to what the format allows: rounding moves it by at most (sum of the five half ulps) /
    (1 + a1 + a2) to first order (1.05 of that for the second order), computed from the f64 design, not from the library's
    output.  Where that is within 4 ulp of one (the wide designs; REACHABLE lists them and is asserted), the gain is one within
    4 ulp of one, as stated; for a narrow section the gain error of the library's coefficients is printed next to the bound
    and held to it"""
    b, a = cs.iirdes_butter_lowpass(n, f32(fc))
    b64, a64 = R.butter_lowpass_sos64(n, float(f32(fc)))
    four = 4.0 * float(np.spacing(f32(1.0)))
    reachable = True
    for s in range(b.shape[0]):
        num, den = float(b[s].astype(np.float64).sum()), float(a[s].astype(np.float64).sum())
        ulp = float(np.spacing(f32(max(np.abs(a[s]).max(), np.abs(b[s]).max()))))
        print(f"({n}, {fc}) section {s}: sum b = {num:.9g}, sum a = {den:.9g}, difference {abs(num - den) / ulp:.2f} ulp")
        assert abs(num - den) <= 4.0 * ulp
        assert abs(b64[s].sum() - a64[s].sum()) <= 4.0 * np.spacing(np.abs(a64[s]).max())
        half = 0.5 * np.spacing(np.abs(np.concatenate([b64[s], a64[s, 1:]])).astype(f32)).astype(np.float64)
        rb = 1.05 * float(half.sum()) / float(a64[s].sum())
        gain_err = abs(num / den - 1.0)
        tol = max(four, rb)
        reachable = reachable and rb <= four
        print(f"    DC gain - 1 = {gain_err:.3e}; 4 ulp of one = {four:.3e}, rounding bound {rb:.3e}, bound used {tol:.3e}")
        assert gain_err <= tol
    assert reachable == ((n, fc) in REACHABLE), "which designs reach 4 ulp of one follows from the format: see REACHABLE"


# the designs every section of which can have unit DC gain within 4 ulp of one in f32 coefficients (rounding bound <= 4 ulp)
REACHABLE = {(1, .1), (3, .1), (16, .1), (16, .25), (6, .45)}


BAD_DESIGNS = [(0, 0.1), (17, 0.1), (3, 0.0), (3, -0.1), (3, 0.5), (3, 0.7), (3, float("nan"))]


@pytest.mark.parametrize("n,fc", BAD_DESIGNS, ids=[f"{n}-{fc}" for n, fc in BAD_DESIGNS])
def test_design_refusals_need_no_gpu(n, fc):
    b, a = np.zeros(24, f32), np.zeros(24, f32)
    assert _lib.lib().csdr_iirdes_butter_lowpass(n, fc, _ptr(b), _ptr(a)) == _lib.ERR_INVALID
    assert not b.any() and not a.any()
    h = C.c_void_p()
    for cplx in (0, 1):
        assert _lib.lib().csdr_iirsos_create_prototype(n, fc, 0.0, 10.0, 10.0, cplx, 1, 64, C.byref(h)) == _lib.ERR_INVALID
        assert not h.value
    with pytest.raises(cs.CsdrError) as e:
        cs.iirdes_butter_lowpass(n, fc)
    assert e.value.code == _lib.ERR_INVALID


def test_design_and_create_refuse_null_pointers_and_bad_counts():
    L = _lib.lib()
    b, a = np.zeros(24, f32), np.zeros(24, f32)
    assert L.csdr_iirdes_butter_lowpass(3, 0.1, None, _ptr(a)) == _lib.ERR_INVALID
    assert L.csdr_iirdes_butter_lowpass(3, 0.1, _ptr(b), None) == _lib.ERR_INVALID
    assert L.csdr_iirdes_butter_lowpass(16, 0.1, _ptr(b), _ptr(a)) == 0 and b.all() and a[1::3].all()
    h = C.c_void_p()
    gb, ga = cs.iirdes_butter_lowpass(4, 0.1)
    assert L.csdr_iirsos_create_prototype(3, 0.1, 0.0, 10.0, 10.0, 1, 1, 64, None) == _lib.ERR_INVALID
    assert L.csdr_iirsos_create_prototype(3, 0.1, 0.0, 10.0, 10.0, 1, 0, 64, C.byref(h)) == _lib.ERR_INVALID     # nchan 0
    assert L.csdr_iirsos_create_sos(None, _ptr(ga), 2, 0, 1, 64, C.byref(h)) == _lib.ERR_INVALID
    assert L.csdr_iirsos_create_sos(_ptr(gb), None, 2, 0, 1, 64, C.byref(h)) == _lib.ERR_INVALID
    assert L.csdr_iirsos_create_sos(_ptr(gb), _ptr(ga), 2, 0, 1, 64, None) == _lib.ERR_INVALID
    assert L.csdr_iirsos_create_sos(_ptr(gb), _ptr(ga), 2, 0, 0, 64, C.byref(h)) == _lib.ERR_INVALID             # nchan 0
    nine = np.tile(gb[0], 9), np.tile(ga[0], 9)
    assert L.csdr_iirsos_create_sos(_ptr(nine[0]), _ptr(nine[1]), 0, 0, 1, 64, C.byref(h)) == _lib.ERR_INVALID
    assert L.csdr_iirsos_create_sos(_ptr(nine[0]), _ptr(nine[1]), 9, 0, 1, 64, C.byref(h)) == _lib.ERR_INVALID
    assert not h.value
    assert L.csdr_iirsos_get_nsec(None) == 0
    assert L.csdr_iirsos_get_sos(None, _ptr(b), _ptr(a)) == _lib.ERR_INVALID
    assert L.csdr_iirsos_reset(None) == _lib.ERR_INVALID
    assert L.csdr_iirsos_process(None, _ptr(b), 4, _ptr(a)) == _lib.ERR_INVALID
    assert L.csdr_iirsos_destroy(None) == 0


# a (a0, a1, a2): a0 = 0; on and outside the stability triangle |a2| < 1, |a1| < 1 + a2 (after the division by a0)
UNSTABLE = [(0.0, 0.5, 0.1), (1.0, 0.0, 1.0), (1.0, 0.0, -1.0), (1.0, 2.0, 1.0), (1.0, -1.5, 0.5), (1.0, 1.5, 0.5), (1.0, 0.0, 1.5),
            (2.0, 0.0, 2.0), (1.0, float("nan"), 0.0), (1.0, 1.0, 0.0), (1.0, -1.0, 0.0)]


@pytest.mark.parametrize("a", UNSTABLE, ids=[str(a) for a in UNSTABLE])
def test_create_sos_refuses_sections_that_are_not_strictly_stable(a):
    """refused before a device is looked for; a good section in front does not help"""
    gb, ga = cs.iirdes_butter_lowpass(2, 0.1)
    b = np.concatenate([gb[0], np.array([1.0, 0.0, 0.0], f32)])
    aa = np.concatenate([ga[0], np.array(a, f32)])
    h = C.c_void_p()
    for cplx in (0, 1):
        assert _lib.lib().csdr_iirsos_create_sos(_ptr(b), _ptr(aa), 2, cplx, 1, 64, C.byref(h)) == _lib.ERR_INVALID
    assert not h.value
    with pytest.raises(cs.CsdrError) as e:
        cs.IirSos(b, aa, is_complex=False)
    assert e.value.code == _lib.ERR_INVALID
    with pytest.raises(cs.CsdrError):
        cs.IirSos(np.ones(4, f32), np.ones(4, f32))          # not [S][3]


def test_no_gpu_means_loud_failure_not_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    b, a = cs.iirdes_butter_lowpass(3, 0.1)
    for make in (lambda: cs.IirSos(b, a), lambda: cs.IirSos.prototype(3, 0.1), lambda: cs.iirCFilter(3, 0.1, 0.0, 10.0, 10.0)._start(),
                 lambda: cs.iirFilterN(5, 0.1)._start(), lambda: cs.iirFilterSOS(b, a)._start()):
        with pytest.raises(cs.CsdrError) as e:
            make()
        assert e.value.code == -3 and "no CPU fallback" in str(e.value)


def test_existing_iirfilter_still_refuses_other_orders_before_anything_else():
    """csdr_iirfilt_create is untouched: order != 2 is CSDR_ERR_INVALID with or without a GPU"""
    h = C.c_void_p()
    assert _lib.lib().csdr_iirfilt_create(4, 0.1, 0.0, 10.0, 10.0, 1, 64, C.byref(h)) == _lib.ERR_INVALID


def _signal(shape, cplx, seed):
    rng = np.random.default_rng(seed)
    n = shape[-1]
    x = np.sin(2 * np.pi * 0.01 * np.arange(n)) + 0.3 * rng.standard_normal(shape)
    if cplx:
        x = x + 1j * (np.cos(2 * np.pi * 0.013 * np.arange(n)) + 0.3 * rng.standard_normal(shape))
    return x.astype(np.complex64 if cplx else f32)


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_restatement_f32_cascade_follows_f64_and_carries_its_state(cplx):
    """filter_f32 is the reference side of the GPU tests' bound: it has to be a sound sequential cascade.  Against the same
    coefficients in f64 (the figures the issue quotes for 6000 samples of sine + 0.3 noise: 2e-7 at (1, 0.1) .. 2.7e-5 at
    (8, 0.01)), and bit-identical under any chunking"""
    x = _signal((2, 6000), cplx, seed=5)
    for (n, fc), cap in (((1, 0.1), 2e-6), ((16, 0.1), 1e-5), ((7, 0.02), 5e-5), ((8, 0.01), 3e-4)):
        b, a = R.butter_lowpass_sos(n, f32(fc))
        y, st = R.filter_f32(b, a, x)
        err = float(np.abs(y - R.filter_f64(b, a, x)).max())
        print(f"({n}, {fc}) {'complex' if cplx else 'real'}: |filter_f32 - f64|max = {err:.2e}")
        assert y.dtype == x.dtype and err <= cap              # ten times the quoted figures: only a sanity cap
        outs, state, pos = [], None, 0
        for c in (1, 0, 1000, 7, 4992):
            o, state = R.filter_f32(b, a, x[:, pos:pos + c], state)
            outs.append(o)
            pos += c
        got = np.concatenate(outs, axis=1)
        assert pos == 6000 and np.array_equal(got.view(np.uint32), y.view(np.uint32)) and np.array_equal(state, st)


HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_k_iirsos_keeps_its_block_in_registers_and_static_lds(tmp_path):
    """both instantiations (real, complex): a thread's 16 samples, the prefetched next block and the scan state are register
    arrays indexed by unrolled loops (in scratch memory every section would pay a round trip per sample), and the block, the
    scan's ping-pong buffers and the carried states fit the 64 KiB of static LDS a workgroup may ask for"""
    src = os.path.join(ROOT, "composable_sdr_amd", "csrc", "kernels_iirsos.hip")
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-c", src, "-o", str(tmp_path / "iirsos.o"),
                          "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    blocks = [b for b in re.split(r"remark: Function Name: ", out.stderr)[1:] if "k_iirsos" in b.splitlines()[0]]
    assert len(blocks) == 2
    for b in blocks:
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, b[:400]
        assert int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) == 0, b[:400]
        assert int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1)) <= 64 * 1024, b[:400]
