"""Stereo FM decoding (DeFMS) without a GPU: the CPU restatement's design and behaviour, and the new C ABI /
Python / C++ surface being present (creating the object must fail loudly with no device)."""
import functools
import os
import subprocess

import numpy as np
import pytest

import fms_cases as K
import fms_restatement as F
import oracle_lib as O
from host_exe import host_exe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("M", [4, 16, 64, 256])
def test_restatement_kaiser_is_the_oracle_prototype(M):
    """the anchor: liquid_firdes_kaiser as restated here gives the oracle's PFB prototype (n = 2 M m + 1, fc = 0.5 / M) bit for bit"""
    h = F.firdes_kaiser(2 * M * 7 + 1, 0.5 / M, 80.0)
    assert np.array_equal(h, O.kaiser_prototype(M, 7, 80.0))


def test_restatement_nco_arithmetic_is_the_oracle_s():
    x = np.random.default_rng(0).uniform(-30, 30, 3000).astype(np.float32)
    x[:4] = [0.0, -1e-12, 1e-12, -0.0]
    assert [int(v) for v in F.constrain(x)] == [O.nco_constrain(v) for v in x]
    th = np.random.default_rng(1).integers(0, 2 ** 32, 3000, dtype=np.uint64).astype(np.uint32)
    ph = F.phase(th)
    got = F._cos(ph) + 1j * F._sin(ph)
    want = np.array([O.nco_phasor(int(t)) for t in th])
    assert np.abs(got - want).max() <= 2 ** -23              # f64-then-rounded cos / sin vs libm's cosf / sinf: <= 1 ulp


def test_hs_atan2_quadrants():
    y = np.array([1, 1, -1, -1, 0, -0.0, 0, -0.0, 1, -1], np.float32)
    x = np.array([1, -1, 1, -1, -1, -1, 0, -0.0, 0, 0], np.float32)
    np.testing.assert_allclose(F.hs_atan2(y, x), np.arctan2(y, x), atol=3e-7)
    assert np.signbit(F.hs_atan2(np.float32(-0.0), np.float32(1.0)))


@pytest.mark.parametrize("q,N,d", [(192e3, 142, 71), (2.56e6, 1896, 948)])
def test_taps_and_delay(q, N, d):
    """N = round(q / 1350); d = round(groupdelay(pilot FIR, 100 / q)): the symmetric N-tap filter's (N - 1) / 2 plus f32 error,
    which at 192 kHz lands above 70.5 (70.500008), so d = 71 there"""
    P = F.design(q)
    assert (P["N"], P["d"]) == (N, d)
    assert abs(P["group_delay"] - (N - 1) / 2) < 1e-3
    assert P["d_nco"] == O.nco_constrain(np.float32(19000.0 * 2 * np.pi / q))


@pytest.mark.parametrize("q", sorted(K.DESIGNS))
def test_taps_and_delay_at_the_rates_of_the_shape_tests(q):
    """odd N (176.4 and 250 kHz), the limits of quad_rate, and the even N whose x.5 group delay f32 rounding decides: 240 kHz lands
    below 88.5, 256 kHz above 94.5.  tests/test_fmstereo_shapes_gpu.py holds the handle to the same literals"""
    P = F.design(q)
    print(f"{q:g} Hz: N {P['N']}, group delay {P['group_delay']:.6f} -> d {P['d']}")
    assert (P["N"], P["d"]) == K.DESIGNS[q]
    assert abs(P["group_delay"] - (P["N"] - 1) / 2) < 1e-3


@pytest.mark.parametrize("sums", ["f64", "f32"])
def test_decode_rows_over_calls_is_decode_of_each_row(sums):
    """decode_rows(calls=...) decimates per call as decode(calls=...) does; each row bit for bit, the PLL words too"""
    q, decim, calls = 40e3, 3, [7, 2, 0, 300, 1, 290]
    X = np.stack([np.float32(0.3 + r) * F.stereo_mpx(sum(calls), q, fl=400.0 + 300 * r, seed=70 + r) for r in range(3)])
    X[1] = np.float32(-0.0)
    got, th, dth = F.decode_rows(X, q, decim, calls=calls, sums=sums)
    assert got.shape == (3, 2 * sum(c // decim for c in calls))
    for r in range(3):
        want, st = F.decode(X[r], q, decim, calls=calls, sums=sums)
        assert np.array_equal(got[r].view(np.uint32), want.view(np.uint32)), r
        assert (int(th[r]), int(dth[r])) == (st["theta"], st["dtheta"]), r
    one, _, _ = F.decode_rows(X, q, decim, sums=sums)          # the default is one call
    assert one.shape == (3, 2 * (sum(calls) // decim))
    assert np.array_equal(one[0], F.decode(X[0], q, decim, sums=sums)[0])


def test_rounding_variant_of_the_restatement():
    """sums="f32" (FIR sums accumulated in f32, cosf / sinf from libm) is another rounding of the same decoder: the default is
    unchanged by the argument, the variant differs from it, by rounding noise only"""
    q, n = 40e3, 2048
    x = F.stereo_mpx(n, q, seed=5)
    base, st = F.decode(x, q, 2)
    same, _ = F.decode(x, q, 2, sums="f64")
    alt, st_alt = F.decode(x, q, 2, sums="f32")
    assert np.array_equal(base, same)
    assert not np.array_equal(base, alt)
    (l1, l2), (r1, r2) = K.stats(alt, base)
    assert max(l1, r1) < 1e-5 and max(l2, r2) < 1e-4
    assert abs(st["dtheta"] - st_alt["dtheta"]) / 2 ** 32 * q < 0.01
    h, v = F.firdes_kaiser(30, 0.02), np.random.default_rng(0).standard_normal(100).astype(np.float32)
    np.testing.assert_allclose(F._fir(h, v, np.float32(1), "f32"), F._fir(h, v, np.float32(1)), atol=1e-6)
    with pytest.raises(ValueError):
        F.decode(x, q, 2, sums="f16")


def _assert_caps(tag, pair, bounds):
    for ch, ((t1, t2), (b1, b2)) in enumerate(zip(pair, bounds)):
        print(f"{tag} {'LR'[ch]}: pair T1 {t1:.2e} T2 {t2:.2e} -> bound1 {b1:.2e} bound2 {b2:.2e}")
        assert K.MARGIN * t1 <= K.T1_CAP and K.MARGIN * t2 <= K.T2_CAP, (tag, t1, t2)
        assert 1e-5 <= b1 <= K.T1_CAP and 4e-5 <= b2 <= K.T2_CAP


@pytest.mark.parametrize("case", K.ONE_CALL, ids=[f"{q:g}-{decim}" for q, decim, _, _ in K.ONE_CALL])
def test_reference_pair_is_within_the_caps_one_call(case):
    """the bounds of tests/test_fmstereo_shapes_gpu.py come from the restatement's own rounding; for its inputs they stay
    below 2e-4 (T1) and 2e-3 (T2), far below what one wrong sample does (tests/fms_cases.py)"""
    x, ref = K.one_call(*case)
    assert ref.want.size == 2 * (x.size // case[1]) and np.all(np.isfinite(ref.want))
    _assert_caps(f"{case[0]:g} Hz decim {case[1]}", ref.pair, ref.bounds)


def test_reference_pair_is_within_the_caps_seams():
    x, calls, ref = K.seams()
    need = {1, 4, 5, 6, 15, 16, 17, 87, 88, 89, 176, 177, 178, 255, 256, 257, 264, 265, 266, 0}
    big = calls.index(max(calls))
    assert sum(calls) == x.size and need <= set(calls[:big]) and need <= set(calls[big + 1:]) and 2500 <= calls[big] <= 3500
    assert ref.want.size == 2 * sum(c // K.SEAM_DECIM for c in calls)
    _assert_caps("240 kHz decim 5 seams", ref.pair, ref.bounds)


def test_reference_pair_is_within_the_caps_67_rows():
    X, calls, ref = K.rows()
    assert X.shape == (K.ROWS_C, sum(calls)) and not np.any(X[1]) and not np.any(X[2])
    assert not np.any(np.signbit(X[1])) and np.all(np.signbit(X[2]))
    for r in range(K.ROWS_C):
        if r in K.ROWS_SILENT:
            assert not np.any(ref.want[r])                     # a silent row decodes to zeros (of either sign)
        else:
            _assert_caps(f"row {r}", ref.pair[r], ref.bounds[r])


@pytest.mark.parametrize("q", [40e3, 250e3])
def test_chunk_calls_hold_every_seam(q):
    N, d = K.DESIGNS[q]
    Hx = N - 1 + d
    calls = K.chunk_calls(q)
    need = {1, 2, 3, 15, 16, 17, d - 1, d, d + 1, N - 2, N - 1, N, Hx - 1, Hx, Hx + 1, 255, 256, 257, 0}
    big = calls.index(max(calls))
    assert sum(calls) == 8192 and need <= set(calls[:big]) and need <= set(calls[big + 1:]) and calls[big] > 3000


@functools.lru_cache(maxsize=None)
def _decoded(offset_hz):
    q, n = 192e3, 57600                                        # 0.3 s
    x = F.stereo_mpx(n, q, pilot_offset_hz=offset_hz, seed=3)
    return F.decode(x, q, 4)


@pytest.mark.parametrize("offset_hz", [0.0, 20.0])
def test_restatement_pll_locks(offset_hz):
    """after 0.3 s the PLL's step is within 1 Hz of the pilot: constrain(ncoF), plus the offset for an offset pilot"""
    q = 192e3
    _, st = _decoded(offset_hz)
    want = O.nco_constrain(np.float32(2 * np.pi * (19000.0 + offset_hz) / q))
    err_hz = (st["dtheta"] - want) / 2 ** 32 * q
    print(f"offset {offset_hz} Hz: d_theta {st['dtheta']} vs {want}: {err_hz:+.3f} Hz")
    assert abs(err_hz) < 1.0


@pytest.mark.parametrize("offset_hz", [0.0, 20.0])
def test_restatement_separates_channels(offset_hz):
    """L carries the 1 kHz tone, R the 3 kHz tone; after 50 ms each holds the other's at <= -20 dB"""
    q = 192e3
    lr, _ = _decoded(offset_hz)
    k = int(0.05 * q / 4)
    L, R = lr[0::2][k:], lr[1::2][k:]
    xl = 10 * np.log10(F.tone_power(L, 3000, q / 4) / F.tone_power(L, 1000, q / 4))
    xr = 10 * np.log10(F.tone_power(R, 1000, q / 4) / F.tone_power(R, 3000, q / 4))
    print(f"offset {offset_hz} Hz: cross-talk L {xl:.1f} dB, R {xr:.1f} dB")
    assert xl <= -20 and xr <= -20


def test_header_library_and_signatures_carry_fmstereo():
    import ctypes as C
    import composable_sdr_amd as cs
    from composable_sdr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "csdr.h")).read()
    names = ["csdr_fmstereo_create", "csdr_fmstereo_process", "csdr_fmstereo_process_device", "csdr_fmstereo_reset",
             "csdr_fmstereo_get_delay", "csdr_fmstereo_get_pll", "csdr_fmstereo_destroy"]
    if not os.path.exists(cs.lib_path()):
        cs.build_library()
    lib = C.CDLL(cs.lib_path())
    for n in names:
        assert n + "(" in hdr and n in _lib.SIGNATURES and hasattr(lib, n), n


def test_stereo_decoder_without_gpu_is_nodev():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import composable_sdr_amd as cs
    with pytest.raises(cs.CsdrError) as e:
        cs.stereoFMDecoder(192e3, 4)._start()
    assert e.value.code == -3


def test_cpp_host_parses_defms(tmp_path):
    """`--demod DeFMS 4` is an option of the C++ host (it used to stop with "unknown option 4")"""
    exe = host_exe("soapy_sdr_file")
    r = subprocess.run([exe, "--filename", "/nonexistent.cf32", "-n", "16", "--demod", "DeFMS", "4", "--audio", "AU", "-o",
                        str(tmp_path / "fms")], capture_output=True, text=True, timeout=120, env=dict(os.environ, CSDR_QUIET="1"))
    assert "unknown option" not in r.stderr, r.stderr
    assert r.returncode != 2, r.stderr


def test_fms_sequential_kernels_have_no_scratch(tmp_path):
    """k_fms_pll keeps (theta, d_theta) and the staged block in registers / LDS for the whole call: a scratch access would sit
    inside the per-sample recurrence.  Same for k_fms_deemph."""
    import re
    import shutil
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "composable_sdr_amd", "csrc", "kernels_fmstereo.hip")
    out = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-c", src, "-o", str(tmp_path / "fms.o"),
                          "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    blocks = {b.splitlines()[0]: b for b in re.split(r"remark: Function Name: ", out.stderr)[1:]}
    seen = 0
    for name, b in blocks.items():
        if "k_fms_pll" in name or "k_fms_deemph" in name:
            seen += 1
            assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, name
            assert int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) == 0, name
    assert seen == 2
