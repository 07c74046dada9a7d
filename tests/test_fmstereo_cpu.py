"""Stereo FM decoding (DeFMS) without a GPU: the CPU restatement's design and behaviour, and the new C ABI /
Python / C++ surface being present (creating the object must fail loudly with no device)."""
import functools
import os
import subprocess

import numpy as np
import pytest

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
