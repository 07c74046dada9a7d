"""fskDemodulator without a GPU: the design's known answers, and the f32 arithmetic the kernel uses
(fsk_restatement.demod_f32) against the algorithm as liquid states it (demod_ref: f64, zero-padded K-point FFT).

Error model: a magnitude is the length of a sum of k products x_j W, each factor W a rounded table entry, each product and each
accumulation rounded once in f32, so |E32 - E64| <= (k + 8) 2^-24 sum_j |x_j| per symbol (a wrong bin would be off by the order
of sum |x|).  A decision may differ only where the two largest f64 magnitudes lie closer than twice that bound; the share of such
symbols is asserted to stay at or below 0.1 %."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fsk_restatement as F

f32 = np.float32

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


def _noise(n, seed):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)).astype(np.complex64)


def _fsk(m, k, bw, nsym, snr_db, seed):
    rng = np.random.default_rng(seed)
    sym = rng.integers(0, 1 << m, nsym).astype(np.uint32)
    return F.fskmod(sym, m, k, bw) + F.awgn(nsym * k, snr_db, rng), sym


@pytest.mark.parametrize("mkb,K,dmap", DESIGNS, ids=[str(d[0]) for d in DESIGNS])
def test_design_known_answers(mkb, K, dmap):
    gK, gmap = F.design(*mkb)
    assert gK == K and gmap.tolist() == dmap


INPUTS = [
    ("noise", (1, 8, 0.25), 400000),
    ("noise", (2, 10, 0.45), 200000),
    ("noise", (3, 32, 0.2), 60000),
    ("noise", (4, 64, 0.25), 30000),
    ("fsk3dB", (2, 16, 0.25), 60000),
    ("fsk0dB", (1, 2048, 0.25), 1500),
]


@pytest.mark.parametrize("kind,mkb,nsym", INPUTS, ids=[f"{i[0]}-{i[1]}" for i in INPUTS])
def test_f32_magnitudes_and_decisions_against_the_f64_statement(kind, mkb, nsym):
    m, k, bw = mkb
    if kind == "noise":
        x = _noise(nsym * k, seed=11 + k)
    else:
        x, _ = _fsk(m, k, bw, nsym, 3.0 if kind == "fsk3dB" else 0.0, seed=23 + k)
    s32, E32 = F.demod_f32(x, m, k, bw)
    s64, E64 = F.demod_ref(x, m, k, bw)
    B = F.bound(x, k)
    err = np.abs(E32.astype(np.float64) - E64).max(axis=1)
    unit = 2.0 ** -24 * np.abs(x.astype(np.complex128)).reshape(nsym, k).sum(axis=1)
    print(f"{kind} {mkb}: max |E32 - E64| = {(err / unit).max():.2f} units of 2^-24 sum|x| (bound {k + 8})")
    assert np.all(err <= B)
    top = np.sort(E64, axis=1)
    close = (top[:, -1] - top[:, -2]) < 2.0 * B
    share = close.mean()
    print(f"{kind} {mkb}: {close.sum()} of {nsym} symbols within twice the bound of a tie (share {share:.2e}); "
          f"{int((s32 != s64).sum())} decisions differ")
    assert share <= 1e-3
    assert np.array_equal(s32[~close], s64[~close])


@pytest.mark.parametrize("mkb", [(1, 8, 0.25), (2, 16, 0.25), (3, 32, 0.2)], ids=str)
def test_fsk_at_10_db_comes_back_without_errors(mkb):
    m, k, bw = mkb
    x, sym = _fsk(m, k, bw, 4000, 10.0, seed=5 + m)
    assert np.array_equal(F.demod_f32(x, m, k, bw)[0], sym)
    assert np.array_equal(F.demod_ref(x, m, k, bw)[0], sym)


def test_all_zero_input_gives_symbol_0():
    for m, k, bw in ((1, 8, 0.25), (3, 32, 0.2)):
        s, E = F.demod_f32(np.zeros(5 * k, np.complex64), m, k, bw)
        assert not s.any() and not E.any()


def test_exact_tie_gives_the_lower_index():
    # (1, 4, .25): K = 4, bins [3, 1].  x = (a, 0, b, 0) meets only W[0] and W[2] in both bins: the two sums are the same
    # operations on the same numbers, so the magnitudes are equal bit for bit whatever a and b are
    rng = np.random.default_rng(3)
    x = np.zeros((50, 4), np.complex64)
    x[:, 0] = rng.standard_normal(50) + 1j * rng.standard_normal(50)
    x[:, 2] = rng.standard_normal(50) + 1j * rng.standard_normal(50)
    x[0] = [2, 0, -2, 0]                                      # e^{2 pi i 3 j / 4} + e^{2 pi i j / 4}: both tones at once
    s, E = F.demod_f32(x.reshape(-1), 1, 4, 0.25)
    assert np.array_equal(E[:, 0].view(np.uint32), E[:, 1].view(np.uint32)) and E[0, 0] == 4.0
    assert not s.any()
    # (2, 8, .25): K = 12, bins [9, 11, 1, 3], all odd: sample 6 meets W[6] in every one of them, so (a, 0 .. 0, b, 0) ties all four
    y = np.zeros((20, 8), np.complex64)
    y[:, 0] = rng.standard_normal(20) + 1j * rng.standard_normal(20)
    y[:, 6] = rng.standard_normal(20) + 1j * rng.standard_normal(20)
    s, E = F.demod_f32(y.reshape(-1), 2, 8, 0.25)
    assert np.all(E.view(np.uint32) == E[:, :1].view(np.uint32)) and E.all() and not s.any()


HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_k_fskdem_keeps_its_accumulators_and_staged_loads_in_registers(tmp_path):
    """every instantiation (2, 4, 8, 16 tones per pass x 8- / 16-byte loads x table in LDS / global): the accumulators and the
    block in flight are register arrays indexed by unrolled loops; in scratch memory they would cost a round trip per sample"""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "composable_sdr_amd", "csrc", "kernels_fskdem.hip")
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-c", src, "-o", str(tmp_path / "fsk.o"),
                          "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    blocks = [b for b in re.split(r"remark: Function Name: ", out.stderr)[1:] if "k_fskdem" in b.splitlines()[0]]
    assert len(blocks) == 16
    for b in blocks:
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, b[:400]
        assert int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) == 0, b[:400]
