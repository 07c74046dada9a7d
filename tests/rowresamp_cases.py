"""The cases tests/test_rowresamp_cpu.py and tests/test_rowresamp_gpu.py share: the rates, the (rate, m, kind) cases of the GPU
tests with their inputs, the launch shape as a dictionary, and the call sizes that end a call just short of, at and just behind a
tile of the kernel."""
import ctypes as C
import math

import numpy as np

import rowresamp_restatement as R
from composable_sdr_amd import _lib

FIELDS = ("P", "TO", "window", "lds", "wgs_per_cu", "tiles", "items_per_run", "runs")
RATES = [0.125, 0.16, 0.48, 0.5, 0.75, 1.0, 1.6, 8.0, 44100 / 48000]
AS_DB = 60.0
# (rate, m, complex): the largest bank at 0.125; mu = 0 always at 1.0; the shortest filter at the highest rate at (8, 1)
CASES = [(0.48, 7, True), (0.125, 7, True), (0.16, 7, False), (1.0, 7, False), (1.6, 7, True), (8.0, 1, False), (44100 / 48000, 4, True)]
IDS = [f"r{r:.4g}-m{m}-{'c' if c else 'r'}" for r, m, c in CASES]
ROWS = 3


def shape(rate, m, cplx, n_out, nchan, cus, T=0):
    s = (C.c_uint32 * 8)()
    _lib.check(_lib.lib().csdr_rowresamp_launch_shape(float(rate), m, int(cplx), n_out, nchan, cus, T, s))
    return dict(zip(FIELDS, (int(v) for v in s)))


def samples_for(T, delta, c):
    """the shortest call from time T that yields at least c >= 1 outputs (exactly c at rates <= 1)"""
    return ((T + (c - 1) * delta) >> 32) + 1


def length(rate, m):
    """samples per row of a case: about 3000, and enough for three calls of about a tile each with something left over"""
    TO = shape(rate, m, True, 1, 1, 256)["TO"]
    return max(3000, int(math.ceil((3 * TO + 2) / rate)) + 50)


def rows(nrows, n, cplx, seed):
    """unit-variance noise plus one tone per row, F32 or CF32 [nrows][n]"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    f = 0.05 + 0.31 * rng.random(nrows)
    if cplx:
        x = (rng.standard_normal((nrows, n)) + 1j * rng.standard_normal((nrows, n))) / np.sqrt(2.0) + np.exp(2j * np.pi * f[:, None] * t[None, :])
        return x.astype(np.complex64)
    return (rng.standard_normal((nrows, n)) + np.cos(2.0 * np.pi * f[:, None] * t[None, :])).astype(np.float32)


def tile_cuts(rate, m, n):
    """call sizes that yield one output fewer than a tile, a tile exactly, one more than a tile (at rates above 1: the nearest
    count from above), and the rest of n"""
    delta = R.delta_of(rate)
    TO = shape(rate, m, True, 1, 1, 256)["TO"]
    T, cuts = 0, []
    for c in (TO - 1, TO, TO + 1):
        k = samples_for(T, delta, c)
        got, T = R.step(T, delta, k)
        assert got >= c and (rate > 1 or got == c)
        cuts.append(k)
    assert sum(cuts) < n, (cuts, n)
    return cuts + [n - sum(cuts)]


# the end-to-end case: 2-FSK at 25 / 3 samples per symbol behind 4 zeros, resampled by 0.48 to 4 samples per symbol
FSK_SYMBOLS, FSK_SPS, FSK_K, FSK_BW, FSK_PAD, FSK_LAG = 400, 25.0 / 3.0, 4, 0.25, 4, 3


def fsk_rows(seed=17):
    """(symbols [3][400], x CF32 [3][4 + 3333])"""
    rng = np.random.default_rng(seed)
    sym = rng.integers(0, 2, (ROWS, FSK_SYMBOLS))
    x = np.stack([np.concatenate([np.zeros(FSK_PAD, np.complex64), R.fskmod(s, FSK_SPS, FSK_BW * 0.48)]) for s in sym])
    return sym.astype(np.uint32), x
