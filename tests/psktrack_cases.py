"""The signals and the scoring that tests/test_psktrack_cpu.py and tests/test_psktrack_gpu.py share."""
import math

import numpy as np

import symsyncc_restatement as SC

# (carrier offset in cycles per symbol, carrier phase in radians, amplitude)
CONDITIONS = [(0.0, 0.3, 1.0), (0.002, 2.0, 0.05), (-0.003, 1.0, 20.0)]
CHANNELS = [np.array([1.0, 0.3 * np.exp(1j)]), np.array([1.0, 0.0, 0.3 * np.exp(1j)])]      # two paths, T/2 taps
M_RRC, BETA = 5, 0.25
DELAY = 2 * 2 * M_RRC                                            # shaping + matched filter at 2 samples per symbol


def symbols(nsym, bits, seed):
    """(points complex128 of unit modulus, symbol numbers in the block's Gray code: bit 0 = re < 0, bit 1 = im < 0)"""
    rng = np.random.default_rng(seed)
    bI = rng.integers(0, 2, nsym)
    if bits == 1:
        return (1.0 - 2.0 * bI) + 0j, bI.astype(np.uint32)
    bQ = rng.integers(0, 2, nsym)
    return ((1.0 - 2.0 * bI) + 1j * (1.0 - 2.0 * bQ)) / math.sqrt(2.0), (bI | (bQ << 1)).astype(np.uint32)


def matched(sym, channel=None):
    """the symbols shaped by RRC(k 2, m 5, beta 0.25), through `channel` (T/2 taps) and the matched filter, at 2 samples per
    symbol and ideal timing: symbol i sits at sample DELAY + 2 i with gain 1 (complex128)"""
    h = SC.rrc_f64(2, M_RRC, BETA)
    up = np.zeros(2 * sym.size, np.complex128)
    up[::2] = sym
    x = np.convolve(up, h)
    if channel is not None:
        x = np.convolve(x, channel)
    return np.convolve(x, h) / 2.0


def impaired(x2, offset, phase, amp):
    """x2 (2 samples per symbol) with a carrier of `offset` cycles per symbol, a phase and an amplitude"""
    t = np.arange(x2.size)
    return amp * x2 * np.exp(1j * (2.0 * math.pi * offset * t / 2.0 + phase))


def rows(nsym, bits, sps, seed=0, channel=None, conditions=CONDITIONS):
    """one row per condition, complex64 [len(conditions)][n]: at sps 2 the matched signal from its first sample (symbol
    instants at even samples: phase 0), at sps 1 its symbol instants only.  Returns (rows, points, symbol numbers)"""
    pts, num = symbols(nsym, bits, seed)
    x2 = matched(pts, channel)
    X = np.stack([impaired(x2, *c) for c in conditions])
    if sps == 1:
        X = X[:, ::2]
    return X.astype(np.complex64), pts, num


def score(y, k, pts, num, bits, skip):
    """decisions k and soft symbols y after the first `skip` outputs against the transmitted symbols at the best lag (within 16
    symbols of the filters' delay) and the best rotation of the modem's ambiguity (BPSK 0, pi; QPSK multiples of pi / 2):
    (decision errors, compared, evm).  The errors are counted on the block's own decisions k, mapped back through the
    rotation; evm = rms |y / g - rot sym| with g the least-squares real gain"""
    y = np.asarray(y, np.complex128)[skip:]
    k = np.asarray(k)[skip:]
    rots = [1, -1] if bits == 1 else [1, 1j, -1, -1j]
    first = skip - DELAY // 2
    best = None
    for lag in range(max(0, first - 16), first + 17):
        ref, rnum = pts[lag:lag + y.size], num[lag:lag + y.size]
        n = min(ref.size, y.size)
        if n < 16:
            continue
        for rot in rots:
            want = rot * ref[:n]
            if bits == 1:
                wk = (want.real < 0).astype(np.uint32)
            else:
                wk = (want.real < 0).astype(np.uint32) | ((want.imag < 0).astype(np.uint32) << 1)
            e = int(np.sum(wk != k[:n]))
            g = float(np.real(np.vdot(want, y[:n])) / n)
            evm = float(np.sqrt(np.mean(np.abs(y[:n] / g - want) ** 2))) if g > 0 else float("inf")
            if best is None or (e, evm) < (best[0], best[2]):
                best = (e, n, evm)
    return best
