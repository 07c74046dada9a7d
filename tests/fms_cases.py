"""The inputs, call lists and error bounds of tests/test_fmstereo_shapes_gpu.py, in one place so that
tests/test_fmstereo_cpu.py asserts the caps on exactly what the GPU file runs.  Test infrastructure.

How close the kernels must be to the restatement is not a number per rate: it is taken, per case, from the restatement alone.
`F.decode(..., sums="f32")` is the same decoder with its FIR sums accumulated in f32 and its cos / sin from libm's cosf / sinf;
the distance between it and the default (f64 sums, rounded once) is one sample of how far the output moves under rounding.  The
kernels (FMA sums, the device sincosf / atanf) are a third sample of the same noise, and the difference of two such samples is
sqrt 2 of one, so with
    T1 = rel-RMS of got - want,  T2 = max |got - want| / rms(want)           per channel (L, R) and row
the bounds are
    bound1 = 4 max(T1(pair), 2.5e-6)  (never below the project's 1e-5),  bound2 = 4 max(T2(pair), 1e-5).
The margin of 4 leaves room for the tail without hiding a wrong sample: one output wrong by 1 % of the signal in 4096 moves T2
by 1e-2, and the caps 4 T1(pair) <= 2e-4, 4 T2(pair) <= 2e-3 (asserted on the CPU for every case here) keep every bound below that.
"""
import collections
import functools

import numpy as np

import fms_restatement as F

MARGIN, T1_FLOOR, T2_FLOOR = 4.0, 2.5e-6, 1e-5
T1_CAP, T2_CAP = 2e-4, 2e-3

# quad_rate -> (N, d) as the restatement's design gives them (every rate is exact in f32).  For even N the group delay is x.5
# and f32 rounding decides d: 240 kHz rounds down (88.49998), 192 and 256 kHz round up (70.50001, 94.50005)
DESIGNS = {40e3: (30, 15), 176.4e3: (131, 65), 240e3: (178, 88), 250e3: (185, 92), 256e3: (190, 95), 2.7e6: (2000, 1000)}

# (quad_rate, decim, n, tone frequencies): one row, one call.  The last is the decimation limit: five outputs per channel from an
# 81921-tap decimator that is mostly history; its tones sit inside that decimator's 23 Hz passband so that the outputs have a scale
ONE_CALL = [(40e3, 1, 8192, (1000.0, 3000.0)), (240e3, 5, 12288, (1000.0, 3000.0)), (250e3, 3, 12288, (1000.0, 3000.0)),
            (2.7e6, 8, 16384, (1000.0, 3000.0)), (2.7e6, 64, 16384, (1000.0, 3000.0)),
            (192e3, 4096, 5 * 4096 + 7, (5.0, 9.0))]

Ref = collections.namedtuple("Ref", "want theta dtheta pair bounds")


def stats(got, want):
    """interleaved L, R -> ((T1, T2) of L, (T1, T2) of R)"""
    out = []
    for ch in (0, 1):
        g, w = np.asarray(got[ch::2], np.float64), np.asarray(want[ch::2], np.float64)
        rms = np.sqrt(np.mean(w ** 2))
        out.append((float(np.sqrt(np.mean((g - w) ** 2)) / rms), float(np.abs(g - w).max() / rms)))
    return tuple(out)


def bounds(pair):
    return tuple((MARGIN * max(t1, T1_FLOOR), MARGIN * max(t2, T2_FLOOR)) for t1, t2 in pair)


def within_caps(pair):
    return all(MARGIN * t1 <= T1_CAP and MARGIN * t2 <= T2_CAP for t1, t2 in pair)


def check(tag, got, ref_want, ref_bounds, ref_pair):
    """print both statistics and both bounds per channel, then assert; returns the statistics"""
    st = stats(got, ref_want)
    for ch, ((t1, t2), (b1, b2), (p1, p2)) in enumerate(zip(st, ref_bounds, ref_pair)):
        print(f"{tag} {'LR'[ch]}: T1 {t1:.2e} (pair {p1:.2e}, bound {b1:.2e})  T2 {t2:.2e} (pair {p2:.2e}, bound {b2:.2e})")
    for ch, ((t1, t2), (b1, b2)) in enumerate(zip(st, ref_bounds)):
        assert t1 <= b1 and t2 <= b2, (tag, "LR"[ch], t1, b1, t2, b2)
    return st


def _ref(x, q, decim, calls):
    want, st = F.decode(x, q, decim, calls=calls)
    pair = stats(F.decode(x, q, decim, calls=calls, sums="f32")[0], want)
    want.setflags(write=False)
    return Ref(want, st["theta"], st["dtheta"], pair, bounds(pair))


@functools.lru_cache(maxsize=None)
def one_call(q, decim, n, tones):
    """-> (x, Ref) of one ONE_CALL entry"""
    x = F.stereo_mpx(n, q, fl=tones[0], fr=tones[1], pilot_offset_hz=0.0, seed=11)
    x.setflags(write=False)
    return x, _ref(x, q, decim, None)


def _both_sides(small, n):
    """the small call sizes, one long call, the small sizes again in reverse: n samples in all"""
    long = n - 2 * sum(small)
    assert long > 0
    return list(small) + [long] + list(small)[::-1]


# ---- call seams, decim 5 at 240 kHz: N = 178, d = 88, Hx = 265 -------------------------------------------------------------
SEAM_Q, SEAM_DECIM, SEAM_N = 240e3, 5, 8192
SEAM_CALLS = _both_sides([1, 4, 5, 6, 15, 16, 17, 87, 88, 89, 176, 177, 178, 255, 256, 257, 264, 265, 266, 0], SEAM_N)


@functools.lru_cache(maxsize=None)
def seams():
    """-> (x, calls, Ref)"""
    x = F.stereo_mpx(SEAM_N, SEAM_Q, pilot_offset_hz=0.0, seed=11)
    x.setflags(write=False)
    return x, SEAM_CALLS, _ref(x, SEAM_Q, SEAM_DECIM, SEAM_CALLS)


# ---- chunking at decim 1 (GPU against itself) -------------------------------------------------------------------------------
def chunk_calls(q, n=8192):
    N, d = DESIGNS[q]
    Hx = N - 1 + d
    return _both_sides([1, 2, 3, 15, 16, 17, d - 1, d, d + 1, N - 2, N - 1, N, Hx - 1, Hx, Hx + 1, 255, 256, 257, 0], n)


# ---- 67 rows at (250 kHz, 3): a partial wave in k_fms_pll (3 lanes) and in k_fms_deemph (6 lanes), two silent rows ----------
ROWS_Q, ROWS_DECIM, ROWS_C, ROWS_CALLS = 250e3, 3, 67, [1500, 2, 2594]
ROWS_SILENT = (1, 2)                                           # all +0.0, all -0.0
RowsRef = collections.namedtuple("RowsRef", "want theta dtheta pair bounds")


@functools.lru_cache(maxsize=None)
def rows():
    """-> (X [67][4096], calls, RowsRef): rows differ in pilot phase, tone frequencies and amplitude (0.05 .. 1.5), all on
    frequency; pair and bounds hold None for the silent rows"""
    n = sum(ROWS_CALLS)
    amp = np.geomspace(0.05, 1.5, ROWS_C).astype(np.float32)
    X = np.stack([amp[r] * F.stereo_mpx(n, ROWS_Q, fl=300.0 + 40.0 * r, fr=2500.0 + 55.0 * r, pilot_offset_hz=0.0, seed=200 + r)
                  for r in range(ROWS_C)]).astype(np.float32)
    X[1] = np.float32(0.0)
    X[2] = np.float32(-0.0)
    X.setflags(write=False)
    want, th, dth = F.decode_rows(X, ROWS_Q, ROWS_DECIM, calls=ROWS_CALLS)
    alt, _, _ = F.decode_rows(X, ROWS_Q, ROWS_DECIM, calls=ROWS_CALLS, sums="f32")
    pair = [None if r in ROWS_SILENT else stats(alt[r], want[r]) for r in range(ROWS_C)]
    want.setflags(write=False)
    return X, ROWS_CALLS, RowsRef(want, th, dth, pair, [None if p is None else bounds(p) for p in pair])
