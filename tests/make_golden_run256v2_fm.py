#!/usr/bin/env python3
"""Records tests/golden/run256v2_fm_small.npz: what k_run256v2<FM> (256 channels, FM, AGC off, through the C ABI) writes for the
small plans of tests/test_run256v2_fm_bitexact.py.

This is a BUILD golden, not a reference golden: the numbers come from the library as built from the PARENT of the commit that
changed the tile loop's LDS waits and read placement (csrc/kernels_fused_v2.hip), run on an MI355X.  That
commit changes no floating-point operation and no order of operations, so its outputs must equal the parent's bit for bit; the
oracle comparison in the test is separate.  Re-record only from a build whose arithmetic is meant to be the new truth (needs the
GPU), from the repo root:
    python tests/make_golden_run256v2_fm.py

The whole outputs are 3.4 MB of float32 (256 rows x 256 / 768 / 784 / 2 x 768 frames), more than a committed file may hold, so the fixture
keeps per case the sha256 of the output's bytes ([256][frames] float32, C order) and, to say where a mismatch sits, the four rows around
DC (126..129) and the first 16 frames of every row in full.

Input: integers from numpy's PCG64 scaled by 2^-15, so every sample is exact in float32 and the same on every machine (no libm call
in its making); its sha256 is in the fixture too.  |DC| = 0.36 as in test_chain_params_gpu._input: a wrong run-start state shows."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "run256v2_fm_small.npz")

M, KF, ALPHA, SEED = 256, 0.3, 0.0005, 2609
NF = 2 * 16 * 48                                   # frames of the stream; every case takes a prefix
# (id, frames of each call on one handle).  Runs are at least 8 tiles long (FusedPlan::run_kernel), boundaries on even tiles:
#   16 x 16   two runs of eight tiles, the smallest plan with a cold run start
#   16 x 48   six runs of eight: even and odd tiles of a pair in every run (the held half-lines of the even tile)
#   16 x 49   the last run has nine tiles: its last tile is an even tile without a partner and stores its own half-lines
#   2 calls   stash, DC state and FIR window carried into the second call; its run 0 starts from them, not cold
CASES = [
    ("two_runs_16x16", [16 * 16]),
    ("six_runs_16x48", [16 * 48]),
    ("odd_last_tile_16x49", [16 * 49]),
    ("two_calls_16x48", [16 * 48, 16 * 48]),
]
DC_ROWS = [126, 127, 128, 129]


def stream():
    rng = np.random.Generator(np.random.PCG64(SEED))
    v = rng.integers(-4096, 4096, size=(M * NF, 2), dtype=np.int64) + np.array([9830, 6554])
    return (v.astype(np.float32) / np.float32(32768.0)).view(np.complex64).reshape(-1)


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def run_case(cs, x, frames, flags):
    """the calls of one case on a fresh handle: output [256][sum(frames)], timed kernel of each call"""
    ch = cs.Chain(channels=M, kf=KF, demod="fm", dc_alpha=ALPHA, max_frames=max(frames), flags=flags)
    outs, names, pos = [], [], 0
    for f in frames:
        outs.append(ch.process(x[pos * M:(pos + f) * M]))
        names.append(ch.kernel_time()[0])
        pos += f
    ch.close()
    return np.ascontiguousarray(np.concatenate(outs, axis=-1), dtype=np.float32), names


if __name__ == "__main__":
    os.environ["CSDR_DIAG"] = "1"
    os.environ["CSDR_RUN_MIN_TILES"] = "1"
    sys.path.insert(0, os.path.dirname(HERE))
    import composable_sdr_amd as cs
    from composable_sdr_amd import _lib
    x = stream()
    rec = {"x_sha256": digest(x)}
    for tag, frames in CASES:
        got, names = run_case(cs, x, frames, _lib.FLAG_QUIET | _lib.FLAG_TIME_KERNELS)
        again, _ = run_case(cs, x, frames, _lib.FLAG_QUIET | _lib.FLAG_TIME_KERNELS)
        assert all(n == "k_run256v2<FM>" for n in names), names
        assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), tag
        rec[tag + "_sha256"] = digest(got)
        rec[tag + "_dc_rows"] = got[DC_ROWS]
        rec[tag + "_head"] = got[:, :16]
        print(tag, names, got.shape, bytes(rec[tag + "_sha256"]).hex())
    np.savez_compressed(GOLD, **rec)
    print(GOLD, os.path.getsize(GOLD))
