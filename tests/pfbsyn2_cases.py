"""What test_pfbsyn2_cpu.py and test_pfbsyn2_gpu.py share: the launch shape of k_pfb2s (csdr_pfbsyn2_launch_shape, no GPU needed), the
shapes and cuts of the parity cases, and the synthesizer's input: the analyzer's f64 closed form of the test stream, as CF32."""
import ctypes as C

import numpy as np

import pfbch2_restatement as A
from composable_sdr_amd import _lib

FIELDS = ("F", "tiles", "tiles_per_run", "runs", "wgs_per_cu", "lds")
SHAPES = [(4, 1), (8, 3), (32, 7), (64, 2), (256, 7), (256, 8)]
CUTS = [37, 1, 0, 9, 67]                  # frames per call: shorter than the reach of 4 m frames, empty, odd (the parity is carried)
FRAMES = sum(CUTS)


def shape(M, m, frames, cus):
    """how a call of `frames` frames runs on a device of `cus` compute units"""
    s = (C.c_uint32 * 6)()
    _lib.check(_lib.lib().csdr_pfbsyn2_launch_shape(M, m, frames, cus, s))
    return dict(zip(FIELDS, (int(v) for v in s)))


def runs_frames(M, m, cus):
    """a frame count at which at least three workgroups walk two tiles each and the last tile is ragged: one tile more than the
    device has workgroup slots, and 5 frames"""
    s = shape(M, m, 1, cus)
    return (cus * s["wgs_per_cu"] + 1) * s["F"] + 5


def rows(M, m, frames, seed):
    """realistic rows, computed on the CPU: the f64 closed form of the analyzer (its own prototype, 80 dB, fc = 1 / M) of
    pfbch2_restatement.stream, rounded to CF32; [M][frames]"""
    h = A.design(M, m, 80.0)[:2 * M * m]
    return np.ascontiguousarray(A.truth(h, A.stream(M, frames, seed), M).astype(np.complex64))
