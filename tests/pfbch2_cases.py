"""What test_pfbch2_cpu.py and test_pfbch2_gpu.py share about the launch shape of k_pfb2 (csdr_pfbch2_launch_shape, no GPU needed)."""
import ctypes as C

from composable_sdr_amd import _lib

FIELDS = ("F", "tiles", "tiles_per_run", "runs", "wgs_per_cu", "lds")


def shape(M, m, frames, cus):
    """how a call of `frames` frames runs on a device of `cus` compute units"""
    s = (C.c_uint32 * 6)()
    _lib.check(_lib.lib().csdr_pfbch2_launch_shape(M, m, frames, cus, s))
    return dict(zip(FIELDS, (int(v) for v in s)))


def runs_frames(M, m, cus):
    """a frame count at which at least three workgroups walk two tiles each and the last tile is ragged: one tile more than the
    device has workgroup slots, and 5 frames"""
    s = shape(M, m, 1, cus)
    return (cus * s["wgs_per_cu"] + 1) * s["F"] + 5
