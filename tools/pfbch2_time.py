"""Time of k_pfb2 (csdr_pfbch2_*) on device-resident buffers, one JSON line: per (M, m) the median and the
minimum hipEvent time of `--reps` calls of `--frames` frames after `--warmup` warm-up calls, the input rate in GS/s and the share
of 8 TB/s that 24 algorithmic bytes per input sample amount to (8 read, 16 written: two CF32 outputs per input at twice the
critical rate).  Every call continues the stream of the one before.  Events bracket one launch each, so the figure is the
kernel's time plus the events' own cost on the stream (a few microseconds); the clock the device held is not read.

  python tools/pfbch2_time.py                        (256, 7) and (64, 7) at 2^18 frames per call
  python tools/pfbch2_time.py --shape 32:7 --frames 65536"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12
BYTES_PER_SAMPLE = 24


def run(M, m, frames, reps, warmup):
    import numpy as np
    import torch
    import composable_sdr_amd as cs
    n = frames * (M // 2)
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    d_x = torch.randn((n, 2), generator=g, device="cuda", dtype=torch.float32) * 0.7071
    d_y = torch.empty((M, frames, 2), device="cuda", dtype=torch.float32)
    h = cs.Firpfbch2.kaiser(M, m, 80.0, 0.0, max_frames=frames)
    stream = torch.cuda.current_stream().cuda_stream
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for i in range(warmup + reps):
        ev[0].record()
        h.process_device(d_x.data_ptr(), n, d_y.data_ptr(), stream)
        ev[1].record()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(ev[0].elapsed_time(ev[1]) * 1e3)
    h.close()
    assert bool(torch.isfinite(d_y).all())
    us = float(np.median(times))
    return dict(M=M, m=m, frames=frames, samples=n, us=round(us, 1), min_us=round(float(np.min(times)), 1),
                gsps=round(n / us * 1e-3, 2), share_of_8TBps=round(BYTES_PER_SAMPLE * n / (us * 1e-6) / HBM_BYTES_PER_S, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", default=[], help="M:m (may be given more than once)")
    ap.add_argument("--frames", type=int, default=1 << 18)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split(":")) for s in a.shape] or [(256, 7), (64, 7)]
    print(json.dumps(dict(tool="pfbch2_time", bytes_per_sample=BYTES_PER_SAMPLE, runs=[run(M, m, a.frames, a.reps, a.warmup) for M, m in shapes])))


if __name__ == "__main__":
    main()
