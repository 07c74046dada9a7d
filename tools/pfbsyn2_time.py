"""Time of k_pfb2s (csdr_pfbsyn2_*) on device-resident buffers, one JSON line: per (M, m) the median and the
minimum hipEvent time of `--reps` calls of `--frames` frames after `--warmup` warm-up calls, the output rate in GS/s and the share
of 8 TB/s that 24 algorithmic bytes per output sample amount to (16 read, 8 written: two CF32 inputs per output at twice the
critical rate).  The analyzer (k_pfb2, tools/pfbch2_time.py's figure) is timed on the same shapes in the same run, for context.
Every call continues the stream of the one before.  Events bracket one launch each, so the figure is the kernel's time plus the
events' own cost on the stream (a few microseconds); the clock the device held is not read.

  python tools/pfbsyn2_time.py                        (256, 7) and (64, 7) at 2^18 frames per call
  python tools/pfbsyn2_time.py --shape 32:7 --frames 65536"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12
BYTES_PER_SAMPLE = 24


def _timed(call, reps, warmup):
    import numpy as np
    import torch
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for i in range(warmup + reps):
        ev[0].record()
        call()
        ev[1].record()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(ev[0].elapsed_time(ev[1]) * 1e3)
    return float(np.median(times)), float(np.min(times))


def run(M, m, frames, reps, warmup):
    import torch
    import composable_sdr_amd as cs
    n = frames * (M // 2)
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    d_y = torch.randn((M, frames, 2), generator=g, device="cuda", dtype=torch.float32) * 0.7071
    d_x = torch.empty((n, 2), device="cuda", dtype=torch.float32)
    stream = torch.cuda.current_stream().cuda_stream
    syn = cs.Firpfbch2Synth.kaiser(M, m, 80.0, 0.0, max_frames=frames)
    us, min_us = _timed(lambda: syn.process_device(d_y.data_ptr(), frames, d_x.data_ptr(), stream), reps, warmup)
    syn.close()
    assert bool(torch.isfinite(d_x).all())
    # the analyzer on the same shape: x -> rows, the same 24 bytes per sample of the full-rate stream
    d_rows = torch.empty((M, frames, 2), device="cuda", dtype=torch.float32)
    ana = cs.Firpfbch2.kaiser(M, m, 80.0, 0.0, max_frames=frames)
    ana_us, ana_min = _timed(lambda: ana.process_device(d_x.data_ptr(), n, d_rows.data_ptr(), stream), reps, warmup)
    ana.close()
    return dict(M=M, m=m, frames=frames, samples=n, us=round(us, 1), min_us=round(min_us, 1), gsps=round(n / us * 1e-3, 2),
                share_of_8TBps=round(BYTES_PER_SAMPLE * n / (us * 1e-6) / HBM_BYTES_PER_S, 3),
                analyzer_us=round(ana_us, 1), analyzer_min_us=round(ana_min, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", default=[], help="M:m (may be given more than once)")
    ap.add_argument("--frames", type=int, default=1 << 18)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split(":")) for s in a.shape] or [(256, 7), (64, 7)]
    print(json.dumps(dict(tool="pfbsyn2_time", bytes_per_sample=BYTES_PER_SAMPLE, runs=[run(M, m, a.frames, a.reps, a.warmup) for M, m in shapes])))


if __name__ == "__main__":
    main()
