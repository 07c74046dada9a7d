"""Time of k_rowresamp (csdr_rowresamp_*) on device-resident buffers, one JSON line: per (rate, kind) the median
and the minimum hipEvent time of `--reps` calls of `--rows` rows x `--samples` samples after `--warmup` warm-up calls, the input
rate in GS/s and the share of 8 TB/s that 8 (1 + r) (complex) or 4 (1 + r) (real) algorithmic bytes per input sample amount to.
Every call continues the stream of the one before.  Events bracket one launch each, so the figure is the kernel's time plus the
events' own cost on the stream (a few microseconds); the clock the device held is not read.

  python tools/rowresamp_time.py                          r in {0.48, 0.16, 1.6}, complex and real, 256 rows x 65536 samples
  python tools/rowresamp_time.py --case 0.125:c --rows 64"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12


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


def run(rate, cplx, m, rows, samples, reps, warmup):
    import torch
    import composable_sdr_amd as cs
    per = 2 if cplx else 1
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    d_x = torch.randn((rows, samples, per), generator=g, device="cuda", dtype=torch.float32)
    h = cs.RowResamp(rate, m, 60.0, 0.0, cplx, rows, samples)
    d_y = torch.zeros((rows * h.max_out(samples) * per,), device="cuda", dtype=torch.float32)
    stream = torch.cuda.current_stream().cuda_stream
    counts = []
    us, min_us = _timed(lambda: counts.append(h.process_device(d_x.data_ptr(), samples, d_y.data_ptr(), stream)), reps, warmup)
    bank, _ = h.design()
    h.close()
    assert bool(torch.isfinite(d_y).all())
    nbytes = 4 * per * (1.0 + rate) * rows * samples
    return dict(rate=rate, kind="c" if cplx else "r", m=m, P=int(bank.shape[1]), rows=rows, samples=samples, n_out=counts[-1], us=round(us, 1),
                min_us=round(min_us, 1), gsps_in=round(rows * samples / us * 1e-3, 2), share_of_8TBps=round(nbytes / (us * 1e-6) / HBM_BYTES_PER_S, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", action="append", default=[], help="rate:c or rate:r (may be given more than once)")
    ap.add_argument("--m", type=int, default=7)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--samples", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    cases = [(float(c.split(":")[0]), c.split(":")[1] == "c") for c in a.case] or [(r, k) for r in (0.48, 0.16, 1.6) for k in (True, False)]
    print(json.dumps(dict(tool="rowresamp_time", runs=[run(r, k, a.m, a.rows, a.samples, a.reps, a.warmup) for r, k in cases])))


if __name__ == "__main__":
    main()
