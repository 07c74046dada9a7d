"""Time of k_iirsos (csdr_iirsos_*) on device-resident planes, one JSON line: the median hipEvent time of
`--reps` calls after one warm-up call, with the achieved GB/s on the algorithmic bytes (one read and one write per sample,
whatever the number of sections), for
  real, S = 1 (order 2)        on [64][n]
  complex, S = 4 (order 8)     on [64][n]
A row is one workgroup's work, so 64 rows occupy 64 of the device's compute units: the figures are those of a latency-bound
launch, not of the memory system.  The clock the device held during a run is not read.

With `--trace DIR` a child process runs the yardstick pair under `rocprofv3 --kernel-trace --stats` (no counters): on one
[64][n] F32 plane, iirFilter 2 (k_biquad, through the host path) and k_iirsos<real> at S = 1 with the same design, alternating,
`--reps` + 1 launches each.  The kernels' own times from the trace (mean, min, max, standard deviation) are reported: k_iirsos at
S = 1 is meant to take no longer than k_biquad plus k_biquad's own run-to-run spread in that trace."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = [(False, 2, 64), (True, 8, 64)]
FC = 0.025


def plane(C, n, cplx):
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    return torch.randn((C, n, 2) if cplx else (C, n), generator=g, device="cuda", dtype=torch.float32) * 0.7071


def run(C, n, cplx, order, reps):
    import numpy as np
    import torch
    import composable_sdr_amd as cs
    d_x = plane(C, n, cplx)
    d_y = torch.empty_like(d_x)
    h = cs.IirSos.prototype(order, FC, is_complex=cplx, nchan=C, max_samples=n)
    S = h.nsec
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for i in range(reps + 1):
        ev[0].record()
        h.process_device(d_x.data_ptr(), n, d_y.data_ptr(), torch.cuda.current_stream().cuda_stream)
        ev[1].record()
        torch.cuda.synchronize()
        if i:
            times.append(ev[0].elapsed_time(ev[1]) * 1e3)
    h.close()
    us = float(np.median(times))
    el = 8 if cplx else 4
    return dict(kind="complex" if cplx else "real", sections=S, plane=[C, n], us=round(us, 1), min_us=round(float(np.min(times)), 1),
                max_us=round(float(np.max(times)), 1), gbps=round(2 * el * C * n / us * 1e-3, 1))


def yardstick(C, n, reps):
    """iirFilter 2 (host path) and k_iirsos<real> at S = 1 with the same design on the same plane, alternating"""
    import torch
    import composable_sdr_amd as cs
    d_x = plane(C, n, False)
    d_y = torch.empty_like(d_x)
    x = d_x.cpu().numpy()
    old = cs.iirFilter(2, FC, nchan=C, max_samples=n)
    r = old._start()
    new = cs.IirSos.prototype(2, FC, is_complex=False, nchan=C, max_samples=n)
    for _ in range(reps + 1):
        old._process(r, x)
        new.process_device(d_x.data_ptr(), n, d_y.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    old._done(r)
    new.close()


def trace(a):
    os.makedirs(a.trace, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", a.trace, "-o", "t", "--", sys.executable, os.path.abspath(__file__),
           "--reps", str(a.reps), "--n", str(a.n), "--yardstick-child"]
    log = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
    if log.returncode != 0:
        raise SystemExit(f"traced run failed ({log.returncode}): {log.stderr[-2000:]}")
    out = {}
    for f in glob.glob(os.path.join(a.trace, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            name = row["Name"]
            key = "k_iirsos<real>" if "k_iirsos<false>" in name else "k_biquad" if "k_biquad(" in name else None
            if key:
                out[key] = dict(calls=int(row["Calls"]), avg_us=round(float(row["AverageNs"]) * 1e-3, 1), min_us=round(float(row["MinNs"]) * 1e-3, 1),
                                max_us=round(float(row["MaxNs"]) * 1e-3, 1), std_us=round(float(row.get("StdDev", "nan")) * 1e-3, 2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--trace", default="", help="directory for a rocprofv3 kernel trace of a child run of the yardstick pair")
    ap.add_argument("--yardstick-child", action="store_true", help="run the yardstick pair only (what --trace starts)")
    ap.add_argument("--timeout", type=int, default=400)
    a = ap.parse_args()
    if a.yardstick_child:
        yardstick(64, a.n, a.reps)
        return
    res = dict(tool="iirsos_time", runs=[run(C, a.n, cplx, order, a.reps) for cplx, order, C in CONFIGS])
    if a.trace:
        res["yardstick_plane"] = [64, a.n]
        res["kernel_trace_us"] = trace(a)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
