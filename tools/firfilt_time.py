"""Time of k_firfilt (csdr_firfilt_*) on device-resident planes, one JSON line: the median hipEvent time of
`--reps` calls after one warm-up call, with the achieved GB/s on the algorithmic bytes (one read and one write per sample) and
GFLOP/s at 2 L flops per real and 4 L per complex sample, for
  (real, 21 taps) and (complex, 65 taps) on [256][n]     bound by memory
  (complex, 889 taps) on [16][n]                         bound by the multiply-adds
The clock the device held during a run is not read.

With `--trace DIR` a child process runs the yardstick pair under `rocprofv3 --kernel-trace --stats` (no counters): on one
[64][n] F32 plane, firDecimator 1 (k_firdecim at decimation 1: 21 taps, every input re-read 21 times through the caches, nothing
staged; through the host path) and k_firfilt<real> with the same 21 taps, alternating, `--reps` launches each.  The kernels' own
times from the trace (mean, min, max, standard deviation) are reported: k_firfilt is meant to take no longer than k_firdecim."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = [(False, 21, 256), (True, 65, 256), (True, 889, 16)]


def plane(C, n, cplx):
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    return torch.randn((C, n, 2) if cplx else (C, n), generator=g, device="cuda", dtype=torch.float32) * 0.7071


def run(C, n, cplx, L, reps):
    import numpy as np
    import torch
    import composable_sdr_amd as cs
    d_x = plane(C, n, cplx)
    d_y = torch.empty_like(d_x)
    h = cs.FirFilt.kaiser(L, 0.1, 60.0, is_complex=cplx, nchan=C, max_samples=n)
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
    flops = (4 if cplx else 2) * L * C * n
    return dict(kind="complex" if cplx else "real", taps=L, plane=[C, n], us=round(us, 1), min_us=round(float(np.min(times)), 1),
                gbps=round(2 * el * C * n / us * 1e-3, 1), gflops=round(flops / us * 1e-3, 1))


def yardstick(C, n, reps):
    """firDecimator 1 (host path) and k_firfilt<real> with the same taps on the same plane, alternating"""
    import torch
    import composable_sdr_amd as cs
    d_x = plane(C, n, False)
    d_y = torch.empty_like(d_x)
    x = d_x.cpu().numpy()
    dec = cs.firDecimator(1, nchan=C, max_samples=n)
    r = dec._start()
    fir = cs.FirFilt(cs.firdes_kaiser(21, 0.5, 60.0), 1.0, is_complex=False, nchan=C, max_samples=n)
    for _ in range(reps + 1):
        dec._process(r, x)
        fir.process_device(d_x.data_ptr(), n, d_y.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    dec._done(r)
    fir.close()


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
            key = "k_firfilt<real>" if "k_firfilt<false>" in name else "k_firdecim" if "k_firdecim(" in name else None
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
    res = dict(tool="firfilt_time", runs=[run(C, a.n, cplx, L, a.reps) for cplx, L, C in CONFIGS])
    if a.trace:
        res["yardstick_plane"] = [64, a.n]
        res["kernel_trace_us"] = trace(a)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
