"""Time of k_fskdem (csdr_fskdem_*) on a device-resident [256][262144] CF32 plane, one JSON line: for
(m, k) = (1, 8), (2, 16), (4, 64) at bw 0.25 the median hipEvent time of `--reps` calls after one warm-up call, and the achieved
GB/s on 8 B read per sample + 4 B written per symbol.

With `--trace DIR` the same work runs once more in a child process under `rocprofv3 --kernel-trace --stats`, followed by
amDemodulator on the same plane (k_am: 16 B read + 4 B written per sample, through the host path), and the kernels' own times
from the trace are reported next to the event times: k_fskdem at (1, 8) is meant to take no longer than k_am."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = [(1, 8), (2, 16), (4, 64)]
BW = 0.25


def plane(C, n):
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    return torch.randn((C, n, 2), generator=g, device="cuda", dtype=torch.float32) * 0.7071


def run(d_x, C, n, m, k, reps):
    import numpy as np
    import torch
    import composable_sdr_amd as cs
    d_sym = torch.empty(C * (n // k), dtype=torch.int32, device="cuda")
    h = cs.FskDem(m, k, BW, nchan=C, max_samples=n)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for i in range(reps + 1):
        ev[0].record()
        h.process_device(d_x.data_ptr(), n, d_sym.data_ptr(), 0, torch.cuda.current_stream().cuda_stream)
        ev[1].record()
        torch.cuda.synchronize()
        if i:
            times.append(ev[0].elapsed_time(ev[1]) * 1e3)
    K, _ = h.design()
    h.close()
    us = float(np.median(times))
    nbytes = 8 * C * n + 4 * C * (n // k)
    return dict(m=m, k=k, K=K, us=round(us, 1), gbps=round(nbytes / us * 1e-3, 1), symbols=C * (n // k))


def run_am(d_x, C, n, calls):
    import numpy as np
    import composable_sdr_amd as cs
    x = d_x.cpu().numpy().view(np.complex64).reshape(C, n)
    p = cs.amDemodulator(nchan=C, max_samples=n)
    r = p._start()
    for _ in range(calls):
        p._process(r, x)
    p._done(r)


def trace(a):
    os.makedirs(a.trace, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", a.trace, "-o", "t", "--", sys.executable, os.path.abspath(__file__),
           "--reps", str(a.reps), "--channels", str(a.channels), "--n", str(a.n), "--am-calls", "3"]
    log = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
    if log.returncode != 0:
        raise SystemExit(f"traced run failed ({log.returncode}): {log.stderr[-2000:]}")
    out = {}
    for f in glob.glob(os.path.join(a.trace, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            name = row["Name"]
            if "k_fskdem<" in name:
                tg = int(name.split("k_fskdem<")[1].split(",")[0])
                out[f"k_fskdem<{tg}>"] = dict(calls=int(row["Calls"]), avg_us=round(float(row["AverageNs"]) * 1e-3, 1),
                                              min_us=round(float(row["MinNs"]) * 1e-3, 1))
            elif "k_am(" in name:
                out["k_am"] = dict(calls=int(row["Calls"]), avg_us=round(float(row["AverageNs"]) * 1e-3, 1),
                                   min_us=round(float(row["MinNs"]) * 1e-3, 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--am-calls", type=int, default=0, help="also run amDemodulator on the plane this many times (for a trace)")
    ap.add_argument("--trace", default="", help="directory for a rocprofv3 kernel trace of a child run")
    ap.add_argument("--timeout", type=int, default=400)
    a = ap.parse_args()
    d_x = plane(a.channels, a.n)
    res = dict(tool="fskdem_time", plane=[a.channels, a.n], bw=BW,
               runs=[run(d_x, a.channels, a.n, m, k, a.reps) for m, k in CONFIGS])
    if a.am_calls:
        run_am(d_x, a.channels, a.n, a.am_calls)
    del d_x
    if a.trace:
        res["kernel_trace_us"] = trace(a)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
