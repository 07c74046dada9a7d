"""hipEvent time of k_gmskdem (csdr_gmskdem_*), one JSON line: gmskdem (4, 3, 0.3) on 1, 64 and 1024 GMSK rows of
`--n` samples each in one device-resident call.  One warm-up call, then `--reps` timed calls; the median is reported with the
achieved GB/s on 8 B read per sample + 8 B written per symbol (bits and soft values) and its share of 8 TB/s.

The same result from the blocks that were there before is fmDemodulator then firFilterR(taps, 1.0) on the same plane, every
sample filtered (20 B per sample).  fmDemodulator has a host entry only, so event times would count its copies: with
`--trace DIR` the work runs once more in a child process under `rocprofv3 --kernel-trace`, and the kernels' own times
(k_gmskdem against k_fm + k_firfilt, medians per row count) are reported from the trace."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

K, M, BT = 4, 3, 0.3
ROWS = (1, 64, 1024)
FM_CALLS = 2


def plane(C, n):
    import numpy as np
    from gmsk_restatement import gmskmod
    rng = np.random.default_rng(11)
    x = gmskmod(rng.integers(0, 2, n // K + 64), K, M, BT, offset=0.01, snr_db=20.0, rng=rng)
    return np.stack([x[(7 * c) % 256:][:n] for c in range(C)])


def run(C, n, reps, composition):
    import numpy as np
    import torch
    import composable_sdr_amd as cs
    X = plane(C, n)
    d_x = torch.from_numpy(X.view(np.float32).copy()).cuda()
    d_sym = torch.empty(C * (n // K), dtype=torch.int32, device="cuda")
    d_soft = torch.empty(C * (n // K), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(call):
        times = []
        for i in range(reps + 1):
            ev[0].record()
            call()
            ev[1].record()
            torch.cuda.synchronize()
            if i:
                times.append(ev[0].elapsed_time(ev[1]) * 1e3)
        return float(np.median(times))

    h = cs.GmskDem(K, M, BT, nchan=C, max_samples=n)
    us = timed(lambda: h.process_device(d_x.data_ptr(), n, d_sym.data_ptr(), d_soft.data_ptr(), stream))
    h.close()
    nbytes = 8 * C * n + 8 * C * (n // K)
    res = dict(rows=C, samples_per_row=n, us=round(us, 1), gbps=round(nbytes / us * 1e-3, 1), share_of_8tbps=round(nbytes / us * 1e-6 / 8.0, 3))
    if composition:
        fm = cs.fmDemodulator(1.0 / (2.0 * np.pi), nchan=C, max_samples=n)
        r = fm._start()
        for _ in range(FM_CALLS):
            phi = fm._process(r, X)
        fm._done(r)
        d_phi = torch.from_numpy(phi).cuda()
        d_y = torch.empty(C * n, dtype=torch.float32, device="cuda")
        f = cs.FirFilt(cs.firdes_gmskrx(K, M, BT), 1.0, False, nchan=C, max_samples=n)
        res["firfilt_us"] = round(timed(lambda: f.process_device(d_phi.data_ptr(), n, d_y.data_ptr(), stream)), 1)
        f.close()
    return res


def trace(a):
    os.makedirs(a.trace, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "-f", "csv", "-d", a.trace, "-o", "t", "--", sys.executable, os.path.abspath(__file__),
           "--reps", str(a.reps), "--n", str(a.n), "--composition"]
    log = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
    if log.returncode != 0:
        raise SystemExit(f"traced run failed ({log.returncode}): {log.stderr[-2000:]}")
    disp = {"k_gmskdem": [], "k_fm": [], "k_firfilt": []}
    for f in glob.glob(os.path.join(a.trace, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            for name in disp:
                if name + "(" in row["Kernel_Name"] or name + "<" in row["Kernel_Name"]:
                    disp[name].append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    per = {"k_gmskdem": a.reps + 1, "k_fm": FM_CALLS, "k_firfilt": a.reps + 1}
    out = []
    for i, C in enumerate(ROWS):
        e = dict(rows=C)
        for name, d in disp.items():
            d = sorted(d)[i * per[name]:(i + 1) * per[name]][1:]            # in launch order; the first call of a shape warms up
            if len(d) != per[name] - 1:
                raise SystemExit(f"{name}: {len(disp[name])} dispatches in the trace, {per[name] * len(ROWS)} expected")
            d = sorted(t1 - t0 for t0, t1 in d)
            e[name + "_us"] = round(d[len(d) // 2] * 1e-3, 1)
        e["composition_us"] = round(e["k_fm_us"] + e["k_firfilt_us"], 1)
        out.append(e)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=1 << 16)
    ap.add_argument("--composition", action="store_true", help="also run fmDemodulator and firFilterR on the plane (for a trace)")
    ap.add_argument("--trace", default="", help="directory for a rocprofv3 kernel trace of a child run")
    ap.add_argument("--timeout", type=int, default=500)
    a = ap.parse_args()
    res = dict(tool="gmskdem_time", kmb=[K, M, BT], runs=[run(C, a.n, a.reps, a.composition) for C in ROWS])
    if a.trace:
        res["kernel_trace"] = trace(a)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
