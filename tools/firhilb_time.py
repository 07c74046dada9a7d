"""hipEvent time of k_firhilb_decim (csdr_firhilb_decim_device), one JSON line: realToComplex (m = 5, 60 dB) on
n = 2^24 complex samples out (the streaming case: 8 B read and 8 B written per sample, so the bound is HBM) and on the
reference's n = 512 (one source chunk of 1024 floats: a launch, not a bandwidth, measurement).  One warm-up call, then
`--reps` timed calls; the median is reported with the traffic rate it amounts to."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import composable_sdr_amd as cs  # noqa: E402


def run(n, reps):
    x = np.random.default_rng(5).standard_normal(2 * n).astype(np.float32)
    d_x = torch.from_numpy(x).cuda()
    d_y = torch.empty(2 * n, dtype=torch.float32, device="cuda")
    h = cs.FirHilb(max_samples=n)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    stream = torch.cuda.current_stream().cuda_stream
    times = []
    for i in range(reps + 1):
        ev[0].record()
        h.decim_device(d_x.data_ptr(), n, d_y.data_ptr(), stream)
        ev[1].record()
        torch.cuda.synchronize()
        if i:
            times.append(ev[0].elapsed_time(ev[1]) * 1e3)
    h.close()
    us = float(np.median(times))
    return dict(samples=n, us=round(us, 2), us_min=round(float(np.min(times)), 2), msps=round(n / us, 1),
                gbytes_per_s=round(16.0 * n / us / 1e3, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    print(json.dumps(dict(tool="firhilb_time", runs=[run(n, a.reps) for n in (1 << 24, 512)])))


if __name__ == "__main__":
    main()
