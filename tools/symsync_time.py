"""hipEvent time of k_symsync (csdr_symsync_*), one JSON line: symSyncR 4 4 0 64 on 1, 64, 256 and 1024
FM-demodulated FSK streams of `--n` samples each in one device-resident call.  One warm-up call, then `--reps` timed calls;
the median is reported, with the per-stream and aggregate input rates."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import composable_sdr_amd as cs  # noqa: E402
from symsync_restatement import freqdem, nrz_fsk_iq  # noqa: E402


def run(C, n, reps):
    x, _ = nrz_fsk_iq(n // 4 + 8, k=4, offset=0.37, ppm=200.0, seed=5)
    m = freqdem(x, np.float32(0.08))[:n]
    X = np.stack([np.roll(m, 3 * c) for c in range(C)])
    d_x = torch.from_numpy(X).cuda()
    d_y = torch.empty(C * n, dtype=torch.float32, device="cuda")
    d_ny = torch.empty(C, dtype=torch.int32, device="cuda")
    h = cs.SymSync(4, 4, 0.0, 64, nchan=C, max_samples=n)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for i in range(reps + 1):
        ev[0].record()
        h.process_device(d_x.data_ptr(), n, d_y.data_ptr(), d_ny.data_ptr(), torch.cuda.current_stream().cuda_stream)
        ev[1].record()
        torch.cuda.synchronize()
        if i:
            times.append(ev[0].elapsed_time(ev[1]) * 1e3)
        h.reset()
    ny = d_ny.cpu().numpy()
    h.close()
    us = float(np.median(times))
    return dict(streams=C, samples_per_stream=n, us=round(us, 1), outputs_per_stream=int(np.median(ny)),
                msps_per_stream=round(n / us, 2), aggregate_msps=round(C * n / us, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=1 << 16)
    a = ap.parse_args()
    res = dict(tool="symsync_time", runs=[run(C, a.n, a.reps) for C in (1, 64, 256, 1024)])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
