"""hipEvent time of k_symsyncc (csdr_symsync_process_c_device), one JSON line: symSyncC 3 2 (k 2, m 3, npfb 32)
and (k 4, m 4, npfb 64), both with lf_bw 0.01 and output rate 1, on 1, 64, 256 and 1024 QPSK streams of `--n` samples each in one
device-resident call.  The same run times k_symsync (csdr_symsync_process_device) on the real parts of the same rows with the
same banks and parameters.  One warm-up call, then `--reps` timed calls; the medians are reported."""
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
from symsyncc_restatement import psk  # noqa: E402


def timed(h, call, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for i in range(reps + 1):
        ev[0].record()
        call()
        ev[1].record()
        torch.cuda.synchronize()
        if i:
            times.append(ev[0].elapsed_time(ev[1]) * 1e3)
        h.reset()
    return float(np.median(times))


def run(k, m, npfb, C, n, reps, x):
    X = np.stack([np.roll(x, 3 * c) for c in range(C)])
    stream = torch.cuda.current_stream().cuda_stream
    d_ny = torch.empty(C, dtype=torch.int32, device="cuda")
    h = cs.SymSync(k, m, 0.0, npfb, nchan=C, max_samples=n, lf_bw=0.01, k_out=1)
    h.set_rnyquist(cs.CSDR_FIRFILT_ARKAISER, 0.5)
    d_x = torch.from_numpy(X.view(np.float32).copy()).cuda()
    d_y = torch.empty(2 * C * n, dtype=torch.float32, device="cuda")
    us_c = timed(h, lambda: h.process_c_device(d_x.data_ptr(), n, d_y.data_ptr(), d_ny.data_ptr(), stream), reps)
    ny_c = int(np.median(d_ny.cpu().numpy()))
    d_r = torch.from_numpy(np.ascontiguousarray(X.real)).cuda()
    us_r = timed(h, lambda: h.process_device(d_r.data_ptr(), n, d_y.data_ptr(), d_ny.data_ptr(), stream), reps)
    ny_r = int(np.median(d_ny.cpu().numpy()))
    h.close()
    return dict(k=k, m=m, npfb=npfb, streams=C, samples_per_stream=n, us_complex=round(us_c, 1), us_real=round(us_r, 1),
                ratio=round(us_c / us_r, 2), outputs_complex=ny_c, outputs_real=ny_r, msps_per_stream=round(n / us_c, 2),
                aggregate_msps=round(C * n / us_c, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=1 << 16)
    a = ap.parse_args()
    runs = []
    for k, m, npfb in ((2, 3, 32), (4, 4, 64)):
        x = psk(a.n // k + 2 * m + 8, k, m, offset=0.37, ppm=200.0, seed=5)[0][:a.n]
        assert x.size == a.n
        runs += [run(k, m, npfb, C, a.n, a.reps, x) for C in (1, 64, 256, 1024)]
    print(json.dumps(dict(tool="symsyncc_time", runs=runs)))


if __name__ == "__main__":
    main()
