"""hipEvent time per kernel of the stereo FM decoder (csdr_fmstereo_*), one JSON line:
one stream at 192 kHz x 10 s in one call, and a 128-stream batch (128 x 192 kHz x 1 s per call), device-resident input.
Each configuration: one warm-up call, then `--reps` timed calls; the median per kernel is reported."""
import argparse
import json
import os
import sys

os.environ.setdefault("CSDR_DIAG", "1")
os.environ.setdefault("CSDR_FMS_TIME", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import composable_sdr_amd as cs  # noqa: E402
from fms_restatement import stereo_mpx  # noqa: E402

KERNELS = ["k_fms_front", "k_fms_pll", "k_fms_back", "k_fms_deemph", "k_fms_decim"]


def run(C, n, reps, q=192e3):
    X = np.stack([stereo_mpx(n, q, pilot_offset_hz=float(c % 5), seed=c) for c in range(C)])
    d_in = torch.from_numpy(X).cuda()
    d_out = torch.empty(C * 2 * (n // 4), dtype=torch.float32, device="cuda")
    dec = cs.FmStereo(q, 4, nchan=C, max_samples=n)
    times = []
    for i in range(reps + 1):
        dec.process_device(d_in.data_ptr(), n, d_out.data_ptr(), 0)
        t = dec.kernel_times()
        if i:
            times.append(t)
    dec.close()
    med = np.median(np.array(times), axis=0)
    total = float(med.sum())
    return dict(streams=C, samples_per_stream=n, us={k: round(float(v), 1) for k, v in zip(KERNELS, med)}, total_us=round(total, 1),
                pll_ns_per_sample_per_stream=round(1e3 * float(med[1]) / n, 2),
                realtime_factor=round(n / q / (total * 1e-6), 1), aggregate_msps=round(C * n / total, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    res = dict(tool="fms_time", one_stream_10s=run(1, 1920000, a.reps), batch_128x1s=run(128, 192000, a.reps))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
