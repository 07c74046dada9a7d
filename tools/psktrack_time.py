"""hipEvent time of k_psktrack (csdr_psktrack_process_device), one JSON line: BPSK, sps 2, 9 taps, constant modulus
(the symTracker setting) and QPSK, sps 1, no equaliser, on 1, 64, 256 and 1024 rows of `--n` samples each in one device-resident
call.  The same run times k_symsyncc (csdr_symsync_process_c_device: k 4, m 4, npfb 16, RRC 0.25, output rate 2) on the same rows
for scale.  One warm-up call, then `--reps` timed calls; the medians are reported."""
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


def timed(call, again, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for i in range(reps + 1):
        ev[0].record()
        call()
        ev[1].record()
        torch.cuda.synchronize()
        if i:
            times.append(ev[0].elapsed_time(ev[1]) * 1e3)
        again()
    return float(np.median(times))


def run(C, n, reps, x):
    X = np.stack([np.roll(x, 3 * c) for c in range(C)])
    stream = torch.cuda.current_stream().cuda_stream
    d_x = torch.from_numpy(X.view(np.float32).copy()).cuda()
    d_y = torch.empty(2 * C * n, dtype=torch.float32, device="cuda")
    d_ny = torch.empty(C, dtype=torch.int32, device="cuda")
    out = dict(rows=C, samples_per_row=n)
    for name, kw in (("us_bpsk_sps2_cm9", dict(bits=1, sps=2, eq_len=9, eq_mode=cs.CSDR_PSKTRACK_EQ_CM)), ("us_qpsk_sps1", dict(bits=2))):
        h = cs.PskTrack(nchan=C, max_samples=n, **kw)
        out[name] = round(timed(lambda: h.process_device(d_x.data_ptr(), n, 0, d_y.data_ptr(), 0, d_ny.data_ptr(), stream), h.restart, reps), 1)
        h.close()
    s = cs.SymSync(4, 4, 0.0, 16, nchan=C, max_samples=n, lf_bw=0.01, k_out=2)
    s.set_rnyquist(cs.CSDR_FIRFILT_RRC, 0.25)
    out["us_symsyncc"] = round(timed(lambda: s.process_c_device(d_x.data_ptr(), n, d_y.data_ptr(), d_ny.data_ptr(), stream), s.reset, reps), 1)
    s.close()
    out["msps_per_row"] = round(n / out["us_bpsk_sps2_cm9"], 2)
    out["aggregate_msps"] = round(C * n / out["us_bpsk_sps2_cm9"], 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=1 << 16)
    a = ap.parse_args()
    x, _ = psk(a.n // 4 + 64, 4, 4, 9, 0.25, 1.6, 100.0, bits_per_symbol=1, seed=3)
    x = x[:a.n]
    print(json.dumps(dict(tool="psktrack_time", device=torch.cuda.get_device_name(0), reps=a.reps,
                          runs=[run(C, a.n, a.reps, x) for C in (1, 64, 256, 1024)])))


if __name__ == "__main__":
    main()
