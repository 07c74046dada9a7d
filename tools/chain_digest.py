#!/usr/bin/env python3
"""One SHA-256 per chain route: does a build compute the same bits as another one?

Every cell of CELLS is one chain configuration (the routes of csdr_route_table(), their tails and flags) run for two or three calls on
the seeded synthetic signal (tests/synth.py); the digest covers the bytes of all outputs.  A cell may carry diagnostics knobs (DESIGN.md
6.1) that force a run kernel onto a small input: they are set, with CSDR_DIAG=1, around the cell's create and calls, and removed after.  Only the public Python API is used, so
the file runs unchanged against any checkout, or against another build of the library (CSDR_LIB=/path/to/libcsdr_hip.so).

    python tools/chain_digest.py                       # id, digest, path, timed kernels
    python tools/chain_digest.py --save DIR            # ... and keep the outputs (one .npy per cell)
    python tools/chain_digest.py --against DIR         # ... and, where a digest differs from DIR's, max |difference|

A route with a look-back scan may sum in a timing-dependent order: two runs of one build can then differ in the last bit.  Compare
a build with another one only against what two runs of the same build differ by.

tests/test_chain_routes_gpu.py pins the path and the timed kernels of the same cells."""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from composable_sdr_amd import Chain, _lib  # noqa: E402

F = _lib
SMALL, BIG, WB = [96, 75], [64, 43], [96, 76]       # frames of the two calls: the second one ragged (WBFM: whole decimations)


def _cell(id, channels, frames=None, flags=0, knobs=None, **kw):
    frames = frames or (BIG if channels >= 4096 else SMALL)
    kw.update(channels=channels, max_frames=max(frames), flags=F.FLAG_TIME_KERNELS | F.FLAG_QUIET | flags, knobs=knobs or {})
    return id, kw, frames


CELLS = [
    _cell("m1_deno", 1),
    _cell("m1_fm_agc", 1, demod="fm", agc=-10.0),
    _cell("m20_deno", 20),
    _cell("m20_fm", 20, demod="fm"),
    _cell("m20_fm_mix", 20, demod="fm", mix=True),
    _cell("m20_deno_mix", 20, mix=True),
    _cell("m20_deno_mix_noid", 20, mix=True, flags=F.FLAG_NO_MIX_IDENTITY),
    _cell("m32_deno", 32),
    _cell("m256_generic_fm_agc", 256, demod="fm", agc=-10.0, flags=F.FLAG_FORCE_GENERIC),
    _cell("m256_generic_deno_agc_seq", 256, agc=-10.0, flags=F.FLAG_FORCE_GENERIC | F.FLAG_AGC_SEQUENTIAL),
    _cell("m256_dc_scan", 256, dc_alpha=5e-5),
    _cell("m1024_generic_fm", 1024, demod="fm", flags=F.FLAG_FORCE_GENERIC),
    _cell("m512_g2_deno", 512, chan_stride=2),
    _cell("m4096_deno_mix", 4096, mix=True),
    _cell("m4096_g2_deno_mix", 4096, mix=True, chan_stride=2),
    _cell("m4096_shard1024_fm", 4096, demod="fm", chan_first=0, chan_count=1024),
    _cell("m20_am", 20, demod="am"),
    _cell("m20_am_mix", 20, demod="am", mix=True),
    _cell("m20_wbfm", 20, WB, demod="wbfm"),
    _cell("m20_wbfm_mix", 20, WB, demod="wbfm", mix=True),
    _cell("m20_deno_backward", 20, dft_backward=True),
]
for _m in (64, 256, 1024, 4096):
    CELLS += [_cell(f"fused{_m}_fm", _m, demod="fm"), _cell(f"fused{_m}_fm_agc", _m, demod="fm", agc=-10.0)]
CELLS.append(_cell("tail_only_fm", 8, demod="fm", agc=-10.0, tail_only=True))
# the run kernels, at the smallest shapes tests/test_chain_params_gpu.py forces them onto
R256, RUN256 = [2048, 1029], {"CSDR_RUN_MIN_TILES": "1"}
CELLS += [
    _cell("run256v2_fm", 256, R256, knobs=RUN256, demod="fm"),
    _cell("run256v2_fm_wu", 256, R256, knobs=dict(RUN256, CSDR_NOWU="0"), demod="fm"),
    _cell("run256v2_cf32_agc", 256, R256, knobs=RUN256, agc=-10.0),
    _cell("run256v2_fm_g8", 256, R256, knobs=RUN256, demod="fm", chan_stride=8, chan_first=6),      # channel 126: next to DC
    _cell("run64v2_cf32", 64, [8192, 5, 6144], knobs={"CSDR_RUN64_V2_ALL": "1"}),
    _cell("run1024v3_fm", 1024, [2048, 5, 1024], knobs={"CSDR_RUN1024_V3_RUNS": "8"}, demod="fm"),
    _cell("run1024v3_cf32_agc", 1024, [2048, 5, 1024], knobs={"CSDR_RUN1024_V3_RUNS": "8"}, agc=-10.0),
    _cell("shard1024_fm_g8", 1024, [1024, 5, 1024], knobs={"CSDR_SHARD1024_RUNS": "4"}, demod="fm", chan_stride=8),
    _cell("run1024v2_fm_g2", 1024, [1024, 5, 1024], knobs={"CSDR_RUN1024_RUNS": "4"}, demod="fm", chan_stride=2),
    _cell("fused256_fm_mix", 256, demod="fm", mix=True),
    _cell("fused1024_fm_mix", 1024, demod="fm", mix=True),
    _cell("run1024v2_fm_g4", 1024, [1024, 5, 1024], knobs={"CSDR_NO_SHARD1024": "1", "CSDR_RUN1024_RUNS": "4"}, demod="fm", chan_stride=4),
    _cell("shard1024_cf32_g8_agc", 1024, [1024, 5, 1024], knobs={"CSDR_SHARD1024_RUNS": "4"}, agc=-10.0, chan_stride=8),      # tile-major plane
    _cell("run64v2_cf32_agc", 64, [8192, 5, 6144], knobs={"CSDR_RUN64_V2_ALL": "1"}, agc=-10.0),                             # tile-major plane
]


def run_cell(kw, frames, x):
    """(path, timed kernel before the first call, [timed kernel after each call], [output of each call])"""
    kw = dict(kw)
    M, knobs = kw["channels"], dict(kw.pop("knobs", {}))
    if knobs:
        knobs["CSDR_DIAG"] = "1"
    before = {k: os.environ.get(k) for k in knobs}
    os.environ.update(knobs)
    try:
        ch = Chain(**kw)
        try:
            path, names, outs, pos = ch.path, [ch.kernel_time()[0]], [], 0
            for nf in frames:
                outs.append(ch.process(x[pos:pos + nf * M]))
                names.append(ch.kernel_time()[0])
                pos += nf * M
            ch.status()
        finally:
            ch.close()
    finally:
        for k, v in before.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    return path, names[0], names[1:], outs


def main():
    from synth import synth_cf32
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--save", metavar="DIR", help="keep every cell's outputs under DIR")
    ap.add_argument("--against", metavar="DIR", help="outputs of an earlier --save run to compare with")
    a = ap.parse_args()
    if a.save:
        os.makedirs(a.save, exist_ok=True)
    inputs = {}
    for id, kw, frames in CELLS:
        M, n = kw["channels"], kw["channels"] * sum(frames)
        if (M, n) not in inputs:
            inputs[(M, n)] = synth_cf32(n, M, seed=20261019)
        path, name0, names, outs = run_cell(kw, frames, inputs[(M, n)])
        flat = np.concatenate([o.ravel() for o in outs])
        line = f"{id:28s} {hashlib.sha256(flat.tobytes()).hexdigest()}  {path}  {name0} -> {', '.join(names)}"
        if a.against:
            ref = np.load(os.path.join(a.against, id + ".npy"))
            if ref.tobytes() != flat.tobytes():
                line += f"  DIFFERS: max |difference| = {np.max(np.abs(flat.astype(np.complex128) - ref)):.3e} (max |output| = {np.max(np.abs(ref)):.3e})"
        if a.save:
            np.save(os.path.join(a.save, id + ".npy"), flat)
        print(line, flush=True)


if __name__ == "__main__":
    main()
