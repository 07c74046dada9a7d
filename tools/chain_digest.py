#!/usr/bin/env python3
"""One SHA-256 per chain route: does a build compute the same bits as another one?

Every cell of CELLS is one chain configuration (the routes of csdr_route_table(), their tails and flags) run for two calls on the
seeded synthetic signal (tests/synth.py); the digest covers the bytes of both outputs.  Only the public Python API is used, so
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


def _cell(id, channels, frames=None, flags=0, **kw):
    kw.update(channels=channels, max_frames=256, flags=F.FLAG_TIME_KERNELS | F.FLAG_QUIET | flags)
    return id, kw, frames or (BIG if channels >= 4096 else SMALL)


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


def run_cell(kw, frames, x):
    """(path, timed kernel before the first call, [timed kernel after each call], [output of each call])"""
    M = kw["channels"]
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
