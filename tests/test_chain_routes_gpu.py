"""What a chain handle says about its route, and what its device entry point answers to a bad call, as literal strings.

ROUTES: for every cell of tools/chain_digest.py (the any-M route's kernels and endings, the AM / WBFM / backward tails, the four fused
sizes with and without the AGC, a tail-only handle): Chain.path, the timed kernel before the first call and after each of two calls
(the second one ragged).  ERRORS: return code, *n_out (0xdeadbeef: left as the caller had it) and the first 40 characters of
csdr_last_error for calls a WBFM, an AM and a backward handle refuse or have nothing to do for.

Both tables were recorded from the library as it stood before the any-M route became a ChainPlan (GenericPlan, plan_generic.hip), not
from the code they test: the texts are read by tools and logs, and that change was to keep every one of them.  The rows of the run-kernel
cells (run*, shard*, fused*_fm_mix: knobs force the kernels onto small calls) were recorded the same way, from the library before the
plans came to share their stream state, DC constants and cold-start setup; the last three (run1024v2_fm_g4, shard1024_cf32_g8_agc,
run64v2_cf32_agc) from the library before the plans' kernel choice moved into ChainPlan."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

cs = pytest.importorskip("composable_sdr_amd")
from composable_sdr_amd import _lib  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from chain_digest import CELLS, run_cell  # noqa: E402

# id: (path, timed kernel before the first call, timed kernel after each call)
ROUTES = {
    'm1_deno': ('generic', 'k_dc_apply', ['k_dc_apply', 'k_dc_apply']),
    'm1_fm_agc': ('generic+agc-spec', 'k_dc_apply', ['k_dc_apply', 'k_dc_apply']),
    'm20_deno': ('generic', 'k_pfb_fir', ['k_pfb_fir', 'k_pfb_fir']),
    'm20_fm': ('generic', 'k_pfb_fir', ['k_pfb_fir', 'k_pfb_fir']),
    'm20_fm_mix': ('generic', 'k_pfb_fir', ['k_pfb_fir', 'k_pfb_fir']),
    'm20_deno_mix': ('generic+mix-identity', 'k_dc_tile', ['k_dc_tile', 'k_dc_tile']),
    'm20_deno_mix_noid': ('generic', 'k_pfb_fir', ['k_pfb_fir', 'k_pfb_fir']),
    'm32_deno': ('generic', 'k_pfb_fir', ['k_pfb_fir', 'k_pfb_fir']),
    'm256_generic_fm_agc': ('generic+agc-spec', 'k_pfb_fir', ['k_pfb_fir', 'k_pfb_fir']),
    'm256_generic_deno_agc_seq': ('generic', 'k_pfb_fir', ['k_pfb_fir', 'k_pfb_fir']),
    'm256_dc_scan': ('generic+dc-scan', 'k_pfb_fir', ['k_pfb_fir', 'k_pfb_fir']),
    'm1024_generic_fm': ('generic+pfb1024', 'k_pfb1024', ['k_pfb1024', 'k_pfb1024']),
    'm512_g2_deno': ('generic+pruned-dft', 'k_pfb_fir', ['k_pfb_fir', 'k_pfb_fir']),
    'm4096_deno_mix': ('generic+mix-identity', 'k_dc_fold', ['k_dc_fold', 'k_dc_fold']),
    'm4096_g2_deno_mix': ('generic+pruned-dft+shard-mix-identity', 'k_dc_fold8', ['k_dc_fold8', 'k_dc_fold8']),
    'm4096_shard1024_fm': ('generic', 'k_pfb_fir', ['k_pfb_fir', 'k_pfb_fir']),
    'm20_am': ('generic+am', 'k_pfb_fir', ['k_pfb_fir', 'k_pfb_fir']),
    'm20_am_mix': ('generic+am', 'k_pfb_fir', ['k_pfb_fir', 'k_pfb_fir']),
    'm20_wbfm': ('generic+wbfm', 'k_pfb_fir', ['k_pfb_fir', 'k_pfb_fir']),
    'm20_wbfm_mix': ('generic+wbfm', 'k_pfb_fir', ['k_pfb_fir', 'k_pfb_fir']),
    'm20_deno_backward': ('generic+dft-backward', 'k_pfb_fir', ['k_pfb_fir', 'k_pfb_fir']),
    'fused64_fm': ('fused-k_run64<FM>', 'k_run64<FM>', ['k_run64<FM>', 'k_run64<FM>']),
    'fused64_fm_agc': ('fused-k_run64<CF32>+agc-spec', 'k_run64<CF32>', ['k_run64<CF32>', 'k_run64<CF32>']),
    'fused256_fm': ('fused-256|k_tile256<FM>', 'k_tile256<FM>', ['k_tile256<FM>', 'k_tile256<FM>']),
    'fused256_fm_agc': ('fused-256|k_tile256<CF32>+agc-spec', 'k_tile256<CF32>', ['k_tile256<CF32>', 'k_tile256<CF32>']),
    'fused1024_fm': ('fused-k_run1024v3<FM>', 'k_run1024v3<FM>', ['k_run1024v3<FM>', 'k_run1024<FM>']),
    'fused1024_fm_agc': ('fused-k_run1024v3<CF32>+agc-spec', 'k_run1024v3<CF32>', ['k_run1024v3<CF32>', 'k_run1024<CF32>']),
    'fused4096_fm': ('fused-4096|k_front4096+k_back4096<FM>', 'k_front4096+k_back4096<FM>', ['k_front4096+k_back4096<FM>', 'k_front4096+k_back4096<FM>']),
    'fused4096_fm_agc': ('fused-4096|k_front4096+k_back4096<CF32>+agc-spec', 'k_front4096+k_back4096<CF32>', ['k_front4096+k_back4096<CF32>', 'k_front4096+k_back4096<CF32>']),
    'tail_only_fm': ('tail-only+agc-spec', 'k_agc_spec', ['k_agc_spec', 'k_agc_spec']),
    'run256v2_fm': ('fused-256|k_tile256<FM>', 'k_tile256<FM>', ['k_run256v2<FM>', 'k_run256v2<FM>']),
    'run256v2_fm_wu': ('fused-256|k_tile256<FM>', 'k_tile256<FM>', ['k_run256v2<FM>', 'k_run256v2<FM>']),
    'run256v2_cf32_agc': ('fused-256|k_tile256<CF32>+agc-spec', 'k_tile256<CF32>', ['k_run256v2<CF32>', 'k_run256v2<CF32>']),
    'run256v2_fm_g8': ('fused-256|k_tile256<FM>+interleaved-shard', 'k_tile256<FM>', ['k_run256v2<FM>/G8', 'k_run256v2<FM>/G8']),
    'run64v2_cf32': ('fused-k_run64<CF32>', 'k_run64<CF32>', ['k_run64v2', 'k_run64<CF32>', 'k_run64v2']),
    'run1024v3_fm': ('fused-k_run1024v3<FM>', 'k_run1024v3<FM>', ['k_run1024v3<FM>', 'k_run1024<FM>', 'k_run1024v3<FM>']),
    'run1024v3_cf32_agc': ('fused-k_run1024v3<CF32>+agc-spec', 'k_run1024v3<CF32>', ['k_run1024v3<CF32>', 'k_run1024<CF32>', 'k_run1024v3<CF32>']),
    'shard1024_fm_g8': ('fused-k_shard1024<FM>/G8+interleaved-shard', 'k_shard1024<FM>/G8', ['k_shard1024<FM>/G8', 'k_run1024<FM>', 'k_shard1024<FM>/G8']),
    'run1024v2_fm_g2': ('fused-k_run1024v2<FM>/G2+interleaved-shard', 'k_run1024v2<FM>/G2', ['k_run1024v2<FM>/G2', 'k_run1024<FM>', 'k_run1024v2<FM>/G2']),
    'fused256_fm_mix': ('fused-256|k_tile256<FM>', 'k_tile256<FM>', ['k_tile256<FM>', 'k_tile256<FM>']),
    'fused1024_fm_mix': ('fused-k_run1024v3<FM>', 'k_run1024v3<FM>', ['k_run1024v3<FM>', 'k_run1024<FM>']),
    'run1024v2_fm_g4': ('fused-k_run1024v2<FM>/G4+interleaved-shard', 'k_run1024v2<FM>/G4', ['k_run1024v2<FM>/G4', 'k_run1024<FM>', 'k_run1024v2<FM>/G4']),
    'shard1024_cf32_g8_agc': ('fused-k_shard1024<CF32>/G8+interleaved-shard+agc-spec', 'k_shard1024<CF32>/G8', ['k_shard1024<CF32>/G8', 'k_run1024<CF32>', 'k_shard1024<CF32>/G8']),
    'run64v2_cf32_agc': ('fused-k_run64<CF32>+agc-spec', 'k_run64<CF32>', ['k_run64v2', 'k_run64<CF32>', 'k_run64v2']),
}
UNTOUCHED = 0xdeadbeef
# handle: [(call, return code, *n_out, csdr_last_error()[:40] of a refused call)]
ERRORS = {
    'wbfm': [
        ('n_in = 0', 0, 0, ''),
        ('null d_out', -1, 0, 'chain: null buffer'),
        ('n_in % M', -4, 0, 'chain: n_in=163 is not a multiple of cha'),
        ('n_in > max', -4, 0, 'chain: n_in=5200 exceeds max_frames*chan'),
        ('frames % decim', -4, 0, 'chain: 6 frames per call are not a multi'),
    ],
    'am': [
        ('n_in = 0', 0, 0, ''),
        ('null d_out', -1, 0, 'chain: null buffer'),
        ('n_in % M', -4, 0, 'chain: n_in=163 is not a multiple of cha'),
        ('n_in > max', -4, 0, 'chain: n_in=5200 exceeds max_frames*chan'),
    ],
    'backward': [
        ('n_in = 0', 0, 0, ''),
        ('null d_out', -1, 0, 'chain: null buffer'),
        ('n_in % M', -4, UNTOUCHED, 'chain: n_in=163 is not a multiple of cha'),
        ('n_in > max', -4, UNTOUCHED, 'chain: n_in=5200 exceeds max_frames*chan'),
    ],
}
M, MAX_NF = 20, 256
HANDLES = {"wbfm": dict(demod="wbfm"), "am": dict(demod="am"), "backward": dict(dft_backward=True)}
CALLS = [  # (call, n_in, null d_out, handles)
    ("n_in = 0", 0, False, HANDLES),
    ("null d_out", M * 8, True, HANDLES),
    ("n_in % M", M * 8 + 3, False, HANDLES),
    ("n_in > max", M * (MAX_NF + 4), False, HANDLES),
    ("frames % decim", M * 6, False, ("wbfm",)),
]


def observe_route(id):
    _, kw, frames = next(c for c in CELLS if c[0] == id)
    x = np.random.default_rng(7).standard_normal((kw["channels"] * sum(frames), 2), dtype=np.float32).view(np.complex64).ravel()
    path, name0, names, outs = run_cell(kw, frames, x)
    assert all(np.isfinite(o.view(np.float32)).all() for o in outs)
    return path, name0, names


def observe_errors(handle):
    import torch
    d_in = torch.zeros(M * (MAX_NF + 4), dtype=torch.complex64, device="cuda")
    d_out = torch.zeros(M * (MAX_NF + 4), dtype=torch.complex64, device="cuda")
    ch = cs.Chain(channels=M, max_frames=MAX_NF, flags=_lib.FLAG_TIME_KERNELS | _lib.FLAG_QUIET, **HANDLES[handle])
    rows = []
    try:
        for call, n_in, null_out, handles in CALLS:
            if handle not in handles:
                continue
            n_out = C.c_uint32(UNTOUCHED)
            rc = cs.lib().csdr_chain_process_device(ch.h, C.c_void_p(d_in.data_ptr()), n_in, None if null_out else C.c_void_p(d_out.data_ptr()),
                                                    C.byref(n_out), None)
            rows.append((call, rc, n_out.value, cs.lib().csdr_last_error().decode()[:40] if rc else ""))
        torch.cuda.synchronize()
    finally:
        ch.close()
    return rows


def test_tables_cover_the_cells():
    assert list(ROUTES) == [c[0] for c in CELLS]
    assert list(ERRORS) == list(HANDLES)


@pytest.mark.parametrize("id", [c[0] for c in CELLS])
def test_route_strings(id):
    got = observe_route(id)
    print(id, got)
    assert got == ROUTES[id]


@pytest.mark.parametrize("handle", list(HANDLES))
def test_error_table(handle):
    got = observe_errors(handle)
    print(handle, got)
    assert got == ERRORS[handle]
