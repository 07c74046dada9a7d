"""The life-cycle of the chain handle on a device (what shows without one: test_chain_lifecycle_cpu.py): the refusals of
csdr_chain_create that come behind the device, each followed by a handle of the same kind that works; create / close cycles of
every kind of handle without a call; one handle through all three families of entry points, reset, and a fresh handle's bits.
Every handle has 8 channels and max_frames = 16 unless a case says otherwise."""
import ctypes as C

import numpy as np
import pytest

from composable_sdr_amd import Chain, _lib
from composable_sdr_amd.pipes import host_array
from synth import synth_cf32
from test_chain_lifecycle_cpu import VALID, cfg_of, create

pytestmark = pytest.mark.gpu
F = _lib
M, NF = 8, 16
TOO_BIG = "chain: max_frames*channels exceeds 2^32-1 samples"
AGC = dict(agc_threshold_db=-10.0)

# (id, the refused configuration, csdr_last_error, a valid configuration of the same kind)
REFUSED = [
    ("too_big", dict(channels=65536, max_frames=65536), TOO_BIG, dict()),                         # before any plane is allocated
    ("too_big_tail_only", dict(channels=65536, max_frames=65536, flags=F.FLAG_TAIL_ONLY, **AGC), TOO_BIG, dict(flags=F.FLAG_TAIL_ONLY, **AGC)),
    ("backward_shard", dict(flags=F.FLAG_DFT_BACKWARD, chan_count=4, **AGC),                        # behind the plan and the AGC buffers
     "chain: CSDR_FLAG_DFT_BACKWARD is built for whole-band handles (no channel shard)", dict(flags=F.FLAG_DFT_BACKWARD, **AGC)),
    ("wbfm_deemph_fc", dict(demod=F.DEMOD_WBFM, deemph_fc=0.5), "chain: deemph_fc 0.5 out of (0, 0.5)", dict(demod=F.DEMOD_WBFM)),   # behind the plan
]


def _one_call(h, c):
    """one call of NF frames through csdr_chain_process: the number of elements the handle says it wrote, and the output"""
    x = synth_cf32(M * NF, M, seed=20261020)
    out = np.full(M * NF, np.nan, np.complex64 if _lib.lib().csdr_chain_out_elem_size(h) == 8 else np.float32)
    n = C.c_uint32()
    _lib.check(_lib.lib().csdr_chain_process(h, x.ctypes.data_as(C.c_void_p), x.size, out.ctypes.data_as(C.c_void_p), C.byref(n)))
    return n.value, out


@pytest.mark.parametrize("id,bad,text,good", REFUSED, ids=[r[0] for r in REFUSED])
def test_a_refusal_behind_the_device_leaves_nothing_in_the_way(id, bad, text, good):
    rc, err, h = create(cfg_of(**bad))
    assert (rc, err) == (F.ERR_INVALID, text)
    assert not h.value
    c = cfg_of(**good)
    rc, err, h = create(c)
    assert rc == 0 and h.value, err
    try:
        n, out = _one_call(h, c)
        assert n == M * NF // (4 if c.demod == F.DEMOD_WBFM else 1)
        assert np.isfinite(out[:n]).all()
    finally:
        assert _lib.lib().csdr_chain_destroy(h) == 0


@pytest.mark.parametrize("id,kw", VALID, ids=[v[0] for v in VALID])
def test_five_create_close_cycles_without_a_call(id, kw):
    for _ in range(5):
        rc, err, h = create(cfg_of(**kw))
        assert rc == 0 and h.value, err
        assert _lib.lib().csdr_chain_destroy(h) == 0


def _stream(ch, x, calls):
    return [ch.process(x[i * M * NF:(i + 1) * M * NF]) for i in range(calls)]


def test_every_family_of_entry_points_then_reset_is_a_fresh_handle():
    import torch
    x = synth_cf32(4 * M * NF, M, seed=20261020)
    chunk = [x[i * M * NF:(i + 1) * M * NF] for i in range(4)]
    kw = dict(channels=M, max_frames=NF, demod="fm", agc=-10.0)
    fresh = Chain(**kw)
    try:
        want = _stream(fresh, x, 4)
    finally:
        fresh.close()
    ch = Chain(**kw)
    try:
        got = [ch.process(chunk[0])]                                                      # pageable buffers
        pin, pout = host_array((M * NF,), np.complex64), host_array((M, NF), np.float32)
        pin.a[:] = chunk[1]; pout.a[:] = np.nan
        n = C.c_uint32()
        _lib.check(_lib.lib().csdr_chain_process(ch.h, pin.a.ctypes.data_as(C.c_void_p), M * NF, pout.a.ctypes.data_as(C.c_void_p), C.byref(n)))
        assert n.value == M * NF
        got.append(pout.a.copy())                                                         # page-locked buffers
        ch.submit(chunk[2])
        got.append(ch.collect().copy())
        xd = torch.from_numpy(chunk[3].view(np.float32).copy()).cuda()
        yd = torch.full((M, NF), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        assert ch.submit_device(xd.data_ptr(), M * NF, yd.data_ptr()) == M * NF
        ch.wait_device()
        got.append(yd.cpu().numpy())
        ch.status()
        for i, (g, w) in enumerate(zip(got, want)):
            assert np.isfinite(g).all() and g.tobytes() == w.tobytes(), f"call {i}: the four entry points continue one stream"
        ch.reset()
        again = _stream(ch, x, 4)
        for i, (g, w) in enumerate(zip(again, want)):
            assert g.tobytes() == w.tobytes(), f"call {i} after reset()"
    finally:
        ch.close()
