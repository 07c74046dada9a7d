"""The life-cycle of the chain handle as far as it shows without a GPU (the block handles: test_block_lifecycle_cpu.py):
csdr_chain_create refuses a bad configuration before it looks for a device, with the code and the text the C ABI promises; a
good one is ERR_NODEV with "no CPU fallback" when no GPU is visible and a handle that destroys cleanly when one is; destroy takes
NULL, every other entry point refuses it.  VALID and cfg_of() also serve test_chain_lifecycle_gpu.py."""
import ctypes as C

import pytest

from composable_sdr_amd import _lib

F = _lib
TAIL_ONLY_TEXT = ("chain: CSDR_FLAG_TAIL_ONLY needs the AGC on (-a != 0) and demod none / FM "
                  "(without the AGC a time stripe needs no tail shard)")
SHARD_TEXT = "chain: interleaved shard %u of %u needs chan_stride | channels (8), chan_first < chan_stride, chan_count 0 or channels/chan_stride"


def cfg_of(channels=8, max_frames=16, flags=0, **fields):
    """csdr_chain_cfg_default's configuration with `fields` on top; quiet"""
    c = _lib.ChainCfg()
    _lib.lib().csdr_chain_cfg_default(C.byref(c), channels)
    c.channels, c.max_frames, c.flags = channels, max_frames, flags | F.FLAG_QUIET
    for k, v in fields.items():
        setattr(c, k, v)
    return c


def create(c):
    """(return code, csdr_last_error, handle) of csdr_chain_create"""
    h = C.c_void_p()
    rc = _lib.lib().csdr_chain_create(C.byref(c) if c is not None else None, C.byref(h))
    return rc, _lib.lib().csdr_last_error().decode(), h


# refused before the device is looked for: (id, configuration or None, csdr_last_error)
REFUSED = [
    ("null_cfg", lambda: None, "chain: null argument"),
    ("struct_size", lambda: cfg_of(struct_size=7), f"chain: cfg.struct_size 7 != {C.sizeof(_lib.ChainCfg)}"),
    ("demod_4", lambda: cfg_of(demod=4), "chain: unknown demod 4"),
    ("channels_0", lambda: cfg_of(channels=0), "chain: channels 0 out of range"),
    ("channels_65537", lambda: cfg_of(channels=65537), "chain: channels 65537 out of range"),
    ("tail_only_agc_off", lambda: cfg_of(flags=F.FLAG_TAIL_ONLY), TAIL_ONLY_TEXT),
    ("tail_only_am", lambda: cfg_of(flags=F.FLAG_TAIL_ONLY, agc_threshold_db=-10.0, demod=F.DEMOD_AM), TAIL_ONLY_TEXT),
    ("tail_only_wbfm", lambda: cfg_of(flags=F.FLAG_TAIL_ONLY, agc_threshold_db=-10.0, demod=F.DEMOD_WBFM), TAIL_ONLY_TEXT),
    ("tail_only_fm_kf_0", lambda: cfg_of(flags=F.FLAG_TAIL_ONLY, agc_threshold_db=-10.0, demod=F.DEMOD_FM, kf=0.0), "chain: FM needs kf > 0"),
    ("fm_kf_0", lambda: cfg_of(demod=F.DEMOD_FM, kf=0.0), "chain: FM needs kf > 0"),
    ("dc_alpha_0", lambda: cfg_of(dc_block=1, dc_alpha=0.0), "chain: dc_alpha out of (0,1)"),
    ("dc_alpha_1", lambda: cfg_of(dc_block=1, dc_alpha=1.0), "chain: dc_alpha out of (0,1)"),
    ("pfb_m_33", lambda: cfg_of(pfb_m=33), "chain: pfb_m 33 out of 1..32 (0 = 7)"),
    ("chan_stride_3", lambda: cfg_of(chan_stride=3), SHARD_TEXT % (0, 3)),
    ("chan_first_ge_stride", lambda: cfg_of(chan_stride=2, chan_first=2), SHARD_TEXT % (2, 2)),
    ("chan_count_ne_share", lambda: cfg_of(chan_stride=2, chan_count=3), SHARD_TEXT % (0, 2)),
    ("contiguous_6_4", lambda: cfg_of(chan_first=6, chan_count=4), "chain: channel shard [6,+4) outside 0..8"),
]

# valid at channels = 8, max_frames = 16: (id, cfg_of's arguments)
VALID = [(f"{name}{'_agc' if agc else ''}", dict(demod=demod, agc_threshold_db=agc))
         for name, demod in (("deno", F.DEMOD_NONE), ("fm", F.DEMOD_FM), ("am", F.DEMOD_AM), ("wbfm", F.DEMOD_WBFM)) for agc in (0.0, -10.0)]
VALID += [
    ("fm_agc_mix", dict(demod=F.DEMOD_FM, agc_threshold_db=-10.0, mix=1)),
    ("fm_agc_sequential", dict(demod=F.DEMOD_FM, agc_threshold_db=-10.0, flags=F.FLAG_AGC_SEQUENTIAL)),
    ("deno_backward", dict(flags=F.FLAG_DFT_BACKWARD)),
    ("tail_only_fm_agc", dict(demod=F.DEMOD_FM, agc_threshold_db=-10.0, flags=F.FLAG_TAIL_ONLY)),
]


@pytest.mark.parametrize("id,make,text", REFUSED, ids=[r[0] for r in REFUSED])
def test_a_bad_configuration_is_refused_before_the_device_is_looked_for(id, make, text):
    rc, err, h = create(make())
    assert (rc, err) == (F.ERR_INVALID, text)
    assert not h.value


@pytest.mark.parametrize("id,kw", VALID, ids=[v[0] for v in VALID])
def test_a_valid_configuration_needs_a_device_and_nothing_else(id, kw):
    rc, err, h = create(cfg_of(**kw))
    if _lib.lib().csdr_device_count() > 0:
        assert rc == 0, err
        assert h.value
        assert _lib.lib().csdr_chain_destroy(h) == 0
    else:
        assert rc == F.ERR_NODEV and "no CPU fallback" in err
        assert not h.value


def test_destroy_takes_null_and_reset_does_not():
    assert _lib.lib().csdr_chain_destroy(None) == 0
    assert _lib.lib().csdr_chain_reset(None) == F.ERR_INVALID


NULL_HANDLE = [
    ("csdr_chain_process_device", (None, 0, None, None, None)),
    ("csdr_chain_submit_device", (None, 0, None, None, None)),
    ("csdr_chain_submit", (None, 0, None)),
    ("csdr_chain_collect", (None,)),
    ("csdr_chain_process", (None, 0, None, None)),
    ("csdr_chain_wait_device", (None,)),
    ("csdr_chain_status", ()),
]


@pytest.mark.parametrize("name,args", NULL_HANDLE, ids=[n[0] for n in NULL_HANDLE])
def test_an_entry_point_refuses_a_null_handle(name, args):
    _lib.lib().csdr_chain_create(None, None)        # (another text in csdr_last_error first)
    assert getattr(_lib.lib(), name)(None, *args) == F.ERR_INVALID
    assert _lib.lib().csdr_last_error().decode() == "chain: null handle"
