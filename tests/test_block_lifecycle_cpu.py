"""The life-cycle every block handle of include/csdr.h shares, as far as it shows without a GPU: a create validates its
arguments before it looks for a device (a bad argument is ERR_INVALID with or without a GPU; a good one is ERR_NODEV with
"no CPU fallback" when no GPU is visible, and a handle that destroys cleanly when one is), destroy takes NULL, reset does not.
One case per create entry point: eighteen blocks, firfilt, iirsos, pfbch2 and pfbsyn2 with two creates each.  The three newest
blocks spell create `open` and reset `rewind`; they are the same life-cycle steps."""
import ctypes as C

import numpy as np
import pytest

import composable_sdr_amd as cs
from composable_sdr_amd import _lib

f32 = np.float32
INF = float("inf")
TAPS = np.ones(5, f32)
SOS_B = np.array([0.2, 0.4, 0.2], f32)
SOS_A = np.array([1.0, -0.5, 0.25], f32)                      # |a2| < 1, |a1| < 1 + a2
SOS_A0 = np.array([0.0, -0.5, 0.25], f32)
PFB_TAPS = np.ones(8, f32)                                    # 2 M m taps at M = 4, m = 1


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# (create entry point, block (names its destroy), the smallest valid arguments, one invalid set): nchan = 0 where the block
# takes nchan, otherwise the first range the create checks
CREATES = [
    ("csdr_dcblock_create", "dcblock", (0.0005, 16), (1.0, 16)),
    ("csdr_nco_create", "nco", (0.1, 16), (INF, 16)),
    ("csdr_agc_create", "agc", (-10.0, 1, 16), (-10.0, 0, 16)),
    ("csdr_freqdem_create", "freqdem", (0.3, 1, 16), (0.3, 0, 16)),
    ("csdr_iirfilt_create", "iirfilt", (2, 0.1, 0.0, 10.0, 10.0, 1, 16), (2, 0.1, 0.0, 10.0, 10.0, 0, 16)),
    ("csdr_firdecim_create", "firdecim", (2, 1, 16), (2, 0, 16)),
    ("csdr_resamp_create", "resamp", (0.5, 60.0, 16), (-1.0, 60.0, 16)),
    ("csdr_ampdem_create", "ampdem", (0.8, 1, 16), (0.8, 0, 16)),
    ("csdr_fmstereo_create", "fmstereo", (200000.0, 4, 1, 16), (200000.0, 4, 0, 16)),
    ("csdr_symsync_create", "symsync", (4, 4, 0.0, 64, 0.05, 2, 1, 16), (4, 4, 0.0, 64, 0.05, 2, 0, 16)),
    ("csdr_firhilb_create", "firhilb", (5, 60.0, 16), (1, 60.0, 16)),
    ("csdr_fskdem_create", "fskdem", (1, 8, 0.25, 1, 16), (1, 8, 0.25, 0, 16)),
    ("csdr_firfilt_create_taps", "firfilt", (_p(TAPS), 5, 1.0, 0, 1, 16), (_p(TAPS), 5, 1.0, 0, 0, 16)),
    ("csdr_firfilt_create_kaiser", "firfilt", (21, 0.25, 60.0, 0.0, 0, 1, 16), (21, 0.25, 60.0, 0.0, 0, 0, 16)),
    ("csdr_gmskdem_create", "gmskdem", (4, 3, 0.3, 1, 16), (4, 3, 0.3, 0, 16)),
    ("csdr_iirsos_create_sos", "iirsos", (_p(SOS_B), _p(SOS_A), 1, 0, 1, 16), (_p(SOS_B), _p(SOS_A0), 1, 0, 1, 16)),
    ("csdr_iirsos_create_prototype", "iirsos", (3, 0.1, 0.0, 10.0, 10.0, 0, 1, 16), (3, 0.1, 0.0, 10.0, 10.0, 0, 0, 16)),
    ("csdr_pfbch2_open_taps", "pfbch2", (_p(PFB_TAPS), 4, 1, 16), (_p(PFB_TAPS), 4, 1, 0)),
    ("csdr_pfbch2_open_kaiser", "pfbch2", (4, 1, 60.0, 0.0, 16), (2, 1, 60.0, 0.0, 16)),
    ("csdr_pfbsyn2_open_taps", "pfbsyn2", (_p(PFB_TAPS), 4, 1, 16), (_p(PFB_TAPS), 4, 1, 0)),
    ("csdr_pfbsyn2_open_kaiser", "pfbsyn2", (4, 1, 60.0, 0.0, 16), (2, 1, 60.0, 0.0, 16)),
    ("csdr_rowresamp_open", "rowresamp", (0.48, 7, 60.0, 0.0, 1, 1, 16), (0.48, 7, 60.0, 0.0, 1, 0, 16)),
]
BLOCKS = sorted({block for _, block, _, _ in CREATES})
# the blocks whose C ABI has a reset, and what it is called
RESETS = {"fmstereo": "reset", "symsync": "reset", "firhilb": "reset", "firfilt": "reset", "gmskdem": "reset", "iirsos": "reset",
          "pfbch2": "rewind", "pfbsyn2": "rewind", "rowresamp": "rewind"}
IDS = [name[len("csdr_"):] for name, _, _, _ in CREATES]


def test_the_cases_cover_every_block_create_of_the_header():
    want = sorted(n for n in _lib.SIGNATURES if ("_create" in n or "_open" in n) and not n.startswith(("csdr_chain_", "csdr_comm_")))
    assert sorted(n for n, _, _, _ in CREATES) == want and len(want) == 22 and len(BLOCKS) == 18
    resets = sorted(n for n in _lib.SIGNATURES if n.endswith(("_reset", "_rewind")) and n != "csdr_chain_reset")
    assert resets == sorted(f"csdr_{b}_{step}" for b, step in RESETS.items()) and len(resets) == 9


@pytest.mark.parametrize("name,block,good,bad", CREATES, ids=IDS)
def test_valid_arguments_need_a_device_and_nothing_else(name, block, good, bad):
    h = C.c_void_p()
    rc = getattr(_lib.lib(), name)(*good, C.byref(h))
    if _lib.lib().csdr_device_count() > 0:
        _lib.check(rc)
        assert h.value
        assert getattr(_lib.lib(), f"csdr_{block}_destroy")(h) == 0
    else:
        with pytest.raises(cs.CsdrError) as e:
            _lib.check(rc)
        assert e.value.code == _lib.ERR_NODEV and "no CPU fallback" in str(e.value)
        assert not h.value


@pytest.mark.parametrize("name,block,good,bad", CREATES, ids=IDS)
def test_invalid_arguments_are_refused_before_the_device_is_looked_for(name, block, good, bad):
    h = C.c_void_p()
    with pytest.raises(cs.CsdrError) as e:
        _lib.check(getattr(_lib.lib(), name)(*bad, C.byref(h)))
    assert e.value.code == _lib.ERR_INVALID
    assert not h.value


@pytest.mark.parametrize("block", BLOCKS)
def test_destroy_takes_null(block):
    assert getattr(_lib.lib(), f"csdr_{block}_destroy")(None) == 0


@pytest.mark.parametrize("block", RESETS)
def test_reset_refuses_null(block):
    assert getattr(_lib.lib(), f"csdr_{block}_{RESETS[block]}")(None) == _lib.ERR_INVALID
