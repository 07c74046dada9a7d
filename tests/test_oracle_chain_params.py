"""The oracle's chain with non-default DC blocker and prototype settings (csdr_chain_cfg::dc_alpha, pfb_m, pfb_as):
the extended constructors are the same composition as the default ones, with the settings passed through.
The GPU side of these settings is pinned in test_chain_params_gpu.py."""
import numpy as np
import pytest

import oracle_lib as O
from synth import synth_cf32


@pytest.mark.parametrize("M", [1, 20, 64])
@pytest.mark.parametrize("alpha", [5e-5, 2e-4, 5e-3, 0.3])
def test_chain_dc_alpha_is_dcblock_then_chain_without_dc(M, alpha):
    x = synth_cf32(M * 96, max(M, 4), seed=7, dc=0.3 + 0.2j)
    got = O.Chain(M, demod="fm", kf=0.3, dc_alpha=alpha).process(x)
    want = O.Chain(M, demod="fm", kf=0.3, dc_block=False).process(O.DcBlock(alpha).execute(x))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_chain_default_keywords_are_the_default_chain():
    M = 64
    x = synth_cf32(M * 64, M, seed=3)
    a = O.Chain(M).process(x)
    b = O.Chain(M, dc_alpha=0.0005, pfb_m=7, pfb_as=80.0).process(x)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert np.array_equal(O.Chain(M).taps, O.Pfb(M).taps)


@pytest.mark.parametrize("M,m,As", [(20, 1, 60.0), (20, 3, 80.0), (64, 4, 60.0), (256, 7, 100.0), (256, 12, 80.0), (1024, 16, 80.0)])
def test_chain_channelizer_uses_the_designed_prototype(M, m, As):
    ch = O.Chain(M, pfb_m=m, pfb_as=As)
    assert np.array_equal(ch.taps, O.Pfb(M, m, As).taps)
    # the chain's DeNo output without a DC blocker is the channelizer's
    x = synth_cf32(M * (2 * m + 8), M, seed=11)
    got = O.Chain(M, dc_block=False, pfb_m=m, pfb_as=As).process(x)
    want = O.Chan(M, m, As).process(x)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
