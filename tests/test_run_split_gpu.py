"""k_run256v2<FM> + k_run256_dcfix on the weighted split of csrc/run_split.h (whole tile pairs, the same total on every CU).

256 channels, FM, three workgroups per CU.  The weighted split engages when a call has one run per workgroup slot and the
youngest class still gets 8 tiles: nf = 32 cus q frames for the smallest such q (q = 19 pairs per CU with the shipped shares:
(9, 6, 4) pairs; _pairs below restates make_split's choice).  Three sizes: that one, + 16 frames (an odd last tile) and + 32 x 37 frames (pairs that do not divide over the
CUs).  Every size is fed behind a first call of 16 x 9 + 5 frames, so that the big call starts from a carried state (DC state,
FIR window, FM history) and on an odd frame.

Yardstick: the same handle type with equal shares (CSDR_RUN_WEIGHTS=1,1,1), and the f32 oracle for the channels 126..129, where
k_run256_dcfix puts back what a run start without warm-up window left out -- a wrong run boundary shows there, in the frames
behind it.  All frames of those four rows are compared (every run boundary is inside), both for the shipped split and for the
yardstick.

Bounds: FM values are compared modulo 1/kf and weighted by min(|r_t|, |r_t-1|) / max|r| like everywhere in the suite
(test_chain_params_gpu._compare); there a GPU result may be 2 x the oracle's own distance to an f64 truth + 2e-5 in RMS and
4 x + 2 ref 1e-4 per element.  Here both sides are f32 results of the same arithmetic, so only the constant terms are allowed:
2e-5 RMS, 2 ref 1e-4 per element.  One stream and one oracle pass serve all cases."""
import numpy as np
import pytest

import oracle_lib as O
from test_chain_params_gpu import KF, REF, TIMED, _input
from util import knob, wrap_pm

pytestmark = pytest.mark.gpu

cs = pytest.importorskip("composable_sdr_amd")

M, ALPHA, FIRST = 256, 0.0005, 16 * 9 + 5
SHARES = (1.6, 1.0, 0.6)        # csrc/kernels_fused.hip v2_weight_fm3
ROWS = [126, 127, 128, 129]
RMS_BOUND, EL_BOUND = 2e-5, 2 * REF * 1e-4
_REF = {}


def _pairs(q, shares):
    """make_split's largest-remainder choice (csrc/run_split.h)"""
    w = [float(np.float32(s)) for s in shares]
    ideal = [q * v / sum(w) for v in w]
    p = [int(v) for v in ideal]
    frac = [v - n for v, n in zip(ideal, p)]
    for _ in range(q - sum(p)):
        k = max(range(len(p)), key=lambda i: (frac[i], -i))
        p[k] += 1
        frac[k] = -1.0
    return p


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _q():
    q = 12
    while min(_pairs(q, SHARES)) < 4:
        q += 1
    return q


def _stream():
    if "x" not in _REF:
        nf = FIRST + 32 * _cus() * _q() + 32 * 37
        x = _input(M, nf, 2207)
        y = O.Chain(M, dc_alpha=ALPHA, demod="none", kf=KF).process(x)
        r = np.abs(y)
        _REF["x"] = x
        _REF["w"] = (np.minimum(r, np.concatenate([np.zeros((M, 1), r.dtype), r[:, :-1]], axis=1)) / r.max()).astype(np.float32)
        _REF["fm"] = np.stack([O.FreqDem(KF).demodulate_block(y[c]) for c in ROWS])
    return _REF["x"]


def _run(x, frames):
    ch = cs.Chain(channels=M, kf=KF, demod="fm", dc_alpha=ALPHA, max_frames=max(frames), flags=TIMED)
    outs, names, pos = [], [], 0
    for f in frames:
        outs.append(ch.process(x[pos * M:(pos + f) * M]))
        names.append(ch.kernel_time()[0])
        pos += f
    ch.close()
    return np.concatenate(outs, axis=-1), names


def _err(a, b, w):
    return np.abs(wrap_pm(a.astype(np.float32) - b.astype(np.float32), np.float32(1.0 / KF))) * w


@pytest.mark.parametrize("extra", [0, 16, 32 * 37], ids=["whole_pairs", "odd_tile", "pairs_left_over"])
def test_weighted_split_matches_equal_shares_and_oracle(extra, monkeypatch):
    x = _stream()
    q = _q()
    frames = [FIRST, 32 * _cus() * q + extra]
    n = sum(frames)
    got, names = _run(x, frames)                        # no knob: the split every caller gets
    knob(monkeypatch, "CSDR_RUN_WEIGHTS", "1,1,1")
    uni, names_u = _run(x, frames)
    assert names[1] == names_u[1] == "k_run256v2<FM>", (names, names_u)
    assert got.shape == uni.shape == (M, n)
    assert np.isfinite(got).all()
    w = _REF["w"][:, :n]
    e = _err(got, uni, w)
    rms, mx = float(np.sqrt(np.mean(e.astype(np.float64) ** 2))), float(e.max())
    eo = _err(got[ROWS], _REF["fm"][:, :n], w[ROWS])
    eu = _err(uni[ROWS], _REF["fm"][:, :n], w[ROWS])
    print(f"q = {q} pairs per CU {_pairs(q, SHARES)}, {frames} frames: against equal shares rms {rms:.3e} max {mx:.3e}; "
          f"channels 126..129 against the oracle: max {float(eo.max()):.3e} (equal shares {float(eu.max()):.3e}), bounds {RMS_BOUND:.1e} / {EL_BOUND:.3e}")
    assert rms <= RMS_BOUND and mx <= EL_BOUND, (rms, mx)
    assert float(eu.max()) <= EL_BOUND, float(eu.max())      # the yardstick itself
    assert float(eo.max()) <= EL_BOUND, float(eo.max())
