"""k_run256v2<FM> in its one-buffer form (one tile buffer, three workgroups per CU; csrc/kernels_fused_v2.hip) on tiny plans.

256 channels, FM, CSDR_RUN_MIN_TILES=1 so that a few hundred frames take the run kernel, CSDR_RESIDENT_WGS to set the number of runs.
One stream of 405 frames with strong DC (test_chain_params_gpu._input) and one set of references serve every case; a case takes a
prefix of the stream.  Compared with O.Chain by the rules of test_chain_params_gpu._compare: the four channels around DC on every
frame (every run boundary is inside), every channel over the first 128 frames of each call.  Every case runs twice on a fresh handle
and the two outputs must be bit-identical: the next tile's DMA lands in the buffer the tile in work has just left, and the kernel
waits for it with a counted s_waitcnt, so a race would show as outputs that differ from run to run before it shows as an error.

What the plan makes of the cases (make_split, run boundaries on even tiles):
  400 frames, 3 runs      tiles [0, 8) [8, 16) [16, 25): even and odd run lengths; the last run ends on an even tile that stores its own
                          half-lines instead of holding them for a partner
  16*17 then 16*8+5       call 1: 2 runs [0, 8) [8, 17); call 2: one run from the carried state, then 5 frames through k_tile256
  256 frames, 1 run       the run start from the carried state with no other run beside it
  CSDR_NOWU=0             cold run starts with read-only warm-up windows (no batched six-tile load in this form)"""
import numpy as np
import pytest

from test_chain_params_gpu import KF, TIMED, _compare, _dc_rows, _input, _references
from util import knob

pytestmark = pytest.mark.gpu

cs = pytest.importorskip("composable_sdr_amd")

M, NF, ALPHA = 256, 405, 0.0005
_REF = {}


def _stream():
    x = _input(M, NF, 1156)
    if "ref" not in _REF:
        _REF["ref"] = _references(x, M, ALPHA, "fm")
        _REF["rows"] = _dc_rows(M).tolist()
    return x


def _run(x, frames):
    ch = cs.Chain(channels=M, kf=KF, demod="fm", dc_alpha=ALPHA, max_frames=max(frames), flags=TIMED)
    outs, names, pos = [], [], 0
    for f in frames:
        outs.append(ch.process(x[pos * M:(pos + f) * M]))
        names.append(ch.kernel_time()[0])
        pos += f
    ch.close()
    return np.concatenate(outs, axis=-1), names


CASES = [
    ("three_runs_8_8_9", {"CSDR_RESIDENT_WGS": "3"}, [400]),
    ("two_calls_ragged", {"CSDR_RESIDENT_WGS": "3"}, [16 * 17, 16 * 8 + 5]),
    ("one_run", {"CSDR_RESIDENT_WGS": "1"}, [16 * 16]),
    ("three_runs_warmup_windows", {"CSDR_RESIDENT_WGS": "3", "CSDR_NOWU": "0"}, [400]),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_run256v2_fm_one_buffer(case, monkeypatch):
    tag, knobs, frames = case
    knob(monkeypatch, "CSDR_RUN_MIN_TILES", "1")
    for k, v in knobs.items():
        knob(monkeypatch, k, v)
    x = _stream()
    n = sum(frames)
    got, names = _run(x, frames)
    again, _ = _run(x, frames)
    assert all(nm == "k_run256v2<FM>" for nm in names), names
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), f"{tag}: two runs of the same calls differ"
    truth, orc, r = _REF["ref"]
    starts = np.cumsum([0] + frames[:-1]).tolist()
    _compare(f"{tag} {names}", got, truth[:, :n], orc[:, :n], r[:, :n], _REF["rows"], starts, True)
