"""k_run256v2<FM> (256 channels, FM, AGC off, through the C ABI) on small plans: against the oracle, and bit for bit against what the
build in front of the LDS-wait change of the tile loop wrote (tests/golden/run256v2_fm_small.npz, recorded by
tests/make_golden_run256v2_fm.py on an MI355X from that parent build -- a build golden, not a reference golden).

That change makes the loop's kernarg-pointer stores global (so that hipcc counts the LDS waits instead of draining them) and issues LDS
reads (the FIR taps table, a thread's run of the raw image) ahead of their use; it changes no floating-point operation, so every output
bit must stay.  A read that moved in front of the barrier or the write it depends on, or a wait counted wrongly, would show here as a
changed digest: the cases cover both tile parities (the held half-lines of an even tile), a last tile without a partner, cold run
starts with their side stores and a run 0 that carries stash, DC state and FIR window over from the previous call.

CSDR_RUN_MIN_TILES=1 sends these few hundred frames to the run kernel; the plan makes runs of at least eight tiles
(make_golden_run256v2_fm.CASES says what each shape becomes).  One stream and one set of references serve every case.
Oracle comparison: the rules and bounds of test_chain_params_gpu._compare, as in test_run256_occ3_gpu."""
import numpy as np
import pytest

import make_golden_run256v2_fm as G
from test_chain_params_gpu import TIMED, _compare, _dc_rows, _references
from util import knob

pytestmark = pytest.mark.gpu

cs = pytest.importorskip("composable_sdr_amd")

_REF = {}


def _shared():
    if not _REF:
        x = G.stream()
        _REF["x"] = x
        _REF["ref"] = _references(x, G.M, G.ALPHA, "fm")
        _REF["rows"] = _dc_rows(G.M).tolist()
        _REF["gold"] = dict(np.load(G.GOLD))
    return _REF


@pytest.mark.parametrize("case", G.CASES, ids=[c[0] for c in G.CASES])
def test_run256v2_fm_small_plans(case, monkeypatch):
    tag, frames = case
    knob(monkeypatch, "CSDR_RUN_MIN_TILES", "1")
    S = _shared()
    gold = S["gold"]
    assert np.array_equal(G.digest(S["x"]), gold["x_sha256"]), "the input stream is not the one the fixture was recorded with"
    got, names = G.run_case(cs, S["x"], frames, TIMED)
    assert all(nm == "k_run256v2<FM>" for nm in names), names
    n = sum(frames)
    assert got.shape == (G.M, n) and got.dtype == np.float32
    truth, orc, r = S["ref"]
    starts = np.cumsum([0] + frames[:-1]).tolist()
    _compare(f"{tag} {names}", got, truth[:, :n], orc[:, :n], r[:, :n], S["rows"], starts, True)
    # bit for bit against the parent build: first the parts the fixture keeps in full (they say where a difference sits), then the digest
    bad_dc = np.flatnonzero((got[G.DC_ROWS].view(np.uint32) != gold[tag + "_dc_rows"].view(np.uint32)).any(axis=0))
    assert bad_dc.size == 0, f"{tag}: rows {G.DC_ROWS} differ from the parent build at frames {bad_dc[:8].tolist()} ({bad_dc.size} in all)"
    bad_head = np.argwhere(got[:, :16].view(np.uint32) != gold[tag + "_head"].view(np.uint32))
    assert bad_head.size == 0, f"{tag}: first tile differs from the parent build at (row, frame) {bad_head[:8].tolist()} ({len(bad_head)} in all)"
    assert bytes(G.digest(got)).hex() == bytes(gold[tag + "_sha256"]).hex(), f"{tag}: output differs from the parent build"
