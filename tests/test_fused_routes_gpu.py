"""The CF32 planes of the hand-written fused routes (k_tile256, k_run256v2[/G], k_run64, k_run64v2, k_run1024v3, k_shard1024,
k_front4096 + k_back4096 and the *_dcfix kernels behind them) per channel, per frame and per element against the f64 truth: the case
table, the fixtures F0 / F1 / F2, the two row groups and the bounds (a), (b), (c) with their d are in fused_cases.py;
test_fused_routes_cpu.py asserts what this file relies on (the table against its sources, the fixture conditions, the mutations the
bounds catch, the oracle inside them).

Every case opens its handle with the case's knobs, makes the case's calls (process, or submit_device / wait_device for the entry-point
case), asserts csdr_chain_path, the timed kernel of every call and a finite output, evaluates the three bounds per row group and prints
one line: path, kernels, the three worst ratios and where each occurs (band row, frame).  On F0 (blocker off) a second cutting of the
same stream, every frame on the same kernel, must give the same bits.  The worst ratio per route and fixture is printed at the end
(DESIGN.md 5 carries the table as measured on an MI355X)."""
import numpy as np
import pytest

import fused_cases as F
from util import knob

pytestmark = pytest.mark.gpu

cs = pytest.importorskip("composable_sdr_amd")
from composable_sdr_amd import _lib  # noqa: E402

TIMED = _lib.FLAG_QUIET | _lib.FLAG_TIME_KERNELS
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def worst_ratios():
    yield
    print("\nworst (a) / (b) / (c) ratio per route and fixture")
    for (cid, fx), (a, b, c) in _WORST.items():
        print(f"  {cid:24s} {fx}  {a:.3f}  {b:.3f}  {c:.3f}")


def _open(c, fixture, calls, monkeypatch):
    for k, v in c.knobs.items():
        knob(monkeypatch, k, v)
    ch = cs.Chain(channels=c.M, kf=F.KF, dc_block=F.FIXTURES[fixture][0], dc_alpha=F.ALPHA, max_frames=max(calls), flags=TIMED, **F.chain_kw(c))
    assert ch.path == c.path, (c.id, ch.path, c.path)
    return ch


def _close(c, ch, monkeypatch):
    ch.close()
    for k in c.knobs:
        monkeypatch.delenv(k, raising=False)


def _process(c, fixture, x, calls, monkeypatch, timed=None):
    """one handle, the calls through process -> (output, timed kernel of every call); the kernels asserted against `timed`"""
    ch = _open(c, fixture, calls, monkeypatch)
    outs, names, pos, M = [], [], 0, c.M
    try:
        for f in calls:
            outs.append(ch.process(x[pos * M:(pos + f) * M]))
            names.append(ch.kernel_time()[0])
            pos += f
        assert ch.path == c.path, (c.id, ch.path)
    finally:
        _close(c, ch, monkeypatch)
    if timed is not None:
        assert names == timed, (c.id, names, timed)
    return np.concatenate(outs, axis=-1), names


def _submit_device(c, fixture, x, calls, monkeypatch):
    """csdr_chain_submit_device on HBM-resident chunks, one wait_device behind them -> (output, kernels); >= 2 independent launches"""
    import torch
    dev = torch.device("cuda", 0)
    M, C = c.M, F.rows_of(c).size
    xd = torch.from_numpy(x.view(np.float32).copy()).to(dev)
    ch = _open(c, fixture, calls, monkeypatch)
    outs, pos = [], 0
    try:
        for f in calls:
            o = torch.empty(C * f, dtype=torch.complex64, device=dev)
            n_out = ch.submit_device(xd.data_ptr() + pos * M * 8, M * f, o.data_ptr())
            assert n_out == C * f, (c.id, n_out)
            outs.append(o)
            pos += f
        ch.wait_device()
        torch.cuda.synchronize()
        n_indep, name = ch.independent_launches(), ch.kernel_time()[0]
    finally:
        _close(c, ch, monkeypatch)
    assert n_indep >= 2, (c.id, n_indep)
    assert name == c.timed[-1], (c.id, name)
    return np.concatenate([o.cpu().numpy().reshape(C, -1) for o in outs], axis=1), [name] * len(calls) + [f"{n_indep} independent"]


@pytest.mark.parametrize("c,fixture", F.PARAMS, ids=F.PARAM_IDS)
def test_fused_route_per_channel_frame_and_element(c, fixture, monkeypatch):
    R = F.refs(c, fixture)
    x = R["x"]
    if c.entry == "submit_device":
        got, names = _submit_device(c, fixture, x, c.calls, monkeypatch)
    else:
        got, names = _process(c, fixture, x, c.calls, monkeypatch, c.timed)
    assert got.shape == R["r"].shape and got.dtype == np.complex64, (c.id, got.shape, R["r"].shape)
    assert np.isfinite(got.view(np.float32)).all(), f"{c.id} {fixture}: non-finite output"
    res = F.check_groups(c, got, R)
    a, b, cc = F.worst(res)
    _WORST[(c.id, fixture)] = (a, b, cc)
    print(f"{c.id} {fixture} [{c.path}] {names}: d {F.d_of(c):.2f}  worst (a) {a:.3f} (b) {b:.3f} (c) {cc:.3f}  |  {F.describe(res)}")
    assert a <= 1.0, (c.id, fixture, "(a)", F.describe(res))
    assert b <= 1.0, (c.id, fixture, "(b)", F.describe(res))
    assert cc <= 1.0, (c.id, fixture, "(c)", F.describe(res))
    if fixture == "F0" and c.split is not None:
        # blocker off: FIR, DFT and pre-mix indices do not depend on where the calls are cut, and every frame stays on its kernel
        other, onames = _process(c, fixture, x, c.split, monkeypatch, c.split_timed)
        diff = (other.view(np.uint32) != got.view(np.uint32)).reshape(got.shape + (2,)).any(axis=2)
        print(f"{c.id} {fixture} split {c.split} {onames}: {int(diff.sum())} of {diff.size} elements differ")
        assert np.array_equal(other.view(np.uint32), got.view(np.uint32)), (c.id, c.split, int(diff.sum()), np.argwhere(diff)[:4].tolist())
