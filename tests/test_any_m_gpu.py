"""The any-M chain route (csrc/plan_generic.hip, kernels_generic.hip, kernels_dc_tile.hip) per channel, at every DFT kernel of
launch_dft, every frame-major ending and every kind of shard: the case table, the truth, the bounds and their derivation are in
any_m_cases.py; test_any_m_cpu.py asserts what this file relies on (the oracle inside the bounds, the emulated kernels inside half of
the d U terms, the mutations the bounds catch).

Every case creates its handle, asserts csdr_chain_path and the timed kernel of every call (k_pfb_fir, or k_pfb1024), runs the calls
of the table and prints one line: case, path, worst per-channel ratio of (a), worst per-element ratio of (b)."""
import numpy as np
import pytest

import any_m_cases as A
import chain_truth as T
from util import knob

pytestmark = pytest.mark.gpu

cs = pytest.importorskip("composable_sdr_amd")
from composable_sdr_amd import _lib  # noqa: E402

TIMED = _lib.FLAG_QUIET | _lib.FLAG_TIME_KERNELS


def _ids(cases):
    return [c.id for c in cases]


def _run(c, x, monkeypatch, calls=None, seek=0, **over):
    """one handle of case c (keywords overridden by `over`), the calls on x -> output, route asserted"""
    calls = c.calls if calls is None else calls
    kw = dict(c.kw)
    flags = TIMED
    for f in c.flags:
        flags |= getattr(_lib, f)
    flags |= over.pop("flags", 0)
    want_path = over.pop("path", c.path)
    kw.update(over)
    for k, v in c.knobs.items():
        knob(monkeypatch, k, v)
    M = c.M
    ch = cs.Chain(channels=M, kf=A.KF, max_frames=(c.max_frames if calls is c.calls and c.max_frames else max(calls)), flags=flags, **kw)
    try:
        assert ch.path == want_path, (c.id, ch.path, want_path)
        if seek:
            ch.seek_frames(seek)
        outs, pos = [], seek
        for f in calls:
            outs.append(ch.process(x[pos * M:(pos + f) * M]))
            assert ch.kernel_time()[0] == c.timed, (c.id, ch.kernel_time()[0])
            pos += f
    finally:
        ch.close()
        for k in c.knobs:
            monkeypatch.delenv(k, raising=False)
    return np.concatenate(outs, axis=-1)


def _refs(c, f0=0, seek=0):
    G, rows = A.shard_of(c)
    return A.sub(A.refs(c.M, c.kw.get("dc_block", True)), rows, seek + f0, seek + sum(c.calls))


def _check(c, monkeypatch):
    """the bounds of any_m_cases.py on one case of blocks A and B"""
    R = _refs(c)
    fm, mix = c.kw.get("demod") == "fm", bool(c.kw.get("mix"))
    tag = f"{c.id} [{c.path}]"
    if not fm:
        got = _run(c, R["x"], monkeypatch)
        truth, orc = (R["r"].sum(axis=0), A.fold32(R["orc_r"])) if mix else (R["r"], R["orc_r"])
        assert got.shape == truth.shape, (c.id, got.shape, truth.shape)
        a, b = A.check_cf32(tag, got, truth, orc, A.d_of(c))
        assert a <= 1.0, (c.id, a)
        assert b <= 1.0, (c.id, b)
        return
    # FM: E from the route's own CF32 output of the same shard (k_transpose in place of the FM ending)
    cf = _run(c, R["x"], monkeypatch, demod="none", mix=False)
    assert cf.shape == R["r"].shape and np.isfinite(cf.view(np.float32)).all(), c.id
    E = float(np.abs(cf.astype(np.complex128) - R["r"]).max())
    got = _run(c, R["x"], monkeypatch)
    if mix:
        assert got.shape == (R["r"].shape[1],) and np.isfinite(got).all(), (c.id, got.shape)
        ratio, out = A.fm_mix_ratio(got, R, E)
        print(f"{tag}: E {E:.3e}  FM --mix worst per-element ratio {ratio:.3f}  ({100 * out:.2f} % of the samples left out)")
        assert out <= 0.01, (c.id, out)
        assert ratio <= 1.0, (c.id, ratio)
    else:
        worst, bias, bb = T.check_fm(tag, got, R, E, T.phi17())
        assert worst <= 1.0, (c.id, worst)
        assert np.abs(bias).max() <= bb, (c.id, bias, bb)


# --------------------------------------------------------------------------- A: every DFT kernel, whole band
@pytest.mark.parametrize("c", A.A_CASES, ids=_ids(A.A_CASES))
def test_dft_sweep(c, monkeypatch):
    _check(c, monkeypatch)


@pytest.mark.parametrize("c", A.SPLIT_CASES, ids=_ids(A.SPLIT_CASES))
def test_split_stream_equals_one_call_bitwise(c, monkeypatch):
    """DC blocker off: FIR, DFT and NCO indices do not depend on where the calls are cut"""
    R = _refs(c)
    split = _run(c, R["x"], monkeypatch)
    whole = _run(c, R["x"], monkeypatch, calls=[sum(c.calls)])
    a, b = A.check_cf32(f"{c.id} [{c.path}]", split, R["r"], R["orc_r"], A.d_of(c))
    assert a <= 1.0 and b <= 1.0, (c.id, a, b)
    diff = split.view(np.uint32) != whole.view(np.uint32)
    assert not diff.any(), (c.id, int(diff.sum()), np.argwhere(diff)[:4].tolist())


# --------------------------------------------------------------------------- B: the endings on shards
@pytest.mark.parametrize("c", A.B_CASES, ids=_ids(A.B_CASES))
def test_endings_on_shards(c, monkeypatch):
    _check(c, monkeypatch)


# --------------------------------------------------------------------------- C: seek, the AGC tail behind odd C, the backward handle
@pytest.mark.parametrize("c", A.SEEK_CASES, ids=_ids(A.SEEK_CASES))
def test_seek_to_an_odd_frame(c, monkeypatch):
    """seek_frames(33), then the stream from frame 33 on: behind the window fill the output is the un-seeked stream's"""
    R0 = A.refs(c.M, False)
    got = _run(c, R0["x"], monkeypatch, seek=A.SEEK)[:, 14:]
    R = _refs(c, f0=14, seek=A.SEEK)
    a, b = A.check_cf32(f"{c.id} [{c.path}]", got, R["r"], R["orc_r"], A.d_of(c))
    assert a <= 1.0, (c.id, a)
    assert b <= 1.0, (c.id, b)


@pytest.mark.parametrize("c", A.AGC_CASES, ids=_ids(A.AGC_CASES))
def test_agc_tail_behind_odd_channel_counts(c, monkeypatch):
    """the time-parallel AGC tail against CSDR_FLAG_AGC_SEQUENTIAL, bitwise: the last workgroup of 64 streams holds 3, 36 and 1"""
    R0 = A.refs(c.M)
    thr = A.agc_threshold_db(c.M)
    spec = _run(c, R0["x"], monkeypatch, agc=thr)
    seq = _run(c, R0["x"], monkeypatch, agc=thr, flags=_lib.FLAG_AGC_SEQUENTIAL, path="generic")
    open_share = float((spec != 0).mean())
    diff = spec.view(np.uint32) != seq.view(np.uint32)
    print(f"{c.id} [{c.path}]: threshold {thr:g} dB, {100 * open_share:.1f} % of the samples unmuted, {int(diff.sum())} differ")
    assert np.isfinite(spec.view(np.float32)).all() and open_share > 0.5, (c.id, open_share)
    assert not diff.any(), (c.id, int(diff.sum()), np.argwhere(diff)[:4].tolist())


@pytest.mark.parametrize("c", A.BACKWARD_CASES, ids=_ids(A.BACKWARD_CASES))
def test_backward_rows_are_the_forward_rows_reversed(c, monkeypatch):
    """odd frame counts: rows of 2 nf words, no whole 16-byte vectors: the k_rows_reversed<1> arm"""
    assert all(f % 2 for f in c.calls if f)
    R = _refs(c)
    back = _run(c, R["x"], monkeypatch)
    fwd = _run(c, R["x"], monkeypatch, dft_backward=False, path="generic")
    a, b = A.check_cf32(f"{c.id} forward [generic]", fwd, R["r"], R["orc_r"], A.d_of(c))
    assert a <= 1.0 and b <= 1.0, (c.id, a, b)
    want = fwd[(c.M - np.arange(c.M)) % c.M]
    assert np.array_equal(back.view(np.uint32), want.view(np.uint32)), c.id
