"""The AM and WBFM tails of the chain handle (capi.hip chain_call: k_am; k_biquad + k_firdecim; launch_mix; the backward handle's row
reversal), per row, on every route and staging: the case table, the truth, the bounds and their sources are in chain_tail_cases.py;
test_chain_tails_cpu.py asserts what this file relies on (the twin decomposition is the oracle's own, the truths, the table, the
mutations the bounds catch).

Every case runs its handle and the handle's twin (same configuration, demod "none" for AM, "fm" at kf = 0.6 for WBFM, no --mix) on the
same input in the same calls, asserts csdr_chain_path, the timed kernel of the calls the table makes a claim for and
agc_tile_major_calls() on both, holds the handle's output to the f64 tail of the twin's rows -- every row, every sample -- and prints
one line: case, path, the timed kernels, worst ratio d_c / bound_c and its row (its output sample when mixing).
  A  seams of k_am / k_biquad / k_firdecim on small handles, seven and more calls
  B  every route and kind of shard, short ragged calls, with and without --mix
  C  the AGC stagings: FLAG_AGC_SEQUENTIAL (AM: in place on d_amz), the row-major time-parallel tail, the tile-major plane
  D  backward handles
  E  submit / collect, submit_device / wait_device, reset, seek_frames, a row against a one-row shard: bit for bit"""
import numpy as np
import pytest

import chain_tail_cases as K
from util import knob

pytestmark = pytest.mark.gpu

cs = pytest.importorskip("composable_sdr_amd")
from composable_sdr_amd import _lib  # noqa: E402

TIMED = _lib.FLAG_QUIET | _lib.FLAG_TIME_KERNELS
_TWIN, _REF = {}, {}
WORST = {}                                     # (group, demod) -> (ratio, case, row)


@pytest.fixture(scope="module", autouse=True)
def _summary():
    """behind the file's last test: the worst ratio of every group that ran"""
    yield
    for (g, dem), (w, cid, at) in sorted(WORST.items()):
        print(f"group {g} {dem}: worst ratio {w:.3f} ({cid}, at {at})")


def _ids(cases):
    return [c.id for c in cases]


def _flags(c):
    flags = TIMED
    for f in c.flags:
        flags |= getattr(_lib, f)
    return flags


def _open(c, kw, monkeypatch):
    for k, v in c.knobs.items():
        knob(monkeypatch, k, v)
    return cs.Chain(channels=c.M, max_frames=c.max_frames, flags=_flags(c), **kw)


def _shut(c, ch, monkeypatch):
    ch.close()
    for k in c.knobs:
        monkeypatch.delenv(k, raising=False)


def _own_kw(c):
    return dict(c.kw, demod=c.demod)


def _calls(ch, M, x, calls, pos=0):
    """the calls through csdr_chain_process -> (outputs, timed kernel of every call)"""
    outs, names = [], []
    for f in calls:
        outs.append(ch.process(x[pos * M:(pos + f) * M]))
        names.append(ch.kernel_time()[0])
        pos += f
    return outs, names


def _run(c, kw, x, monkeypatch, path):
    """one handle with keywords kw, the case's calls on x -> output; path, timed kernels and the tile-major count asserted"""
    ch = _open(c, kw, monkeypatch)
    try:
        got_path = ch.path
        assert all(s in got_path for s in path) and not any(s in got_path for s in c.nopath), (c.id, got_path, path, c.nopath)
        outs, names = _calls(ch, c.M, x, c.calls)
        for f, want, name in zip(c.calls, c.timed, names):
            assert want is None or name.startswith(want), (c.id, f, want, names)
        if c.tm is not None:
            assert ch.agc_tile_major_calls() == len(c.tm), (c.id, ch.agc_tile_major_calls(), c.tm)
        ch.status()
    finally:
        _shut(c, ch, monkeypatch)
    return np.concatenate(outs, axis=-1), f"{got_path}; {', '.join(dict.fromkeys(names))}"


def _twin(c, x, monkeypatch):
    key = K.twin_key(c)
    if key not in _TWIN:
        if len(_TWIN) > 2:
            _TWIN.clear()
            _REF.clear()
        z, _ = _run(c, K.twin_kw(c), x, monkeypatch, c.path[:-1])
        assert z.shape == (K.rows_of(c), sum(c.calls)) and z.dtype == (np.complex64 if c.demod == "am" else np.float32), (c.id, z.shape, z.dtype)
        assert np.isfinite(z.view(np.float32)).all(), c.id
        z.setflags(write=False)
        _TWIN[key] = z
    return _TWIN[key]


def _ref(c, twin):
    key = (K.twin_key(c), c.kw.get("deemph_fc"), c.kw.get("decim"))
    if key not in _REF:
        _REF[key] = K.reference(c.demod, twin, c.kw.get("deemph_fc"), c.kw.get("decim"))
    return _REF[key]


def _hold(c, got, ref, path):
    """dtype, n_out, finiteness and the bound; prints and records the worst ratio"""
    no = sum(c.calls) // c.kw.get("decim", 1)
    assert got.dtype == np.float32 and got.size == K.n_out(c, sum(c.calls)), (c.id, got.dtype, got.size)
    assert got.shape == ((no,) if K.mixed(c) else (K.rows_of(c), no)), (c.id, got.shape)
    assert np.isfinite(got).all(), f"{c.id}: non-finite output"
    w, at = K.worst(got, ref, K.mixed(c))
    print(f"{c.id} [{path}]: worst ratio {w:.3f} at {'sample' if K.mixed(c) else 'row'} {at}")
    if w >= WORST.get((c.group, c.demod), (-1.0,))[0]:
        WORST[(c.group, c.demod)] = (w, c.id, at)
    assert w <= 1.0, (c.id, w, at)


def _check(c, monkeypatch):
    x = K.fixture(c.fix, c.M, sum(c.calls))
    twin = _twin(c, x, monkeypatch)
    ref = _ref(c, twin)
    got, path = _run(c, _own_kw(c), x, monkeypatch, c.path)
    _hold(c, got, ref, path)
    return twin, got


# --------------------------------------------------------------------------- A: seams on small handles
@pytest.mark.parametrize("c", K.A_CASES, ids=_ids(K.A_CASES))
def test_seams_on_small_handles(c, monkeypatch):
    _check(c, monkeypatch)


# --------------------------------------------------------------------------- B: every route, short calls
@pytest.mark.parametrize("c", K.B_CASES, ids=_ids(K.B_CASES))
def test_every_route_short_calls(c, monkeypatch):
    _check(c, monkeypatch)


# --------------------------------------------------------------------------- C: the AGC stagings
@pytest.mark.parametrize("c", K.C_CASES, ids=_ids(K.C_CASES))
def test_agc_stagings(c, monkeypatch):
    twin, got = _check(c, monkeypatch)
    muted = (twin == 0).mean(axis=1)
    print(f"{c.id}: {100 * float((twin == 0).mean()):.1f} % of the plane muted; rows that open and mute inside the stream: "
          f"{int(np.sum((muted > 0.1) & (muted < 0.9)))} of {twin.shape[0]}")
    assert 0.02 < float((twin == 0).mean()) < 0.98 and np.sum((muted > 0.1) & (muted < 0.9)) >= 2, c.id     # the squelch opens and closes


# --------------------------------------------------------------------------- D: backward handles
@pytest.mark.parametrize("c", K.D_CASES, ids=_ids(K.D_CASES))
def test_backward_handles(c, monkeypatch):
    """row k against the tail of twin row k (the twin is a backward handle too); and the twin's rows are the forward handle's, reversed:
    a reversal in front of the tail instead of behind it would give the same rows, one that lost its place would not"""
    twin, got = _check(c, monkeypatch)
    x = K.fixture(c.fix, c.M, sum(c.calls))
    ch = _open(c, dict(K.twin_kw(c), dft_backward=False), monkeypatch)
    try:
        fwd = np.concatenate(_calls(ch, c.M, x, c.calls)[0], axis=-1)
    finally:
        _shut(c, ch, monkeypatch)
    want = fwd[(c.M - np.arange(c.M)) % c.M]
    assert np.array_equal(twin.view(np.uint32), want.view(np.uint32)), c.id


# --------------------------------------------------------------------------- E: entry points and state
def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("c", K.E_CASES, ids=_ids(K.E_CASES))
def test_submit_collect_reset_and_seek(c, monkeypatch):
    """csdr_chain_process over seven calls inside the bound; then, bit for bit: reset() and the same stream; submit / collect with three
    chunks in flight, page-locked buffers and one pageable pair (out_bytes = n_out * 4: the buffers are pre-filled with NaN);
    seek_frames(33) on the used handle against a fresh handle after the same seek"""
    from composable_sdr_amd.pipes import host_array
    M, calls, d = c.M, c.calls, c.kw.get("decim", 1)
    x = K.fixture(c.fix, M, sum(calls))
    twin = _twin(c, x, monkeypatch)
    a = _open(c, _own_kw(c), monkeypatch)
    b = _open(c, _own_kw(c), monkeypatch)
    f = _open(c, _own_kw(c), monkeypatch)
    try:
        want, _ = _calls(a, M, x, calls)
        _hold(c, np.concatenate(want, axis=-1), _ref(c, twin), a.path)
        a.reset()
        again, _ = _calls(a, M, x, calls)
        assert all(_same(g, w) for g, w in zip(again, want)), (c.id, "reset")
        C = K.rows_of(c)
        ins = [host_array((max(calls) * M,), np.complex64) for _ in range(3)]
        outs = [host_array((C * (max(calls) // d),), np.float32) for _ in range(3)]
        got, pend, pos = [], 0, 0
        for i, nf in enumerate(calls):
            if pend == 3:
                got.append(b.collect().copy()); pend -= 1
            k = i % 3
            ins[k].a[:nf * M] = x[pos * M:(pos + nf) * M]; pos += nf
            if i == 4:                                           # a pageable pair in the middle of the stream
                b.submit(ins[k].a[:nf * M].copy(), np.full((C, nf // d), np.nan, np.float32))
            else:
                outs[k].a[:] = np.nan
                b.submit(ins[k].a[:nf * M], outs[k].a[:C * (nf // d)].reshape(C, nf // d))
            pend += 1
        while pend:
            got.append(b.collect().copy()); pend -= 1
        b.status()
        assert all(_same(g, w) for g, w in zip(got, want)), (c.id, "submit / collect", [bool(_same(g, w)) for g, w in zip(got, want)])
        a.seek_frames(K.E_SEEK)
        f.seek_frames(K.E_SEEK)
        ya, _ = _calls(a, M, x, calls[1:], pos=K.E_SEEK)
        yf, _ = _calls(f, M, x, calls[1:], pos=K.E_SEEK)
        assert all(_same(g, w) for g, w in zip(ya, yf)), (c.id, "seek_frames")
        assert not _same(ya[0], want[1])                          # (the seek did move the stream)
    finally:
        for h in (a, b, f):
            _shut(c, h, monkeypatch)


@pytest.mark.parametrize("c", K.E_CASES, ids=_ids(K.E_CASES))
def test_submit_device_is_process_device(c, monkeypatch):
    """csdr_chain_submit_device + csdr_chain_wait_device against csdr_chain_process_device on a second handle, bit for bit"""
    import torch
    M, calls, d, C = c.M, c.calls, c.kw.get("decim", 1), K.rows_of(c)
    x = K.fixture(c.fix, M, sum(calls))
    xd = torch.from_numpy(np.ascontiguousarray(x).view(np.float32).copy()).cuda()
    a = _open(c, _own_kw(c), monkeypatch)
    b = _open(c, _own_kw(c), monkeypatch)
    try:
        oa = [torch.full((C * (nf // d),), float("nan"), dtype=torch.float32, device="cuda") for nf in calls]
        ob = [torch.full_like(o, float("nan")) for o in oa]
        torch.cuda.synchronize()
        pos = 0
        for nf, ya, yb in zip(calls, oa, ob):
            ptr = xd.data_ptr() + pos * M * 8
            assert a.process_device(ptr, M * nf, ya.data_ptr(), 0) == K.n_out(c, nf)
            assert b.submit_device(ptr, M * nf, yb.data_ptr()) == K.n_out(c, nf)
            pos += nf
        b.wait_device()
        torch.cuda.synchronize()
        a.status(); b.status()
        for nf, ya, yb in zip(calls, oa, ob):
            assert torch.isfinite(ya).all() and torch.equal(ya.view(torch.int32), yb.view(torch.int32)), (c.id, nf)
    finally:
        _shut(c, a, monkeypatch)
        _shut(c, b, monkeypatch)


@pytest.mark.parametrize("c", [c for c in K.E_CASES if c.M == 256], ids=_ids([c for c in K.E_CASES if c.M == 256]))
def test_a_row_is_the_one_row_shards_row(c, monkeypatch):
    """row r of the whole-band handle against a handle that owns channel r alone, bit for bit: the first, a middle and the last row"""
    x = K.fixture(c.fix, c.M, sum(c.calls))
    whole_twin = _twin(c, x, monkeypatch)
    whole, _ = _run(c, _own_kw(c), x, monkeypatch, c.path)
    for r in (0, 137, c.M - 1):
        sh = dict(chan_first=r, chan_count=1)
        for kw, full in ((dict(K.twin_kw(c), **sh), whole_twin), (dict(_own_kw(c), **sh), whole)):
            ch = _open(c, kw, monkeypatch)
            try:
                row = np.concatenate(_calls(ch, c.M, x, c.calls)[0], axis=-1)
            finally:
                _shut(c, ch, monkeypatch)
            assert row.shape == (1, full.shape[1]) and _same(row[0], full[r]), (c.id, r, kw["demod"])
