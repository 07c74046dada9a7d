"""The row resampler on the GPU (csdr_rowresamp_*, k_rowresamp), through the C ABI: every element against the f64
truth of tests/rowresamp_restatement.py under the derived bound (P + 3) 2^-24 A_k; against itself bit for bit wherever the
contract says the output does not depend on something (the chunking, the tile an output falls into, the rows beside a row, a
rewind, host versus device entry, refused calls in between, the C++ host); and in front of fskDemodulator, where a channel rate of
25 / 3 samples per symbol has to decode.

Every test runs under a time limit of its own: a watchdog thread ends the process if a GPU call does not come back."""
import ctypes as C
import faulthandler
import functools
import subprocess

import numpy as np
import pytest

import rowresamp_restatement as R
from host_exe import host_exe
from rowresamp_cases import AS_DB, CASES, FSK_BW, FSK_K, FSK_LAG, IDS, ROWS, fsk_rows, length, rows as _rows, shape as _shape, tile_cuts

pytestmark = pytest.mark.gpu

cs = pytest.importorskip("composable_sdr_amd")
from composable_sdr_amd import _lib  # noqa: E402
from composable_sdr_amd import RowResamp, rowResampler, firdes_rowresamp  # noqa: E402,F401  (nothing here runs without them)

f32 = np.float32
LIMIT_S = 120
NCASE = list(range(len(CASES)))


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _same(got, want, what=""):
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert g.dtype == w.dtype and g.shape == w.shape and g.size > 0, (what, g.dtype, w.dtype, g.shape, w.shape)
    g, w = g.view(np.uint32), w.view(np.uint32)
    assert np.array_equal(g, w), (what, int((g != w).sum()), g.size)


def _cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _make(i, nchan=ROWS, max_samples=None):
    rate, m, cplx = CASES[i]
    return RowResamp(rate, m, AS_DB, 0.0, cplx, nchan, max_samples or length(rate, m))


@functools.lru_cache(maxsize=None)
def _case(i):
    """(x [3][n], one call's output [3][n_out], bank, delta, the f64 truth [3][n_out], the bound's A); computed once, never written to"""
    rate, m, cplx = CASES[i]
    x = _rows(ROWS, length(rate, m), cplx, 100 + i)
    h = _make(i)
    (bank, delta), y = h.design(), h.process(x)
    assert h.delay() == bank.shape[1] // 2 and h.time() == R.step(0, delta, x.shape[1])[1]
    h.close()
    truth, A = R.truth(bank, delta, x)
    out = (x, y, bank, truth, A)
    for a in out:
        a.setflags(write=False)
    return out[:3] + (delta,) + out[3:]


def _in_calls(h, x, cuts):
    pos, parts = 0, []
    for c in cuts:
        want = h.count(c)
        parts.append(h.process(x[:, pos:pos + c]))
        assert parts[-1].shape == (x.shape[0], want)
        pos += c
    assert pos == x.shape[1]
    return np.concatenate(parts, axis=1)


@pytest.mark.parametrize("i", NCASE, ids=IDS)
def test_every_element_is_within_the_bound_of_the_truth(i):
    x, y, bank, delta, truth, A = _case(i)
    assert y.shape == truth.shape == (ROWS, R.count(0, delta, x.shape[1])) and np.isfinite(y.view(f32)).all()
    assert np.array_equal(bank, cs.firdes_rowresamp(CASES[i][0], CASES[i][1], AS_DB)[0]) and delta == R.delta_of(CASES[i][0])
    ratio = R.worst_ratio(y, truth, A, bank.shape[1])
    print(f"rowresamp {IDS[i]}: P {bank.shape[1]}, {y.shape[1]} outputs per row, worst |d| / ((P + 3) 2^-24 A_k) = {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("i", NCASE, ids=IDS)
def test_short_and_empty_calls_equal_one_call_bit_for_bit(i):
    x, y, bank = _case(i)[:3]
    P, n = bank.shape[1], x.shape[1]
    cuts = [37, 1, 0, 9, P - 2]
    h = _make(i)
    got = _in_calls(h, x, cuts + [n - sum(cuts)])
    h.close()
    _same(got, y, f"{IDS[i]} cuts {cuts}")


@pytest.mark.parametrize("i", NCASE, ids=IDS)
def test_calls_that_end_around_a_tile_equal_one_call_bit_for_bit(i):
    """calls that yield one output fewer than a tile of the kernel, a tile exactly and one more than a tile (at rates above 1, where
    a sample brings several outputs, the nearest count from above), then the rest"""
    x, y = _case(i)[:2]
    rate, m, _ = CASES[i]
    h = _make(i)
    got = _in_calls(h, x, tile_cuts(rate, m, x.shape[1]))
    h.close()
    _same(got, y, f"{IDS[i]} tile cuts")


def test_calls_that_yield_nothing_carry_the_stream():
    """r = 1/8 in calls of 3 samples: five calls of eight yield nothing and still move the history and the clock on"""
    i = 1
    assert CASES[i][0] == 0.125
    x, y = _case(i)[:2]
    n = 600
    h = _make(i, max_samples=3)
    parts, counts = [], []
    for pos in range(0, n, 3):
        parts.append(h.process(x[:, pos:pos + 3]))
        counts.append(parts[-1].shape[1])
    h.close()
    assert counts[0] == 1 and set(counts) == {0, 1} and counts.count(0) > counts.count(1) and sum(counts) == n // 8
    got = np.concatenate(parts, axis=1)
    _same(got, y[:, :n // 8], "calls of 3 samples at r = 1/8")


@pytest.mark.parametrize("i", NCASE, ids=IDS)
def test_a_row_alone_equals_the_same_row_among_three(i):
    x, y = _case(i)[:2]
    h = _make(i, nchan=1)
    got2 = h.process(x[1:2])                         # [1][n] -> [1][n_out]
    h.rewind()
    got1 = h.process(x[1])                           # [n] -> [n_out]
    h.close()
    _same(got2, y[1:2], f"{IDS[i]} row 1 alone")
    _same(got1, y[1], f"{IDS[i]} row 1 alone, one-dimensional")


@pytest.mark.parametrize("i", [0, 2, 5], ids=[IDS[0], IDS[2], IDS[5]])
def test_rewind_gives_the_state_after_open(i):
    x, y, bank = _case(i)[:3]
    h = _make(i)
    h.process(x[:, :37])                             # history and clock both differ from the open state
    assert h.time() != 0 or CASES[i][0] >= 1
    h.rewind()
    assert h.time() == 0
    got = h.process(x)
    h.rewind()
    h.rewind()
    again = _in_calls(h, x, [100, x.shape[1] - 100])
    h.close()
    _same(got, y, "after rewind")
    _same(again, y, "after two rewinds, in calls")


@pytest.mark.parametrize("i", [0, 3], ids=[IDS[0], IDS[3]])
def test_process_device_on_a_stream_of_the_callers_equals_process(i):
    import torch
    x, y, bank, delta = _case(i)[:4]
    n = x.shape[1]
    cuts = (1001, n - 1001)
    h = _make(i)
    d_x = [torch.from_numpy(np.ascontiguousarray(x[:, a:a + c]).view(f32).copy()).cuda() for a, c in zip((0, cuts[0]), cuts)]
    per = 2 if CASES[i][2] else 1
    d_y = [torch.zeros((ROWS * h.max_out(c) * per,), device="cuda", dtype=torch.float32) for c in cuts]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    counts = []
    with torch.cuda.stream(s):
        for dx, dy, c in zip(d_x, d_y, cuts):
            want = h.count(c)
            counts.append(h.process_device(dx.data_ptr(), c, dy.data_ptr(), s.cuda_stream))
            assert counts[-1] == want <= h.max_out(c)
    s.synchronize()
    h.close()
    got = np.concatenate([t.cpu().numpy()[:ROWS * c * per].view(y.dtype).reshape(ROWS, c) for t, c in zip(d_y, counts)], axis=1)
    _same(got, y, "process_device")


def test_refused_calls_leave_the_stream_where_it_was():
    i = 0
    rate, m, cplx = CASES[i]
    x, y = _case(i)[:2]
    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(L.csdr_rowresamp_open(rate, m, AS_DB, 0.0, 1, ROWS, 2000, C.byref(h)))
    room = L.csdr_rowresamp_max_out(h, 2000)
    assert room == R.count(0, R.delta_of(rate), 2000)
    out = np.empty(ROWS * room, np.complex64)
    n, t0, t1 = C.c_uint32(12345), C.c_uint64(), C.c_uint64()
    parts, pos = [], 0

    def good(c):
        nonlocal pos
        xs = np.ascontiguousarray(x[:, pos:pos + c])
        want = C.c_uint32()
        _lib.check(L.csdr_rowresamp_count(h, c, C.byref(want)))
        _lib.check(L.csdr_rowresamp_process(h, _p(xs), c, _p(out), C.byref(n)))
        assert n.value == want.value
        parts.append(out[:ROWS * n.value].reshape(ROWS, n.value).copy())
        pos += c

    good(37)
    n.value = 12345
    _lib.check(L.csdr_rowresamp_get_time(h, C.byref(t0)))
    x9 = np.ascontiguousarray(x[:, :9])
    big = np.zeros((ROWS, 2001), np.complex64)
    assert L.csdr_rowresamp_process(h, _p(big), 2001, _p(out), C.byref(n)) == _lib.ERR_SIZE              # more than max_samples
    assert "max" in L.csdr_last_error().decode()
    assert L.csdr_rowresamp_process(h, None, 9, _p(out), C.byref(n)) == _lib.ERR_INVALID
    assert L.csdr_rowresamp_process(h, _p(x9), 9, None, C.byref(n)) == _lib.ERR_INVALID
    assert L.csdr_rowresamp_process(h, _p(x9), 9, _p(out), None) == _lib.ERR_INVALID
    assert L.csdr_rowresamp_process(h, _p(out), 9, _p(out), C.byref(n)) == _lib.ERR_INVALID             # the same buffer
    assert L.csdr_rowresamp_process_device(h, None, 9, None, C.byref(n), None) == _lib.ERR_INVALID
    assert L.csdr_rowresamp_process_device(h, _p(out), 9, _p(out), C.byref(n), None) == _lib.ERR_INVALID
    assert L.csdr_rowresamp_process_device(h, _p(x9), 9, _p(out), None, None) == _lib.ERR_INVALID
    assert L.csdr_rowresamp_process_device(h, _p(x9), 2001, _p(out), C.byref(n), None) == _lib.ERR_SIZE
    assert L.csdr_rowresamp_count(h, 2001, C.byref(n)) == _lib.ERR_SIZE
    assert L.csdr_rowresamp_count(h, 9, None) == _lib.ERR_INVALID
    assert L.csdr_rowresamp_get_time(h, None) == _lib.ERR_INVALID
    _lib.check(L.csdr_rowresamp_get_time(h, C.byref(t1)))
    assert n.value == 12345 and t0.value == t1.value
    good(1)
    good(0)
    good(9)
    while pos < x.shape[1]:
        good(min(2000, x.shape[1] - pos))
    assert L.csdr_rowresamp_destroy(h) == 0
    _same(np.concatenate(parts, axis=1), y, "around refused calls")


@pytest.mark.parametrize("i", [0, 2], ids=[IDS[0], IDS[2]])
def test_the_host_program_writes_the_python_pipes_bytes(i, tmp_path):
    rate, m, cplx = CASES[i]
    x = _case(i)[0]
    src, dst = tmp_path / "in.raw", tmp_path / "out.raw"
    np.ascontiguousarray(x).tofile(src)
    cuts = [37, 1, 9, 1500]
    subprocess.run([host_exe("rowresamp_host"), "c" if cplx else "r", f"{rate!r}:{m}:{AS_DB:g}:0", str(ROWS), ",".join(str(c) for c in cuts),
                    str(src), str(dst)], check=True, timeout=LIMIT_S)
    pipe = cs.rowResampler(rate, m, AS_DB, 0.0, cplx, ROWS, max(cuts))
    r = pipe._start()
    parts, pos, k = [], 0, 0
    while pos < x.shape[1]:
        c = min(cuts[k % len(cuts)], x.shape[1] - pos)
        parts.append(pipe._process(r, x[:, pos:pos + c]).reshape(-1))       # the rows of every call, row after row
        pos, k = pos + c, k + 1
    pipe._done(r)
    _same(np.fromfile(dst, dtype=x.dtype), np.concatenate(parts), "rowresamp_host")


# ---------------------------------------------------------------------------- two wide shapes
@pytest.mark.parametrize("rate,m,cplx,nrows,n", [(0.48, 7, True, 300, 64), (1.6, 7, True, 700, 2100)], ids=["300x64", "700x2100"])
def test_many_rows(rate, m, cplx, nrows, n):
    """300 rows of 64 samples: more one-tile rows than a CU holds workgroups, one item per workgroup; 700 rows of 2100 samples at
    r = 1.6: 2800 items, so every workgroup walks several items, of several rows"""
    s = _shape(rate, m, cplx, R.count(0, R.delta_of(rate), n), nrows, _cus())
    assert s["items_per_run"] >= (1 if nrows == 300 else 2) and s["tiles"] == (1 if nrows == 300 else 4), s
    x = _rows(nrows, n, cplx, nrows)
    h = RowResamp(rate, m, AS_DB, 0.0, cplx, nrows, n)
    (bank, delta), y = h.design(), h.process(x)
    h.close()
    truth, A = R.truth(bank, delta, x)
    ratio = R.worst_ratio(y, truth, A, bank.shape[1])
    print(f"rowresamp {nrows} rows of {n} at r = {rate}: {s['runs']} runs of {s['items_per_run']} items, worst ratio {ratio:.3f}")
    assert y.shape == truth.shape and ratio <= 1.0


# ---------------------------------------------------------------------------- end to end: the point of the block
def test_fsk_at_a_fractional_number_of_samples_per_symbol_decodes_behind_the_resampler():
    """3 rows of 2-FSK at 25 / 3 samples per symbol (1200 baud in a 10 kHz channel), 400 symbols behind 4 zeros:
    fskDemodulator(1, 4, 0.25) . rowResampler(0.48); delay (21) plus padding (4) is 25 samples = 3 symbols"""
    sym, x = fsk_rows()
    pipe = cs.compose(cs.fskDemodulator(1, FSK_K, FSK_BW, nchan=ROWS), cs.rowResampler(0.48, nchan=ROWS))
    r = pipe._start()
    got = pipe._process(r, x)
    pipe._done(r)
    rs, dem = cs.RowResamp(0.48, nchan=ROWS), cs.FskDem(1, FSK_K, FSK_BW, nchan=ROWS)
    assert rs.delay() + 4 == 25
    by_hand = dem.process(rs.process(x))
    rs.close()
    dem.close()
    ns = got.shape[1]
    assert got.dtype == np.uint32 and got.shape == (ROWS, ns) and ns >= 399
    errors = int((got[:, FSK_LAG:] != sym[:, :ns - FSK_LAG]).sum())
    print(f"rowresamp end to end: {errors} symbol errors of {ROWS} x {ns - FSK_LAG}")
    assert errors == 0
    assert np.array_equal(got, by_hand)


# ---------------------------------------------------------------------------- life-cycle, as test_block_lifecycle_gpu.py has it
@pytest.mark.parametrize("kind", ["class", "pipe"])
def test_two_handles_are_independent_and_close_is_idempotent(kind):
    i = 0
    rate, m, cplx = CASES[i]
    x = _case(i)[0]
    x1, x2 = x[:, :777], x[:, 777:]
    if kind == "class":
        make, run, done = (lambda: _make(i)), (lambda r, a: r.process(a)), (lambda r: r.close())
    else:
        pipe = cs.rowResampler(rate, m, AS_DB, 0.0, cplx, ROWS, x.shape[1])
        make, run, done = pipe._start, pipe._process, pipe._done
    a, b = make(), make()
    _same(run(a, x1), run(b, x1), "two fresh handles, the same input")
    done(b)
    got = run(a, x2)                                          # the survivor goes on from its own state, in its own buffers
    c = make()
    run(c, x1)
    _same(got, run(c, x2), "the survivor of a destroy against a third fresh handle")
    for r in (a, b, c):
        done(r)
        done(r)                                               # a second close (a second _done) is fine
    for r in (a, b, c):
        for use in (lambda: r.h, lambda: r.process(x1)):
            with pytest.raises(cs.CsdrError) as e:
                use()
            assert e.value.code == _lib.ERR_INVALID and "already destroyed" in str(e.value)
