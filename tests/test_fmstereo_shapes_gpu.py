"""Stereo FM decoding (csdr_fmstereo_*) on the GPU away from FmStereo(192e3, 4): other taps and delays (odd N,
the smallest and the largest design, the rates at which f32 rounding decides the delay), decimations 1 ... 4096, call sizes that
are no multiple of the decimation or shorter than the histories, a partial wave of rows, and silent rows.

Comparisons against the restatement use an on-frequency pilot (the acquisition of an offset pilot amplifies LSB differences,
see tests/test_fmstereo_gpu.py) and the per-case bounds of tests/fms_cases.py, which come from the restatement's own rounding
(F.decode(sums="f32") against the default); tests/test_fmstereo_cpu.py asserts their caps for the same inputs.  Offset pilots
appear only where the GPU is compared with itself, bit for bit.  Nothing here drives the GPU into an error path."""
import faulthandler

import numpy as np
import pytest

import fms_cases as K
import fms_restatement as F

pytestmark = pytest.mark.gpu

cs = pytest.importorskip("composable_sdr_amd")


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(120, exit=True)          # a GPU call that does not come back ends the process
    yield
    faulthandler.cancel_dump_traceback_later()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(got, want, what):
    assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want)), what


def _words_diff(a, b):
    return [((int(x) - int(y) + 2 ** 31) % 2 ** 32) - 2 ** 31 for x, y in zip(a, b)]


def _check_words(tag, got, want, q):
    """the PLL end words (theta, d_theta) against the restatement's: the loops track the same pilot, |d d_theta| / 2^32 q < 0.01 Hz"""
    dw = _words_diff(got, want)
    print(f"{tag}: theta {got[0]} ({dw[0]:+d} LSB), d_theta {got[1]} ({dw[1]:+d} LSB = {dw[1] / 2 ** 32 * q:+.2e} Hz)")
    assert abs(dw[1]) / 2 ** 32 * q < 0.01


def _feed(dec, x, calls):
    """x [n] or [C][n] through `calls` -> (the concatenated output, the per-call output lengths per row)"""
    outs, pos = [], 0
    for c in calls:
        outs.append(dec.process(x[..., pos:pos + c]))
        pos += c
    assert pos == x.shape[-1]
    return np.concatenate(outs, axis=-1), [o.shape[-1] for o in outs]


# ---- a. the design at other rates -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", sorted(K.DESIGNS))
def test_taps_and_delay_of_the_handle(q):
    """(30, 15), (131, 65), (178, 88), (185, 92), (190, 95), (2000, 1000): odd and even N, both limits of quad_rate, and the
    three even-N rates at which the x.5 group delay is rounded by its f32 error (240 kHz down, 256 kHz up)"""
    assert float(np.float32(q)) == q                           # create takes a float
    P = F.design(q)
    dec = cs.FmStereo(q, 4, max_samples=16)
    got = (dec.taps_len, dec.delay)
    dec.close()
    print(f"{q:g} Hz: handle (N, d) = {got}, restatement ({P['N']}, {P['d']}), group delay {P['group_delay']:.6f}")
    assert got == (P["N"], P["d"]) == K.DESIGNS[q]


# ---- b. one row, one call -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.ONE_CALL, ids=[f"{q:g}-{decim}" for q, decim, _, _ in K.ONE_CALL])
def test_one_call_matches_restatement(case):
    q, decim, n, _ = case
    x, ref = K.one_call(*case)
    dec = cs.FmStereo(q, decim, max_samples=n)
    assert (dec.taps_len, dec.delay) == (F.design(q)["N"], F.design(q)["d"])
    got = dec.process(x)
    words = dec.pll()
    dec.close()
    assert got.shape == ref.want.shape == (2 * (n // decim),)
    K.check(f"DeFMS {q:g} Hz decim {decim}", got, ref.want, ref.bounds, ref.pair)
    _check_words(f"DeFMS {q:g} Hz decim {decim}", words, (ref.theta, ref.dtheta), q)


# ---- c. call seams against the restatement, decim 5 at 240 kHz --------------------------------------------------------------
def test_call_seams_match_restatement():
    """calls of 0, 1, decim +- 1, the 16-step staging block +- 1, d +- 1, N - 1 +- 1, the 256-output tile +- 1 and Hx +- 1 samples on
    both sides of a long call: the decimator drops the n % 5 tail of every call and its history comes from the consumed part"""
    q, decim = K.SEAM_Q, K.SEAM_DECIM
    x, calls, ref = K.seams()
    one = cs.FmStereo(q, decim, max_samples=x.size)
    one.process(x)
    w_one = one.pll()
    one.close()
    dec = cs.FmStereo(q, decim, max_samples=max(calls))
    assert (dec.taps_len, dec.delay) == K.DESIGNS[q]
    got, lens = _feed(dec, x, calls)
    words = dec.pll()
    dec.close()
    assert lens == [2 * (c // decim) for c in calls]
    assert got.shape == ref.want.shape
    K.check("DeFMS 240 kHz decim 5 over the seam calls", got, ref.want, ref.bounds, ref.pair)
    _check_words("DeFMS 240 kHz decim 5 over the seam calls", words, (ref.theta, ref.dtheta), q)
    assert words == w_one                                      # the loop sees every sample whatever the decimator drops


# ---- d. chunking bit for bit at decim 1 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [40e3, 250e3])
def test_chunking_at_decim_1_is_bit_identical(q):
    """every call size is a multiple of 1, so any chunking equals one call: 1, 2, 3, 16 +- 1, d +- 1, N - 1 +- 1, Hx +- 1, 256 +- 1 and 0
    samples on both sides of a long call, with a 5 Hz pilot offset"""
    calls = K.chunk_calls(q)
    n = sum(calls)
    x = F.stereo_mpx(n, q, pilot_offset_hz=5.0, seed=12)
    ref = cs.FmStereo(q, 1, max_samples=n)
    one = ref.process(x)
    w_one = ref.pll()
    ref.close()
    assert one.shape == (2 * n,) and np.all(np.isfinite(one)) and np.abs(one).max() > 0.1
    dec = cs.FmStereo(q, 1, max_samples=max(calls))
    got, lens = _feed(dec, x, calls)
    words = dec.pll()
    dec.close()
    assert lens == [2 * c for c in calls]
    _same(got, one, "chunked output")
    assert words == w_one


# ---- e. 67 rows: a partial wave, neighbours, silent rows --------------------------------------------------------------------
def test_67_rows_match_restatement_and_one_row_handles():
    """(250e3, 3) in calls [1500, 2, 2594] with max_samples 2594: k_fms_pll's second workgroup has three live lanes, k_fms_deemph's
    third has six.  Row 1 is all +0.0 and row 2 all -0.0: hs_atan2's signed-zero branches next to live neighbours"""
    q, decim, C = K.ROWS_Q, K.ROWS_DECIM, K.ROWS_C
    X, calls, ref = K.rows()
    multi = cs.FmStereo(q, decim, nchan=C, max_samples=max(calls))
    got, lens = _feed(multi, X, calls)
    words = [multi.pll(r) for r in range(C)]
    multi.close()
    assert lens == [2 * (c // decim) for c in calls] and got.shape == ref.want.shape == (C, 2 * sum(c // decim for c in calls))
    worst = [0.0, 0.0, 0.0, 0.0]
    for r in range(C):
        if r in K.ROWS_SILENT:
            continue
        st = K.check(f"row {r}", got[r], ref.want[r], ref.bounds[r], ref.pair[r])
        _check_words(f"row {r}", words[r], (ref.theta[r], ref.dtheta[r]), q)
        worst = [max(a, b) for a, b in zip(worst, (st[0][0], st[1][0], st[0][1], st[1][1]))]
    print(f"67 rows: worst T1 {max(worst[:2]):.2e}, worst T2 {max(worst[2:]):.2e}")
    for r in K.ROWS_SILENT:                                    # magnitude exactly 0: the sign of a zero is not the contract
        assert np.all(np.isfinite(got[r])) and not np.any(got[r]), r
        assert not np.any(ref.want[r]), r
    for r in (0, 1, 2, 3, 63, 64, 66):                         # ... and no row sees its neighbours
        one = cs.FmStereo(q, decim, max_samples=max(calls))
        g1, _ = _feed(one, X[r], calls)
        w1 = one.pll()
        one.close()
        _same(g1, got[r], f"row {r} against its one-row handle")
        assert w1 == words[r], r


# ---- f. the device entry with n < max_samples on a non-default stream -------------------------------------------------------
def test_process_device_short_calls_on_a_side_stream_equal_the_host_entry():
    """(240e3, 5), 3 rows, calls of 2003 and 1501 samples into a handle made for 4096: the planes are laid out by n, the u rows by
    max_samples"""
    import torch
    q, decim, C, cap, calls = 240e3, 5, 3, 4096, [2003, 1501]
    X = np.stack([F.stereo_mpx(sum(calls), q, pilot_offset_hz=3.0 * r - 2.0, seed=40 + r, fl=700.0 + 90.0 * r) for r in range(C)])
    host = cs.FmStereo(q, decim, nchan=C, max_samples=cap)
    want = [host.process(np.ascontiguousarray(X[:, a:a + c])) for a, c in zip(np.cumsum([0] + calls), calls)]
    w_host = [host.pll(r) for r in range(C)]
    host.close()
    dev = cs.FmStereo(q, decim, nchan=C, max_samples=cap)
    side = torch.cuda.Stream()
    pos = 0
    for c, w in zip(calls, want):
        d_in = torch.from_numpy(np.ascontiguousarray(X[:, pos:pos + c])).cuda()
        d_out = torch.full((C * 2 * (c // decim) + 8,), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        assert dev.process_device(d_in.data_ptr(), c, d_out.data_ptr(), side.cuda_stream) == C * 2 * (c // decim)
        side.synchronize()
        got = d_out.cpu().numpy()
        assert np.all(np.isnan(got[-8:]))                      # nothing written behind the output
        _same(got[:-8].reshape(C, -1), w, f"call of {c}")
        pos += c
    assert [dev.pll(r) for r in range(C)] == w_host
    dev.close()
