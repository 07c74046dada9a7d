"""The f64 restatement of the chain (chain_truth.py) against the f32 oracle, and the conditions test_fm_phase_routes_gpu.py relies on.

No GPU.  One stream of white noise per shape (chain_truth.noise, seed 7 + M) and everything derived from it is computed once.

Truth against oracle: with the DC blocker off the oracle's channel samples sit 8.7e-8 .. 8.9e-8 rel-RMS from the truth at every M (one
f32 rounding of the taps' products and sums; the oracle's DFT is f64), exactly on it at M = 1; the bound is 2e-7.  With the f32 DC
blocker in front (alpha = 0.0005: a state of ~16 sigma, rounded every sample) the distance is ~1e-6, which is why the GPU file takes
the oracle's own distance as its yardstick there.  The oracle's FM output meets the per-sample bound (a) and the octant-bias bound
(b) of the GPU file with its own numbers: E its largest channel-sample error, phi = phi17 (libm's atan2f is far inside it).

Fixture: at most 3 % of the counted samples are left out by `kept`, every octant of the true angle holds at least 8 % of the kept
ones (measured 1.6 .. 2.1 % and >= 10.7 %).

Emulation: the library's two polynomials restated in numpy f32 (chain_truth.emu_fm15 / emu_fm17) meet (a) and (b) on the oracle's
channel samples; a copy with hp off by 1e-6 relative fails (b), one with pi off by 1e-5 fails (a) and (b)."""
import numpy as np
import pytest

import chain_truth as T
import oracle_lib as O
from util import rel_rms

KF, ALPHA, SHAPES = T.KF, T.ALPHA, T.SHAPES
refs, check_fm, cf32_E = T.refs, T.check_fm, T.cf32_E


@pytest.mark.parametrize("dc", [False, True], ids=["nodc", "dc"])
@pytest.mark.parametrize("M,nf", SHAPES, ids=[f"M{m}_{n}" for m, n in SHAPES])
def test_truth_against_oracle_and_fixture_conditions(M, nf, dc):
    R = refs(M, nf, dc)
    e = rel_rms(R["orc_r"], R["r"])
    n_counted, n_kept = int(R["counted"].sum()), int(R["kept"].sum())
    left_out = 1.0 - n_kept / n_counted
    _, cnt = T.octant_bias(np.zeros(R["fm"].shape), R["angle"], R["kept"])
    print(f"M={M} nf={nf} dc={dc}: oracle rel-rms {e:.3e}; left out {left_out:.4f}; octant shares " + " ".join(f"{c / n_kept:.3f}" for c in cnt))
    if not dc:
        assert e <= 2e-7, e
        if M == 1:
            assert e == 0.0
    assert left_out <= 0.03, left_out
    assert cnt.min() >= 0.08 * n_kept, cnt
    worst, bias, bb = check_fm(f"oracle M={M} dc={dc}", R["orc_fm"], R, cf32_E(R), T.phi17())
    assert worst <= 1.0, worst
    assert np.abs(bias).max() <= bb          # (trivially: the oracle's bias is what the bound is made of; printed for DESIGN)
    # power-of-two scaling: every kept sample's |conj(r') r| stays inside [2^-100, 2^100] at 2^-44 and 2^44.  The unnormalised DFT makes
    # |r|^2 grow with M: at 4096 channels the largest products are 2^12.7, so 2^44 takes them to 2^100.7, one binade past the stated
    # domain and 25 binades short of v_rcp_f32's flush at 2^126; the GPU file asserts the same bitwise equality there all the same.
    q = (np.abs(R["r"]) * T.prev(np.abs(R["r"])))[R["kept"]]
    top = 2.0 ** 100 if M < 4096 else 2.0 ** 101
    assert q.min() * 2.0 ** -88 >= 2.0 ** -100 and q.max() * 2.0 ** 88 <= top, (q.min(), q.max())


@pytest.mark.parametrize("M,nf", [(64, 3141), (256, 405)])
def test_oracle_is_invariant_under_power_of_two_scaling(M, nf):
    """what the GPU file asserts of every route holds bit for bit on the f32 oracle: nothing in the linear chain rounds differently
    at another exponent, and arg() does not see a common factor"""
    x = refs(M, nf, True)["x"]
    y0 = O.Chain(M).process(x)
    f0 = O.Chain(M, demod="fm", kf=KF).process(x)
    for k in (-44, -24, 24, 44):
        xs = (x * np.float32(2.0 ** k)).astype(np.complex64)
        y = O.Chain(M).process(xs)
        f = O.Chain(M, demod="fm", kf=KF).process(xs)
        assert np.array_equal((y * np.float32(2.0 ** -k)).view(np.uint32), y0.view(np.uint32)), k
        assert np.array_equal(f.view(np.uint32), f0.view(np.uint32)), k


@pytest.mark.parametrize("kf", [0.3, 0.05])
def test_phi_terms_stay_below_the_cap(kf):
    print(f"kf={kf}: phi15 {T.phi15(kf):.3e} phi17 {T.phi17():.3e} rad")
    assert T.phi15(kf) <= 1e-6 and T.phi17() <= 1e-6


EMU = [("deg15", T.emu_fm15, T.phi15), ("deg17", T.emu_fm17, lambda kf: T.phi17())]


@pytest.mark.parametrize("kf", [0.3, 0.05])
@pytest.mark.parametrize("name,emu,phi", EMU, ids=[e[0] for e in EMU])
def test_emulated_phase_functions_meet_the_bounds_and_a_wrong_constant_does_not(name, emu, phi, kf):
    """on the oracle's channel samples (so E is the oracle's), M = 256, DC blocker off"""
    M, nf = 256, 405
    R = refs(M, nf, False, kf=kf)
    rc = R["orc_r"]
    rp = T.prev(rc)
    E = cf32_E(R)
    worst, bias, bb = check_fm(f"{name} kf={kf}", emu(rp, rc, kf), R, E, phi(kf), kf)
    assert worst <= 1.0 and np.abs(bias).max() <= bb, (worst, bias, bb)
    worst, bias, bb = check_fm(f"{name} kf={kf} hp (1 + 1e-6)", emu(rp, rc, kf, hp_rel=1e-6), R, E, phi(kf), kf, sane=False)
    assert np.abs(bias).max() > bb, (bias, bb)
    worst, bias, bb = check_fm(f"{name} kf={kf} pi (1 + 1e-5)", emu(rp, rc, kf, pi_rel=1e-5), R, E, phi(kf), kf, sane=False)
    assert worst > 1.0 and np.abs(bias).max() > bb, (worst, bias, bb)
