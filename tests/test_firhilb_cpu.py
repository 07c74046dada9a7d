"""The firhilbf restatement (tests/firhilb_restatement.py) on its own: the taps, and the property that decides
tap order and sign -- a real tone at f cycles per real sample leaves the decimator as the UPPER sideband, a complex tone at 2 f
cycles per complex sample, with the image at -2 f suppressed.

The bounds: the float64 run of the recall gives images of -61.76 dB at f = 0.1 / 0.4 and -63.3 dB at 0.2 - 0.3 and gains of
0.9993 - 1.0008 (Hann-windowed 8192-point spectrum, power within +-0.01 of each line); the asserted -58 dB and 5e-3 leave 3 dB
and a factor of six for window leakage choices, not for arithmetic."""
import numpy as np
import pytest

import firhilb_restatement as F

f32 = np.float32
HQ_M5_AS60 = [0.0065559, 0.0252240, 0.0689129, 0.1714716, 0.6219635, -0.6219635, -0.1714716, -0.0689129, -0.0252240, -0.0065559]


def test_taps_are_antisymmetric_and_as_listed():
    hq = F.design(5, 60.0)
    assert hq.size == 10
    assert np.array_equal(hq, -hq[::-1])
    np.testing.assert_allclose(hq, HQ_M5_AS60, rtol=0, atol=1e-6)
    assert np.array_equal(F.FirHilb().hq, hq.astype(f32))


def _line_power(spec_pow, freqs, f0, half=0.01):
    d = np.abs((freqs - f0 + 0.5) % 1.0 - 0.5)
    return spec_pow[d <= half].sum()


@pytest.mark.parametrize("f", [0.1, 0.2, 0.2875, 0.3, 0.4])
def test_real_tone_becomes_the_upper_sideband(f):
    N = 8192
    n = np.arange(2 * (N + 64))
    x = np.cos(2 * np.pi * f * n + 0.3).astype(f32)
    y = F.FirHilb().decim(x)[64:64 + N]                      # behind the filter's transient
    w = np.hanning(N)
    S = np.abs(np.fft.fft(y.astype(np.complex128) * w)) ** 2
    fr = np.fft.fftfreq(N)
    up, im = _line_power(S, fr, 2 * f), _line_power(S, fr, -2 * f)
    # a unit real tone is two lines of amplitude 1/2; the decimator keeps one of them at gain 2 h_centre ~ 1 -> amplitude 1
    ref = _line_power(np.abs(np.fft.fft(np.exp(2j * np.pi * 2 * f * np.arange(N)) * w)) ** 2, fr, 2 * f)
    gain = np.sqrt(up / ref)
    image_db = 10 * np.log10(im / up)
    print(f"f = {f}: gain {gain:.5f}, image {image_db:.2f} dB")
    assert abs(gain - 1.0) < 5e-3
    assert image_db <= -58.0


def test_chunking_does_not_change_a_bit_and_odd_tail_is_dropped():
    rng = np.random.default_rng(3)
    x = rng.standard_normal(2 * 3000).astype(f32)
    one = F.FirHilb().decim(x)
    calls = [0, 1, 7, 0, 512, 3, 1000, 1477]
    assert sum(calls) == 3000
    got = F.run_calls(F.FirHilb(), x, calls)
    assert np.array_equal(got.view(np.uint32), one.view(np.uint32))
    assert np.array_equal(F.FirHilb().decim(x[:2001]), one[:1000])


def test_interp_of_decim_is_the_delayed_quadrature_of_a_band_limited_signal():
    """interp(decim(x)): the decimator delays the odd samples by 2 m - 1 and estimates the quadrature xq (cos -> sin) at their
    instants from the even ones; the interpolator hands the imaginary part, xq, to its delay branch and filters the real part
    with the same taps, which again estimates xq.  So the round trip is xq delayed by 4 m - 1 real samples: the amplitude
    spectrum of x with every tone turned by -90 degrees, which is what the recalled interpolator does, not a copy of x.
    Bound: the image level of the tone test, -58 dB, on the rms error over the band 0.1 .. 0.4."""
    m, N = 5, 16384
    x, xq = F.band_limited(N)
    y = F.FirHilb().interp(F.FirHilb().decim(x.astype(f32))).astype(np.float64)
    d = 4 * m - 1
    err = y[d + 200:] - xq[200:-d]
    rel_db = 20 * np.log10(np.sqrt(np.mean(err ** 2)) / np.sqrt(np.mean(x ** 2)))
    print(f"round trip: delay {d}, error {rel_db:.2f} dB")
    assert rel_db <= -58.0
