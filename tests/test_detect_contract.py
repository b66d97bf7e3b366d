"""Quadrature detection, host side (no GPU): mcrt_detect_taps, mcrt_detect_gain and mcrt_psf_carrier against tests/detect_mirror.py, the
errors, and -- on the mirror and the oracle -- the point of the feature: what each detector makes of a tone of constant amplitude, and the
speckle statistics of the detected image."""
import ctypes as C
import numpy as np
import pytest

import detect_mirror as dm
import image_cases as ic

f32 = np.float32
INVALID = -1
PI = 3.141592653589793


@pytest.mark.parametrize("n_taps", [3, 7, 15, 31, 63])
def test_taps_match_the_mirror(mcrt, n_taps):
    t = mcrt.host_detect_taps(n_taps)
    M = (n_taps - 1) // 2
    ic.assert_same_bits(t, dm.taps(n_taps), "taps %d" % n_taps)
    odd = np.arange(1, M + 1, 2)
    assert np.array_equal(t[M + odd].view(np.uint32) ^ np.uint32(0x80000000), t[M - odd].view(np.uint32))      # antisymmetric bit for bit
    even = np.arange(0, M + 1, 2)
    assert not t[M + even].view(np.uint32).any() and not t[M - even].view(np.uint32).any()                     # +0.0, not -0.0
    assert (t[M + odd] > 0).all()


def test_default_options(mcrt):
    o = mcrt.DetectOpts()
    o.n_taps = 0
    L = mcrt.load_library()
    assert L.mcrt_default_detect_opts(C.byref(o)) == 0 and o.n_taps == 31
    assert L.mcrt_default_detect_opts(None) == INVALID
    assert mcrt.detect_opts_struct().n_taps == 31 and mcrt.detect_opts_struct(n_taps=7).n_taps == 7
    assert C.sizeof(mcrt.DetectOpts) == 4
    ic.assert_same_bits(mcrt.host_detect_taps(), dm.taps(31), "default taps")


def test_bad_n_taps_leave_the_output_untouched(mcrt):
    L = mcrt.load_library()
    for bad in (0, 1, 5, 9, 33, 65, 67):
        o = mcrt.DetectOpts(); o.n_taps = bad
        out = np.full(80, 7.0, f32)
        assert L.mcrt_detect_taps(C.byref(o), out.ctypes.data_as(C.c_void_p)) == INVALID, bad
        assert (out == 7.0).all(), bad
        g = C.c_double(7.0)
        assert L.mcrt_detect_gain(out.ctypes.data_as(C.c_void_p), bad, 0.25, C.byref(g)) == INVALID and g.value == 7.0, bad
        with pytest.raises(mcrt.McrtError):
            mcrt.host_detect_taps(bad)
    o = mcrt.DetectOpts(); o.n_taps = 31
    out = np.full(80, 7.0, f32)
    assert L.mcrt_detect_taps(None, out.ctypes.data_as(C.c_void_p)) == INVALID and (out == 7.0).all()
    assert L.mcrt_detect_taps(C.byref(o), None) == INVALID
    g = C.c_double(7.0)
    assert L.mcrt_detect_gain(None, 31, 0.25, C.byref(g)) == INVALID and g.value == 7.0
    assert L.mcrt_detect_gain(out.ctypes.data_as(C.c_void_p), 31, 0.25, None) == INVALID
    assert L.mcrt_psf_carrier(4.5, 145, None) == INVALID


def test_carrier(mcrt):
    for freq, want in ((4.5, 0.3475), (5.5, 0.2025), (3.5, 0.4925)):
        got = mcrt.host_psf_carrier(freq, 145)
        assert abs(got - want) < 1e-12, (freq, got)
        assert got == dm.carrier(freq, 145)
    assert mcrt.host_psf_carrier(4.5) == mcrt.host_psf_carrier(4.5, 145)
    for freq, res in ((3.3, 145), (7.0, 100), (2.0, 250), (4.5, 322)):
        assert mcrt.host_psf_carrier(freq, res) == dm.carrier(freq, res) and 0.0 <= dm.carrier(freq, res) <= 0.5


def test_gain(mcrt):
    for n_taps in (3, 7, 15, 31, 63):
        t = mcrt.host_detect_taps(n_taps)
        for f in (0.0, 0.01, 0.05, 0.10, 0.2025, 0.25, 0.3475, 0.40, 0.45, 0.4925, 0.5):
            assert abs(mcrt.host_detect_gain(t, f) - dm.gain(t, f)) < 1e-12, (n_taps, f)
    t = mcrt.host_detect_taps(31)
    for f in (0.05, 0.2025, 0.3475, 0.45):
        g = mcrt.host_detect_gain(t, f)
        print("31 taps: gain(%.4f) = %.6f" % (f, g))
        assert abs(g - 1.0) < 0.01, (f, g)
    assert mcrt.host_detect_gain(t, 0.4925) < 0.5
    # the passbands the header states: within 1 % from 0.05 to 0.45 at 31 taps, from 0.10 to 0.40 at 15
    for n_taps, lo, hi in ((31, 0.05, 0.45), (15, 0.10, 0.40)):
        t = mcrt.host_detect_taps(n_taps)
        worst = max(abs(dm.gain(t, f) - 1.0) for f in np.linspace(lo, hi, 401))
        print("%d taps: worst |G - 1| over %.2f..%.2f = %.5f" % (n_taps, lo, hi, worst))
        assert worst < 0.01


def test_a_tone_of_constant_amplitude(mcrt, orc):
    """cos(2 pi 0.3475 r + 0.3), R = 465: the pulse's own carrier.  The mirror's envelope over the rows [M, R - M) stays within |G - 1| + 1e-5
    of 1 (env^2 = cos^2 + G^2 sin^2), G from mcrt_detect_gain.  The oracle's envelope -- the reference's, joining the local maxima of the
    samples -- deviates from 1 by more than 0.25 over the rows [20, R - 20).  Measured: the mirror 0.002792 (|G - 1| = 0.002792), the oracle
    0.5334."""
    R, n_taps = 465, 31
    M = (n_taps - 1) // 2
    x = np.cos(2.0 * PI * 0.3475 * np.arange(R) + 0.3).astype(f32)
    G = mcrt.host_detect_gain(mcrt.host_detect_taps(n_taps), 0.3475)
    env, _ = dm.detect(x, n_taps)
    dev_q = float(np.abs(env[M:R - M].astype(np.float64) - 1.0).max())
    ref = orc.envelope(np.ascontiguousarray(x[:, None]))[:, 0]
    dev_r = float(np.abs(ref[20:R - 20].astype(np.float64) - 1.0).max())
    print("tone 0.3475: quadrature %.6f (|G - 1| = %.6f), the oracle's envelope %.4f" % (dev_q, abs(G - 1.0), dev_r))
    assert dev_q <= abs(G - 1.0) + 1e-5
    assert dev_r > 0.25


def test_q_of_a_cosine_is_the_gain_times_the_sine(mcrt):
    """a line cos(w r) gives q = G(w) sin(w r) away from the ends: to the float rounding of 16 products and sums of values <= 1 (1e-5)"""
    R, n_taps = 465, 31
    M = (n_taps - 1) // 2
    t = mcrt.host_detect_taps(n_taps)
    r = np.arange(R)
    for f in (0.10, 0.2025, 0.3475, 0.45):
        q = dm.quadrature(np.cos(2.0 * PI * f * r).astype(f32), n_taps)
        want = mcrt.host_detect_gain(t, f) * np.sin(2.0 * PI * f * r)
        assert np.abs(q[M:R - M] - want[M:R - M]).max() < 1e-5, f


def test_speckle_statistics(mcrt):
    """dense Gaussian RF of 64 x 465 (seed 1), convolved axially with host_psf()'s 7 taps, the mirror's envelope over the rows 40 .. R - 40:
    mean / std within 1.91 +- 0.06 (Rayleigh: 1.913).  Measured with seed 1: 1.9185."""
    E, R = 64, 465
    ax, _ = mcrt.host_psf()
    rf = np.random.default_rng(1).standard_normal((E, R))
    conv = np.stack([np.convolve(line, ax.astype(np.float64), mode="same") for line in rf]).astype(f32)
    env, _ = dm.detect(conv, 31)
    a = env[:, 40:R - 40].astype(np.float64)
    snr = a.mean() / a.std()
    print("speckle: mean / std = %.4f" % snr)
    assert abs(snr - 1.91) <= 0.06


def test_mirror_edges_and_special_values():
    """the contract's corner cases on the mirror itself: R <= M, what a NaN reaches, a NaN line, a -0.0 line"""
    for n_taps in (3, 31, 63):
        M = (n_taps - 1) // 2
        for R in (1, 2, M, M + 1):
            x = (np.arange(R) + 1).astype(f32)
            env, iq = dm.detect(x, n_taps)
            assert env.shape == (R,) and iq.shape == (R, 2) and np.isfinite(env).all()
            assert np.array_equal(iq[:, 0], x)
        R, r0 = 100, 41
        x = np.ones(R, f32); x[r0] = np.nan
        env, iq = dm.detect(x, n_taps)
        assert sorted(np.flatnonzero(np.isnan(env))) == dm.reached(r0, R, n_taps)
        assert sorted(np.flatnonzero(np.isnan(iq[:, 1]))) == [r for r in dm.reached(r0, R, n_taps) if r != r0]
        env, _ = dm.detect(np.full(R, np.nan, f32), n_taps)
        assert np.isnan(env).all()
        env, iq = dm.detect(np.full(R, -0.0, f32), n_taps)
        assert not env.view(np.uint32).any() and not iq[:, 1].view(np.uint32).any() and (iq[:, 0].view(np.uint32) == 0x80000000).all()
