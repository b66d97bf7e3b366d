"""Spectral Doppler without a GPU (include/mcrt.h: mcrt_spectral_opts, mcrt_gate, mcrt_sonogram_opts and the host helpers
mcrt_spectral_rotor / phase / profile / rates / window / twiddles / draws, mcrt_pulse_waveform): the helpers against tests/spectral_mirror.py
bit for bit, the structs and their defaults, every refusal that needs no device, the draws' known answer and moments, the mirror's FFT
against numpy's in double, what a sonogram shows on the mirror (the peak bin, aliasing, a parabolic lumen, a pulsatile waveform, clutter,
the rotor table's spurs), and the kernels' resources."""
import ctypes as C
import math
import os
import re
import subprocess
import numpy as np
import pytest

import flow_mirror as fm
import spectral_mirror as sm

f32 = np.float32
INVALID, LIMIT = -1, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONES = 0xFFFFFFFF
V_NYQ = 333.33
bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)


# ------------------------------------------------------------------ structs and defaults
def test_structs_and_defaults(mcrt):
    L = mcrt.load_library()
    o = mcrt.SpectralOpts()
    names = ("n_pulses", "gate_rows", "n_fft", "hop", "wall", "wall_bins", "sigma", "seed")
    assert C.sizeof(o) == 32 and [getattr(mcrt.SpectralOpts, n).offset for n in names] == list(range(0, 32, 4))
    assert L.mcrt_default_spectral_opts(C.byref(o)) == 0
    assert tuple(getattr(o, n) for n in names) == (2048, 8, 128, 32, 1, 2, 0.0, 0x53504543)
    assert L.mcrt_default_spectral_opts(None) == INVALID
    assert C.sizeof(mcrt.Gate) == 12 and [getattr(mcrt.Gate, n).offset for n in ("image", "line", "row0")] == [0, 4, 8]
    s = mcrt.SonogramOpts()
    assert C.sizeof(s) == 12 and [getattr(mcrt.SonogramOpts, n).offset for n in ("dynamic_range_db", "gain_db", "ref")] == [0, 4, 8]
    assert L.mcrt_default_sonogram_opts(C.byref(s)) == 0 and (s.dynamic_range_db, s.gain_db, s.ref) == (40.0, 0.0, 0.0)
    assert L.mcrt_default_sonogram_opts(None) == INVALID
    assert mcrt.SPECTRAL_WALLS == {"none": 0, "mean": 1} and mcrt.SPECTRAL_WINDOWS == {"rect": 0, "hann": 1}
    o = mcrt.spectral_opts_struct(n_pulses=100, gate_rows=64, n_fft=512, hop=7, wall="none", wall_bins=0, sigma=0.25, seed=7)
    assert tuple(getattr(o, n) for n in names) == (100, 64, 512, 7, 0, 0, 0.25, 7)
    s = mcrt.sonogram_opts_struct(dynamic_range_db=60, gain_db=-3, ref=2.5)
    assert (s.dynamic_range_db, s.gain_db, s.ref) == (60.0, -3.0, 2.5)
    with pytest.raises(ValueError):
        mcrt.spectral_opts_struct(wall="linear")
    with pytest.raises(ValueError):
        mcrt.host_spectral_window("hamming", 64)
    assert L.mcrt_version() == 109                                     # additive: the number stays


# ------------------------------------------------------------------ the tables
def test_rotor_window_and_twiddles_equal_the_mirrors(mcrt):
    L = mcrt.load_library()
    lut = mcrt.host_spectral_rotor()
    assert lut.dtype == f32 and lut.shape == (4096, 2) and np.array_equal(bits(lut), bits(sm.rotor()))
    assert tuple(lut[0]) == (1.0, 0.0) and lut[1024, 1] == 1.0 and lut[2048, 0] == -1.0 and lut[3072, 1] == -1.0
    assert L.mcrt_spectral_rotor(None) == INVALID
    for N in sm.FFT_SIZES:
        for kind, name in ((0, "rect"), (1, "hann")):
            h = mcrt.host_spectral_window(name, N)
            assert h.shape == (N,) and np.array_equal(bits(h), bits(sm.window(kind, N))) and np.array_equal(h, mcrt.host_spectral_window(kind, N))
        assert (mcrt.host_spectral_window("rect", N) == 1.0).all() and mcrt.host_spectral_window("hann", N)[0] == 0.0 and mcrt.host_spectral_window("hann", N)[N // 2] == 1.0
        tw = mcrt.host_spectral_twiddles(N)
        assert tw.shape == (N // 2, 2) and np.array_equal(bits(tw), bits(sm.twiddles(N)))
        assert tuple(tw[0]) == (1.0, 0.0) and tw[0, 1].view(np.uint32) in (0, 0x80000000) and tw[N // 4, 1] == -1.0
    buf = np.full(1024, -7.0, f32)
    for N in (0, 1, 16, 48, 100, 1024):
        assert L.mcrt_spectral_window(1, N, vp(buf)) == INVALID and L.mcrt_spectral_twiddles(N, vp(buf)) == INVALID
    assert L.mcrt_spectral_window(2, 64, vp(buf)) == INVALID and L.mcrt_spectral_window(1, 64, None) == INVALID and L.mcrt_spectral_twiddles(64, None) == INVALID
    assert (buf == -7.0).all()


# ------------------------------------------------------------------ the phase
def test_phase_equals_the_mirrors(mcrt):
    rng = np.random.default_rng(0)
    for T, lo, hi in ((1, 0, 1), (2, -50, 50), (777, -2 * V_NYQ, 2 * V_NYQ), (16384, -400, 650)):
        speed = rng.uniform(lo, hi, T).astype(f32)
        ph = mcrt.host_spectral_phase(V_NYQ, speed)
        assert ph.dtype == np.int64 and ph.tolist() == sm.phase(V_NYQ, speed)
    # negative speeds take the phase below zero; a step beyond 2^31 (above the Nyquist velocity) and of exactly 2^32 (twice) are allowed
    ph = mcrt.host_spectral_phase(100.0, [-50.0, -50.0, 150.0, 200.0, -200.0, 0.0])
    assert ph.tolist() == [0, -(1 << 30), -(1 << 31), (1 << 30), (1 << 30) + (1 << 32), (1 << 30)]
    assert mcrt.host_spectral_phase(V_NYQ, [V_NYQ / 2] * 3).tolist() == sm.phase(V_NYQ, [V_NYQ / 2] * 3)


def test_phase_refuses(mcrt):
    L = mcrt.load_library()
    out = np.full(16385, -5, np.int64)
    sp = np.zeros(16385, f32)
    call = lambda nyq=100.0, s=sp, T=4, o=out: L.mcrt_spectral_phase(nyq, vp(s), T, vp(o))
    assert call(s=None) == INVALID and call(o=None) == INVALID and call(T=0) == INVALID and call(T=16385) == LIMIT
    for nyq in (0.0, -1.0, np.nan, np.inf):
        assert call(nyq=nyq) == INVALID
    for bad in (np.nan, np.inf, -np.inf):
        s = sp.copy(); s[3] = bad
        assert call(s=s) == INVALID
    for bad in (200.001, -200.001, 1e30):                              # more than twice the Nyquist velocity
        s = sp.copy(); s[2] = bad
        assert call(s=s) == LIMIT
    assert (out == -5).all()
    assert call(T=16384) == 0 and not out[:16384].any() and out[16384] == -5


# ------------------------------------------------------------------ the profile and the rates
LINE = np.array([0] * 5 + [1] * 12 + [0] * 3 + [1] + [0] * 2 + [2] * 7 + [9, 255, 1, 1], np.uint8)      # a lumen of 12 rows, one of 1 row, another
MOVING = [0, 1, 1]                                                                                      # material's, labels past the table, two rows at the end


@pytest.mark.parametrize("exponent", [0.0, 1.0, 2.0, 3.5, 9.0])
def test_profile_equals_the_mirrors(mcrt, exponent):
    R = LINE.size
    for row0, G in ((0, R), (5, 12), (0, 11), (11, 12), (20, 1), (19, 3), (23, 7), (28, 6), (R - 1, 1)):
        got = mcrt.host_spectral_profile(LINE, row0, G, MOVING, exponent)
        assert got.dtype == f32 and np.array_equal(bits(got), bits(sm.profile(LINE, row0, G, MOVING, exponent))), (row0, G)
    whole = mcrt.host_spectral_profile(LINE, 0, R, MOVING, exponent)
    still = np.isin(np.arange(R), [0, 1, 2, 3, 4, 17, 18, 19, 21, 22, 30, 31])
    assert not bits(whole[still]).any()                                # what does not move, labels >= n_labels and 255: +0.0f
    assert whole[20] == 1.0                                            # a lumen of one row is its own axis
    assert np.array_equal(whole[5:17], whole[5:17][::-1]) and np.array_equal(whole[23:30], whole[23:30][::-1])      # symmetric about the axis
    assert whole[26] == 1.0 and (whole[~still] > 0).all() and (whole <= 1).all()
    if exponent == 0.0:
        assert (whole[~still] == 1.0).all()                            # plug flow
    if exponent == 2.0:
        assert whole[5] == f32(1.0 - (5.5 / 6.0) ** 2)                 # row 5 of the run [5, 16]: x = (5 - 10.5) / 6
    half = mcrt.host_spectral_profile(LINE, 0, 11, MOVING, exponent)   # a gate half outside the lumen reads the lumen's own profile
    assert np.array_equal(bits(half), bits(whole[:11]))


def test_profile_refuses(mcrt):
    L = mcrt.load_library()
    out = np.full(70, -7.0, f32)
    mv = np.array(MOVING + [0] * 300, np.uint8)
    call = lambda t=LINE, R=LINE.size, row0=5, G=8, m=mv, n=3, e=2.0, o=out: L.mcrt_spectral_profile(vp(t), R, row0, G, vp(m), n, e, vp(o))
    assert call(t=None) == INVALID and call(m=None) == INVALID and call(o=None) == INVALID
    assert call(R=0) == INVALID and call(G=0) == INVALID and call(n=0) == INVALID
    assert call(G=65) == LIMIT and call(n=255) == LIMIT
    assert call(row0=LINE.size - 7) == INVALID and call(row0=ONES, G=2) == INVALID
    for e in (0.5, -1.0, np.nan, np.inf, 0.999):
        assert call(e=e) == INVALID
    assert (out == -7.0).all() and call() == 0 and (out[:8] != -7.0).all() and (out[8:] == -7.0).all()


def test_rates_equal_the_mirrors_and_refuse(mcrt):
    L = mcrt.load_library()
    rng = np.random.default_rng(1)
    frac = np.concatenate([rng.uniform(0, 1, 60), [0.0, 1.0, 0.5, 2.0 ** -17]]).astype(f32)
    for axial in (1.0, -1.0, 0.0, 0.5, -0.7071067811865476, 1e-9):
        got = mcrt.host_spectral_rates(frac, axial)
        assert got.dtype == np.int32 and np.array_equal(got, sm.rates(frac, axial)) and np.abs(got).max() <= 65536
    assert mcrt.host_spectral_rates([1.0, 0.0, 0.5], -1.0).tolist() == [-65536, 0, -32768]
    assert mcrt.host_spectral_rates([2.0 ** -17, 3 * 2.0 ** -17], 1.0).tolist() == [0, 2]      # ties go to even
    out = np.full(70, -9, np.int32)
    call = lambda f=frac, G=4, a=0.5, o=out: L.mcrt_spectral_rates(vp(f), G, a, vp(o))
    assert call(f=None) == INVALID and call(o=None) == INVALID and call(G=0) == INVALID and call(G=65) == LIMIT
    for a in (1.0000001, -1.5, np.nan, np.inf):
        assert call(a=a) == INVALID
    for bad in (np.nan, -0.001, 1.001, np.inf):
        f = frac.copy(); f[2] = bad
        assert call(f=f) == INVALID
    assert (out == -9).all()


# ------------------------------------------------------------------ the draws
def test_draws_known_answer_and_mirror(mcrt):
    """Random123's kat_vector for philox4x32_10 at all ones, through the helper itself: line = row0 = ONES would need counter word 2 to be
    ONES too, so the known answer is the mirror's block function (the one the helper is compared with), and the helper's is its fold"""
    assert [int(x) for x in fm.philox4x32_10(ONES, ONES, ONES, ONES, ONES, ONES)] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    o = [int(x) for x in fm.philox4x32_10(3, 4, 0x53504543, 5, 1, 2)]
    d = mcrt.host_spectral_draws(1, 2, 3, 4, 6)
    fold = lambda a, b: (a & 0xffff) + (a >> 16) + (b & 0xffff) + (b >> 16) - 131070
    assert d[5].tolist() == [fold(o[0], o[1]), fold(o[2], o[3])]
    for seed, image_id, line, row0, T in ((0x53504543, 0, 0, 0, 1), (0x5EED, 1, 511, 2047, 100), (3, ONES, ONES, ONES, 16384)):
        d = mcrt.host_spectral_draws(seed, image_id, line, row0, T)
        assert d.dtype == np.int32 and d.shape == (T, 2) and np.array_equal(d, sm.draws(seed, image_id, line, row0, T))
        assert np.abs(d.astype(np.int64)).max() <= 131070


def test_draws_are_not_the_colour_stages(mcrt):
    """counter word 2 differs: the same seed, image, scan-line, row and pulse give other numbers than mcrt_flow_draws"""
    s = mcrt.host_spectral_draws(5, 9, 2, 7, 16)
    c = mcrt.host_flow_draws(5, 9, 3, 8, 16)[:, 2, 7]
    assert s.shape == c.shape and not (s == c).any()


def test_draw_moments(mcrt):
    """mcrt_flow_draws' Irwin-Hall sum: mean 0 and variance 1431655765 exactly, held to five standard errors as test_flow_contract does"""
    d = np.concatenate([mcrt.host_spectral_draws(0x53504543, i, 7, 100 + i, 16384) for i in range(8)]).astype(np.float64)
    n, var = d.size, 1431655765.0
    assert abs(d.mean()) < 5.0 * math.sqrt(var / n)
    assert abs(d.var() - var) < 5.0 * var * math.sqrt((3.0 - 0.3 - 1.0) / n)
    assert abs((d[:, 0] * d[:, 1]).mean()) < 5.0 * var / math.sqrt(n / 2)      # I and Q are uncorrelated


def test_draws_and_waveform_refuse(mcrt):
    L = mcrt.load_library()
    d = np.full(2 * 16384 + 8, -12345, np.int32)
    assert L.mcrt_spectral_draws(1, 2, 3, 4, 5, None) == INVALID and L.mcrt_spectral_draws(1, 2, 3, 4, 0, vp(d)) == INVALID
    assert L.mcrt_spectral_draws(1, 2, 3, 4, 16385, vp(d)) == LIMIT and (d == -12345).all()
    assert L.mcrt_spectral_draws(1, 2, 3, 4, 16384, vp(d)) == 0 and (d[-8:] == -12345).all()
    s = np.full(16385 + 4, -7.0, f32)
    call = lambda prf=4000.0, bpm=72.0, pk=500.0, mn=50.0, T=10, o=s: L.mcrt_pulse_waveform(prf, bpm, pk, mn, T, vp(o))
    assert call(o=None) == INVALID and call(T=0) == INVALID and call(T=16385) == LIMIT
    for bad in (0.0, -1.0, np.nan, np.inf):
        assert call(prf=bad) == INVALID and call(bpm=bad) == INVALID
    for bad in (np.nan, np.inf):
        assert call(pk=bad) == INVALID and call(mn=bad) == INVALID
    assert (s == -7.0).all()


def test_pulse_waveform_equals_the_mirrors(mcrt):
    for prf, bpm, pk, mn, T in ((4000.0, 72.0, 500.0, 50.0, 16384), (2500.0, 120.0, -300.0, 20.0, 5000), (8000.0, 60.0, 100.0, 100.0, 1)):
        w = mcrt.host_pulse_waveform(prf, bpm, pk, mn, T)
        assert w.dtype == f32 and np.array_equal(bits(w), bits(sm.pulse_waveform(prf, bpm, pk, mn, T)))
        assert w[0] == f32(mn) and min(pk, mn) <= w.min() and w.max() <= max(pk, mn)
    w = mcrt.host_pulse_waveform(4000.0, 60.0, 500.0, 50.0, 8000)      # one beat a second: systole peaks at 0.15 s, diastole from 0.3 s on
    assert w[600] == 500.0 and (w[1200:4000] == 50.0).all() and np.array_equal(w[:4000], w[4000:])


# ------------------------------------------------------------------ the mirror's FFT
# max |X - numpy.fft(double)| / max |X| over 8 windows of seeded complex noise, measured when the test was written:
FFT_ERROR = {32: 1.26e-7, 64: 1.22e-7, 128: 1.15e-7, 256: 1.18e-7, 512: 1.47e-7}


@pytest.mark.parametrize("N", sm.FFT_SIZES)
def test_mirror_fft_against_numpy(N):
    """the contract's radix-2 order in float32 against numpy's FFT of the same float32 points in double: four times the measured error
    (which is log2 N roundings of 2^-24 each, and no more)"""
    rng = np.random.default_rng(N)
    y = rng.standard_normal((8, N, 2)).astype(f32)
    X = sm.fft(y, sm.twiddles(N)).astype(np.float64)
    ref = np.fft.fft(y[..., 0].astype(np.float64) + 1j * y[..., 1].astype(np.float64), axis=-1)
    err = np.abs((X[..., 0] + 1j * X[..., 1]) - ref).max() / np.abs(ref).max()
    print("N=%d: the mirror's FFT is within %.3e of numpy's, relative to the peak" % (N, err))
    assert err <= 4.0 * FFT_ERROR[N]
    impulse = np.zeros((1, N, 2), f32); impulse[0, 1, 0] = 1.0        # X_k = exp(-2 pi i k / N): the twiddles' sign
    X = sm.fft(impulse, sm.twiddles(N))[0]
    assert abs(X[1, 0] - math.cos(2 * math.pi / N)) < 1e-6 and abs(X[1, 1] + math.sin(2 * math.pi / N)) < 1e-6


# ------------------------------------------------------------------ what a sonogram shows, on the mirror
def _speckle(G, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal((1, 1, G, 2)) * scale).astype(f32)


def _gate_series(speed, frac, axial=1.0, seed=0, clutter=None, sigma=0.0):
    G = len(frac)
    gates = np.array([[0, 0, 0]], np.uint32)
    return sm.series(clutter, _speckle(G, seed), gates, np.ones(G, f32), sm.rates(frac, axial)[None], sm.phase(V_NYQ, speed), sigma=sigma)


def test_plug_flow_peaks_at_its_velocity():
    """plug flow at 100 mm/s, v_nyq 333.33, N = 128: every column's brightest bin is rint(64 + 100 / 333.33 * 64) = 83"""
    z = _gate_series(np.full(1024, 100.0, f32), np.ones(8, f32))
    power, mean = sm.spectrum(z, sm.window(1, 128), V_NYQ)
    assert power.shape == (1, 29, 128) and (power[0].argmax(axis=1) == 83).all()
    assert np.abs(mean[0] - 100.0).max() < 2 * V_NYQ / 128           # within half a bin


def test_aliasing_shows_as_aliasing():
    """a speed of 1.5 v_nyq peaks where -0.5 v_nyq does: bin 64 - 32"""
    hi, _ = sm.spectrum(_gate_series(np.full(512, 1.5 * V_NYQ, f32), np.ones(4, f32)), sm.window(1, 128), V_NYQ)
    lo, _ = sm.spectrum(_gate_series(np.full(512, -0.5 * V_NYQ, f32), np.ones(4, f32)), sm.window(1, 128), V_NYQ)
    assert (hi[0].argmax(axis=1) == 32).all() and (lo[0].argmax(axis=1) == 32).all()


def test_a_gate_across_a_parabolic_lumen_fills_the_spectrum():
    """a 32-row gate across a parabolic lumen at 200 mm/s: the power lies between 0 and 200 mm/s, two bins allowed on either side.  The
    share measured on the mirror when the test was written is in the comment below; 0.99 is required"""
    line = np.ones(32, np.uint8)
    frac = sm.profile(line, 0, 32, [0, 1], 2.0)
    assert frac.max() < 1.0 and frac[0] == f32(1.0 - (15.5 / 16.0) ** 2)
    for seed in (1, 2, 3):
        power, _ = sm.spectrum(_gate_series(np.full(2048, 200.0, f32), frac, seed=seed), sm.window(1, 128), V_NYQ, wall=sm.WALL_NONE, wall_bins=0)
        top = int(round(64 + 200.0 / V_NYQ * 64))
        p = power[0].astype(np.float64)
        share = p[:, 64 - 2:top + 3].sum() / p.sum()
        spread = (p.sum(axis=0) > 1e-3 * p.sum(axis=0).max()).sum()
        print("seed %d: share of the power between 0 and 200 mm/s %.6f, bins above -30 dB %d" % (seed, share, spread))
        assert share >= 0.99                                          # measured 0.999955, 0.999971, 0.999996
        assert spread >= 20                                           # ... and it FILLS that range (38 bins wide): measured 36, 35, 36


def test_the_mean_trace_follows_a_pulsatile_waveform():
    """under a sinusoidal waveform the mean velocity of a small gate on the axis follows the truth -- the true centre-line velocity
    averaged over each window -- to within two bin widths (2 x 5.2 mm/s); the worst error measured on the mirror is in the comment"""
    T, N, hop = 4096, 128, 32
    speed = (150.0 + 100.0 * np.sin(2 * np.pi * np.arange(T) / 1024.0)).astype(f32)
    z = _gate_series(speed, np.ones(2, f32), seed=5)
    _, mean = sm.spectrum(z, sm.window(1, N), V_NYQ, N=N, hop=hop, wall=sm.WALL_NONE, wall_bins=0)
    truth = np.array([speed[c * hop:c * hop + N].astype(np.float64).mean() for c in range(mean.shape[1])])
    err = np.abs(mean[0] - truth).max()
    print("pulsatile waveform: worst error of the mean trace %.3f mm/s (a bin is %.3f mm/s)" % (err, 2 * V_NYQ / N))
    assert err <= 2 * (2 * V_NYQ / N)                                 # measured 1.9 mm/s
    assert mean[0].max() - mean[0].min() > 180.0                      # it follows: the waveform swings by 200 mm/s


def test_the_wall_filter_and_the_wall_bins_remove_clutter():
    """clutter 40 dB above the blood: without a wall filter the brightest bin is the clutter's at zero velocity; with MEAN and wall_bins
    it is the blood's"""
    clutter = _speckle(8, 9, scale=100.0)
    z = _gate_series(np.full(1024, 100.0, f32), np.ones(8, f32), seed=3, clutter=clutter)
    none, _ = sm.spectrum(z, sm.window(1, 128), V_NYQ, wall=sm.WALL_NONE, wall_bins=0)
    both, mean = sm.spectrum(z, sm.window(1, 128), V_NYQ, wall=sm.WALL_MEAN, wall_bins=2)
    assert (none[0].argmax(axis=1) == 64).all() and (both[0].argmax(axis=1) == 83).all()
    assert not bits(both[0][:, 63:66]).any() and np.abs(mean[0] - 100.0).max() < 2 * V_NYQ / 128


def test_the_rotor_tables_spurs():
    """tones through the 4096-entry table at phase steps that are no multiple of a table entry (k * 2^18: a quarter of an entry per pulse and
    its multiples), each on a bin's centre of a Hann window of 16384 pulses, so that what lies outside the main lobe is the table's own:
    the largest spur is below -65 dB (measured -68.3 dB; the same tones through 1024 entries read -60.0 dB)"""
    lut = sm.rotor().astype(np.float64)
    L_, worst = 16384, -400.0
    for k in (1, 2, 3, 5, 6, 7, 333, 1001, 4099, 8191, 12345):
        idx = sm.rotor_index([t * (k << 18) for t in range(L_)], 65536)
        z = (lut[idx, 0] + 1j * lut[idx, 1]) * (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(L_) / L_))
        P = np.abs(np.fft.fft(z)) ** 2
        at = int(P.argmax())
        assert at == k
        outside = np.ones(L_, bool); outside[np.arange(at - 2, at + 3) % L_] = False
        worst = max(worst, 10 * math.log10(P[outside].max() / P[at]))
    print("rotor table: worst spur %.1f dB" % worst)
    assert worst < -65.0


def test_mirror_identities():
    """what holds tests/test_gpu_spectral.py honest: a series that stands still has no power under mean removal; the pairwise sum of N
    equal floats is N times the float; the sonogram's row 0 is the highest velocity"""
    z = np.tile(np.array([[1234.567, -0.001]], f32), (1, 300, 1))
    for N in sm.FFT_SIZES:
        if N <= 256:
            power, mean = sm.spectrum(z, sm.window(1, N), V_NYQ, N=N, hop=N // 4, wall=sm.WALL_MEAN, wall_bins=0)
            assert not bits(power).any() and not bits(mean).any()
        assert sm.pair_sum(np.full(N, f32(0.1)), 0) == f32(0.1) * f32(N)
    p = np.full((1, 3, 32), f32(1e-9)); p[0, :, 31] = 1.0
    grey, peak = sm.sonogram(p)
    assert grey.shape == (1, 32, 3) and (grey[0, 0] == 255).all() and not grey[0, 1:].any() and peak[0] == 1.0


# ------------------------------------------------------------------ the kernels' resources
def test_spectral_kernels_use_no_scratch():
    """the compiler's own report for mcrt_spectral.hip: k_gate_series, the five k_spectrum<N>, k_sonogram_peak and k_sonogram without spills
    or scratch; the LDS of k_spectrum<N> is its wavefront's 8 N bytes, k_sonogram's its byte tile, the others' none"""
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "mcray-tracing_amd"), "resources", "KERNELS=mcrt_spectral"], capture_output=True, text=True).stderr
    blocks = {b.split()[0]: b for b in out.split("Function Name: ")[1:]}
    lds = {"_ZN4mcrt13k_gate_seriesENS_14GateSeriesArgsE": 0, "_ZN4mcrt15k_sonogram_peakENS_12SonogramArgsE": 0, "_ZN4mcrt10k_sonogramENS_12SonogramArgsE": 16 * 17}
    lds.update({"_ZN4mcrt10k_spectrumILj%dEEEvNS_12SpectrumArgsE" % N: 8 * N for N in sm.FFT_SIZES})
    assert set(lds) <= set(blocks), sorted(blocks)
    for name, want in lds.items():
        b = blocks[name]
        val = lambda key: int(re.search(key + r": (\d+)", b).group(1))
        assert val("VGPRs Spill") == 0 and val("SGPRs Spill") == 0 and val(r"ScratchSize \[bytes/lane\]") == 0, b[:900]
        assert val(r"LDS Size \[bytes/block\]") == want and val("VGPRs") <= 64, b[:900]
