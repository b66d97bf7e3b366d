"""Shear-wave elastography without a GPU (include/mcrt.h: mcrt_shear_opts, mcrt_default_shear_opts, mcrt_shear_table, mcrt_shear_pitch,
mcrt_shear_shape, mcrt_shear_decay, mcrt_shear_draws, mcrt_shear_map): the host helpers against tests/shear_mirror.py bit for bit, the
struct and its defaults, every refusal that needs no device, the pitch against mcrt_scan_maps' geometry, and the properties of the model
on the float32 mirror: what the time-to-peak estimator recovers of a uniform medium and of a fast inclusion under noise, a fluid, and the
zero-push identity.

THE MEASURED ACCURACY of the float32 mirror (one medium of 64 scan-lines x 96 rows, 300 um pitch, 10 kHz, 64 pulses, a = 8, b = 4, rows
averaged over +- 2, a raised cosine of 12 pulses, a peak of 0.1 row, the push on line 32; the median relative error of the speed against
truth_speed over the samples of quality >= 0.9): uniform 2 m/s without noise 0.068 %; an inclusion of 4 m/s over 16 lines in 2 m/s with
noise 28 dB below the speckle: 2.9 % outside, 6.8 % inside (median speed inside 3.78 m/s), 0.7 % of the inside samples below quality 0.9.
The tests assert twice these figures.
(The four model tests read tests/shear_mirror.py alone: they hold the model to its properties whatever the library does, and the model
is tied to the device by tests/test_gpu_shear.py, bit for bit.  Every other test here calls the library's new symbols.)"""
import ctypes as C
import numpy as np
import pytest

import shear_mirror as sh

f32 = np.float32
INVALID, LIMIT = -1, -5
CARRIER = 0.3475
p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)


# ------------------------------------------------------------------ the struct and its defaults
def test_struct_and_defaults(mcrt):
    L = mcrt.load_library()
    o = mcrt.ShearOpts()
    names = ("n_pulses", "window_rows", "prf_hz", "sigma", "seed", "push_line", "push_row0", "push_rows", "peak_q24", "speed_lines", "avg_rows", "density")
    assert C.sizeof(o) == 48 and [getattr(mcrt.ShearOpts, n).offset for n in names] == list(range(0, 48, 4))
    assert L.mcrt_default_shear_opts(C.byref(o)) == 0
    assert tuple(getattr(o, n) for n in names) == (64, 8, 10000.0, 0.0, 0x53484552, 0, 0, 0, 1677722, 4, 2, 1.0)
    assert {n: getattr(o, n) for n in names} == sh.DEFAULTS
    assert L.mcrt_default_shear_opts(None) == INVALID
    o = mcrt.shear_opts_struct(n_pulses=256, window_rows=0, prf_hz=5000.0, sigma=0.5, seed=9, push_line=3, push_row0=4, push_rows=5, peak_q24=-8388608,
                               speed_lines=16, avg_rows=0, density=1.5)
    assert tuple(getattr(o, n) for n in names) == (256, 0, 5000.0, 0.5, 9, 3, 4, 5, -8388608, 16, 0, 1.5)


# ------------------------------------------------------------------ the tables
def test_table_equals_the_mirrors(mcrt):
    speeds = [2.0, 0.0, 1.5, 3.0, 0.7, 12.0, 1e-3]
    for prf in (10000.0, 5000.0, 12345.678):
        slow, spf = mcrt.host_shear_table(speeds, prf)
        ms, mf = sh.shear_table(speeds, prf)
        assert slow.dtype == np.int64 and spf.dtype == f32 and np.array_equal(slow, ms) and np.array_equal(spf.view(np.uint32), mf.view(np.uint32)), prf
    slow, spf = mcrt.host_shear_table([2.0, 0.0], 10000.0)
    assert list(slow) == [21474836, 0] and list(spf) == [2.0, 0.0]           # 2^32 * 1e4 / 2e6 ticks per um in Q16; a fluid


def test_table_refuses(mcrt):
    L = mcrt.load_library()
    c = np.array([2.0, 1.5], np.float64)
    slow = np.full(2, -7, np.int64); spf = np.full(2, -7.0, f32)
    call = lambda s=c, n=2, prf=10000.0, a=slow, b=spf: L.mcrt_shear_table(p(s), n, prf, p(a), p(b))
    assert call(s=None) == INVALID and call(a=None) == INVALID and call(b=None) == INVALID and call(n=0) == INVALID
    assert L.mcrt_shear_table(p(np.ones(255)), 255, 1e4, p(np.zeros(255, np.int64)), p(np.zeros(255, f32))) == LIMIT
    for bad in (np.nan, np.inf, -np.inf, 0.0, -1.0):
        assert call(prf=bad) == INVALID
    for bad in (np.nan, np.inf, -1.0, 1e-9, 1e12):                       # (1e-9 m/s: above 2^38; 1e12 m/s: rounds to 0)
        assert call(s=np.array([2.0, bad])) == INVALID, bad
    assert (slow == -7).all() and (spf == -7.0).all()
    assert call() == 0 and (slow != -7).all()


@pytest.mark.parametrize("E,R,radius,angle", [(128, 465, 30.0, 1.0471975511965976), (1, 1, 0.25, 0.5), (192, 2048, 60.0, 1.2), (64, 100, 10.0, 0.3)])
def test_pitch_equals_the_mirrors(mcrt, E, R, radius, angle):
    q8, mm = mcrt.host_shear_pitch(E, R, radius, angle)
    mq, mf = sh.shear_pitch(E, R, radius, angle)
    assert q8.dtype == np.uint32 and np.array_equal(q8, mq) and np.array_equal(mm.view(np.uint32), mf.view(np.uint32))
    q8, mm = mcrt.host_shear_pitch(E, R, radius, angle, 80, 1540)
    mq, mf = sh.shear_pitch(E, R, radius, angle, 80, 1540)
    assert np.array_equal(q8, mq) and np.array_equal(mm.view(np.uint32), mf.view(np.uint32))


def test_pitch_follows_the_scan_maps(mcrt):
    """THE CONVENTION: neighbouring scan-lines are total_angle / E apart and row r lies r depth / R below the arc, as mcrt_scan_maps has them.
    On the picture's centre column one pixel sideways is `ratio` mm and moves the column coordinate by atan(1 / fi) / total_angle * E
    scan-lines: their quotient is the pitch at the depth that pixel's row coordinate names (the arc against its chord: below 1e-4)"""
    E, R, radius, angle, orows, ocols = 128, 465, 30.0, 1.0471975511965976, 400, 500
    map_row, map_col = mcrt.host_scan_maps(E, R, radius, angle, out_rows=orows, out_cols=ocols)
    _, mm = mcrt.host_shear_pitch(E, R, radius, angle)
    depth = 150.0
    ratio = ((depth + radius) - radius * np.cos(angle / 2.0)) / orows
    j = ocols // 2                                                       # fj = 0 here, 1 one pixel to the right
    checked = 0
    for i in range(20, orows - 20, 37):
        row = float(map_row[i, j])
        if not (0.0 <= row <= R - 1):
            continue
        lines = float(map_col[i, j + 1]) - float(map_col[i, j])
        want = ratio / lines
        got = float(np.interp(row, np.arange(R), mm.astype(np.float64)))
        assert abs(got - want) <= 2e-3 * want, (i, row, got, want)
        checked += 1
    assert checked >= 5
    assert abs(float(mm[0]) - radius * angle / E) < 1e-6 and abs(float(mm[R - 1]) - (radius + (R - 1) * depth / R) * angle / E) < 1e-6


def test_pitch_refuses(mcrt):
    L = mcrt.load_library()
    q8 = np.full(8, 7, np.uint32); mm = np.full(8, -7.0, f32)
    call = lambda E=4, R=8, radius=30.0, angle=1.0, us=100, sos=1500, a=q8, b=mm: L.mcrt_shear_pitch(E, R, radius, angle, us, sos, p(a), p(b))
    assert call(a=None, b=None) == INVALID and call(E=0) == INVALID and call(R=0) == INVALID and call(us=0) == INVALID and call(sos=0) == INVALID
    for bad in (np.nan, np.inf, -1.0):
        assert call(radius=bad) == INVALID
    for bad in (np.nan, np.inf, 0.0, -1.0):
        assert call(angle=bad) == INVALID
    big = np.zeros(2049, np.uint32)
    assert L.mcrt_shear_pitch(4, 2049, 30.0, 1.0, 100, 1500, p(big), None) == LIMIT
    assert call(radius=0.0, R=1) == LIMIT                                # a pitch of 0 at the arc's centre
    assert call(radius=1e5) == LIMIT                                     # 25 m between neighbours
    assert (q8 == 7).all() and (mm == -7.0).all()
    assert call(b=None) == 0 and (q8 != 7).all() and (mm == -7.0).all()
    assert call(a=None) == 0 and (mm != -7.0).all()


def test_shape_and_decay_equal_the_mirrors(mcrt):
    for w in (1, 12, 256):
        s = mcrt.host_shear_shape(w)
        assert s.dtype == np.uint32 and s.shape == (64 * w,) and np.array_equal(s, sh.shear_shape(w)) and s.max() <= 65536
        assert np.array_equal(s, s[::-1])                                # symmetric about its middle
    for n, d0 in ((1, 8.0), (129, 8.0), (1000, 0.5), (64, 1e9)):
        a = mcrt.host_shear_decay(n, d0)
        assert a.dtype == np.uint32 and np.array_equal(a, sh.shear_decay(n, d0)) and a[0] == 65536 and (np.diff(a.astype(np.int64)) <= 0).all()
    L = mcrt.load_library()
    buf = np.full(64, 7, np.uint32)
    assert L.mcrt_shear_shape(1, None) == INVALID and L.mcrt_shear_shape(0, p(buf)) == INVALID and L.mcrt_shear_shape(257, p(buf)) == LIMIT
    assert L.mcrt_shear_decay(4, 8.0, None) == INVALID and L.mcrt_shear_decay(0, 8.0, p(buf)) == INVALID
    for bad in (0.0, -1.0, np.nan, np.inf):
        assert L.mcrt_shear_decay(4, bad, p(buf)) == INVALID
    assert (buf == 7).all()


# ------------------------------------------------------------------ the draws
@pytest.mark.parametrize("E,R", [(1, 1), (3, 65), (2, 2048)])
def test_draws_equal_the_mirrors(mcrt, E, R):
    for seed, image, pulse in ((0x53484552, 0, 0), (7, 0xFFFFFFFF, 255), (7, 1, 3)):
        got = mcrt.host_shear_draws(seed, image, E, R, pulse)
        assert got.shape == (E, R, 2) and np.array_equal(got, sh.draws(seed, image, E, R, pulse))


def test_draws_are_a_stream_of_their_own(mcrt):
    """counter word 2 differs from the tracer's, the noise stage's, flow's, spectral's and strain's: the same key gives other draws"""
    import flow_mirror as fm
    import strain_mirror as sm
    d = mcrt.host_shear_draws(5, 3, 4, 33, 0)
    assert not np.array_equal(d, mcrt.host_strain_draws(5, 3, 4, 33))
    assert not np.array_equal(d, fm.draws(5, 3, 4, 33, 2)[0])
    assert not np.array_equal(d[0, 0], mcrt.host_spectral_draws(5, 3, 0, 0, 1)[0])
    assert not np.array_equal(d, mcrt.host_shear_draws(5, 3, 4, 33, 1))   # and every pulse has its own
    assert sh.COUNTER not in (0x4E4F4953, 0x464C4F57, 0x53504543, sm.COUNTER) and sh.COUNTER >= 16


def test_draws_refuse(mcrt):
    L = mcrt.load_library()
    d = np.full((2, 3, 2), -7, np.int32)
    assert L.mcrt_shear_draws(1, 2, 2, 3, 0, None) == INVALID and L.mcrt_shear_draws(1, 2, 0, 3, 0, p(d)) == INVALID and L.mcrt_shear_draws(1, 2, 2, 0, 0, p(d)) == INVALID
    assert L.mcrt_shear_draws(1, 2, 1, 2049, 0, p(d)) == LIMIT and L.mcrt_shear_draws(1, 2, 2, 3, 256, p(d)) == LIMIT
    assert (d == -7).all()


# ------------------------------------------------------------------ the colour table
def test_map(mcrt):
    lut = mcrt.host_shear_map()
    assert lut.dtype == np.uint8 and np.array_equal(lut, sh.shear_map())
    assert tuple(lut[0]) == (0, 0, 255) and tuple(lut[128]) == (0, 255, 0) and tuple(lut[255]) == (254, 1, 0)      # soft blue, green at the reference, stiff red
    assert np.array_equal(lut, mcrt.host_strain_map())                  # mcrt_strain_map stays as it is: the same bytes, read the other way
    L = mcrt.load_library()
    buf = np.full((256, 3), 9, np.uint8)
    assert L.mcrt_shear_map(0, None) == INVALID and L.mcrt_shear_map(1, p(buf)) == INVALID and (buf == 9).all()


# ------------------------------------------------------------------ the model, on the mirror
E_, R_, T_, PUSH = 64, 96, 64, 32


def speckle(F, E, R, seed=0):
    """finite speckle-like pairs: a carrier at CARRIER cycles per row under a smooth random envelope"""
    rng = np.random.default_rng(seed)
    b = rng.standard_normal((F, E, R + 6, 2))
    b = sum(b[:, :, i:i + R] for i in range(7)) / 7.0
    ph = 2.0 * np.pi * CARRIER * np.arange(R)
    z = (b[..., 0] + 1j * b[..., 1]) * np.exp(1j * ph)
    return np.stack([z.real, z.imag], axis=-1).astype(f32)


def model(speeds, tissue, sigma=0.0, **opts):
    """the whole chain on the mirror at 300 um pitch and 10 kHz -> (iq, wave's outputs, speed's outputs)"""
    iq = speckle(1, E_, R_)
    slow, spf = sh.shear_table(speeds, 10000.0)
    o = dict(dict(n_pulses=T_, window_rows=8, push_line=PUSH), **opts)
    w = sh.wave(iq, tissue, slow, spf, np.full(R_, 300 * 256, np.uint32), sh.shear_shape(12), sh.shear_decay(E_, 8.0), CARRIER, sigma=sigma, **o)
    s = sh.speed(w["peak_time"], np.full(R_, 0.3, f32), push_line=PUSH, speed_lines=4, avg_rows=2)
    return iq, w, s


def window_inside():
    e = np.arange(E_)
    return np.broadcast_to(((e - 4 >= 0) & (e + 4 < E_) & ~((e - 4 <= PUSH) & (PUSH <= e + 4)))[None, :, None], (1, E_, R_))


def median_error(s, w, where):
    err = np.abs(s["speed"][where] - w["truth_speed"][where]) / w["truth_speed"][where]
    return float(np.median(err))


def test_uniform_medium_reads_its_speed():
    """2 m/s, no noise: the median relative error over the samples of quality >= 0.9.  Measured 0.068 %; asserted at twice that, below 2 %"""
    iq, w, s = model([2.0], np.zeros((1, E_, R_), np.uint8))
    good = s["quality"] >= f32(0.9)
    assert good.sum() > 0.9 * window_inside().sum() and not (good & ~window_inside()).any()
    err = median_error(s, w, good)
    print("uniform medium: median relative error %.5f %% over %d samples" % (100 * err, good.sum()))
    assert err <= 2 * 0.00068 <= 0.02
    assert np.isnan(s["speed"][~window_inside()]).all() and not s["quality"][~window_inside()].any()       # the window is not clipped
    A = w["arrival"][0, :, 0]
    assert A[PUSH] == 0 and (np.diff(A[PUSH:]) > 0).all() and (np.diff(A[:PUSH + 1]) < 0).all()            # the wave leaves in both directions
    assert np.array_equal(A[PUSH + 1:PUSH + 20], A[PUSH - 19:PUSH][::-1])


def test_inclusion_at_twice_the_speed():
    """4 m/s over 16 lines in 2 m/s, noise 28 dB below the speckle.  Measured: 2.9 % outside, 6.8 % inside, 0.7 % of the inside lost"""
    tissue = np.zeros((1, E_, R_), np.uint8); tissue[:, 40:56] = 1
    rms = float(np.sqrt(np.mean(speckle(1, E_, R_).astype(np.float64) ** 2)))
    iq, w, s = model([2.0, 4.0], tissue, sigma=rms * 10.0 ** (-28.0 / 20.0))
    good = s["quality"] >= f32(0.9)
    inside = (tissue == 1) & window_inside(); outside = (tissue == 0) & window_inside()
    e_out, e_in = median_error(s, w, outside & good), median_error(s, w, inside & good)
    lost = 1.0 - (inside & good).sum() / inside.sum()
    med = float(np.median(s["speed"][inside & good]))
    print("inclusion: median relative error %.3f %% outside, %.3f %% inside; median speed inside %.3f m/s; %.2f %% of the inside below quality 0.9" % (
        100 * e_out, 100 * e_in, med, 100 * lost))
    assert e_out <= 2 * 0.0293 and e_in <= 2 * 0.0676
    assert abs(med - 4.0) < abs(med - 2.0) and lost <= 0.1


def test_fluid_stops_the_wave():
    """a fluid label: the truth arrival is +inf behind it, the quality 0 there, and no speed is shown"""
    tissue = np.zeros((1, E_, R_), np.uint8); tissue[:, 44:47, 20:60] = 1
    iq, w, s = model([2.0, 0.0], tissue)
    behind = np.zeros((1, E_, R_), bool); behind[:, 45:, 20:60] = True
    assert np.isposinf(w["truth_arrival"][behind]).all() and np.isfinite(w["truth_arrival"][~behind]).all()
    assert np.isfinite(w["truth_arrival"][0, 44, 20:60]).all()           # the wave reaches the fluid's first line and does not leave it
    assert (w["truth_speed"][tissue == 1] == 0).all()
    # every line of the fit, every row of its average and every row of their correlation windows (8 + 2 rows) behind the fluid
    deep = np.zeros((1, E_, R_), bool); deep[:, 45 + 4:E_ - 4, 30:50] = True
    assert not s["quality"][deep].any() and np.isnan(s["speed"][deep]).all() and np.isnan(s["modulus"][deep]).all()
    shown = s["quality"][0, 5:PUSH - 5] >= f32(0.9)
    assert shown.mean() > 0.9                                            # the other side is untouched


def test_no_push_is_the_identity():
    """peak_q24 = 0 and sigma 0: every frame of the movie is +0.0f wherever pre is finite and not zero; pulse n's line equals pre"""
    tissue = np.random.default_rng(0).choice(np.array([0, 1, 2, 255], np.uint8), size=(1, E_, R_))
    iq, w, s = model([2.0, 0.0], tissue, peak_q24=0, n_pulses=5)
    assert w["disp"].shape == (1, 5, E_, R_) and not w["disp"].view(np.uint32).any()
    assert np.isnan(w["peak_time"]).all() and not w["peak_disp"].view(np.uint32).any()        # the first maximum is pulse 0
    A = sh.arrival(tissue, sh.shear_table([2.0, 0.0])[0], np.full(R_, 76800, np.uint32), PUSH)
    z = sh.warp(iq, sh.displacement(A, 3, sh.shear_shape(12), sh.shear_decay(E_), 0, PUSH, 0, R_), CARRIER, sh.rotor())
    assert np.array_equal(z.view(np.uint32), iq.view(np.uint32))
