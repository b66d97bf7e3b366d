"""Colour Doppler without a GPU (include/mcrt.h: mcrt_flow_opts, mcrt_default_flow_opts, mcrt_flow_nyquist, mcrt_flow_phasors, mcrt_flow_draws,
mcrt_colour_map, mcrt_colour_opts, mcrt_default_colour_opts): the host helpers against tests/flow_mirror.py bit for bit, the structs and
their defaults, every refusal that needs no device, the mirror's atan2 against double arctan2, the draws' exact moments, what the Kasai
estimator recovers on the mirror with and without the wall filter, aliasing, and the kernels' resources."""
import ctypes as C
import math
import os
import re
import subprocess
import numpy as np
import pytest

import flow_mirror as fm

f32 = np.float32
INVALID, LIMIT = -1, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONES = 0xFFFFFFFF


# ------------------------------------------------------------------ structs and defaults
def test_structs_and_defaults(mcrt):
    o = mcrt.FlowOpts()
    assert C.sizeof(o) == 32
    assert [getattr(mcrt.FlowOpts, n).offset for n in ("n_packets", "wall", "avg_rows", "avg_lines", "prf_hz", "freq_mhz", "sigma", "seed")] == list(range(0, 32, 4))
    L = mcrt.load_library()
    assert L.mcrt_default_flow_opts(C.byref(o)) == 0
    assert (o.n_packets, o.wall, o.avg_rows, o.avg_lines, o.prf_hz, o.freq_mhz, o.sigma, o.seed) == (8, 1, 2, 1, 4000.0, 0.0, 0.0, 0x464C4F57)
    assert L.mcrt_default_flow_opts(None) == INVALID
    c = mcrt.ColourOpts()
    assert C.sizeof(c) == 12 and [getattr(mcrt.ColourOpts, n).offset for n in ("power_thr", "vel_thr_mm_s", "grey_max")] == [0, 4, 8]
    assert L.mcrt_default_colour_opts(C.byref(c)) == 0 and (c.power_thr, c.vel_thr_mm_s, c.grey_max) == (0.0, 0.0, 255)
    assert L.mcrt_default_colour_opts(None) == INVALID
    assert mcrt.FLOW_WALLS == {"none": 0, "mean": 1, "linear": 2}
    o = mcrt.flow_opts_struct(n_packets=16, wall="linear", avg_rows=0, avg_lines=4, prf_hz=2500, freq_mhz=3.5, sigma=0.25, seed=7)
    assert (o.n_packets, o.wall, o.avg_rows, o.avg_lines, o.prf_hz, o.freq_mhz, o.sigma, o.seed) == (16, 2, 0, 4, 2500.0, 3.5, 0.25, 7)
    with pytest.raises(ValueError):
        mcrt.flow_opts_struct(wall="median")
    assert mcrt.load_library().mcrt_version() == 109


# ------------------------------------------------------------------ the Nyquist velocity
def test_nyquist(mcrt):
    assert abs(mcrt.host_flow_nyquist(4.5, 1500.0) - 333.3333333333333) < 1e-9
    for prf, f, sos in ((4000.0, 4.5, 1500.0), (2500.0, 3.5, 1540.0), (12000.0, 7.25, 1480.0)):
        assert mcrt.host_flow_nyquist(f, sos, prf_hz=prf) == fm.nyquist(prf, f, sos)
        assert mcrt.host_flow_nyquist(99.0, sos, opts=mcrt.flow_opts_struct(prf_hz=prf, freq_mhz=f)) ==fm.nyquist(prf, float(f32(f)), sos)      # the options' own frequency wins
    L = mcrt.load_library()
    v = C.c_double(-1.0)
    o = mcrt.flow_opts_struct()
    bad = [mcrt.flow_opts_struct(n_packets=1), mcrt.flow_opts_struct(n_packets=17), mcrt.flow_opts_struct(wall=3), mcrt.flow_opts_struct(avg_rows=9),
           mcrt.flow_opts_struct(avg_lines=5), mcrt.flow_opts_struct(prf_hz=0.0), mcrt.flow_opts_struct(prf_hz=np.inf), mcrt.flow_opts_struct(sigma=-1.0),
           mcrt.flow_opts_struct(sigma=np.nan), mcrt.flow_opts_struct(freq_mhz=np.nan)]
    for b in bad:
        assert L.mcrt_flow_nyquist(C.byref(b), 4.5, 1500.0, C.byref(v)) == INVALID
    assert L.mcrt_flow_nyquist(None, 4.5, 1500.0, C.byref(v)) == INVALID and L.mcrt_flow_nyquist(C.byref(o), 4.5, 1500.0, None) == INVALID
    for f, sos in ((0.0, 1500.0), (-1.0, 1500.0), (np.nan, 1500.0), (4.5, 0.0), (4.5, np.inf)):
        assert L.mcrt_flow_nyquist(C.byref(o), f, sos, C.byref(v)) == INVALID
    assert v.value == -1.0


# ------------------------------------------------------------------ phasors
def _dirs(E, seed=0):
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((E, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)


@pytest.mark.parametrize("L_,E", [(1, 1), (3, 7), (254, 5), (4, 512)])
def test_phasors_equal_the_mirrors(mcrt, L_, E):
    rng = np.random.default_rng(L_ * 1000 + E)
    vel = (rng.standard_normal((L_, 3)) * 300.0).astype(f32)
    vel[0] = 0.0                                                 # at rest
    if L_ > 2:
        vel[2] = (1.0, 0.0, 0.0)
    dirs = _dirs(E, E)
    dirs[0] = (0.0, 0.0, 1.0)                                    # perpendicular to vel[2]: v_t is +0.0, not -0.0
    ph, tr = mcrt.host_flow_phasors(333.3333333333333, vel, dirs)
    want_ph, want_tr = fm.phasors(333.3333333333333, vel, dirs)
    assert np.array_equal(ph.view(np.uint32), want_ph.view(np.uint32)) and np.array_equal(tr.view(np.uint32), want_tr.view(np.uint32))
    assert (ph[0] == (1.0, 0.0)).all() and not tr[0].view(np.uint32).any() and not ph[0, :, 1].view(np.uint32).any()
    if L_ > 2:
        assert tr[2, 0].view(np.uint32) == 0 and tuple(ph[2, 0].view(np.uint32)) == (0x3f800000, 0)
    # truth is the velocity towards the probe: a material that moves against the beam direction reads positive
    ph, tr = mcrt.host_flow_phasors(300.0, [[0.0, 0.0, -150.0]], [[0.0, 0.0, 1.0]])
    assert tr[0, 0] == 150.0 and abs(float(ph[0, 0, 0])) < 1e-7 and ph[0, 0, 1] == 1.0               # a quarter turn


def test_phasors_refuse(mcrt):
    L = mcrt.load_library()
    vel = np.ones((2, 3), f32); dirs = _dirs(4)
    ph = np.full((2, 4, 2), -7.0, f32); tr = np.full((2, 4), -7.0, f32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    call = lambda v=vel, d=dirs, n=2, e=4, nyq=300.0, ph_=ph, tr_=tr: L.mcrt_flow_phasors(nyq, None if v is None else p(v), None if d is None else p(d), n, e,
                                                                                        None if ph_ is None else p(ph_), None if tr_ is None else p(tr_))
    assert call(v=None) == INVALID and call(d=None) == INVALID and call(ph_=None) == INVALID and call(tr_=None) == INVALID
    assert call(n=0) == INVALID and call(e=0) == INVALID and call(n=255) == LIMIT
    for nyq in (0.0, -1.0, np.nan, np.inf):
        assert call(nyq=nyq) == INVALID
    for bad in (np.nan, np.inf, -np.inf):
        v = vel.copy(); v[1, 2] = bad
        assert call(v=v) == INVALID
        d = dirs.copy(); d[3, 0] = bad
        assert call(d=d) == INVALID
    assert (ph == -7.0).all() and (tr == -7.0).all()
    assert call() == 0 and (ph != -7.0).all()


# ------------------------------------------------------------------ the draws
def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32_10"""
    zero = [int(x) for x in fm.philox4x32_10(0, 0, 0, 0, 0, 0)]
    ones = [int(x) for x in fm.philox4x32_10(ONES, ONES, ONES, ONES, ONES, ONES)]
    assert zero == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert ones == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]


@pytest.mark.parametrize("E,R,N", [(1, 1, 2), (3, 5, 3), (7, 257, 8), (2, 2048, 16)])
def test_host_draws_equal_the_mirrors(mcrt, E, R, N):
    for seed, image_id in ((0x464C4F57, 0), (0x5EED, 1), (3, ONES)):
        d = mcrt.host_flow_draws(seed, image_id, E, R, N)
        assert d.dtype == np.int32 and d.shape == (N, E, R, 2)
        assert np.array_equal(d, fm.draws(seed, image_id, E, R, N)), (seed, image_id)
        assert np.abs(d.astype(np.int64)).max() <= 131070


def test_draws_are_not_the_noise_stages(mcrt):
    """counter word 2 differs: the same seed, image, scan-line and row give other numbers than mcrt_noise_draws"""
    d = mcrt.host_flow_draws(5, 9, 4, 64, 2)
    n = mcrt.host_noise_draws(5, 9, 4, 64)
    assert not np.array_equal(d[0, ..., 0] + d[0, ..., 1], n)


def test_draw_moments(mcrt):
    """a sum of four uniform 16-bit words about its mean: mean 0 and variance 4 (65536^2 - 1) / 12 = 1431655765 EXACTLY; a sample of n
    draws is held to five standard errors -- of the mean, sqrt(var / n), and of the variance, var sqrt((kurtosis - 1) / n) with the
    Irwin-Hall excess kurtosis -6 / (5 * 4) = -0.3"""
    assert 4 * (65536 ** 2 - 1) // 12 == 1431655765 and 4 * (65536 ** 2 - 1) % 12 == 0
    assert fm.INV_STD == f32(1.0 / math.sqrt(1431655765.0))
    d = mcrt.host_flow_draws(0x464C4F57, 3, 64, 512, 16).astype(np.float64).reshape(-1)
    n, var = d.size, 1431655765.0
    assert abs(d.mean()) < 5.0 * math.sqrt(var / n)
    assert abs(d.var() - var) < 5.0 * var * math.sqrt((3.0 - 0.3 - 1.0) / n)
    i, q = mcrt.host_flow_draws(1, 2, 32, 256, 8)[..., 0].astype(np.float64), mcrt.host_flow_draws(1, 2, 32, 256, 8)[..., 1].astype(np.float64)
    assert abs((i * q).mean()) < 5.0 * var / math.sqrt(i.size)                 # I and Q are uncorrelated


def test_draws_refuse(mcrt):
    L = mcrt.load_library()
    d = np.full(2 * 4 * 2048 * 2 + 8, -12345, np.int32)
    p = d.ctypes.data_as(C.c_void_p)
    assert L.mcrt_flow_draws(1, 2, 4, 8, 2, None) == INVALID
    assert L.mcrt_flow_draws(1, 2, 0, 8, 2, p) == INVALID and L.mcrt_flow_draws(1, 2, 4, 0, 2, p) == INVALID
    assert L.mcrt_flow_draws(1, 2, 4, 8, 1, p) == INVALID and L.mcrt_flow_draws(1, 2, 4, 8, 17, p) == INVALID
    assert L.mcrt_flow_draws(1, 2, 4, 2049, 2, p) == LIMIT
    assert (d == -12345).all()
    assert L.mcrt_flow_draws(1, 2, 4, 2048, 2, p) == 0
    assert np.array_equal(d[:-8].reshape(2, 4, 2048, 2), fm.draws(1, 2, 4, 2048, 2)) and (d[-8:] == -12345).all()


# ------------------------------------------------------------------ the colour table
def test_colour_map(mcrt):
    lut = mcrt.host_colour_map()
    assert lut.dtype == np.uint8 and lut.shape == (256, 3) and np.array_equal(lut, fm.colour_map())
    assert tuple(lut[128]) == (0, 0, 0) and tuple(lut[0]) == tuple(lut[1])
    assert tuple(lut[129]) == (129, 0, 0) and tuple(lut[255]) == (255, 252, 0)            # red to yellow
    assert tuple(lut[127]) == (0, 0, 129) and tuple(lut[1]) == (0, 252, 255)              # blue to cyan
    towards, away = lut[129:].astype(int), lut[127:0:-1].astype(int)
    assert (np.diff(towards[:, 0]) == 1).all() and (np.diff(towards[:, 1]) >= 0).all() and not towards[:, 2].any()
    assert np.array_equal(away[:, ::-1], towards)                                          # the two ramps mirror each other
    L = mcrt.load_library()
    buf = np.full((256, 3), 9, np.uint8)
    assert L.mcrt_colour_map(1, buf.ctypes.data_as(C.c_void_p)) == INVALID and L.mcrt_colour_map(0, None) == INVALID and (buf == 9).all()


# ------------------------------------------------------------------ the mirror's atan2
def test_atan2_stays_within_its_bound():
    """against double arctan2 over a dense circle at several radii and on the axes: 1e-5 rad, five times the 1.96e-6 measured when the
    coefficients were chosen and 1 / 2000 of a level of the 8-bit colour scale (pi / 127)"""
    th = np.linspace(-math.pi, math.pi, 2_000_001)
    worst = 0.0
    for radius in (1.0, 1e-20, 3e18, 0.37):
        y = (np.sin(th) * radius).astype(f32); x = (np.cos(th) * radius).astype(f32)
        err = np.abs(fm.atan2f(y, x).astype(np.float64) - np.arctan2(y.astype(np.float64), x.astype(np.float64)))
        err = np.minimum(err, 2.0 * math.pi - err)                                   # (the cut at +-pi)
        worst = max(worst, float(err.max()))
    print("det_atan2f: largest error %.3e rad" % worst)
    assert worst < 1e-5
    a = lambda y, x: float(fm.atan2f(f32(y), f32(x)))
    assert a(0.0, 1.0) == 0.0 and a(0.0, 0.0) == 0.0 and a(-0.0, -0.0) == 0.0 and a(0.0, -0.0) == 0.0
    assert abs(a(1.0, 0.0) - math.pi / 2) < 1e-5 and abs(a(-1.0, 0.0) + math.pi / 2) < 1e-5 and abs(a(0.0, -1.0) - math.pi) < 1e-5
    assert abs(a(1.0, 1.0) - math.pi / 4) < 1e-5 and abs(a(-1.0, -1.0) + 3 * math.pi / 4) < 1e-5
    assert np.isnan(a(np.nan, 1.0)) and np.isnan(a(1.0, np.nan)) and np.isnan(a(np.inf, np.inf))
    assert a(1.0, np.inf) == 0.0 and abs(a(np.inf, 1.0) - math.pi / 2) < 1e-6


# ------------------------------------------------------------------ the estimator, on the mirror
def _estimate(step, wall, N=8, seed=1, clutter_db=20.0, snr_db=20.0, E=12, R=96):
    """the median phase step the mirror reads from blood of unit variance per component under clutter and noise"""
    rng = np.random.default_rng(seed)
    blood = rng.standard_normal((1, E, R, 2)).astype(f32)
    clutter = (rng.standard_normal((1, E, R, 2)) * 10.0 ** (clutter_db / 20.0)).astype(f32)
    tissue = np.ones((1, E, R), np.uint8)
    ph = np.zeros((2, E, 2), f32); ph[0] = (1.0, 0.0); ph[1] = (f32(math.cos(step)), f32(math.sin(step)))
    out = fm.flow(clutter, blood, tissue, ph, np.zeros((2, E), f32), math.pi, N=N, wall=wall, avg_rows=2, avg_lines=1,
                  sigma=10.0 ** (-snr_db / 20.0), seed=seed)
    return float(np.median(out["vel"])), out                  # v_nyq = pi: vel is the phase step itself


def test_wall_filter_is_what_removes_clutter():
    """N = 8, clutter 20 dB above blood, SNR 20 dB, a 15-sample window: with mean removal the true step of 1.0 rad is recovered; without
    it the clutter's zero phase wins"""
    for seed in (1, 2, 3):
        got, _ = _estimate(1.0, fm.WALL_MEAN, seed=seed)
        none, _ = _estimate(1.0, fm.WALL_NONE, seed=seed)
        print("seed %d: mean removal %.4f rad, no filter %.4f rad" % (seed, got, none))
        assert abs(got - 1.0) < 0.03           # a first run of the mirror read 0.9884, 0.9881 and 0.9885 (a bias of -0.012 from what the
                                               # filter takes of the blood itself); 0.03 is two and a half times that, and 1.2 colour levels
        assert abs(none) < 0.05


def test_aliasing():
    """a velocity of 1.5 v_nyq turns the phase by 1.5 pi per pulse, which reads as -0.5 pi: -0.5 v_nyq"""
    v_nyq = 333.3333333333333
    E, R = 4, 40
    ph, tr = fm.phasors(v_nyq, [[0.0, 0.0, 0.0], [0.0, 0.0, -1.5 * v_nyq]], np.tile(np.array([0.0, 0.0, 1.0], f32), (E, 1)))
    assert tr[1, 0] == f32(1.5 * v_nyq)
    rng = np.random.default_rng(4)
    blood = (rng.standard_normal((1, E, R, 2)) + 2.0).astype(f32)
    out = fm.flow(None, blood, np.ones((1, E, R), np.uint8), ph, tr, v_nyq, N=8, wall=fm.WALL_NONE, avg_rows=0, avg_lines=0)
    assert np.abs(out["vel"] + 0.5 * v_nyq).max() < 1e-3 * v_nyq
    assert (out["truth"] == f32(1.5 * v_nyq)).all()                               # the ground truth is not aliased


def test_mirror_identities():
    """what holds tests/test_gpu_flow.py honest: a stationary sample under mean removal at a power of two has r0 exactly 0; the split is a
    partition; a window larger than the image is the whole image"""
    rng = np.random.default_rng(0)
    iq = rng.standard_normal((1, 3, 20, 2)).astype(f32)
    tissue = np.zeros((1, 3, 20), np.uint8)
    ph = np.zeros((1, 3, 2), f32); ph[..., 0] = 1.0
    for N in (2, 4, 8, 16):
        out = fm.flow(None, iq, tissue, ph, np.zeros((1, 3), f32), 100.0, N=N, wall=fm.WALL_MEAN)
        assert not out["corr"].view(np.uint32).any() and not out["var"].any() and not out["vel"].any()
    rf = rng.standard_normal((2, 3, 20)).astype(f32); rf[0, 0, :4] = (np.nan, -0.0, np.inf, 1e-40)
    lab = rng.integers(0, 4, (2, 3, 20)).astype(np.uint8); lab[0, 0, 0] = 2; lab[1, 2, 5] = 255; lab[1, 2, 6] = 3
    parts = fm.split(rf, lab, [0, 1, 1])
    mv = (lab == 1) | (lab == 2)
    assert np.array_equal(parts[:, 1].view(np.uint32)[mv], rf.view(np.uint32)[mv]) and not parts[:, 1].view(np.uint32)[~mv].any()
    assert np.array_equal(parts[:, 0].view(np.uint32)[~mv], rf.view(np.uint32)[~mv]) and not parts[:, 0].view(np.uint32)[mv].any()
    x = rng.standard_normal((1, 3, 5)).astype(f32)
    whole = fm.average(x, 8, 4)
    assert np.allclose(whole, x.mean(), rtol=1e-5) and np.array_equal(fm.average(x, 0, 0), x)


# ------------------------------------------------------------------ the kernels' resources
def test_flow_kernels_use_no_scratch():
    """the compiler's own report for mcrt_flow.hip: every instantiation of k_flow<N, WALL> (15 x 3), k_flow_avg, k_flow_split and k_colour
    without spills or scratch and at full occupancy; no LDS anywhere"""
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "mcray-tracing_amd"), "resources", "KERNELS=mcrt_flow"], capture_output=True, text=True).stderr
    blocks = [b for b in out.split("Function Name: ")[1:]]
    names = [b.split()[0] for b in blocks]
    assert sum(n.startswith("_ZN4mcrt6k_flowILj") for n in names) == 45, names
    assert {"_ZN4mcrt10k_flow_avgENS_8FlowArgsE", "_ZN4mcrt12k_flow_splitENS_13FlowSplitArgsE", "_ZN4mcrt8k_colourENS_10ColourArgsE"} <= set(names), names
    for b in blocks:
        val = lambda key: int(re.search(key + r": (\d+)", b).group(1))
        assert val("VGPRs Spill") == 0 and val("SGPRs Spill") == 0 and val(r"ScratchSize \[bytes/lane\]") == 0, b[:900]
        assert val(r"LDS Size \[bytes/block\]") == 0 and val(r"Occupancy \[waves/SIMD\]") == 8 and val("VGPRs") <= 64, b[:900]
