"""Focal zones on the MI355X: mcrt_convolve_frames_depth (k_conv_axial + k_conv_lateral_rows) against the numpy mirror
(tests/focus_mirror.py) bit for bit on synthetic device images, the constant table against mcrt_convolve_frames, passes against single
calls, table uploads between back-to-back calls, argument errors, the Simulator, point targets, the C++ shim and the CLI."""
import ctypes as C
import json
import os
import subprocess
import numpy as np
import pytest

import focus_mirror as fm
import image_cases as ic

pytestmark = pytest.mark.gpu

f32 = np.float32
INVALID, LIMIT = -1, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx(mcrt):
    c = mcrt.Context(0)
    yield c
    c.close()


class Dev:
    """device buffers of one test, freed at the end"""
    def __init__(self, ctx):
        self.ctx, self.bufs = ctx, []

    def __call__(self, nbytes):
        p = self.ctx.alloc(nbytes)
        self.bufs.append(p)
        return p

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self(arr.nbytes)
        self.ctx.h2d(p, arr)
        return p

    def close(self):
        for p in self.bufs:
            self.ctx.free(p)


@pytest.fixture
def dev(ctx):
    d = Dev(ctx)
    yield d
    d.close()


def table(R, n_lat, seed=0):
    """random per-row taps [R][n_lat] with both signs, zeros and -0.0"""
    rng = np.random.default_rng(700 + 31 * R + n_lat + seed)
    t = rng.standard_normal((R, n_lat)).astype(f32)
    t[rng.random((R, n_lat)) < 0.1] = 0.0
    t[rng.random((R, n_lat)) < 0.02] = -0.0
    return t


@pytest.mark.parametrize("n_lat", ic.CONV_LAT)
@pytest.mark.parametrize("n_ax", ic.CONV_AX)
def test_random_tables_match_the_mirror(ctx, dev, n_ax, n_lat):
    """every pixel compared: inside the window the mirror's sums, outside it the input's own bits (NaN / inf taps of the image included)"""
    ax, _ = ic.conv_taps(n_ax, n_lat)
    for E, R in ic.conv_shapes(n_ax, n_lat) + ic.SCAN_SHAPES + [(37, 1001), (130, 2047)]:
        img = ic.conv_image(E, R)
        lat = table(R, n_lat)
        p = dev.upload(img)
        ctx.convolve_frames_depth(p, 1, E, R, ax, lat)
        ic.assert_same_bits(ctx.d2h(p, (E, R)), fm.convolve_depth(img, ax, lat), "depth %dx%d taps %d/%d" % (E, R, n_ax, n_lat))


def test_a_nan_spreads_as_the_mirror_says(ctx, dev):
    E, R, n_ax, n_lat = 40, 120, 7, 13
    ax, _ = ic.conv_taps(n_ax, n_lat, seed=5)
    img = np.zeros((E, R), f32)
    img[20, 60] = np.nan
    img[5, 30] = np.inf
    lat = table(R, n_lat, seed=5)
    lat[40:80, 3] = 0.0                                  # 0 * NaN is NaN too
    p = dev.upload(img)
    ctx.convolve_frames_depth(p, 1, E, R, ax, lat)
    got = ctx.d2h(p, (E, R))
    want = fm.convolve_depth(img, ax, lat)
    ic.assert_same_bits(got, want, "nan")
    assert 20 < np.isnan(want).sum() < E * R // 4       # the NaN reached a patch of the image, not all of it


@pytest.mark.parametrize("n_ax,n_lat", [(1, 1), (7, 13), (16, 32)])
def test_a_constant_table_is_convolve_frames(ctx, dev, n_ax, n_lat):
    F, E, R = 3, 129, 465
    ax, lat = ic.conv_taps(n_ax, n_lat, seed=2)
    frames = np.stack([ic.conv_image(E, R, seed=f) for f in range(F)])
    a, b = dev.upload(frames), dev.upload(frames)
    ctx.convolve_frames(a, F, E, R, ax, lat)
    ctx.convolve_frames_depth(b, F, E, R, ax, np.tile(lat, (R, 1)))
    assert np.array_equal(ctx.d2h(a, (F, E, R)).view(np.uint32), ctx.d2h(b, (F, E, R)).view(np.uint32))


@pytest.mark.parametrize("E,R", [(129, 465), (3, 2048), (512, 465)])
def test_frames_equal_the_per_image_calls(ctx, dev, E, R):
    F, n_ax, n_lat = 4, 7, 13
    ax, _ = ic.conv_taps(n_ax, n_lat, seed=3)
    lat = table(R, n_lat, seed=3)
    frames = np.stack([ic.conv_image(E, R, seed=10 + f) for f in range(F)])
    p = dev.upload(frames)
    ctx.convolve_frames_depth(p, F, E, R, ax, lat)
    got = ctx.d2h(p, (F, E, R))
    one = dev(frames[0].nbytes)
    for f in range(F):
        ctx.h2d(one, frames[f])
        ctx.convolve_frames_depth(one, 1, E, R, ax, lat)
        assert np.array_equal(got[f].view(np.uint32), ctx.d2h(one, (E, R)).view(np.uint32)), f
        ic.assert_same_bits(got[f], fm.convolve_depth(frames[f], ax, lat), "frame %d" % f)


def test_back_to_back_calls_each_get_their_own_table(ctx, dev):
    """no synchronisation between the calls, and the caller's table array rewritten as soon as each call returns"""
    E, R, n_ax, n_lat = 96, 465, 7, 13
    ax, _ = ic.conv_taps(n_ax, n_lat, seed=4)
    tabs = [table(R, n_lat, seed=s) for s in (11, 12, 11, 13)] + [table(2048, 5, seed=14)]
    shapes = [(E, R)] * 4 + [(E, 2048)]
    imgs = [ic.conv_image(e, r, seed=20 + i) for i, (e, r) in enumerate(shapes)]
    ps = [dev.upload(im) for im in imgs]
    ctx.synchronize()
    buf = np.empty((R, n_lat), f32)
    for i, (p, t, (e, r)) in enumerate(zip(ps, tabs, shapes)):
        if t.shape == buf.shape:
            buf[:] = t
            ctx.convolve_frames_depth(p, 1, e, r, ax, buf)
            buf[:] = np.nan                                # the call has returned: the table is the caller's again
        else:
            ctx.convolve_frames_depth(p, 1, e, r, ax[:3], t)
    ctx.synchronize()
    for i, (p, t, im, (e, r)) in enumerate(zip(ps, tabs, imgs, shapes)):
        want = fm.convolve_depth(im, ax if t.shape[0] == R else ax[:3], t)
        ic.assert_same_bits(ctx.d2h(p, (e, r)), want, "call %d" % i)


def test_errors_leave_the_image_untouched(mcrt, ctx, dev):
    E, R = 40, 60
    img = ic.conv_image(E, R)
    p = dev.upload(img)
    big = ic.conv_image(3, 2049)
    q = dev.upload(big)
    ax, _ = ic.conv_taps(7, 13)
    lat = table(R, 13)
    L = ctx.L
    cases = [(lambda: ctx.convolve_frames_depth(p, 1, E, R, ic.conv_taps(17, 13)[0], lat), LIMIT),
             (lambda: ctx.convolve_frames_depth(p, 1, E, R, ax, table(R, 33)), LIMIT),
             (lambda: ctx.convolve_frames_depth(q, 1, 3, 2049, ax, table(2049, 13)), LIMIT)]
    for call, code in cases:
        with pytest.raises(mcrt.McrtError) as e:
            call()
        assert e.value.code == code
    axp, latp = ax.ctypes.data_as(C.c_void_p), lat.ctypes.data_as(C.c_void_p)
    pv = C.c_void_p(p)
    assert L.mcrt_convolve_frames_depth(ctx.h, pv, 1, E, R, axp, 7, None, 13) == INVALID
    assert L.mcrt_convolve_frames_depth(ctx.h, pv, 1, E, R, None, 7, latp, 13) == INVALID
    assert L.mcrt_convolve_frames_depth(ctx.h, None, 1, E, R, axp, 7, latp, 13) == INVALID
    assert L.mcrt_convolve_frames_depth(ctx.h, pv, 0, E, R, axp, 7, latp, 13) == INVALID
    assert L.mcrt_convolve_frames_depth(ctx.h, pv, 1, 0, R, axp, 7, latp, 13) == INVALID
    assert L.mcrt_convolve_frames_depth(ctx.h, pv, 1, E, R, axp, 0, latp, 13) == LIMIT
    assert L.mcrt_convolve_frames_depth(ctx.h, pv, 1, E, R, axp, 7, latp, 0) == LIMIT
    assert L.mcrt_convolve_frames_depth(None, pv, 1, E, R, axp, 7, latp, 13) == INVALID
    with pytest.raises(ValueError):
        ctx.convolve_frames_depth(p, 1, E, R, ax, table(R + 1, 13))
    ctx.synchronize()
    assert np.array_equal(ctx.d2h(p, (E, R)).view(np.uint32), img.view(np.uint32))
    assert np.array_equal(ctx.d2h(q, (3, 2049)).view(np.uint32), big.view(np.uint32))


def test_simulator(mcrt, orc, sphere, tex256):
    """Psf(focus_mm=None) gives today's frame (the oracle's convolution of the traced image); with a focus the frame is the mirror's
    convolution of the same traced image with the psf's table"""
    cfg, sd = sphere
    tr = mcrt.Transducer(48, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    plain = mcrt.Simulator(sd, tr, n_samples=16, texture=tex256, psf=mcrt.Psf(freq=tr.frequency, focus_mm=None))
    try:
        raw = plain.frame(0, convolve=False)
        got = plain.frame(0)
        assert plain.row_mm == 0.322 and not plain.psf.has_focus
        ic.assert_same_bits(got, orc.convolve(raw, plain.psf.axial_kernel, plain.psf.lateral_kernel), "no focus")
    finally:
        plain.close()
    psf = mcrt.Psf(freq=tr.frequency, focus_mm=(30.0, 60.0))
    sim = mcrt.Simulator(sd, tr, n_samples=16, texture=tex256, psf=psf)
    try:
        raw2 = sim.frame(0, convolve=False)
        assert np.array_equal(raw2.view(np.uint32), raw.view(np.uint32))
        lat = psf.lateral_rows(sim.R, sim.row_mm)
        focused = sim.frame(0)
        ic.assert_same_bits(focused, fm.convolve_depth(raw.T, psf.axial_kernel, lat).T, "focus")
        assert not np.array_equal(focused.view(np.uint32), got.view(np.uint32))
        img = sim.bmode(0, dynamic_range_db=50.0)
        assert img.shape == (400, 500) and img.max() > 200
    finally:
        sim.close()


def test_point_targets(mcrt, ctx, dev):
    """an impulse column: after the depth form each row's lateral profile is that row's taps.  Its width is smallest at the focal row,
    never shrinks over the next three focal ranges, and levels out once the beam is wider than the n_lat taps; no row's tap sum exceeds
    the focal row's (the gain keeps the area, the cut-off can only lose some)"""
    E, R, n_lat, c0 = 64, 465, 13, 40
    lat = mcrt.host_psf_focus(0.2, 145, R, 0.322, (40.0,), 20.0, n_lat)
    img = np.zeros((E, R), f32)
    img[c0] = 1.0
    p = dev.upload(img)
    ctx.convolve_frames_depth(p, 1, E, R, np.ones(1, f32), lat)
    out = ctx.d2h(p, (E, R)).astype(np.float64)
    rows = np.arange(1, R - 1)
    prof = out[c0 - n_lat + 1:c0 + 1, 1:R - 1][::-1]              # [k][row]: column c0 - k holds tap k
    assert np.array_equal(prof.T.astype(f32), lat[1:R - 1])
    x = np.arange(n_lat, dtype=np.float64)[:, None]
    s = prof.sum(0)
    mu = (prof * x).sum(0) / s
    w = np.sqrt((prof * x * x).sum(0) / s - mu * mu)
    focal = int(round(40.0 / 0.322))                             # row 124, z = 39.93 mm
    assert rows[np.argmin(w)] == focal
    i0 = focal - 1
    span = w[i0:i0 + int(3 * 20.0 / 0.322) + 1]
    assert (np.diff(span) >= 0).all()
    assert w.max() <= np.sqrt((n_lat * n_lat - 1) / 12.0)          # at most a flat window's width
    assert (w[-1] - w[-51]) < 0.1 * (w[i0 + 50] - w[i0])
    assert (s <= s[i0] * (1 + 1e-6)).all()


def _build_driver(tmp_path):
    pkg = os.path.join(ROOT, "mcray-tracing_amd")
    exe = str(tmp_path / "focus_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(pkg, "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "focus_driver.cpp"), "-L", pkg, "-lmcrt_hip", "-Wl,-rpath," + pkg])
    return exe


@pytest.mark.parametrize("foci,focal_range", [((40.0,), 20.0), ((20.0, 50.0, 90.0), 12.5), ((), 20.0)])
def test_host_shim(mcrt, ctx, dev, tmp_path, foci, focal_range):
    exe = _build_driver(tmp_path)
    out = tmp_path / "focus.bin"
    r = subprocess.run([exe, str(out), str(focal_range)] + [str(f) for f in foci], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    E, R = 64, 465
    both = np.fromfile(str(out), f32).reshape(2, R, E)
    before, after = both[0], both[1]
    assert np.count_nonzero(before) > 1000
    psf = mcrt.Psf(focus_mm=foci, focal_range_mm=focal_range)
    p = dev.upload(np.ascontiguousarray(before.T))
    if foci:
        lat = psf.lateral_rows(R, 322 / 1000.0)
        ctx.convolve_frames_depth(p, 1, E, R, psf.axial_kernel, lat)
        ic.assert_same_bits(after.T, fm.convolve_depth(before.T, psf.axial_kernel, lat), "shim vs mirror")
    else:
        ctx.convolve(p, E, R, psf.axial_kernel, psf.lateral_kernel)
    ic.assert_same_bits(after.T, ctx.d2h(p, (E, R)), "shim vs python")


def test_cli_focus_options(mcrt, tmp_path):
    exe = os.path.join(ROOT, "mcray-tracing_amd", "mattausch_hip")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "mcray-tracing_amd"), "mattausch_hip"])
    cfg, meshes = mcrt.synth.sphere_scene(3)
    cfg["workingDirectory"] = str(tmp_path) + "/"
    for f, (V, F) in meshes.items():
        mcrt.scene_io.save_obj(str(tmp_path / f), V, F)
    (tmp_path / "sphere.scene").write_text(json.dumps(cfg))
    scene = str(tmp_path / "sphere.scene")

    def run(name, *opts):
        r = subprocess.run([exe, scene, "2", "5", str(tmp_path / (name + ".pgm")), str(tmp_path / (name + ".bin"))] + list(opts),
                           capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout + r.stderr
        return (tmp_path / (name + ".pgm")).read_bytes(), (tmp_path / (name + ".bin")).read_bytes()

    plain = run("plain")
    assert run("range_only", "--focal-range-mm", "7") == plain           # without foci the range changes nothing
    focused = run("focus", "--focus-mm", "40,80")
    assert len(focused[0]) == len(plain[0]) and focused[0] != plain[0] and focused[1] != plain[1]
    assert run("focus_db", "--db", "60", "--focus-mm", "40", "--focal-range-mm", "15")[0] != run("db", "--db", "60")[0]
    r = subprocess.run([exe, scene, "1", "5", "--focus-mm", "80,40"], capture_output=True, text=True, timeout=240)
    assert r.returncode == 1 and "ascending" in r.stdout
