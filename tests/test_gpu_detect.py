"""Quadrature detection on the MI355X: mcrt_detect_frames (k_detect) against the numpy mirror (tests/detect_mirror.py) bit for bit at the
shapes around its lane chunks and its LDS line, in every buffer mode, on special values; the argument errors; the Simulator with and
without detect=; Simulator.iq(); the C++ shim and the CLI; and a tone of constant amplitude under both detectors."""
import ctypes as C
import json
import os
import subprocess
import numpy as np
import pytest

import detect_mirror as dm
import elevation_mirror as em
import image_cases as ic

pytestmark = pytest.mark.gpu

f32 = np.float32
INVALID, LIMIT = -1, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = f32(-77.25)
PI = 3.141592653589793

SHAPES = [(1, 1), (1, 2), (3, 63), (2, 64), (5, 65), (2, 465), (1, 2047), (2, 2048)]


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
        p = self.ctx.alloc(max(nbytes, 4))
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


def run_detect(ctx, dev, frames, n_taps, mode):
    """the call on frames [F][E][R] in one buffer mode -> (env or None, iq or None, the input as the device holds it afterwards).  The outputs
    start as a sentinel.  mode: "inplace" (env_dev == rf_dev), "out", "iq", "both", "inplace+iq" """
    F, E, R = frames.shape
    p = dev.upload(frames)
    env_dev = p if mode.startswith("inplace") else dev.upload(np.full((F, E, R), SENTINEL)) if mode in ("out", "both") else None
    iq_dev = dev.upload(np.full((F, E, R, 2), SENTINEL)) if mode in ("iq", "both", "inplace+iq") else None
    ctx.detect_frames(p, F, E, R, env_dev=env_dev, iq_dev=iq_dev, n_taps=n_taps)
    env = ctx.d2h(env_dev, (F, E, R)) if env_dev is not None else None
    iq = ctx.d2h(iq_dev, (F, E, R, 2)) if iq_dev is not None else None
    return env, iq, ctx.d2h(p, (F, E, R))


def stack_of(F, E, R, seed=0):
    return np.stack([ic.envelope_image(E, R, seed=seed + 3 * f) for f in range(F)])


@pytest.mark.parametrize("n_taps", [3, 7, 31, 63])
@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("E,R", SHAPES)
def test_shapes_match_the_mirror(ctx, dev, E, R, F, n_taps):
    """out of place with both outputs, and in place: every family of image_cases' scan-lines (noise, ramps, saws, specials) at every shape"""
    frames = stack_of(F, E, R, seed=n_taps)
    want_env, want_iq = dm.detect(frames, n_taps)
    env, iq, after = run_detect(ctx, dev, frames, n_taps, "both")
    what = "E=%d R=%d F=%d taps=%d" % (E, R, F, n_taps)
    ic.assert_same_bits(env, want_env, "env " + what)
    ic.assert_same_bits(iq, want_iq, "iq " + what)
    ic.assert_same_bits(after, frames, "rf_dev " + what)
    env, _, _ = run_detect(ctx, dev, frames, n_taps, "inplace")
    ic.assert_same_bits(env, want_env, "in place " + what)


@pytest.mark.parametrize("mode", ["inplace", "out", "iq", "both", "inplace+iq"])
@pytest.mark.parametrize("F,E,R", [(2, 5, 65), (1, 7, 465)])
def test_buffer_modes(ctx, dev, F, E, R, mode):
    frames = stack_of(F, E, R, seed=11)
    want_env, want_iq = dm.detect(frames, 31)
    env, iq, after = run_detect(ctx, dev, frames, 31, mode)
    if env is not None:
        ic.assert_same_bits(env, want_env, "env " + mode)
    if iq is not None:
        ic.assert_same_bits(iq, want_iq, "iq " + mode)
    if not mode.startswith("inplace"):
        ic.assert_same_bits(after, frames, "rf_dev is read only (" + mode + ")")


def test_the_default_is_31_taps(ctx, dev):
    frames = stack_of(1, 3, 129, seed=5)
    p = dev.upload(frames)
    ctx.detect_frames(p, 1, 3, 129, env_dev=p)
    ic.assert_same_bits(ctx.d2h(p, (1, 3, 129)), dm.detect(frames, 31)[0], "n_taps=None")


@pytest.mark.parametrize("n_taps", [3, 15, 63])
def test_special_values(ctx, dev, n_taps):
    R, r0 = 200, 77
    rng = np.random.default_rng(n_taps)
    img = rng.standard_normal((6, R)).astype(f32)
    img[0, r0] = np.nan                       # one NaN
    img[2, :] = np.nan                        # a NaN scan-line between two clean ones
    img[3, 5] = np.inf; img[3, 100] = -np.inf; img[3, 150] = np.inf; img[3, 152] = np.inf          # (rows 150 and 152: inf - inf at row 151)
    img[4, :] = -0.0
    img[5, 0] = np.nan; img[5, R - 1] = np.inf                              # at the ends
    env, iq, _ = run_detect(ctx, dev, img[None], n_taps, "both")
    want_env, want_iq = dm.detect(img[None], n_taps)
    ic.assert_same_bits(env, want_env, "env")
    ic.assert_same_bits(iq, want_iq, "iq")
    env, iq = env[0], iq[0]
    reach = dm.reached(r0, R, n_taps)
    assert sorted(np.flatnonzero(np.isnan(env[0]))) == reach
    assert sorted(np.flatnonzero(np.isnan(iq[0, :, 1]))) == [r for r in reach if r != r0]
    assert np.isnan(env[2]).all() and np.isnan(iq[2]).all()
    assert np.isfinite(env[1]).all() and np.isfinite(iq[1]).all()           # its neighbour lines are left alone
    assert sorted(np.flatnonzero(~np.isfinite(env[3]))) == sorted(set().union(*(dm.reached(r, R, n_taps) for r in (5, 100, 150, 152))))
    assert env[3, 5] == np.inf and env[3, 100] == np.inf and np.isnan(env[3, 151]) and np.isnan(iq[3, 151, 1])
    assert not env[4].view(np.uint32).any() and not iq[4, :, 1].view(np.uint32).any() and (iq[4, :, 0].view(np.uint32) == 0x80000000).all()
    assert sorted(np.flatnonzero(~np.isfinite(env[5]))) == sorted(set(dm.reached(0, R, n_taps)) | set(dm.reached(R - 1, R, n_taps)))


def test_errors_leave_the_outputs_untouched(mcrt, ctx, dev):
    L = mcrt.load_library()
    F, E, R = 2, 3, 40
    n = F * E * R
    frames = stack_of(F, E, R)
    opts = mcrt.detect_opts_struct()

    TOTAL = 8192                                                            # floats: rf, then room for env and iq (and for a line of 2049 rows)

    def call(rows=R, frames_=F, lines=E, o=opts, env=n, iq=2 * n, rf=0, null_ctx=False):
        """env, iq, rf: where the buffer starts, in floats from the start of one allocation (None: a null pointer)"""
        big = dev.upload(np.concatenate([frames.reshape(-1), np.full(TOTAL - n, SENTINEL)]))
        at = lambda floats: None if floats is None else C.c_void_p(big + 4 * floats)
        rc = L.mcrt_detect_frames(None if null_ctx else ctx.h, at(rf), frames_, lines, rows, None if o is None else C.byref(o), at(env), at(iq))
        got = ctx.d2h(big, (TOTAL,))
        assert np.array_equal(got[:n].view(np.uint32), frames.reshape(-1).view(np.uint32)) and (got[n:] == SENTINEL).all()
        return rc

    assert call(rows=2049, frames_=1, lines=1) == LIMIT
    assert call(env=None, iq=None) == INVALID
    assert call(iq=n - 2) == INVALID                                        # iq_dev overlaps the end of rf_dev
    assert call(iq=0, env=None) == INVALID
    assert call(env=1) == INVALID                                           # env_dev one float into rf_dev
    assert call(env=2 * n - 1) == INVALID                                   # env_dev overlaps iq_dev
    assert call(null_ctx=True) == INVALID and call(rf=None) == INVALID and call(o=None) == INVALID
    assert call(rows=0) == INVALID and call(frames_=0) == INVALID and call(lines=0) == INVALID
    for bad in (0, 1, 5, 9, 33, 65, 67):
        o = mcrt.DetectOpts(); o.n_taps = bad
        assert call(o=o) == INVALID, bad
    assert call(frames_=1 << 20, lines=1 << 20, rows=1) == LIMIT            # 2^40 floats
    with pytest.raises(mcrt.McrtError):
        ctx.detect_frames(dev(4 * n), F, E, R)                              # neither output


# ------------------------------------------------------------------ the Simulator
@pytest.fixture(scope="module")
def small(mcrt):
    cfg, meshes = mcrt.synth.sphere_scene(3)
    sd = mcrt.scene_io.build_scene(cfg, meshes)
    tr = mcrt.Transducer(48, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    return sd, tr, mcrt.host_texture(32)


def make_sim(mcrt, small, **kw):
    sd, tr, tex = small
    return mcrt.Simulator(sd, tr, n_samples=8, texture=tex, tex_n=32, **kw)


def test_detector_not_selected(mcrt, small):
    """detect=None is the Simulator without the keyword: the same calls, the same bits"""
    pics = []
    for kw in ({}, dict(detect=None)):
        sim = make_sim(mcrt, small, **kw)
        try:
            assert sim.detect is None
            pics.append((sim.bmode(1, out_rows=100, out_cols=120), sim.frame(1)))
            sim._run(1)
            pics[-1] += (sim.ctx.d2h(sim.rf_dev, (sim.E, sim.R)),)
        finally:
            sim.close()
    for a, b in zip(*pics):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert pics[0][0].max() > 0
    for bad in ("hilbert", dict(taps=31)):
        with pytest.raises((ValueError, TypeError)):
            make_sim(mcrt, small, detect=bad)
    with pytest.raises(mcrt.McrtError):
        make_sim(mcrt, small, detect=dict(n_taps=9))


@pytest.mark.parametrize("case", ["plain", "taps15", "bands", "noise", "compound"])
def test_simulator_chain(mcrt, small, case):
    """Simulator(detect="quadrature")'s enveloped stack is trace -> convolve (-> add_noise) -> Context.detect_frames by hand (-> the band fold)"""
    fid = 2
    kw = dict(bands=dict(psf=mcrt.Psf(freq=small[1].frequency, bands=(4.5, 5.5))), noise=dict(noise=40), compound=dict(compound=(-0.1, 0.1))).get(case, {})
    n_taps = 15 if case == "taps15" else 31
    detect = dict(n_taps=15) if case == "taps15" else "quadrature"
    hand = make_sim(mcrt, small, **kw)
    try:
        E, R, (stack, n) = hand.E, hand.R, hand._stack
        hand.trace(fid)
        hand.convolve()
        if hand.noise is not None:
            hand.add_noise(fid)
        if case == "bands":
            B = 2
            imgs = hand.ctx.d2h(hand._band_buf.dev, (n * B, E, R))
            hand.ctx.detect_frames(hand._band_buf.dev, n * B, E, R, env_dev=hand._band_buf.dev, n_taps=n_taps)
            hand.ctx.band_fold_frames(hand._band_buf.dev, n, B, E, R, hand.psf.band_weights(R, hand.row_mm), stack)
            mirror = em.fold(dm.detect(imgs, n_taps)[0].reshape(n, B, E, R), hand.psf.band_weights(R, hand.row_mm))
        else:
            imgs = hand.ctx.d2h(stack, (n, E, R))
            hand.ctx.detect_frames(stack, n, E, R, env_dev=stack, n_taps=n_taps)
            mirror = dm.detect(imgs, n_taps)[0]
        want = hand.ctx.d2h(stack, (n, E, R))
        assert np.count_nonzero(imgs) > 100
        hand._run(fid)                                                      # (the reference's envelope: another picture)
        other = hand.ctx.d2h(stack, (n, E, R))
    finally:
        hand.close()
    assert n == (2 if case == "compound" else 1)
    ic.assert_same_bits(want, mirror, case + ": by hand vs the mirror")
    sim = make_sim(mcrt, small, detect=detect, **kw)
    try:
        sim._run(fid)
        got = sim.ctx.d2h(sim._stack[0], (n, E, R))
        assert not sim._held
        if case == "compound":
            pic = sim.compound_image(fid, out_rows=60, out_cols=80)
            assert pic.shape == (60, 80) and np.isfinite(pic).all() and pic.max() > 0
        else:
            assert sim.bmode(fid, out_rows=60, out_cols=80).max() > 0
    finally:
        sim.close()
    ic.assert_same_bits(got, want, case + ": the Simulator vs by hand")
    assert not np.array_equal(got.view(np.uint32), other.view(np.uint32))


def test_iq(mcrt, small):
    """iq() has frame()'s own bits as its real part; its magnitude, in the mirror's rounding, is the detected frame -- with and without detect="""
    for kw, n_taps in ((dict(detect="quadrature"), 31), ({}, 31), (dict(detect=dict(n_taps=7)), 7)):
        sim = make_sim(mcrt, small, **kw)
        try:
            rf = sim.frame(3)
            z = sim.iq(3)
            assert z.dtype == np.complex64 and z.shape == rf.shape == (sim.R, sim.E) and z.flags["C_CONTIGUOUS"]
            ic.assert_same_bits(z.real, rf, "the real part")
            ic.assert_same_bits(z.imag.T, dm.quadrature(rf.T, n_taps), "the imaginary part")
            assert np.count_nonzero(z.imag) > 100
            raw = sim.iq(3, convolve=False)
            ic.assert_same_bits(raw.real, sim.frame(3, convolve=False), "convolve=False")
            if sim.detect is not None:
                sim._run(3)
                ic.assert_same_bits(dm.magnitude(z.real, z.imag), sim.ctx.d2h(sim.rf_dev, (sim.E, sim.R)).T, "|iq| is the detected frame")
        finally:
            sim.close()
    for kw in (dict(compound=(-0.1, 0.1)), dict(sweep=(3, 0.02)), dict(psf=mcrt.Psf(freq=small[1].frequency, bands=(4.5, 5.5)))):
        sim = make_sim(mcrt, small, **kw)
        try:
            with pytest.raises(RuntimeError):
                sim.iq(0)
        finally:
            sim.close()


# ------------------------------------------------------------------ the C++ shim and the CLI
def _build_driver(tmp_path):
    pkg = os.path.join(ROOT, "mcray-tracing_amd")
    exe = str(tmp_path / "detect_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(pkg, "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "detect_driver.cpp"), "-L", pkg, "-lmcrt_hip", "-Wl,-rpath," + pkg])
    return exe


def test_host_shim(mcrt, ctx, dev, tmp_path):
    """the shim driver's images -- before, rf_image::iq after convolve, convolve + detect, and with bands -- against the Python path"""
    exe = _build_driver(tmp_path)
    E, R, bands, n_taps = 64, 465, (3.5, 5.0), 15
    out = tmp_path / "detect.bin"
    r = subprocess.run([exe, str(out), str(n_taps)] + [str(f) for f in bands], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    blob = np.fromfile(str(out), f32)
    assert blob.size == 5 * E * R
    before = np.ascontiguousarray(blob[:E * R].reshape(R, E).T)
    pair = blob[E * R:3 * E * R].reshape(E, R, 2)
    detected, banded = blob[3 * E * R:4 * E * R].reshape(R, E), blob[4 * E * R:].reshape(R, E)
    assert np.count_nonzero(before) > 1000
    psf = mcrt.Psf()
    p, q = dev.upload(before), dev(E * R * 8)
    ctx.convolve(p, E, R, psf.axial_kernel, psf.lateral_kernel)
    ctx.detect_frames(p, 1, E, R, iq_dev=q, n_taps=n_taps)
    ic.assert_same_bits(pair, ctx.d2h(q, (E, R, 2)), "rf_image::iq")
    ctx.detect_frames(p, 1, E, R, env_dev=p, n_taps=n_taps)
    ic.assert_same_bits(detected.T, ctx.d2h(p, (E, R)), "rf_image::detect")
    ic.assert_same_bits(detected.T, dm.magnitude(pair[..., 0], pair[..., 1]), "|iq| is the detected image")
    B = len(bands)
    bpsf = mcrt.Psf(bands=dict(band_mhz=bands, weights=tuple(range(1, B + 1)), var_x=0.05))
    ax, w = bpsf.axial_rows(R, 0.322), bpsf.band_weights(R, 0.322)
    ctx.h2d(p, before)
    s, o = dev(B * E * R * 4), dev(E * R * 4)
    ctx.convolve_bands_frames(p, 1, E, R, ax, s, lateral=bpsf.lateral_kernel)
    ctx.detect_frames(s, B, E, R, env_dev=s, n_taps=n_taps)
    ctx.band_fold_frames(s, 1, B, E, R, w, o)
    ic.assert_same_bits(banded.T, ctx.d2h(o, (E, R)), "rf_image::detect over the band images")
    assert not np.array_equal(detected, banded)


def test_cli_options(mcrt, tmp_path):
    exe = os.path.join(ROOT, "mcray-tracing_amd", "mattausch_hip")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "mcray-tracing_amd"), "mattausch_hip"])
    cfg, meshes = mcrt.synth.sphere_scene(3)
    cfg["workingDirectory"] = str(tmp_path) + "/"
    for f, (V, F) in meshes.items():
        mcrt.scene_io.save_obj(str(tmp_path / f), V, F)
    (tmp_path / "sphere.scene").write_text(json.dumps(cfg))
    scene = str(tmp_path / "sphere.scene")
    E, R = 512, 465

    def run(name, *opts):
        r = subprocess.run([exe, scene, "2", "5", str(tmp_path / (name + ".pgm")), str(tmp_path / (name + ".bin"))] + list(opts),
                           capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout + r.stderr
        return (tmp_path / (name + ".pgm")).read_bytes(), np.fromfile(str(tmp_path / (name + ".bin")), f32).reshape(R, E)

    plain = run("plain")
    quad = run("quad", "--detect", "quadrature", "--iq", str(tmp_path / "quad.raw"))
    pair = np.fromfile(str(tmp_path / "quad.raw"), f32)
    assert pair.size == E * R * 2
    pair = pair.reshape(E, R, 2)
    assert len(quad[0]) == len(plain[0]) and quad[0] != plain[0]
    ic.assert_same_bits(quad[1].T, dm.magnitude(pair[..., 0], pair[..., 1]), "rf.bin is |iq|")
    ic.assert_same_bits(pair[..., 1], dm.quadrature(pair[..., 0], 31), "the odd floats are the Hilbert transform of the even ones")
    only = run("only", "--iq", str(tmp_path / "only.raw"))                 # --iq alone leaves the run as it is, and writes the same pair
    assert only[0] == plain[0] and np.array_equal(only[1].view(np.uint32), plain[1].view(np.uint32))
    assert (tmp_path / "only.raw").read_bytes() == (tmp_path / "quad.raw").read_bytes()
    assert np.count_nonzero(pair[..., 0]) > 1000
    seven = run("seven", "--detect", "quadrature", "--detect-taps", "7")
    assert not np.array_equal(seven[1], quad[1])
    for bad, word in ((["--detect", "hilbert"], "quadrature"), (["--detect-taps", "31"], "--detect"), (["--detect", "quadrature", "--detect-taps", "9"], "3, 7, 11"),
                      (["--iq", str(tmp_path / "x.raw"), "--compound", "3"], "--iq"), (["--iq", str(tmp_path / "x.raw"), "--freq-compound", "3"], "--iq")):
        r = subprocess.run([exe, scene, "1", "5"] + bad, capture_output=True, text=True, timeout=240)
        assert r.returncode == 1 and word in r.stdout, (bad, r.stdout)


# ------------------------------------------------------------------ the point of the feature
def test_a_tone_of_constant_amplitude(mcrt, ctx, dev):
    """cos(2 pi 0.3475 r + 0.3), R = 465, as 4 identical scan-lines: the device's quadrature envelope over the rows [M, R - M) stays within
    |G - 1| + 1e-5 of 1; mcrt_envelope_frames on a copy deviates by more than 0.25 over the rows [20, R - 20)"""
    R, n_taps = 465, 31
    M = (n_taps - 1) // 2
    x = np.tile(np.cos(2.0 * PI * 0.3475 * np.arange(R) + 0.3).astype(f32), (4, 1))
    G = mcrt.host_detect_gain(mcrt.host_detect_taps(n_taps), 0.3475)
    p, q = dev.upload(x), dev.upload(x)
    ctx.detect_frames(p, 1, 4, R, env_dev=p, n_taps=n_taps)
    ctx.envelope_frames(q, 1, 4, R)
    env, ref = ctx.d2h(p, (4, R)).astype(np.float64), ctx.d2h(q, (4, R)).astype(np.float64)
    dev_q, dev_r = np.abs(env[:, M:R - M] - 1.0).max(), np.abs(ref[:, 20:R - 20] - 1.0).max()
    print("tone 0.3475 on the device: quadrature %.6f (|G - 1| = %.6f), mcrt_envelope_frames %.4f" % (dev_q, abs(G - 1.0), dev_r))
    assert dev_q <= abs(G - 1.0) + 1e-5
    assert dev_r > 0.25
