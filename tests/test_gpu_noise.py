"""Receiver noise on the MI355X (mcrt_noise_frames: k_bmode_peak's peaks, k_noise) against the numpy mirror (tests/noise_mirror.py), bit for
bit: the ragged ends of a lane's 4 rows, of a wavefront's 256 and of a workgroup, one frame and several, one image per frame and several,
both modes, with and without a gain table; the ids; the identity cases; the gain table's cache; the argument errors; a traced scene through
the Simulator and mattausch_hip."""
import ctypes as C
import json
import os
import subprocess
import numpy as np
import pytest

import image_cases as ic
import noise_mirror as nm
from test_gpu_focus import Dev

pytestmark = pytest.mark.gpu

f32 = np.float32
INVALID, LIMIT = -1, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (1, 5), (3, 1), (2, 7), (5, 64), (64, 5), (7, 255), (7, 256), (7, 257), (33, 465), (3, 2048)]
STACKS = [(1, 1), (3, 1), (2, 3)]
MODES = [dict(snr_db=30.0), dict(sigma=0.25)]
FILL = f32(-777.25)             # 64 guard floats behind every stack: a write past the end shows
GUARD = 64


@pytest.fixture(scope="module")
def ctx(mcrt):
    c = mcrt.Context(0)
    yield c
    c.close()


@pytest.fixture
def dev(ctx):
    d = Dev(ctx)
    yield d
    d.close()


def stack(F, N, E, R, seed=0):
    """[F][N][E][R]: noise-free "echoes" with both signs, a flat zero patch, exact zeros, -0.0, NaN, +-inf and 1e-30; every second frame
    four times as loud, so that the frames of a call have peaks of their own"""
    rng = np.random.default_rng(4000 + 131 * E + R + 7 * F + N + seed)
    shape = (F, N, E, R)
    x = (rng.rayleigh(1.0, shape) * np.where(rng.random(shape) < 0.3, -1.0, 1.0) * (1.0 + 3.0 * (np.arange(F).reshape(F, 1, 1, 1) % 2))).astype(f32)
    x[:, :, E // 3:E // 3 + 4, R // 4:R // 4 + 5] = 0.0
    flat = x.reshape(F * N, -1)
    n = flat.shape[1]
    if n >= 6:
        vals = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-30], f32)
        for j in range(F * N):
            k = max(len(vals), n // 40)
            flat[j, rng.permutation(n)[:k]] = np.resize(vals, k)
    return x


def gains(E):
    return np.resize(np.array([0.0, 1.0, 0.5, -2.0], f32), E)


def run(ctx, dev, x, first_id=0, gain=None, want_sigma=True, **opts):
    """x through mcrt_noise_frames on the device -> (out, sigma or None); the guard floats behind the stack and behind sigma are checked"""
    F, N, E, R = x.shape
    p = dev.upload(np.concatenate([x.reshape(-1), np.full(GUARD, FILL)]))
    s = dev.upload(np.full(F + GUARD, FILL)) if want_sigma else None
    ctx.noise_frames(p, F, N, E, R, first_image_id=first_id, element_gain=gain, sigma_dev=s, **opts)
    ctx.synchronize()
    got = ctx.d2h(p, (x.size + GUARD,))
    assert (got[x.size:] == FILL).all(), "the guard behind the stack"
    sig = None
    if want_sigma:
        sig = ctx.d2h(s, (F + GUARD,))
        assert (sig[F:] == FILL).all(), "the guard behind sigma_dev"
        sig = sig[:F]
    return got[:x.size].reshape(x.shape), sig


# ------------------------------------------------------------------ bits against the mirror
@pytest.mark.parametrize("E,R", SHAPES)
def test_bits_against_the_mirror(ctx, dev, E, R):
    for F, N in STACKS:
        x = stack(F, N, E, R)
        for opts in MODES:
            for gain in (None, gains(E)):
                for first_id in (0, 7):
                    want, want_sigma = nm.noise(x, first_id, opts, gain)
                    got, sigma = run(ctx, dev, x, first_id, gain, **opts)
                    what = "E %d R %d F %d N %d %s gain %s id %d" % (E, R, F, N, opts, gain is not None, first_id)
                    ic.assert_same_bits(got, want, what)
                    ic.assert_same_bits(sigma, want_sigma, what + ": sigma")
                    if (F, N) == (3, 1) and "snr_db" in opts and E * R >= 64:
                        # each frame of a multi-frame call has its own peak: the loud frame's sigma is not the quiet ones'
                        assert sigma[1] > 2.0 * sigma[0] and sigma[1] > 2.0 * sigma[2], what


def test_an_unaligned_base(ctx, dev):
    """a stack that starts 4, 8 and 12 bytes past a 16-byte boundary: the lanes' 16-byte accesses follow the address, not the index"""
    E, R = 5, 64
    x = stack(2, 1, E, R)
    want, _ = nm.noise(x, 3, dict(sigma=0.5))
    for off in (1, 2, 3):
        host = np.concatenate([np.full(off, FILL), x.reshape(-1), np.full(GUARD, FILL)])
        p = dev.upload(host)
        ctx.noise_frames(p + 4 * off, 2, 1, E, R, first_image_id=3, sigma=0.5)
        ctx.synchronize()
        got = ctx.d2h(p, host.shape)
        assert (got[:off] == FILL).all() and (got[off + x.size:] == FILL).all(), off
        ic.assert_same_bits(got[off:off + x.size].reshape(x.shape), want, "offset %d floats" % off)


# ------------------------------------------------------------------ the ids are the determinism
def test_a_pass_is_its_images_one_by_one(ctx, dev):
    E, R = 7, 257
    x = stack(2, 3, E, R)
    for seed in (None, 0x5EED):
        kw = {} if seed is None else dict(seed=seed)
        whole, _ = run(ctx, dev, x, 11, sigma=0.25, **kw)
        ic.assert_same_bits(whole, nm.noise(x, 11, dict(sigma=0.25, **kw))[0], "ABS, the pass")
        for j in range(6):
            one, _ = run(ctx, dev, x.reshape(6, 1, 1, E, R)[j], 11 + j, sigma=0.25, **kw)
            ic.assert_same_bits(one[0, 0], whole.reshape(6, E, R)[j], "ABS, image %d alone" % j)
        joint, sig = run(ctx, dev, x, 11, snr_db=30.0, **kw)
        for f in range(2):
            one, s1 = run(ctx, dev, x[f:f + 1], 11 + 3 * f, snr_db=30.0, **kw)
            ic.assert_same_bits(one[0], joint[f], "SNR_DB, frame %d alone" % f)
            assert s1[0] == sig[f]
    a, _ = run(ctx, dev, x, 11, sigma=0.25)
    b, _ = run(ctx, dev, x, 11, sigma=0.25, seed=0x5EED)
    fin = np.isfinite(x)
    for j in range(6):                                      # another seed changes every image
        m = fin.reshape(6, E, R)[j]
        assert (a.reshape(6, E, R)[j][m] != b.reshape(6, E, R)[j][m]).mean() > 0.99


# ------------------------------------------------------------------ identity cases
def test_identity_cases(ctx, dev):
    E, R = 7, 257
    x = stack(2, 2, E, R)
    got, sigma = run(ctx, dev, x, 5, sigma=0.0)
    ic.assert_same_bits(got, x, "ABS, sigma 0, no gain")
    assert np.array_equal(np.signbit(got), np.signbit(x)) and np.signbit(x[x == 0]).any()        # -0.0 kept
    assert (sigma == 0).all()
    g = gains(E)
    got, _ = run(ctx, dev, x, 5, g, sigma=0.0)
    with np.errstate(all="ignore"):
        ic.assert_same_bits(got, x * g.reshape(1, 1, E, 1), "gain only")
    z = np.zeros((2, 2, E, R), f32); z[0, 1, 2, 3] = -0.0
    z[1] = x[1]
    got, sigma = run(ctx, dev, z, 0, snr_db=30.0)
    ic.assert_same_bits(got[0], z[0], "an all-zero frame in SNR_DB")
    assert sigma[0] == 0 and sigma[1] > 0 and np.signbit(got[0, 1, 2, 3])
    ic.assert_same_bits(got, nm.noise(z, 0, dict(snr_db=30.0))[0], "a zero frame beside a loud one")
    # a frame whose only finite value is one spike: sigma_f comes from that spike
    s = np.full((1, 2, E, R), np.nan, f32)
    s[0, 0, ::2] = np.inf; s[0, 1, 1::2] = -np.inf
    s[0, 1, 4, 200] = f32(-3.0)
    got, sigma = run(ctx, dev, s, 0, snr_db=20.0)
    assert sigma[0] == f32(3.0) * nm.snr_factor(20.0)
    ic.assert_same_bits(got, nm.noise(s, 0, dict(snr_db=20.0))[0], "one spike")
    assert np.array_equal(np.isnan(got), np.isnan(s)) and np.array_equal(got[np.isinf(s)], s[np.isinf(s)])
    assert got[0, 1, 4, 200] != f32(-3.0)


# ------------------------------------------------------------------ the gain table is cached by content
def test_the_gain_table_is_cached_by_content(ctx, dev):
    E, R = 33, 100
    x = stack(1, 1, E, R)
    rng = np.random.default_rng(5)
    g1, g2 = rng.standard_normal(E).astype(f32), rng.standard_normal(E).astype(f32)
    for g in (g1, g2, g1, g1, g2):
        p = dev.upload(x)
        host = g.copy()
        ctx.noise_frames(p, 1, 1, E, R, first_image_id=2, element_gain=host, sigma=0.125)
        host[:] = 1e9                                           # the host array is the caller's again the moment the call returns
        ctx.synchronize()
        ic.assert_same_bits(ctx.d2h(p, x.shape), nm.noise(x, 2, dict(sigma=0.125), g)[0], "gain table")
    # another E after these: a table of its own size
    for E2 in (5, 64):
        y = stack(1, 1, E2, 9)
        got, _ = run(ctx, dev, y, 0, gains(E2), sigma=0.125)
        ic.assert_same_bits(got, nm.noise(y, 0, dict(sigma=0.125), gains(E2))[0], "E %d" % E2)


# ------------------------------------------------------------------ every error of the contract
def test_errors_leave_the_buffers_untouched(mcrt, ctx, dev):
    L = ctx.L
    F, N, E, R = 2, 2, 5, 9
    x = stack(F, N, E, R)
    rf = dev.upload(x)
    sfill = np.full(F, FILL)
    sg = dev.upload(sfill)
    good = mcrt.noise_opts_struct(snr_db=30.0)
    gain_ok = gains(E)

    def call(h=ctx.h, p=rf, f=F, n=N, e=E, r=R, first=0, o=good, g=None, s=sg):
        gp = g.ctypes.data_as(C.c_void_p) if g is not None else None
        return L.mcrt_noise_frames(h, C.c_void_p(p) if p else None, f, n, e, r, first, C.byref(o) if o is not None else None, gp, C.c_void_p(s) if s else None)

    def err(code, word, **kw):
        assert call(**kw) == code, kw
        assert word in L.mcrt_last_error(), (kw, L.mcrt_last_error())

    err(INVALID, b"null context", h=None)
    err(INVALID, b"rf_dev", p=None)
    err(INVALID, b"zero", f=0); err(INVALID, b"zero", n=0); err(INVALID, b"zero", e=0); err(INVALID, b"zero", r=0)
    bad = mcrt.noise_opts_struct(); bad.mode = 2
    err(INVALID, b"mode", o=bad)
    for v in (np.nan, np.inf, -np.inf):
        err(INVALID, b"snr_db", o=mcrt.noise_opts_struct(snr_db=v))
    for v in (-1.0, np.nan, np.inf):
        err(INVALID, b"sigma", o=mcrt.noise_opts_struct(sigma=v))
    for v in (np.nan, np.inf):
        g = gain_ok.copy(); g[3] = v
        err(INVALID, b"element_gain[3]", g=g)
    err(LIMIT, b"n_rows", r=2049)
    err(LIMIT, b"n_frames * n_images", f=256, n=256); err(LIMIT, b"n_frames * n_images", f=65536, n=1); err(LIMIT, b"n_frames * n_images", f=1, n=65536)
    err(LIMIT, b"first_image_id", first=0xFFFFFFFF - 2); err(LIMIT, b"first_image_id", first=0xFFFFFFFF)
    err(LIMIT, b"2^31", f=1, n=1, e=1 << 21, r=1 << 10)
    # a snr_db that ABS does not read, a sigma that SNR_DB does not read: fine
    o = mcrt.noise_opts_struct(sigma=0.0); o.snr_db = float("nan")
    assert call(o=o, s=None) == 0
    ctx.synchronize()
    ic.assert_same_bits(ctx.d2h(rf, x.shape), x, "rf_dev after the errors")
    ic.assert_same_bits(ctx.d2h(sg, (F,)), sfill, "sigma_dev after the errors")
    # the ids may end at 2^32 - 1; the context still works; null options are the defaults
    assert call(first=0xFFFFFFFF - 3, o=None) == 0
    ctx.synchronize()
    want, sigma = nm.noise(x, 0xFFFFFFFF - 3, None)
    ic.assert_same_bits(ctx.d2h(rf, x.shape), want, "null options")
    ic.assert_same_bits(ctx.d2h(sg, (F,)), sigma, "null options: sigma")


# ------------------------------------------------------------------ end to end: a traced scene
def _write_scene(mcrt, tmp_path):
    cfg, meshes = mcrt.synth.sphere_scene(3)
    cfg["workingDirectory"] = str(tmp_path) + "/"
    for f, (V, F) in meshes.items():
        mcrt.scene_io.save_obj(str(tmp_path / f), V, F)
    (tmp_path / "sphere.scene").write_text(json.dumps(cfg))
    return cfg, str(tmp_path / "sphere.scene")


def test_simulator_pictures_are_the_stage_by_hand(mcrt, tmp_path):
    """Simulator(noise=40.0) pictures equal Simulator() pictures with Context.noise_frames applied by hand between convolve() and
    envelope(): the plain B-mode frame, a compounded frame (the views share one peak, ids frame * 3 + n) and a cut through a swept volume;
    frame() is the mirror's noise on the plain simulator's frame(); noise=None is today's picture; a dead element is a zero scan-line"""
    cfg, scene = _write_scene(mcrt, tmp_path)
    sd = mcrt.scene_io.load_scene_file(scene)
    E, S, frame = 16, 8, 3
    tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    size = dict(out_rows=80, out_cols=100)
    g = mcrt.cplane_grid(80.0, nu=40, nv=8, pitch_mm=1.0)
    for kw in (dict(), dict(compound=(-0.1, 0.0, 0.1)), dict(sweep=(3, 0.05), sweep_pivot_mm=10.0)):
        plain, noisy, none = mcrt.Simulator(sd, tr, n_samples=S, **kw), mcrt.Simulator(sd, tr, n_samples=S, noise=40.0, **kw), mcrt.Simulator(sd, tr, n_samples=S, noise=None, **kw)
        try:
            assert plain.noise is None and none.noise is None and noisy.noise.snr_db == 40.0 and noisy.noise.mode == mcrt.NOISE_SNR_DB
            picture = lambda s: s.bmode_volume(frame, g) if "sweep" in kw else s.bmode(frame, **size)
            got_pic, today = picture(noisy), picture(none)
            plain.trace(frame); plain.convolve()
            buf, n = plain._stack
            assert n == (1 if not kw else 3)
            plain.ctx.synchronize()
            raw = plain.ctx.d2h(buf, (1, n, E, plain.R))
            plain.ctx.noise_frames(buf, 1, n, E, plain.R, first_image_id=frame * n, snr_db=40.0)
            plain.ctx.synchronize()
            ic.assert_same_bits(plain.ctx.d2h(buf, raw.shape), nm.noise(raw, frame * n, dict(snr_db=40.0))[0], "the stack by hand")
            plain.envelope()
            with plain.ctx.temp(size["out_rows"] * size["out_cols"] * 4) as out:
                if "sweep" in kw:
                    plain.ctx.bmode_volume_frames(buf, 1, E, plain.R, plain.sweep, g, out)
                    want_pic = plain.ctx.d2h(out, (g.nw, g.nv, g.nu), np.uint8)
                elif "compound" in kw:
                    plain.ctx.bmode_compound_frames(buf, 1, E, plain.R, plain.steers, out, **size)
                    want_pic = plain.ctx.d2h(out, (80, 100), np.uint8)
                else:
                    plain.ctx.bmode_frames(buf, 1, E, plain.R, out, **size)
                    want_pic = plain.ctx.d2h(out, (80, 100), np.uint8)
            assert np.array_equal(got_pic, want_pic), kw
            assert np.array_equal(today, picture(plain)), "noise=None is today's picture"
            assert not np.array_equal(today, got_pic), "the noise changed nothing"
            if not kw:
                rf = plain.frame(frame)                                     # [R][E], convolved
                want, _ = nm.noise(np.ascontiguousarray(rf.T).reshape(1, 1, E, plain.R), frame, dict(snr_db=40.0))
                ic.assert_same_bits(noisy.frame(frame), want[0, 0].T, "frame() is noisy RF")
                ic.assert_same_bits(none.frame(frame), rf, "noise=None: frame()")
                raw_rf = plain.frame(frame, convolve=False)                 # the stage runs whether or not convolve ran
                want, _ = nm.noise(np.ascontiguousarray(raw_rf.T).reshape(1, 1, E, plain.R), frame, dict(snr_db=40.0))
                ic.assert_same_bits(noisy.frame(frame, convolve=False), want[0, 0].T, "frame(convolve=False) is noisy RF")
        finally:
            plain.close(); noisy.close(); none.close()
    dead = mcrt.Simulator(sd, tr, n_samples=S, noise=dict(sigma=0.0, dead_elements=(5,)))
    plain = mcrt.Simulator(sd, tr, n_samples=S)
    try:
        got, rf = dead.frame(frame), plain.frame(frame)
        assert np.array_equal(got[:, 5] == 0, np.isfinite(rf[:, 5])) and np.nanmax(np.abs(rf[:, 5])) > 0   # (by the rule a NaN tap stays a NaN)
        keep = np.arange(E) != 5
        ic.assert_same_bits(got[:, keep], rf[:, keep], "the live scan-lines")
    finally:
        dead.close(); plain.close()
    with pytest.raises(ValueError):
        mcrt.Simulator(sd, tr, n_samples=S, noise=dict(snr_db=40.0, sigma=1.0))
    with pytest.raises(ValueError):
        mcrt.Simulator(sd, tr, n_samples=S, noise=dict(dead_elements=(E,)))


def test_cli_noise_options(mcrt, orc, tmp_path):
    """mattausch_hip --noise-db 40 --dead-elements 3,200: the PGM equals the Python Simulator's bytes; rf.bin, which the program writes
    after its envelope, is the oracle's envelope of the mirror's noise on the convolved RF -- and the run with --noise-sigma 0 leaves
    that RF as it is: its rf.bin is the run's without the options --; without the options the PGM is today's; options that make no
    sense end the program before it touches a device"""
    exe = os.path.join(ROOT, "mcray-tracing_amd", "mattausch_hip")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "mcray-tracing_amd"), "mattausch_hip"])
    cfg, scene = _write_scene(mcrt, tmp_path)
    run_ = lambda *a: subprocess.run([exe, scene, "1", "5"] + list(a), capture_output=True, text=True, timeout=240)
    for name, extra in (("n", ["--noise-db", "40", "--dead-elements", "3,200"]), ("z", ["--noise-sigma", "0"]), ("p", [])):
        r = run_(str(tmp_path / (name + ".pgm")), str(tmp_path / (name + ".bin")), "--db", "50", *extra)
        assert r.returncode == 0, r.stdout + r.stderr
    head = b"P5\n500 400\n255\n"
    tr = mcrt.Transducer(512, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    sd = mcrt.scene_io.load_scene_file(scene)
    for name, noise in (("n", dict(snr_db=40.0, dead_elements=(3, 200))), ("z", dict(sigma=0.0)), ("p", None)):
        sim = mcrt.Simulator(sd, tr, n_samples=5, noise=noise)
        try:
            pic = sim.bmode(0, dynamic_range_db=50.0)
            if noise is None:
                conv = sim.frame(0)                                          # [465][512], convolved, no envelope
        finally:
            sim.close()
        assert (tmp_path / (name + ".pgm")).read_bytes() == head + pic.tobytes(), name
    assert (tmp_path / "n.pgm").read_bytes() != (tmp_path / "p.pgm").read_bytes()
    assert (tmp_path / "z.pgm").read_bytes() == (tmp_path / "p.pgm").read_bytes()
    load = lambda name: np.fromfile(str(tmp_path / (name + ".bin")), f32).reshape(465, 512)
    ic.assert_same_bits(load("p"), orc.envelope(conv), "rf.bin without the options")
    ic.assert_same_bits(load("z"), load("p"), "rf.bin with --noise-sigma 0")
    gain = np.ones(512, f32); gain[[3, 200]] = 0.0
    want, _ = nm.noise(np.ascontiguousarray(conv.T).reshape(1, 1, 512, 465), 0, dict(snr_db=40.0), gain)
    ic.assert_same_bits(load("n"), orc.envelope(np.ascontiguousarray(want[0, 0].T)), "rf.bin with --noise-db 40 --dead-elements 3,200")
    assert not np.array_equal(load("n")[:, 3], load("p")[:, 3])
    for bad, word in ((["--noise-db", "nan"], "--noise-db"), (["--noise-sigma", "-1"], "--noise-sigma"), (["--noise-db", "40", "--noise-sigma", "1"], "--noise-sigma"),
                      (["--noise-seed", "5"], "--noise-seed"), (["--noise-db", "40", "--dead-elements", "512"], "--dead-elements")):
        r = subprocess.run([exe, scene, "1", "5"] + bad, capture_output=True, text=True, timeout=240)
        assert r.returncode == 1 and word in r.stdout, (bad, word, r.stdout)
