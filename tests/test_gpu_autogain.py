"""Automatic gain on the MI355X (mcrt_autogain_frames: k_autogain_hist, k_autogain_curve, k_autogain_apply) against the numpy mirror
(tests/autogain_mirror.py), bit for bit: the stack, the row gains, the band levels and the penetration depths -- at the ragged ends of a
lane's 4 rows, of a band, of a wavefront and of a workgroup, one frame and several, one image per frame and several, with the floor from
the options and from the device, applied and estimated only; both forms of the histogram kernel; a pass walked in chunks; the identity
cases; the argument errors; a traced scene through the Simulator and mattausch_hip."""
import ctypes as C
import json
import os
import subprocess
import numpy as np
import pytest

import autogain_mirror as am
import image_cases as ic
import noise_mirror as nm
from test_gpu_focus import Dev

pytestmark = pytest.mark.gpu

f32 = np.float32
INVALID, LIMIT = -1, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (1, 5), (3, 17), (5, 64), (64, 5), (7, 255), (7, 256), (7, 257), (33, 465), (3, 2048)]
BANDS = [4, 7, 16, 256]
STACKS = [(1, 1), (3, 1), (2, 3)]
FILL = f32(-777.25)             # 64 guard words behind every buffer: a write past the end shows
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
    """[F][N][E][R] as tests/test_gpu_noise.py's stack(): "echoes" with both signs, a flat zero patch, exact zeros, -0.0, NaN, +-inf and
    1e-30, every second frame four times as loud -- and decaying with depth to a twentieth, so that the curve has something to do"""
    rng = np.random.default_rng(5000 + 131 * E + R + 7 * F + N + seed)
    shape = (F, N, E, R)
    x = rng.rayleigh(1.0, shape) * np.where(rng.random(shape) < 0.3, -1.0, 1.0) * (1.0 + 3.0 * (np.arange(F).reshape(F, 1, 1, 1) % 2))
    x = (x * np.exp(-3.0 * np.arange(R) / R)).astype(f32)
    x[:, :, E // 3:E // 3 + 4, R // 4:R // 4 + 5] = 0.0
    flat = x.reshape(F * N, -1)
    n = flat.shape[1]
    if n >= 6:
        vals = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-30], f32)
        for j in range(F * N):
            k = max(len(vals), n // 40)
            flat[j, rng.permutation(n)[:k]] = np.resize(vals, k)
    return x


FLOORS = np.array([0.02, 0.0, 0.3, np.nan, 0.1], f32)             # floor_dev: a frame each (0 and NaN: no floor)


def run(ctx, dev, x, floor_dev=None, outputs=True, c=None, **opts):
    """x through mcrt_autogain_frames on the device -> (out, gain, band_bin, pen), the last three None without outputs; the guard words
    behind every buffer are checked"""
    c = c or ctx
    F, N, E, R = x.shape
    nB = am.n_bands(R, opts.get("band_rows", 16))
    p = dev.upload(np.concatenate([x.reshape(-1), np.full(GUARD, FILL)]))
    fl = dev.upload(np.concatenate([np.asarray(floor_dev, f32), np.full(GUARD, FILL)])) if floor_dev is not None else None
    g = dev.upload(np.full(F * R + GUARD, FILL)) if outputs else None
    b = dev.upload(np.full(F * nB + GUARD, -777, np.int32)) if outputs else None
    q = dev.upload(np.full(F + GUARD, 777, np.uint32)) if outputs else None
    c.autogain_frames(p, F, N, E, R, floor_dev=fl, gain_dev=g, band_bin_dev=b, pen_dev=q, **opts)
    c.synchronize()
    got = c.d2h(p, (x.size + GUARD,))
    assert (got[x.size:] == FILL).all(), "the guard behind the stack"
    if not outputs:
        return got[:x.size].reshape(x.shape), None, None, None
    gain, band, pen = c.d2h(g, (F * R + GUARD,)), c.d2h(b, (F * nB + GUARD,), np.int32), c.d2h(q, (F + GUARD,), np.uint32)
    assert (gain[F * R:] == FILL).all() and (band[F * nB:] == -777).all() and (pen[F:] == 777).all(), "the guards behind the outputs"
    if floor_dev is not None:
        ic.assert_same_bits(c.d2h(fl, (F + GUARD,))[F:], np.full(GUARD, FILL), "the guard behind floor_dev")
    return got[:x.size].reshape(x.shape), gain[:F * R].reshape(F, R), band[:F * nB].reshape(F, nB), pen[:F]


def check(got, want, what, applied=True):
    out, gain, band, pen = got
    wout, wgain, wband, wpen = want
    assert np.array_equal(band, wband), (what, band, wband)
    assert np.array_equal(pen, wpen), (what, pen, wpen)
    ic.assert_same_bits(gain, wgain, what + ": gain")
    ic.assert_same_bits(out, wout, what + ": the stack")


# ------------------------------------------------------------------ bits against the mirror
@pytest.mark.parametrize("E,R", SHAPES)
def test_bits_against_the_mirror(ctx, dev, E, R):
    for F, N in STACKS:
        x = stack(F, N, E, R)
        for B in BANDS:
            for floor in (None, FLOORS[:F]):
                opts = dict(band_rows=B) if floor is not None else dict(band_rows=B, floor=0.02)
                want = am.autogain(x, opts, floor)
                what = "E %d R %d F %d N %d band %d floor_dev %s" % (E, R, F, N, B, floor is not None)
                check(run(ctx, dev, x, floor, **opts), want, what)
                check(run(ctx, dev, x, floor, apply=False, **opts), (x,) + want[1:], what + " apply 0")
                if R >= 64 and B <= 16 and floor is None:
                    assert want[1].max() > 2.0 * want[1].min(), what + ": the curve does nothing"
            if B == 16:                                          # no outputs asked for: the gains live in the context
                ic.assert_same_bits(run(ctx, dev, x, None, outputs=False, band_rows=B, floor=0.02)[0], am.autogain(x, dict(band_rows=B, floor=0.02))[0], "no outputs")


def test_options_and_an_unaligned_base(ctx, dev):
    """min_permille, floor_scale and max_gain reach the kernel; a stack that starts 4, 8 and 12 bytes past a 16-byte boundary: the
    16-byte accesses follow the address, not the index"""
    E, R = 5, 64
    x = stack(2, 2, E, R)
    for opts in (dict(min_permille=0), dict(min_permille=1000), dict(min_permille=900, floor=0.05), dict(floor=0.05, floor_scale=0.0),
                 dict(floor=0.01, floor_scale=10.0), dict(max_gain=1.0), dict(max_gain=1.5), dict(band_rows=8, floor=0.2)):
        check(run(ctx, dev, x, **opts), am.autogain(x, opts), str(opts))
    check(run(ctx, dev, x, max_gain_db=12.0), am.autogain(x, dict(max_gain=f32(10.0 ** 0.6))), "max_gain_db 12")
    want = am.autogain(x, dict(floor=0.02))
    for off in (1, 2, 3):
        host = np.concatenate([np.full(off, FILL), x.reshape(-1), np.full(GUARD, FILL)])
        p = dev.upload(host)
        g = dev.upload(np.full(off + 2 * R + GUARD, FILL))
        ctx.autogain_frames(p + 4 * off, 2, 2, E, R, gain_dev=g + 4 * off, floor=0.02)
        ctx.synchronize()
        got, gain = ctx.d2h(p, host.shape), ctx.d2h(g, (off + 2 * R + GUARD,))
        assert (got[:off] == FILL).all() and (got[off + x.size:] == FILL).all() and (gain[:off] == FILL).all() and (gain[off + 2 * R:] == FILL).all(), off
        ic.assert_same_bits(got[off:off + x.size].reshape(x.shape), want[0], "offset %d floats" % off)
        ic.assert_same_bits(gain[off:off + 2 * R].reshape(2, R), want[1], "offset %d floats: gain" % off)


# ------------------------------------------------------------------ identity cases
def test_identity_cases(ctx, dev):
    E, R = 7, 257
    z = np.zeros((2, 2, E, R), f32); z[0, 1, 2, 3] = -0.0; z[0, 0, 1, 5] = np.nan; z[0, 0, 1, 6] = -np.inf
    z[1] = stack(1, 2, E, R)[0]
    out, gain, band, pen = run(ctx, dev, z, floor=0.02)
    assert (gain[0] == 1.0).all() and (band[0] == -1).all() and pen[0] == 0, "an all-zero frame: gains 1, penetration 0"
    assert pen[1] > 0 and (band[1] >= 0).any()
    ic.assert_same_bits(out[0], z[0], "an all-zero frame keeps its bits")
    assert np.signbit(out[0, 1, 2, 3]) and np.isneginf(out[0, 0, 1, 6])
    check((out, gain, band, pen), am.autogain(z, dict(floor=0.02)), "a zero frame beside a loud one")
    # apply == 0 keeps every bit, NaN payloads included
    x = stack(2, 2, E, R)
    x.view(np.uint32)[0, 0, 0, 0] = 0x7FC12345
    out, gain, _, _ = run(ctx, dev, x, floor=0.02, apply=False)
    assert np.array_equal(out.view(np.uint32), x.view(np.uint32))
    ic.assert_same_bits(gain, am.autogain(x, dict(floor=0.02))[1], "apply 0: the curve all the same")
    # a frame is its own: a pass equals its frames one by one, and the images of a frame share one curve
    whole = run(ctx, dev, x, FLOORS[:2])
    for f in range(2):
        one = run(ctx, dev, x[f:f + 1], FLOORS[f:f + 1])
        check(one, tuple(v[f:f + 1] for v in whole), "frame %d alone" % f)
    # everything under the floor: nothing is tissue
    out, gain, band, pen = run(ctx, dev, x, floor=1e30)
    assert (gain == 1.0).all() and (band == -1).all() and (pen == 0).all()
    ic.assert_same_bits(out, x, "everything under the floor")


# ------------------------------------------------------------------ the other histogram form, and a pass in chunks
def _context_with(mcrt, **env):
    saved = {k: os.environ.get(k) for k in env}
    try:
        os.environ.update({k: str(v) for k, v in env.items()})          # (MCRT_TUNING=1 is the suite's: conftest.py; read when a context is made)
        return mcrt.Context(0)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_four_lds_histograms_per_workgroup(mcrt, ctx, dev):
    """MCRT_AUTOGAIN_COPIES=4, the form of k_autogain_hist that is not the default: the same counts"""
    c = _context_with(mcrt, MCRT_AUTOGAIN_COPIES=4)
    try:
        for E, R, B in ((33, 465, 16), (7, 257, 7), (64, 5, 4), (3, 2048, 256)):
            x = stack(2, 3, E, R)
            check(run(ctx, dev, x, FLOORS[:2], c=c, band_rows=B), am.autogain(x, dict(band_rows=B), FLOORS[:2]), "four copies, E %d R %d band %d" % (E, R, B))
    finally:
        c.close()


def test_a_pass_larger_than_the_scratch_is_walked_in_chunks(mcrt, ctx, dev):
    """MCRT_AUTOGAIN_HIST_KB=64 leaves room for 8 band histograms: five frames of four bands go two at a time, five frames of sixteen bands
    one at a time (a frame always fits) -- and equal the mirror and the same call on a context with the full scratch"""
    c = _context_with(mcrt, MCRT_AUTOGAIN_HIST_KB=64)
    try:
        for E, R, B in ((5, 64, 16), (5, 64, 4), (7, 257, 16)):
            x = stack(5, 2, E, R)
            small = run(ctx, dev, x, FLOORS, c=c, band_rows=B)
            check(small, am.autogain(x, dict(band_rows=B), FLOORS), "in chunks, E %d R %d band %d" % (E, R, B))
            check(small, run(ctx, dev, x, FLOORS, band_rows=B), "in chunks against one chunk")
            ic.assert_same_bits(run(ctx, dev, x, FLOORS, outputs=False, c=c, band_rows=B)[0], small[0], "in chunks, the context's gains")
    finally:
        c.close()


# ------------------------------------------------------------------ every error of the contract
def test_errors_launch_nothing(mcrt, ctx, dev):
    L = ctx.L
    F, N, E, R = 2, 2, 5, 9
    x = stack(F, N, E, R)
    rf = dev.upload(x)
    gfill, bfill, pfill = np.full(F * R, FILL), np.full(F * 3, -777, np.int32), np.full(F, 777, np.uint32)
    g, b, q = dev.upload(gfill), dev.upload(bfill), dev.upload(pfill)
    fl = dev.upload(FLOORS[:F])
    good = mcrt.autogain_opts_struct(band_rows=4)

    def call(h=ctx.h, p=rf, f=F, n=N, e=E, r=R, o=good, floor=fl):
        return L.mcrt_autogain_frames(h, C.c_void_p(p) if p else None, f, n, e, r, C.byref(o) if o is not None else None, C.c_void_p(floor) if floor else None,
                                      C.c_void_p(g), C.c_void_p(b), C.c_void_p(q))

    def err(code, word, **kw):
        assert call(**kw) == code, kw
        assert word in L.mcrt_last_error(), (kw, L.mcrt_last_error())

    err(INVALID, b"null context", h=None)
    err(INVALID, b"rf_dev", p=None)
    err(INVALID, b"zero", f=0); err(INVALID, b"zero", n=0); err(INVALID, b"zero", e=0); err(INVALID, b"zero", r=0)
    for v in (0, 3, 257):
        err(INVALID, b"band_rows", o=mcrt.autogain_opts_struct(band_rows=v))
    err(INVALID, b"min_permille", o=mcrt.autogain_opts_struct(min_permille=1001))
    for v in (-1.0, np.nan, np.inf):
        err(INVALID, b"floor", o=mcrt.autogain_opts_struct(floor=v))
        err(INVALID, b"floor_scale", o=mcrt.autogain_opts_struct(floor_scale=v))
    for v in (0.99, -2.0, np.nan, np.inf):
        err(INVALID, b"max_gain", o=mcrt.autogain_opts_struct(max_gain=v))
    err(LIMIT, b"n_rows", r=2049)
    err(LIMIT, b"n_frames * n_images", f=256, n=256); err(LIMIT, b"n_frames * n_images", f=65536, n=1); err(LIMIT, b"n_frames * n_images", f=1, n=65536)
    err(LIMIT, b"2^31", f=1, n=1, e=1 << 21, r=1 << 10)
    ctx.synchronize()
    ic.assert_same_bits(ctx.d2h(rf, x.shape), x, "rf_dev after the errors")
    ic.assert_same_bits(ctx.d2h(g, gfill.shape), gfill, "gain_dev after the errors")
    assert np.array_equal(ctx.d2h(b, bfill.shape, np.int32), bfill) and np.array_equal(ctx.d2h(q, pfill.shape, np.uint32), pfill)
    # the context still works; null options are the defaults (bands of 16 rows: one band of 9)
    assert call(o=None, floor=None) == 0
    ctx.synchronize()
    want = am.autogain(x)
    ic.assert_same_bits(ctx.d2h(rf, x.shape), want[0], "null options")
    ic.assert_same_bits(ctx.d2h(g, (F, R)), want[1], "null options: gain")
    assert np.array_equal(ctx.d2h(b, (F * 3,), np.int32)[:F], want[2].reshape(-1)) and np.array_equal(ctx.d2h(q, (F,), np.uint32), want[3])


# ------------------------------------------------------------------ end to end: a traced scene
def _write_scene(mcrt, tmp_path):
    cfg, meshes = mcrt.synth.sphere_scene(3)
    cfg["workingDirectory"] = str(tmp_path) + "/"
    for f, (V, F) in meshes.items():
        mcrt.scene_io.save_obj(str(tmp_path / f), V, F)
    (tmp_path / "sphere.scene").write_text(json.dumps(cfg))
    return cfg, str(tmp_path / "sphere.scene")


def test_simulator_pictures_are_the_stage_by_hand(mcrt, tmp_path):
    """Simulator(noise=40, autogain=True) pictures equal the pictures of the mirror's gain on the un-gained stack -- traced, convolved,
    noised and enveloped by a plain Simulator by hand, the floor the noise stage's sigma: the plain B-mode frame, a compounded frame (the
    views share one curve) and a cut through a swept volume; gain_curve() and penetration_mm() are the mirror's; without autogain= (and
    with apply=False) the picture is the un-gained one, bit for bit"""
    cfg, scene = _write_scene(mcrt, tmp_path)
    sd = mcrt.scene_io.load_scene_file(scene)
    E, S, frame = 16, 8, 3
    tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    size = dict(out_rows=80, out_cols=100)
    g = mcrt.cplane_grid(80.0, nu=40, nv=8, pitch_mm=1.0)
    for kw in (dict(), dict(compound=(-0.1, 0.0, 0.1)), dict(sweep=(3, 0.05), sweep_pivot_mm=10.0)):
        plain = mcrt.Simulator(sd, tr, n_samples=S, **kw)
        auto = mcrt.Simulator(sd, tr, n_samples=S, noise=40.0, autogain=True, **kw)
        noisy = mcrt.Simulator(sd, tr, n_samples=S, noise=40.0, **kw)
        est = mcrt.Simulator(sd, tr, n_samples=S, noise=40.0, autogain=dict(apply=False), **kw)
        try:
            assert plain.autogain is None and noisy.autogain is None and auto.autogain == {} and auto.gain_curve() is None and auto.penetration_mm() is None
            picture = lambda s: s.bmode_volume(frame, g) if "sweep" in kw else s.bmode(frame, **size)
            got_pic, ungained, est_pic = picture(auto), picture(noisy), picture(est)
            plain.trace(frame); plain.convolve()
            buf, n = plain._stack
            R = plain.R
            with plain.ctx.temp(4) as sig:
                plain.ctx.noise_frames(buf, 1, n, E, R, first_image_id=frame * n, sigma_dev=sig, snr_db=40.0)
                plain.envelope()
                plain.ctx.synchronize()
                sigma = plain.ctx.d2h(sig, (1,))
            env = plain.ctx.d2h(buf, (1, n, E, R))
            assert sigma[0] > 0

            def by_hand(stack_):
                plain.ctx.h2d(buf, stack_)
                with plain.ctx.temp(size["out_rows"] * size["out_cols"] * 4) as out:
                    if "sweep" in kw:
                        plain.ctx.bmode_volume_frames(buf, 1, E, R, plain.sweep, g, out)
                        return plain.ctx.d2h(out, (g.nw, g.nv, g.nu), np.uint8)
                    if "compound" in kw:
                        plain.ctx.bmode_compound_frames(buf, 1, E, R, plain.steers, out, **size)
                    else:
                        plain.ctx.bmode_frames(buf, 1, E, R, out, **size)
                    return plain.ctx.d2h(out, (80, 100), np.uint8)

            want, gain, band, pen = am.autogain(env, None, sigma)
            assert np.array_equal(got_pic, by_hand(want)), kw
            assert np.array_equal(ungained, by_hand(env)), "without autogain= the picture is the un-gained one"
            assert np.array_equal(est_pic, ungained), "apply=False leaves the picture alone"
            assert not np.array_equal(got_pic, ungained), "the gain changed nothing"
            ic.assert_same_bits(auto.gain_curve(), gain[0], "gain_curve()")
            ic.assert_same_bits(est.gain_curve(), gain[0], "gain_curve() with apply=False")
            assert 0 < pen[0] <= R and auto.penetration_mm() == float(pen[0]) * auto.row_mm == est.penetration_mm()
            print("%s: penetration %.2f mm (%d of %d rows), gain %.3g .. %.3g" % (kw or "plain", auto.penetration_mm(), pen[0], R, gain.min(), gain.max()))
        finally:
            plain.close(); auto.close(); noisy.close(); est.close()
    with pytest.raises(TypeError):
        mcrt.Simulator(sd, tr, n_samples=S, autogain=dict(rows=4))


def test_cli_autogain_options(mcrt, tmp_path):
    """mattausch_hip --noise-db 40 --autogain: the PGM equals the Python Simulator's bytes; rf.bin is the mirror's gain on the rf.bin of
    the run without --autogain, whose PGM and rf.bin are those of a run that never heard of the option; the penetration depth is printed
    and --autogain-curve writes the mirror's row gains; options that make no sense end the program before it touches a device"""
    exe = os.path.join(ROOT, "mcray-tracing_amd", "mattausch_hip")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "mcray-tracing_amd"), "mattausch_hip"])
    cfg, scene = _write_scene(mcrt, tmp_path)
    out = {}
    for name, extra in (("a", ["--autogain", "--autogain-curve", str(tmp_path / "curve.txt")]), ("b", ["--autogain", "--autogain-band", "32", "--autogain-floor-scale", "2", "--autogain-max-db", "20"]),
                        ("n", [])):
        r = subprocess.run([exe, scene, "1", "5", str(tmp_path / (name + ".pgm")), str(tmp_path / (name + ".bin")), "--db", "50", "--noise-db", "40"] + extra,
                           capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout + r.stderr
        out[name] = r.stdout
    head = b"P5\n500 400\n255\n"
    tr = mcrt.Transducer(512, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    sd = mcrt.scene_io.load_scene_file(scene)
    pens = {}
    for name, autogain in (("a", True), ("b", dict(band_rows=32, floor_scale=2.0, max_gain_db=20.0)), ("n", None)):
        sim = mcrt.Simulator(sd, tr, n_samples=5, noise=40.0, autogain=autogain)
        try:
            pic = sim.bmode(0, dynamic_range_db=50.0)
            pens[name] = sim.penetration_mm()
            if autogain is None:
                conv = sim.ctx.d2h(sim.rf_dev, (1, 1, 512, 465))                 # (enveloped and noisy: what rf.bin holds)
        finally:
            sim.close()
        assert (tmp_path / (name + ".pgm")).read_bytes() == head + pic.tobytes(), name
    assert (tmp_path / "a.pgm").read_bytes() != (tmp_path / "n.pgm").read_bytes()
    load = lambda name: np.fromfile(str(tmp_path / (name + ".bin")), f32).reshape(465, 512)
    ic.assert_same_bits(load("n"), conv[0, 0].T, "rf.bin without --autogain")
    plain = mcrt.Simulator(sd, tr, n_samples=5)
    try:
        rf = plain.frame(0)
    finally:
        plain.close()
    _, sigma = nm.noise(np.ascontiguousarray(rf.T).reshape(1, 1, 512, 465), 0, dict(snr_db=40.0))
    want, gain, band, pen = am.autogain(conv, None, sigma)
    ic.assert_same_bits(load("a"), want[0, 0].T, "rf.bin with --autogain")
    wb = am.autogain(conv, dict(band_rows=32, floor_scale=2.0, max_gain=f32(10.0)), sigma)
    ic.assert_same_bits(load("b"), wb[0][0, 0].T, "rf.bin with --autogain-band 32 --autogain-floor-scale 2 --autogain-max-db 20")
    assert wb[1].max() <= 10.0 and wb[1].min() >= f32(0.1)
    assert "autogain: penetration depth %g mm (%d of 465 rows)" % (pen[0] * 0.322, pen[0]) in out["a"] and "autogain" not in out["n"], out["a"]
    assert pens["a"] == pen[0] * 0.322 and pens["n"] is None and 0 < pen[0] <= 465
    rows = np.loadtxt(str(tmp_path / "curve.txt"))
    assert rows.shape == (465, 3) and np.array_equal(rows[:, 0], np.arange(465)) and np.allclose(rows[:, 1], np.arange(465) * 0.322, rtol=0, atol=1e-9)
    ic.assert_same_bits(rows[:, 2].astype(f32), gain[0], "--autogain-curve")
    for bad, word in ((["--autogain-band", "16"], "--autogain"), (["--autogain", "--autogain-band", "3"], "--autogain-band"), (["--autogain", "--autogain-band", "257"], "--autogain-band"),
                      (["--autogain", "--autogain-floor-scale", "-1"], "--autogain-floor-scale"), (["--autogain", "--autogain-max-db", "-3"], "--autogain-max-db"),
                      (["--autogain", "--autogain-max-db", "nan"], "--autogain-max-db"), (["--autogain-curve", "x.txt"], "--autogain")):
        r = subprocess.run([exe, scene, "1", "5"] + bad, capture_output=True, text=True, timeout=240)
        assert r.returncode == 1 and word in r.stdout, (bad, word, r.stdout)
