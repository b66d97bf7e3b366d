"""Volume rendering on the MI355X: mcrt_render_frames (k_render) against the numpy mirror (tests/render_mirror.py, fed with the product's own
view floats) -- floats and step indices bit for bit, bytes byte for byte: the rule has no transcendental --, views from outside, one and two
steps, the early stop, a hand-filled view, a pass against single calls, the argument errors, and a traced scene end to end through the
Simulator, the C++ shim and the CLI.  tests/test_render_contract.py shows from the views alone that the cases here look at their blocks."""
import ctypes as C
import json
import math
import os
import subprocess
import numpy as np
import pytest

import image_cases as ic
import render_mirror as rm
from test_gpu_focus import Dev

pytestmark = pytest.mark.gpu

f32 = np.float32
INVALID, LIMIT = -1, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL, FILL8 = -7.25, 0xA5


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


def run(ctx, dev, blocks, view, vol=None, **opts):
    """blocks [F][nw][nv][nu] float32 or uint8 -> (out, out8, depth) [F][ny][nx]; the outputs are pre-filled so that an unwritten pixel shows"""
    F, shape = blocks.shape[0], blocks.shape[1:]
    n = F * view.nx * view.ny
    p = vol if vol is not None else dev.upload(blocks)
    o = dev.upload(np.full(n, FILL, f32)); o8 = dev.upload(np.full(n, FILL8, np.uint8)); d = dev.upload(np.full(n, FILL, f32))
    ctx.render_frames(p, F, shape, view, out_dev=o, out8_dev=o8, depth_dev=d, in_u8=blocks.dtype == np.uint8, **opts)
    pic = (F, view.ny, view.nx)
    return ctx.d2h(o, pic), ctx.d2h(o8, pic, np.uint8), ctx.d2h(d, pic)


def same(got, want, what):
    ic.assert_same_bits(got[0], want[0], what + ": out")
    assert np.array_equal(got[1], want[1]), what + ": out8"
    ic.assert_same_bits(got[2], want[2], what + ": depth")


def blocks_of(block, F, in_u8, seed=0):
    shape = block[::-1]
    return np.stack([(rm.byte_block if in_u8 else rm.float_block)(shape, seed + 10 * f) for f in range(F)])


# ------------------------------------------------------------------ the table
@pytest.mark.parametrize("mode", ["mip", "mean", "surface"])
@pytest.mark.parametrize("bi", range(len(rm.BLOCKS)))
def test_render_matches_the_mirror(mcrt, ctx, dev, bi, mode):
    """every block, direction and picture of the table in both input forms, each with F = 1 and with F = 3 (the first of the three blocks is
    the single one, so the mirror is computed once); NaN, +-inf and -0.0 voxels in the floats"""
    block = rm.BLOCKS[bi]
    lit = 0
    for d, pic in ((d, p) for d in rm.DIRECTIONS for p in rm.PICTURES):
        view = rm.case_view(mcrt, block, d, pic)
        for in_u8 in (False, True):
            blocks = blocks_of(block, 3, in_u8, seed=bi)
            want = rm.render_frames(blocks, view, rm.defaults(in_u8, mode=mode))
            for F in (1, 3):
                got = run(ctx, dev, blocks[:F], view, mode=mode)
                same(got, [w[:F] for w in want], "block %s dir %s picture %s u8 %d F %d %s" % (block, d, pic, in_u8, F, mode))
                lit += int((got[0] > 0).sum())
    assert lit > 100                                                # (pictures, not blanks)


@pytest.mark.parametrize("in_u8", [False, True])
def test_other_options(mcrt, ctx, dev, in_u8):
    """a window inside the data's range, a late and narrow ramp, partial opacity, full and no depth cueing"""
    block = (17, 13, 11)
    blocks = blocks_of(block, 2, in_u8, seed=3)
    k = 255.0 if in_u8 else 1.0
    for d, pic in ((rm.DIRECTIONS[2], (33, 35)), (rm.DIRECTIONS[3], (64, 3))):
        view = rm.case_view(mcrt, block, d, pic)
        for opts in (dict(mode="mip", lo=0.2 * k, hi=0.7 * k), dict(mode="mean", lo=-0.5 * k, hi=2.0 * k),
                     dict(mode="surface", lo=0.1 * k, hi=0.9 * k, threshold=0.6, ramp=0.0625, opacity=0.35, depth_cue=1.0),
                     dict(mode="surface", threshold=0.0, ramp=1.0, opacity=0.125, depth_cue=0.0)):
            same(run(ctx, dev, blocks, view, **opts), rm.render_frames(blocks, view, rm.defaults(in_u8, **opts)), "%s dir %s" % (opts, d))


# ------------------------------------------------------------------ further cases
def test_a_view_from_outside(mcrt, ctx, dev):
    """a picture three times as wide as the block: whole rays miss it -- out 0, depth -1 -- and the others see it"""
    block = (17, 13, 11)
    g = rm.case_grid(mcrt, block)
    L2 = 2.0 * rm.half_diagonal(g)
    for d in rm.DIRECTIONS:
        view = mcrt.render_view(g, d, rm.UP, 3.0 * L2 / 24, L2 / 36, 24, 20)
        missed = ~rm.coverage(view, block[::-1]).any(axis=0)
        assert missed.mean() > 0.3 and (~missed).sum() > 20
        for in_u8 in (False, True):
            blocks = blocks_of(block, 1, in_u8, seed=5)
            for mode in ("mip", "mean", "surface"):
                got = run(ctx, dev, blocks, view, mode=mode)
                same(got, rm.render_frames(blocks, view, rm.defaults(in_u8, mode=mode)), "outside, dir %s %s" % (d, mode))
                assert np.all(got[0][0][missed] == 0) and np.all(got[1][0][missed] == 0) and np.all(got[2][0][missed] == -1)
                assert (got[0][0][~missed] > 0).any()
    # a view that sees nothing at all: the block lies behind the camera's last step
    view = mcrt.render_view(g, (0, 0, 1), rm.UP, L2 / 24, L2 / 36, 24, 20)
    view.origin[2] = 500.0
    got = run(ctx, dev, blocks_of(block, 2, False), view, mode="surface")
    assert np.all(got[0] == 0) and np.all(got[1] == 0) and np.all(got[2] == -1)


@pytest.mark.parametrize("n_steps", [1, 2])
def test_one_and_two_steps(mcrt, ctx, dev, n_steps):
    """n_steps = 1 has inv_steps = 0: no depth cueing; the rays start inside the block"""
    block = (17, 13, 11)
    for d in rm.DIRECTIONS:
        view = rm.case_view(mcrt, block, d, (33, 35))
        for c in range(3):
            view.origin[c] = float(f32(view.origin[c]) + f32(17.0) * f32(view.ds[c]))      # near the middle of the 37 steps
        view.n_steps = n_steps
        assert rm.coverage(view, block[::-1]).mean() > 0.5
        for in_u8 in (False, True):
            blocks = blocks_of(block, 3, in_u8, seed=n_steps)
            for mode in ("mip", "mean", "surface"):
                same(run(ctx, dev, blocks, view, mode=mode, depth_cue=1.0), rm.render_frames(blocks, view, rm.defaults(in_u8, mode=mode, depth_cue=1.0)),
                     "%d steps dir %s %s" % (n_steps, d, mode))


def test_the_early_stop(mcrt, ctx, dev):
    """t_cut = 0 never stops; t_cut = 0.1 stops a ray once a tenth of the light is left, which changes bits exactly where the mirror says:
    on rays that still had something to add"""
    block = (40, 48, 24)
    blocks = blocks_of(block, 1, True, seed=9)
    view = rm.case_view(mcrt, block, rm.DIRECTIONS[2], (33, 35))
    opts = dict(mode="surface", threshold=0.3, ramp=0.5, opacity=0.6)
    full = run(ctx, dev, blocks, view, t_cut=0.0, **opts)
    cut = run(ctx, dev, blocks, view, t_cut=0.1, **opts)
    same(full, rm.render_frames(blocks, view, rm.defaults(True, t_cut=0.0, **opts)), "t_cut 0")
    same(cut, rm.render_frames(blocks, view, rm.defaults(True, t_cut=0.1, **opts)), "t_cut 0.1")
    changed = full[0] != cut[0]
    assert changed.any() and not changed.all() and np.all(cut[0][changed] < full[0][changed])
    assert np.array_equal(full[2], cut[2])                          # the surface (T <= 0.5) lies in front of the stop (T < 0.1)


def test_a_hand_filled_view(mcrt, ctx, dev):
    """twelve arbitrary finite floats: axes that are neither orthogonal nor of one length, a step that is not perpendicular to the picture"""
    block = (33, 35, 5)
    view = mcrt.RenderView()
    for name, val in (("origin", (-3.3, 36.1, -1.7)), ("di", (0.71, -0.37, 0.045)), ("dj", (0.29, -0.9, 0.11)), ("ds", (0.33, 0.12, 0.21))):
        for c in range(3):
            getattr(view, name)[c] = val[c]
    view.nx, view.ny, view.n_steps = 47, 31, 29
    assert rm.coverage(view, block[::-1]).mean() > 0.3
    for in_u8 in (False, True):
        blocks = blocks_of(block, 2, in_u8, seed=11)
        for mode in ("mip", "mean", "surface"):
            same(run(ctx, dev, blocks, view, mode=mode), rm.render_frames(blocks, view, rm.defaults(in_u8, mode=mode)), "hand-filled %s" % mode)
    # a view whose floats overflow on the way (inf - inf): those rays are not covered, nothing is read
    view.di[0] = 3e38; view.dj[0] = -3e38
    view.origin[0] = 2.0; view.origin[1] = 20.0; view.origin[2] = -1.0
    blocks = blocks_of(block, 1, False, seed=12)
    got = run(ctx, dev, blocks, view, mode="mean")
    same(got, rm.render_frames(blocks, view, rm.defaults(False, mode="mean")), "overflowing view")
    assert got[0][0, 0, 0] > 0 and got[0][0, 1, 1] > 0 and np.all(got[0][0, 2:, 2:] == 0)


def test_a_pass_equals_single_calls(mcrt, ctx, dev):
    block = (17, 13, 11)
    F = 5
    view = rm.case_view(mcrt, block, rm.DIRECTIONS[3], (33, 35))
    for in_u8 in (False, True):
        blocks = blocks_of(block, F, in_u8, seed=13)
        p = dev.upload(blocks)
        for mode in ("mip", "mean", "surface"):
            got = run(ctx, dev, blocks, view, vol=p, mode=mode)
            for f in range(F):
                one = run(ctx, dev, blocks[f:f + 1], view, vol=p + f * blocks[0].nbytes, mode=mode)
                same([x[f:f + 1] for x in got], one, "frame %d %s" % (f, mode))
    # each output alone: the other two pointers null
    blocks = blocks_of(block, 2, False, seed=14)
    want = run(ctx, dev, blocks, view, mode="surface")
    n = 2 * view.nx * view.ny
    p = dev.upload(blocks)
    for k, (name, dt) in enumerate((("out_dev", f32), ("out8_dev", np.uint8), ("depth_dev", f32))):
        q = dev.upload(np.zeros(n, dt))
        ctx.render_frames(p, 2, blocks.shape[1:], view, mode="surface", **{name: q})
        assert np.array_equal(ctx.d2h(q, want[k].shape, dt), want[k]), name


def test_the_row_tile_writes_the_same_pictures(mcrt, dev):
    """k_render's other lane layout -- a wavefront owning 64 pixels of one picture row (MCRT_RENDER_ROW_TILE=1, read when a context is made)
    in place of an 8 x 8 tile -- against the mirror: the table's pictures and two whose width is no multiple of 64 and whose height is no
    multiple of 8 (130 x 11: three wavefronts per row, the last with 2 pixels; 65 x 9)"""
    saved = os.environ.get("MCRT_RENDER_ROW_TILE")
    os.environ["MCRT_RENDER_ROW_TILE"] = "1"                        # (MCRT_TUNING=1 is the suite's: conftest.py)
    try:
        row = mcrt.Context(0)
    finally:
        if saved is None:
            del os.environ["MCRT_RENDER_ROW_TILE"]
        else:
            os.environ["MCRT_RENDER_ROW_TILE"] = saved
    try:
        rdev = Dev(row)
        try:
            for block in ((17, 13, 11), (40, 48, 24)):
                for d, pic in zip(rm.DIRECTIONS, rm.PICTURES + [(130, 11)]):
                    for in_u8 in (False, True):
                        view = rm.case_view(mcrt, block, d, pic)
                        blocks = blocks_of(block, 2, in_u8, seed=21)
                        for mode in ("mip", "mean", "surface"):
                            same(run(row, rdev, blocks, view, mode=mode), rm.render_frames(blocks, view, rm.defaults(in_u8, mode=mode)),
                                 "row tile: block %s dir %s picture %s u8 %d %s" % (block, d, pic, in_u8, mode))
            view = rm.case_view(mcrt, (17, 13, 11), rm.DIRECTIONS[2], (65, 9))
            blocks = blocks_of((17, 13, 11), 3, False, seed=22)
            got = run(row, rdev, blocks, view, mode="surface", t_cut=0.1, opacity=0.6)
            same(got, rm.render_frames(blocks, view, rm.defaults(False, mode="surface", t_cut=0.1, opacity=0.6)), "row tile, 65 x 9")
            assert (got[0] > 0).sum() > 100
        finally:
            rdev.close()
    finally:
        row.close()


# ------------------------------------------------------------------ errors
def test_errors_leave_the_outputs_untouched(mcrt, ctx, dev):
    nu, nv, nw = 6, 5, 4
    block = rm.float_block((nw, nv, nu))
    p = dev.upload(block)
    good_v = mcrt.render_view(mcrt.volume_grid((0, 0, 0), (0.5, 0, 0), (0, 0.5, 0), (0, 0, 0.5), nu, nv, nw), (0.3, 0.2, 1), rm.UP, 0.4, 0.3, 8, 7)
    n = 56
    img = np.full(n, FILL, f32); o = dev.upload(img); d = dev.upload(img)
    bytes_ = np.full(n, FILL8, np.uint8); o8 = dev.upload(bytes_)
    L, vp = ctx.L, C.c_void_p
    nan, inf = math.nan, math.inf

    def call(h=ctx.h, vol=p, in_u8=0, F=1, u=nu, v=nv, w=nw, view=good_v, opts=None, out=o, out8=o8, depth=d):
        return L.mcrt_render_frames(h, vp(vol) if vol else None, in_u8, F, u, v, w, C.byref(view) if view is not None else None,
                                    C.byref(opts) if opts is not None else None, vp(out) if out else None, vp(out8) if out8 else None, vp(depth) if depth else None)

    def view(**kw):
        v = mcrt.RenderView.from_buffer_copy(bytes(good_v))
        for k, val in kw.items():
            if isinstance(val, tuple):
                getattr(v, k)[val[0]] = val[1]
            else:
                setattr(v, k, val)
        return v

    def err(rc, word, **kw):
        assert call(**kw) == rc and word in L.mcrt_last_error(), (kw, L.mcrt_last_error())

    err(INVALID, b"null context", h=None)
    err(INVALID, b"vol_dev", vol=None); err(INVALID, b"view", view=None)
    err(INVALID, b"all null", out=None, out8=None, depth=None)
    for kw in (dict(F=0), dict(u=0), dict(v=0), dict(w=0), dict(view=view(nx=0)), dict(view=view(ny=0))):
        err(INVALID, b"zero", **kw)
    for field in ("origin", "di", "dj", "ds"):
        for c, bad in ((0, nan), (1, inf), (2, -inf)):
            err(INVALID, b"not finite", view=view(**{field: (c, bad)}))
    for kw, word in ((dict(mode=3), b"mode"), (dict(lo=1.0, hi=1.0), b"hi"), (dict(lo=2.0, hi=1.0), b"hi"), (dict(hi=inf), b"hi"), (dict(lo=nan), b"lo"),
                     (dict(threshold=1.0), b"threshold"), (dict(threshold=-0.1), b"threshold"), (dict(threshold=nan), b"threshold"), (dict(ramp=0.0), b"ramp"),
                     (dict(ramp=1.5), b"ramp"), (dict(ramp=nan), b"ramp"), (dict(opacity=0.0), b"opacity"), (dict(opacity=1.01), b"opacity"), (dict(opacity=nan), b"opacity"),
                     (dict(depth_cue=-0.1), b"depth_cue"), (dict(depth_cue=1.1), b"depth_cue"), (dict(depth_cue=nan), b"depth_cue"), (dict(t_cut=1.0), b"t_cut"),
                     (dict(t_cut=-0.5), b"t_cut"), (dict(t_cut=nan), b"t_cut")):
        err(INVALID, word, opts=mcrt.render_opts_struct(False, **kw))
    # a window or a ramp so narrow that its reciprocal is no finite float (a subnormal width)
    err(INVALID, b"narrow", opts=mcrt.render_opts_struct(False, lo=0.0, hi=1e-40)); err(INVALID, b"ramp", opts=mcrt.render_opts_struct(False, ramp=1e-40))
    # an output inside the block, on its last bytes, ending just inside its start -- each of the three outputs
    for name in ("out", "out8", "depth"):
        for q in (p, p + block.nbytes - 1, p - 4):
            err(INVALID, b"overlap", **{name: q})
    err(LIMIT, b"n_steps", view=view(n_steps=0)); err(LIMIT, b"n_steps", view=view(n_steps=4097))
    err(LIMIT, b"2^24", u=1 << 24, v=1, w=1); err(LIMIT, b"2^24", u=1, v=1 << 24, w=1); err(LIMIT, b"2^24", u=1, v=1, w=0xFFFFFFFF)
    err(LIMIT, b"voxels", u=1 << 11, v=1 << 10, w=1 << 10); err(LIMIT, b"voxels", u=(1 << 24) - 1, v=(1 << 24) - 1, w=(1 << 24) - 1)
    err(LIMIT, b"pixels", view=view(nx=1 << 16, ny=1 << 15)); err(LIMIT, b"pixels", view=view(nx=0xFFFFFFFF, ny=0xFFFFFFFF))
    err(LIMIT, b"65535", F=65536)
    ctx.synchronize()
    assert np.array_equal(ctx.d2h(o, (n,)).view(np.uint32), img.view(np.uint32)) and np.array_equal(ctx.d2h(d, (n,)).view(np.uint32), img.view(np.uint32))
    assert np.array_equal(ctx.d2h(o8, (n,), np.uint8), bytes_)
    ic.assert_same_bits(ctx.d2h(p, block.shape), block, "the block")
    # the context still works; null options are the defaults of the input form
    assert call() == 0 and call(view=view(n_steps=4096)) == 0 and call() == 0
    ctx.synchronize()
    want = rm.render(block, good_v, rm.defaults(False))
    ic.assert_same_bits(ctx.d2h(o, (7, 8)), want[0], "after the errors"); ic.assert_same_bits(ctx.d2h(d, (7, 8)), want[2], "after the errors")
    assert np.array_equal(ctx.d2h(o8, (7, 8), np.uint8), want[1])
    b8 = rm.byte_block((nw, nv, nu)); p8 = dev.upload(b8)
    assert call(vol=p8, in_u8=1) == 0
    assert np.array_equal(ctx.d2h(o8, (7, 8), np.uint8), rm.render(b8, good_v, rm.defaults(True))[1])


# ------------------------------------------------------------------ end to end: a traced scene
E2E = dict(E=16, S=8, K=8, step=0.05, pivot=10.0, frame=3)
BOX = dict(origin=(-30.0, 105.0, -17.5), voxel=2.5, n=(25, 19, 15))          # the bone sphere (20 mm about y = 135 mm) inside the swept region
LOOK = dict(direction=(0.25, 1.0, 0.15), size=(40, 32), pixel_mm=2.0, step_mm=2.0)


def _box_grid(mcrt, b=BOX):
    v = b["voxel"]
    return mcrt.volume_grid(b["origin"], (v, 0, 0), (0, v, 0), (0, 0, v), *b["n"])


def _write_scene(mcrt, tmp_path):
    cfg, meshes = mcrt.synth.sphere_scene(3)
    cfg["workingDirectory"] = str(tmp_path) + "/"
    for f, (V, F) in meshes.items():
        mcrt.scene_io.save_obj(str(tmp_path / f), V, F)
    (tmp_path / "sphere.scene").write_text(json.dumps(cfg))
    return cfg, str(tmp_path / "sphere.scene")


def test_a_traced_scene_end_to_end(mcrt, tmp_path):
    """Simulator.render is the mirror fed with bmode_volume's bytes, in every mode; the sphere is in the MIP picture; the C++ shim writes
    the same bytes"""
    cfg, scene = _write_scene(mcrt, tmp_path)
    e = E2E
    tr = mcrt.Transducer(e["E"], position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    g = _box_grid(mcrt)
    sim = mcrt.Simulator(mcrt.scene_io.load_scene_file(scene), tr, n_samples=e["S"], sweep=(e["K"], e["step"]), sweep_pivot_mm=e["pivot"])
    pics = {}
    try:
        voxels = sim.bmode_volume(e["frame"], g)
        assert len(np.unique(voxels)) > 20
        view = mcrt.render_view(g, LOOK["direction"], (0, 0, 1), LOOK["pixel_mm"], LOOK["step_mm"], *LOOK["size"])
        assert (rm.coverage(view, voxels.shape).mean(axis=0) >= 0.25).mean() > 0.5
        for mode in ("mip", "mean", "surface"):
            pics[mode] = sim.render(e["frame"], g, mode=mode, **LOOK)
            assert pics[mode].shape == (LOOK["size"][1], LOOK["size"][0]) and pics[mode].dtype == np.uint8
            assert np.array_equal(pics[mode], rm.render(voxels, view, rm.defaults(True, mode=mode))[1]), mode
        # options reach both stages: another dynamic range changes the voxels, another threshold the surface
        other = sim.render(e["frame"], g, mode="surface", dynamic_range_db=40.0, threshold=0.5, **LOOK)
        v40 = sim.bmode_volume(e["frame"], g, dynamic_range_db=40.0)
        assert np.array_equal(other, rm.render(v40, view, rm.defaults(True, mode="surface", threshold=0.5))[1]) and not np.array_equal(other, pics["surface"])
        # looking straight down the depth axis, the bone sphere fills the middle of the maximum-intensity picture
        # (the picture is the block's own x-z face, 60 x 35 mm: no corner looks past the block)
        mip = sim.render(e["frame"], g, (0, 1, 0), size=(24, 14), pixel_mm=2.5, step_mm=2.5, mode="mip").astype(np.float64)
        centre = mip[3:11, 6:18].mean()
        corners = np.concatenate([mip[:3, :6].ravel(), mip[:3, 18:].ravel(), mip[11:, :6].ravel(), mip[11:, 18:].ravel()]).mean()
        print("MIP along the depth axis: central quarter %.1f, corners %.1f" % (centre, corners))
        assert centre > corners
    finally:
        sim.close()
    plain = mcrt.Simulator(mcrt.scene_io.load_scene_file(scene), tr, n_samples=e["S"])
    try:
        with pytest.raises(RuntimeError):
            plain.render(0, g, (0, 1, 0))
    finally:
        plain.close()
    # the C++ shim: rf_image::render after trace(frame, transducer, sweep)
    pkg = os.path.join(ROOT, "mcray-tracing_amd")
    exe = str(tmp_path / "render_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(pkg, "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "render_driver.cpp"), "-L", pkg, "-lmcrt_hip", "-Wl,-rpath," + pkg])
    out = tmp_path / "render.bin"
    args = [scene, str(out), e["frame"], e["S"], e["K"], repr(e["step"]), repr(e["pivot"])] + [repr(x) for x in BOX["origin"]] + [repr(BOX["voxel"])] + list(BOX["n"]) + \
           [repr(x) for x in LOOK["direction"]] + [repr(LOOK["pixel_mm"]), repr(LOOK["step_mm"])] + list(LOOK["size"])
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = np.frombuffer(out.read_bytes(), np.uint8)
    npix = LOOK["size"][0] * LOOK["size"][1]
    assert raw.size == 3 * npix
    for k, mode in enumerate(("mip", "mean", "surface")):
        assert np.array_equal(raw[k * npix:(k + 1) * npix].reshape(pics[mode].shape), pics[mode]), mode
    assert len(np.unique(pics["mip"])) > 10


def test_cli_render_options(mcrt, tmp_path):
    exe = os.path.join(ROOT, "mcray-tracing_amd", "mattausch_hip")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "mcray-tracing_amd"), "mattausch_hip"])
    cfg, scene = _write_scene(mcrt, tmp_path)
    K, step_deg, pivot = 5, 2.0, 10.0
    sweep = ["--sweep", str(K), "--sweep-step-deg", repr(step_deg), "--sweep-pivot-mm", repr(pivot)]
    render = ["--render", "0.25,1,0.15", "--render-box-mm", "-30,105,-7.5,30,150,7.5", "--render-voxel-mm", "2.5"]
    pgm = tmp_path / "render.pgm"
    r = subprocess.run([exe, scene, "2", "5", str(pgm)] + sweep + render + ["--render-mode", "mip", "--render-size", "40,24", "--db", "50"], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = pgm.read_bytes()
    head = b"P5\n40 24\n255\n"
    assert raw.startswith(head) and len(raw) == len(head) + 960
    tr = mcrt.Transducer(512, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    sim = mcrt.Simulator(mcrt.scene_io.load_scene_file(scene), tr, n_samples=5, sweep=(K, float(f32(step_deg * math.pi / 180.0))), sweep_pivot_mm=pivot)
    try:
        g = mcrt.volume_grid((-30, 105, -7.5), (2.5, 0, 0), (0, 2.5, 0), (0, 0, 2.5), 25, 19, 7)
        want = sim.render(1, g, (0.25, 1, 0.15), size=(40, 24), pixel_mm=2.5, step_mm=2.5, mode="mip", dynamic_range_db=50.0)      # the last of the run's two frames
    finally:
        sim.close()
    assert np.array_equal(np.frombuffer(raw, np.uint8, 960, len(head)).reshape(24, 40), want)
    assert len(np.unique(want)) > 10
    for bad, word in ((render, "need --sweep"), (["--render-mode", "mip"], "need --sweep"), (["--render-box-mm", "-30,105,-7.5,30,150,7.5"], "need --sweep"),   # without --sweep
                      (sweep + ["--render", "0,1,0"], "needs --render-box-mm"), (sweep + ["--render", "0,1,0", "--render-voxel-mm", "2.5"], "needs --render-box-mm"),
                      (sweep + render + ["--cplane-mm", "80"], "one of --cplane-mm"), (sweep + render + ["--render-mode", "xray"], "takes mip, mean or surface"),
                      (sweep + ["--render", "0,0,0"] + render[2:], "dir_mm"), (sweep + ["--render", "0,1"] + render[2:], "takes DX,DY,DZ"),
                      (sweep + render[:4] + ["--render-voxel-mm", "0"], "--render-voxel-mm (with --sweep --render) must be > 0"),
                      (sweep + render + ["--render-size", "0,4"], "two positive numbers"), (sweep + ["--render-mode", "mip", "--cplane-mm", "80"], "need --render (with --sweep)"),
                      (sweep + render + ["--labels", str(tmp_path / "l.pgm")], "--labels does not combine")):
        r = subprocess.run([exe, scene, "1", "5"] + bad, capture_output=True, text=True, timeout=240)
        assert r.returncode == 1 and "--sweep" in r.stdout and word in r.stdout, (bad, word, r.stdout)
