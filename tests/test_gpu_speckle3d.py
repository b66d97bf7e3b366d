"""mcrt_speckle_volume_frames on the MI355X: k_srad3 against the numpy mirror of the contract (tests/speckle3d_mirror.py) fed with the product's
own table floats, bit for bit, with the outputs pre-filled so that an unwritten voxel shows -- at the blocks where a tile edge, an in-plane
ring or a chunk seam of the march can go wrong, at even and odd launch counts, in place and out of place, one block and two, every set of
weights; against mcrt_speckle_frames on the device at weights (1, 1, 0); the argument errors; a traced scene through the Simulator, the
C++ shim and mattausch_hip; the recipe for a smoothed surface."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest

import image_cases as ic
import recon_mirror as rcm
import render_mirror as rm
import speckle_mirror as sm
import speckle3d_mirror as s3
from test_gpu_focus import Dev
from test_gpu_recon import _cli_poses, _write_scene

pytestmark = pytest.mark.gpu

f32 = np.float32
INVALID, LIMIT = -1, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mcray-tracing_amd")
_HDR = open(os.path.join(PKG, "csrc", "mcrt_kernels.h")).read()
TV, TU, CW = (int(re.search(r"#define SRAD3_%s (\d+) " % n, _HDR).group(1)) for n in ("TV", "TU", "CW"))      # k_srad3's tile and chunk
SHAPES = [(1, 1, 1), (1, 1, 37), (1, 37, 1), (37, 1, 1), (2, 2, 2), (3, 5, 300), (5, 300, 3)] + \
         [(3, v, u) for v in (TV - 1, TV, TV + 1, 2 * TV + 1) for u in (TU - 1, TU, TU + 1, 2 * TU + 1)] + \
         [(w, TV + 1, TU + 1) for w in (CW - 1, CW, CW + 1, 2 * CW + 1)]                                        # (nw, nv, nu)
N_ITER = (1, 2, 3, 20)          # even and odd launch counts
WEIGHTS = [(1, 1, 1), (1, 1, 0), (1, 0.25, 0.0625), (0, 0, 1)]
FILL = f32(-777.25)             # outputs are pre-filled: a voxel that is not written shows


def test_the_tile_is_the_kernels():
    """the shapes above follow the kernel's constants; the tile is a workgroup's 256 lanes times a whole number of voxels, and the window
    of four slices of X and two of c is what the kernel's comment says"""
    assert TV >= 1 and TU >= 1 and CW >= 1 and (TV * TU) % 256 == 0
    assert 6 * (TV + 3) * (TU + 3) * 4 <= 64 * 1024
    src = open(os.path.join(PKG, "csrc", "mcrt_speckle3d.hip")).read()
    assert "SRAD3_TV" in src and "SRAD3_TU" in src and "SRAD3_CW" in src and "sx[4]" in src and "sc[2]" in src


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


def stack(F, shape, seed=0):
    """[F][nw][nv][nu]: the generator of tests/test_gpu_speckle.py with one axis more -- speckle with both signs, a flat zero patch, exact
    zeros, -0.0, NaN and +-inf"""
    nw, nv, nu = shape
    rng = np.random.default_rng(4000 + 131 * nv + nu + 7919 * nw + seed)
    x = (rng.rayleigh(1.0, (F,) + shape) * np.where(rng.random((F,) + shape) < 0.3, -1.0, 1.0) * (1.0 + 3.0 * (rng.random((F, 1, 1, 1)) < 0.5))).astype(f32)
    x[:, nw // 3:nw // 3 + 2, nv // 3:nv // 3 + 4, nu // 4:nu // 4 + 5] = 0.0
    flat = x.reshape(F, -1)
    n = flat.shape[1]
    if n >= 6:
        vals = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-30], f32)
        for f in range(F):
            k = max(len(vals), n // 40)
            idx = rng.permutation(n)[:k]
            flat[f, idx] = np.resize(vals, k)
    return x


_WANT = {}


def want(mcrt, x, key=None, **opts):
    """the mirror's answer for x with the product's table floats; with a key, computed once, shared and left unchanged"""
    k = None if key is None else (key, x.shape, tuple(sorted((a, tuple(b) if a == "weights" else b) for a, b in opts.items())))
    if k is None or k not in _WANT:
        o = mcrt.speckle3d_opts_struct(**opts)
        y = s3.srad3(x, *mcrt.host_speckle3d_tables(o), tuple(o.weight))
        if k is None:
            return y
        y.setflags(write=False)
        _WANT[k] = y
    return _WANT[k]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_shapes_and_iteration_counts(mcrt, ctx, shape):
    """every shape at every iteration count: two blocks out of place, the first alone (the second stays untouched), and the two in place"""
    d = Dev(ctx)
    try:
        x = stack(2, shape)
        src = d.upload(x); out = d(x.nbytes); inp = d(x.nbytes)
        fill = np.full(x.shape, FILL)
        for n_iter in N_ITER:
            w = want(mcrt, x, "shapes", n_iter=n_iter)
            ctx.h2d(out, fill)
            ctx.speckle_volume_frames(src, 2, shape, out, n_iter=n_iter)
            ctx.synchronize()
            ic.assert_same_bits(ctx.d2h(out, x.shape), w, "out of place, F = 2, n_iter %d" % n_iter)
            ctx.h2d(out, fill)
            ctx.speckle_volume_frames(src, 1, shape, out, n_iter=n_iter)
            ctx.synchronize()
            got = ctx.d2h(out, x.shape)
            ic.assert_same_bits(got[0], w[0], "out of place, F = 1, n_iter %d" % n_iter)
            assert (got[1] == FILL).all(), "F = 1 wrote past its block"
            ctx.h2d(inp, x)
            ctx.speckle_volume_frames(inp, 2, shape, n_iter=n_iter)
            ctx.synchronize()
            ic.assert_same_bits(ctx.d2h(inp, x.shape), w, "in place, F = 2, n_iter %d" % n_iter)
        ic.assert_same_bits(ctx.d2h(src, x.shape), x, "the input of the out-of-place calls")
    finally:
        d.close()


WEIGHT_SHAPES = [(2, 2, 2), (37, 1, 1), (1, 37, 1), (1, 1, 37), (3, TV + 1, TU + 1), (CW + 1, TV + 1, TU + 1)]


@pytest.mark.parametrize("weights", WEIGHTS, ids=lambda w: "w%g_%g_%g" % w)
def test_weights(mcrt, ctx, weights):
    """every set of weights where a tile edge, a ring and a chunk seam meet and on the thin blocks, even and odd launch counts, in place
    and out of place"""
    d = Dev(ctx)
    try:
        for shape in WEIGHT_SHAPES:
            x = stack(2, shape, seed=1)
            src = d.upload(x); out = d.upload(np.full(x.shape, FILL)); inp = d(x.nbytes)
            for n_iter in (2, 3):
                w = want(mcrt, x, n_iter=n_iter, weights=weights)
                ctx.speckle_volume_frames(src, 2, shape, out, n_iter=n_iter, weights=weights)
                ctx.h2d(inp, x)
                ctx.speckle_volume_frames(inp, 2, shape, n_iter=n_iter, weights=weights)
                ctx.synchronize()
                ic.assert_same_bits(ctx.d2h(out, x.shape), w, "%s out of place, n_iter %d" % (shape, n_iter))
                ic.assert_same_bits(ctx.d2h(inp, x.shape), w, "%s in place, n_iter %d" % (shape, n_iter))
    finally:
        d.close()


@pytest.mark.parametrize("shape", [(3, TV + 1, TU + 1), (CW + 1, 5, 9), (1, 2 * TV + 1, 2 * TU + 1)], ids=lambda s: "%dx%dx%d" % s)
def test_weights_1_1_0_are_speckle_frames_on_the_device(mcrt, ctx, dev, shape):
    """weight (1, 1, 0): the block equals Context.speckle_frames over it as nw frames of [nv][nu], device against device, bit for bit -- and
    both equal the 2-D mirror"""
    nw, nv, nu = shape
    x = stack(2, shape, seed=2)
    src = dev.upload(x); a = dev(x.nbytes); b = dev(x.nbytes)
    for n_iter, lam in ((1, 0.5), (2, 1.0), (5, 0.5), (20, 0.5)):
        ctx.h2d(a, np.full(x.shape, FILL)); ctx.h2d(b, np.full(x.shape, FILL))
        ctx.speckle_volume_frames(src, 2, shape, a, n_iter=n_iter, lambda_=lam, weights=(1, 1, 0))
        ctx.speckle_frames(src, 2 * nw, nv, nu, b, n_iter=n_iter, lambda_=lam)
        ctx.synchronize()
        got3, got2 = ctx.d2h(a, x.shape), ctx.d2h(b, x.shape)
        ic.assert_same_bits(got3, got2, "k_srad3 at (1, 1, 0) against k_srad, n_iter %d" % n_iter)
        ic.assert_same_bits(got3, sm.srad(x, *mcrt.host_speckle_tables(n_iter=n_iter, lambda_=lam)), "against the 2-D mirror, n_iter %d" % n_iter)


def test_blocks_off_a_16_byte_boundary(mcrt, ctx, dev):
    """input and output 4, 8 and 12 bytes off a 16-byte boundary, each way round; the floats around the output stay as they were"""
    shape = (3, TV + 1, TU + 1)
    x = stack(1, shape, seed=3)
    n = x.size
    w = want(mcrt, x, n_iter=3)
    src = dev(x.nbytes + 64); out = dev(x.nbytes + 64)
    assert src % 16 == 0 and out % 16 == 0
    for off_in, off_out in ((4, 0), (8, 8), (12, 4), (0, 12)):
        ctx.h2d(src + off_in, x)
        ctx.h2d(out, np.full(n + 16, FILL))
        ctx.speckle_volume_frames(src + off_in, 1, shape, out + off_out, n_iter=3)
        ctx.synchronize()
        got = ctx.d2h(out, (n + 16,))
        ic.assert_same_bits(got[off_out // 4:off_out // 4 + n].reshape(x.shape), w, "offsets %d, %d" % (off_in, off_out))
        assert (got[:off_out // 4] == FILL).all() and (got[off_out // 4 + n:] == FILL).all(), (off_in, off_out)
    ctx.h2d(src + 4, x)
    ctx.speckle_volume_frames(src + 4, 1, shape, n_iter=3)
    ctx.synchronize()
    ic.assert_same_bits(ctx.d2h(src + 4, x.shape), w, "in place, 4 bytes off")


def test_other_options_and_n_iter_zero(mcrt, ctx, dev):
    """options away from the defaults (lambda = 1; q0 = 1 with no decay; 256 iterations on a small block), and n_iter = 0: the input's bits,
    untouched in place"""
    shape = (5, 9, 20)
    x = stack(2, shape, seed=4)
    src = dev.upload(x); out = dev(x.nbytes)
    for opts in (dict(n_iter=5, lambda_=1.0), dict(n_iter=7, q0=1.0, rho=0.0, lambda_=0.25, weights=(1, 0.25, 0.0625)), dict(n_iter=256, q0=2.0, rho=0.01)):
        ctx.h2d(out, np.full(x.shape, FILL))
        ctx.speckle_volume_frames(src, 2, shape, out, **opts)
        ctx.synchronize()
        ic.assert_same_bits(ctx.d2h(out, x.shape), want(mcrt, x, **opts), str(opts))
    ctx.h2d(out, np.full(x.shape, FILL))
    ctx.speckle_volume_frames(src, 2, shape, out, n_iter=0)
    ctx.synchronize()
    ic.assert_same_bits(ctx.d2h(out, x.shape), x, "n_iter = 0, out of place")
    ctx.speckle_volume_frames(src, 2, shape, n_iter=0)
    ctx.synchronize()
    ic.assert_same_bits(ctx.d2h(src, x.shape), x, "n_iter = 0, in place")


def test_the_scratch_is_shared_with_convolve_and_only_grows(mcrt, ctx, dev):
    """a large block after a small one, a convolution and a 2-D filter between two calls: the ping-pong buffer is the context's scratch"""
    small, large = stack(2, (3, 5, 9)), stack(2, (7, 20, 70))
    for x in (small, large, small):
        p = dev.upload(x)
        ctx.speckle_volume_frames(p, 2, x.shape[1:], n_iter=5)
        ctx.synchronize()
        ic.assert_same_bits(ctx.d2h(p, x.shape), want(mcrt, x, n_iter=5), str(x.shape))
        q = dev.upload(np.ones((3, 64, 128), f32))
        ctx.convolve_frames(q, 3, 64, 128, np.ones(3, f32), np.ones(3, f32))
        ctx.speckle_frames(q, 3, 64, 128, n_iter=3)


def test_errors_leave_out_dev_untouched(mcrt, ctx, dev):
    L = ctx.L
    shape = (4, 9, 20)
    nw, nv, nu = shape
    x = stack(2, shape, seed=5)
    src = dev.upload(x)
    fill = np.full(x.shape, FILL)
    out = dev.upload(fill)
    good = mcrt.speckle3d_opts_struct(n_iter=3)

    def call(h=ctx.h, i=src, F=2, u=nu, v=nv, w=nw, o=good, out_=out):
        return L.mcrt_speckle_volume_frames(h, C.c_void_p(i) if i else None, F, u, v, w, C.byref(o) if o is not None else None, C.c_void_p(out_) if out_ else None)

    def err(code, word, **kw):
        assert call(**kw) == code, kw
        assert word in L.mcrt_last_error() and (b"mcrt_speckle" in L.mcrt_last_error() or kw.get("h", 1) is None), (kw, L.mcrt_last_error())

    err(INVALID, b"null context", h=None)
    err(INVALID, b"in_dev", i=None); err(INVALID, b"out_dev", out_=None)
    err(INVALID, b"zero", F=0); err(INVALID, b"zero", u=0); err(INVALID, b"zero", v=0); err(INVALID, b"zero", w=0)
    for opts, code, word in ((dict(n_iter=257), LIMIT, b"n_iter"), (dict(q0=0.0), INVALID, b"q0"), (dict(q0=np.nan), INVALID, b"q0"), (dict(rho=-1.0), INVALID, b"rho"),
                             (dict(rho=np.inf), INVALID, b"rho"), (dict(lambda_=0.0), INVALID, b"lambda"), (dict(lambda_=1.5), INVALID, b"lambda"),
                             (dict(n_iter=256, rho=1.0), INVALID, b"iteration"), (dict(weights=(1, -1, 1)), INVALID, b"weight[1]"),
                             (dict(weights=(1, 1, np.nan)), INVALID, b"weight[2]"), (dict(weights=(np.inf, 1, 1)), INVALID, b"weight[0]"),
                             (dict(weights=(0, 0, 0)), INVALID, b"sum"), (dict(weights=(1e-30, 0, 0)), INVALID, b"weight")):
        err(code, word, o=mcrt.speckle3d_opts_struct(**opts))
    err(LIMIT, b"2^24", F=1, u=1 << 24, v=1, w=1); err(LIMIT, b"2^24", F=1, u=1, v=1 << 24, w=1); err(LIMIT, b"2^24", F=1, u=1, v=1, w=1 << 24)
    err(LIMIT, b"2^31", F=2, u=1 << 10, v=1 << 10, w=1 << 10); err(LIMIT, b"2^31", F=0xFFFFFFFF, u=0xFFFFFF, v=0xFFFFFF, w=0xFFFFFF)
    # any overlap but the same buffer: a stack that starts one float, or one block, into the other
    big = dev.upload(np.concatenate([fill, fill]))
    err(INVALID, b"overlap", i=big, out_=big + 4); err(INVALID, b"overlap", i=big + 4 * nw * nv * nu, out_=big)
    ctx.synchronize()
    ic.assert_same_bits(ctx.d2h(out, x.shape), fill, "out_dev after the errors")
    ic.assert_same_bits(ctx.d2h(big, (4,) + shape), np.concatenate([fill, fill]), "the overlapping buffers after the errors")
    ic.assert_same_bits(ctx.d2h(src, x.shape), x, "in_dev after the errors")
    # the context still works; null options are the defaults
    assert call(o=None) == 0
    ctx.synchronize()
    ic.assert_same_bits(ctx.d2h(out, x.shape), want(mcrt, x), "null options")
    # adjacent buffers do not overlap
    ctx.h2d(big, np.concatenate([x, fill]))
    assert call(i=big, out_=big + x.nbytes) == 0
    ctx.synchronize()
    ic.assert_same_bits(ctx.d2h(big, (4,) + shape)[2:], want(mcrt, x, n_iter=3), "adjacent buffers")


# ------------------------------------------------------------------ end to end: a traced scene
def _sweep_grid(mcrt):
    """a block about the sphere: 1 mm along x and y, 2 mm along z -- weights (1, 1, 0.25)"""
    return mcrt.volume_grid((-12.0, 118.0, -4.0), (1.0, 0, 0), (0, 1.0, 0), (0, 0, 2.0), 25, 30, 5)


def test_simulator_volume_and_the_recipe_for_a_smoothed_surface(mcrt, tmp_path):
    """Simulator(speckle3d=...).volume() equals the plain block pushed through Context.speckle_volume_frames by hand and through the
    mirror, with the grid's weights or the dict's, and differs from the plain block; bmode_volume() and render() refuse, saying why; and
    the recipe of DESIGN.md 5.16 -- volume_frames -> speckle_volume_frames -> render_frames(in_u8=False, lo=, hi=) -- equals
    tests/render_mirror.py on the mirror's block"""
    cfg, scene = _write_scene(mcrt, tmp_path)
    sd = mcrt.scene_io.load_scene_file(scene)
    E, S, frame = 16, 8, 3
    tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    g = _sweep_grid(mcrt)
    shape = (g.nw, g.nv, g.nu)
    kw = dict(n_samples=S, sweep=(5, 0.03), sweep_pivot_mm=10.0)
    assert list(mcrt.host_speckle3d_weights(g)) == [1.0, 1.0, 0.25]
    plain = mcrt.Simulator(sd, tr, **kw)
    try:
        assert plain.speckle3d is None
        raw = plain.volume(frame, g)
        assert np.isfinite(raw).all() and len(np.unique(raw)) > 100
        for spk, by_hand in ((True, dict(weights=(1, 1, 0.25))), (dict(n_iter=5, lambda_=1.0), dict(n_iter=5, lambda_=1.0, weights=(1, 1, 0.25))),
                             (dict(n_iter=4, q0=1.0, weights=(1, 0.5, 1)), dict(n_iter=4, q0=1.0, weights=(1, 0.5, 1)))):
            filt = mcrt.Simulator(sd, tr, speckle3d=spk, **kw)
            try:
                got = filt.volume(frame, g)
                with pytest.raises(RuntimeError, match="no float block"):
                    filt.bmode_volume(frame, g)
                with pytest.raises(RuntimeError, match="no float block"):
                    filt.render(frame, g, (0, 1, 0))
            finally:
                filt.close()
            w = want(mcrt, raw, **by_hand)
            ic.assert_same_bits(got, w, "Simulator.volume under speckle3d=%r against the mirror" % (spk,))
            with plain.ctx.temp(raw.nbytes) as buf:
                plain.ctx.h2d(buf, raw)
                plain.ctx.speckle_volume_frames(buf, 1, shape, **by_hand)
                ic.assert_same_bits(plain.ctx.d2h(buf, shape), got, "by hand")
            assert not np.array_equal(got, raw), "the filter changed nothing"
        # the recipe, at Context level
        c = plain.ctx
        plain._run(frame)
        view = mcrt.render_view(g, (0.3, 1.0, 0.2), (0, 0, 1), 1.0, 1.0, 40, 24)
        hi = float(raw.max())
        with c.temp(raw.nbytes) as vox, c.temp(40 * 24 * 4) as pic, c.temp(40 * 24) as pic8:
            c.volume_frames(plain.sweep_dev, 1, E, plain.R, plain.sweep, g, vox)
            c.speckle_volume_frames(vox, 1, shape, weights=mcrt.host_speckle3d_weights(g))
            c.render_frames(vox, 1, shape, view, out_dev=pic, out8_dev=pic8, in_u8=False, mode="surface", lo=0.0, hi=hi)
            got = c.d2h(pic, (24, 40)), c.d2h(pic8, (24, 40), np.uint8)
        block = want(mcrt, raw, weights=(1, 1, 0.25))
        wpic = rm.render(block, view, rm.defaults(False, mode="surface", lo=0.0, hi=float(f32(hi))))
        ic.assert_same_bits(got[0], wpic[0], "the rendered filtered block")
        assert np.array_equal(got[1], wpic[1]) and len(np.unique(got[1])) > 10
    finally:
        plain.close()
    with pytest.raises(TypeError):
        mcrt.Simulator(sd, tr, speckle3d=dict(iterations=3), **kw)


def _freehand_case(mcrt, cfg, E, N, step_mm, fan_deg, voxel):
    """the poses of mattausch_hip --freehand and a box of `voxel` mm about the middle of the swept cloud's first 150 rows"""
    tr, pos, dirs = _cli_poses(mcrt, cfg, E, N, step_mm, fan_deg)
    row_mm = float(f32(f32(100 * 1500) * f32(0.001))) / 465
    cloud = rcm.positions(pos, dirs, 150, f32(row_mm / 10.0)).reshape(-1, 3).astype(np.float64) * 10.0
    mid, half = np.round(cloud.mean(0)), 0.4 * (cloud.max(0) - cloud.min(0))
    lo, hi = mid - np.floor(half), mid + np.floor(half)
    dims = [int(np.floor((hi[i] - lo[i]) / voxel)) + 1 for i in range(3)]
    return tr, pos, dirs, lo, hi, dims, mcrt.volume_grid(lo, (voxel, 0, 0), (0, voxel, 0), (0, 0, voxel), *dims)


def test_simulator_freehand(mcrt, tmp_path):
    """Simulator(speckle3d=...).freehand() equals the plain block through the call by hand and through the mirror; a hole's `empty`
    value is a value like any other (step 0 applies: |empty|), and counts=True still tells which voxels were empty"""
    cfg, scene = _write_scene(mcrt, tmp_path)
    sd = mcrt.scene_io.load_scene_file(scene)
    E, S, N, frame = 16, 5, 6, 1
    tr, pos, dirs, lo, hi, dims, g = _freehand_case(mcrt, cfg, E, N, 1.5, 2.0, 2.0)
    shape = (g.nw, g.nv, g.nu)
    assert list(mcrt.host_speckle3d_weights(g)) == [1.0, 1.0, 1.0] and min(dims) > 2
    plain = mcrt.Simulator(sd, tr, n_samples=S)
    filt = mcrt.Simulator(sd, tr, n_samples=S, speckle3d=dict(n_iter=6))
    try:
        ropts = dict(fill_radius=0, empty=-3.0)
        raw, cnt = plain.freehand(frame, pos, dirs, g, counts=True, **ropts)
        got, cnt2 = filt.freehand(frame, pos, dirs, g, counts=True, **ropts)
        assert np.array_equal(cnt, cnt2) and (cnt == 0).any() and (cnt > 0).sum() > 50 and (raw[cnt == 0] == -3.0).all()
        ic.assert_same_bits(got, want(mcrt, raw, n_iter=6), "Simulator.freehand under speckle3d= against the mirror")
        assert got.min() >= 0.0 and not np.array_equal(got, raw)
        with plain.ctx.temp(raw.nbytes) as buf:
            plain.ctx.h2d(buf, raw)
            plain.ctx.speckle_volume_frames(buf, 1, shape, n_iter=6, weights=mcrt.host_speckle3d_weights(g))
            ic.assert_same_bits(plain.ctx.d2h(buf, shape), got, "by hand")
    finally:
        plain.close(); filt.close()


def test_host_shim(mcrt, tmp_path):
    """rf_image::volume(grid, filter) and rf_image::reconstruct(grid, opts, counts, filter) (tests/host/speckle3d_driver.cpp) write the
    mirror's filter of what the same calls write without the filter"""
    exe = str(tmp_path / "speckle3d_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(PKG, "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "speckle3d_driver.cpp"), "-L", PKG, "-lmcrt_hip", "-Wl,-rpath," + PKG])
    cfg, scene = _write_scene(mcrt, tmp_path)
    E, S, frame, n_iter = 64, 5, 2, 5
    nu, nv, nw, pitch, depth = 25, 30, 5, 1.0, 132.5
    tr, pos, dirs, lo, hi, dims, g = _freehand_case(mcrt, cfg, E, 6, 1.5, 2.0, 2.0)
    box = ",".join("%.17g" % v for v in list(lo) + list(hi))
    out = tmp_path / "blocks.bin"
    r = subprocess.run([exe, scene, str(out), str(frame), str(S), "5", "0.03", "10.0", repr(depth), str(nu), str(nv), str(nw), repr(pitch), str(n_iter),
                        "6", "1.5", "2.0", box, "2.0"], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "%d x %d x %d" % tuple(dims) in r.stdout
    raw = np.fromfile(str(out), f32)
    n, m = nu * nv * nw, dims[0] * dims[1] * dims[2]
    assert raw.size == 2 * n + 2 * m
    plain, smooth = raw[:n].reshape(nw, nv, nu), raw[n:2 * n].reshape(nw, nv, nu)
    fplain, fsmooth = raw[2 * n:2 * n + m].reshape(dims[::-1]), raw[2 * n + m:].reshape(dims[::-1])
    ic.assert_same_bits(smooth, want(mcrt, plain, n_iter=n_iter, weights=(1, 1, 0.25)), "rf_image::volume(grid, filter)")
    ic.assert_same_bits(fsmooth, want(mcrt, fplain, n_iter=n_iter), "rf_image::reconstruct(grid, opts, counts, filter)")
    assert len(np.unique(plain)) > 100 and not np.array_equal(smooth, plain) and len(np.unique(fplain)) > 50 and not np.array_equal(fsmooth, fplain)


def test_cli_speckle3d_options(mcrt, tmp_path):
    """mattausch_hip --speckle3d: the --freehand-out volume equals the mirror's filter of the volume without the option; each bad option
    ends the program with status 1, naming the option"""
    exe = os.path.join(PKG, "mattausch_hip")
    subprocess.check_call(["make", "-C", PKG, "mattausch_hip"])
    cfg, scene = _write_scene(mcrt, tmp_path)
    S, N = 5, 6
    tr, pos, dirs, lo, hi, dims, g = _freehand_case(mcrt, cfg, 512, N, 1.5, 2.0, 2.0)
    box = ",".join("%.17g" % v for v in list(lo) + list(hi))
    fh = ["--freehand", str(N), "--freehand-step-mm", "1.5", "--freehand-fan-deg", "2.0", "--freehand-box-mm", box, "--freehand-voxel-mm", "2.0"]
    run = lambda name, *a: subprocess.run([exe, scene, "1", str(S), str(tmp_path / (name + ".pgm")), str(tmp_path / (name + ".bin"))] + fh +
                                          ["--freehand-out", str(tmp_path / (name + ".raw"))] + list(a), capture_output=True, text=True, timeout=240)
    r = run("p")
    assert r.returncode == 0, r.stdout + r.stderr
    r = run("s", "--speckle3d", "5", "--speckle3d-lambda", "1", "--speckle3d-q0", "0.75", "--speckle3d-rho", "0.125")
    assert r.returncode == 0, r.stdout + r.stderr
    plain = np.fromfile(str(tmp_path / "p.raw"), f32).reshape(dims[::-1])
    got = np.fromfile(str(tmp_path / "s.raw"), f32).reshape(dims[::-1])
    ic.assert_same_bits(got, want(mcrt, plain, n_iter=5, lambda_=1.0, q0=0.75, rho=0.125), "--freehand-out under --speckle3d")
    assert len(np.unique(plain)) > 50 and not np.array_equal(got, plain)
    assert (tmp_path / "s.pgm").read_bytes() == (tmp_path / "p.pgm").read_bytes()          # the run's own picture is left alone
    for bad, word in ((["--speckle3d-q0", "0.5"], "need --speckle3d"), (["--speckle3d", "257"], "0..256"), (["--speckle3d", "-1"], "0..256"),
                      (["--speckle3d", "3", "--speckle3d-lambda", "2"], "lambda"), (["--speckle3d", "3", "--speckle3d-q0", "0"], "q0"),
                      (["--speckle3d", "200", "--speckle3d-rho", "2"], "iteration")):
        r = subprocess.run([exe, scene, "1", str(S)] + fh + ["--freehand-out", str(tmp_path / "x.raw")] + bad, capture_output=True, text=True, timeout=240)
        assert r.returncode == 1 and "--speckle3d" in r.stdout and word in r.stdout, (bad, word, r.stdout)
    r = subprocess.run([exe, scene, "1", str(S), "--speckle3d", "3"], capture_output=True, text=True, timeout=240)
    assert r.returncode == 1 and "--speckle3d needs --freehand" in r.stdout, r.stdout
    assert not (tmp_path / "x.raw").exists()
