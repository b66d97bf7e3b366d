"""Freehand 3-D reconstruction without a GPU (include/mcrt.h: mcrt_recon_opts, mcrt_default_recon_opts, mcrt_recon_transform,
mcrt_recon_frames): the struct and its defaults, the host transform against numpy's double inverse, every refusal that needs no device, and
the properties of the numpy mirror (tests/recon_mirror.py) that hold tests/test_gpu_recon.py honest -- the order of the frames leaves
every bit, a constant stack stays that constant, holes are filled from sampled voxels only -- and that the voxels lie where the poses say."""
import ctypes as C
import os
import re
import numpy as np
import pytest

import recon_mirror as rm

f32 = np.float32
INVALID, LIMIT = -1, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sweep_poses(mcrt, F, E, step_cm=0.1, fan_deg=0.0, wobble=True):
    """a hand-held sweep: the probe moved along z (its elevation) in F steps about the origin, tilted a little more at every step, with a
    drift and a roll that no regular wobble has -> (pos [F][E][3], dir [F][E][3]) in cm"""
    k = np.arange(F) - (F - 1) / 2.0
    positions = np.stack([0.03 * np.sin(k) * wobble, 0.02 * np.cos(2 * k) * wobble, k * step_cm], 1)
    angles = np.stack([k * fan_deg, 1.5 * np.sin(0.7 * k) * wobble, 2.0 * np.cos(0.3 * k) * wobble], 1)
    return mcrt.Transducer(E).poses(positions, angles)


def box_grid(mcrt, lo, hi, p):
    """an axis-aligned grid of pitch p [mm] whose voxel centres start at lo and stay below hi"""
    n = [max(1, int(np.floor((hi[i] - lo[i]) / p)) + 1) for i in range(3)]
    return mcrt.volume_grid(lo, (p, 0, 0), (0, p, 0), (0, 0, p), *n)


# ------------------------------------------------------------------ struct, defaults, header
def test_struct_defaults_and_header(mcrt):
    O = mcrt.ReconOpts
    assert C.sizeof(O) == 20 and [getattr(O, n).offset for n in ("mode", "value_max", "fill_radius", "fill_min", "empty")] == [0, 4, 8, 12, 16]
    L = mcrt.load_library()
    o = O()
    C.memset(C.byref(o), 0xA5, 20)
    assert L.mcrt_default_recon_opts(C.byref(o)) == 0
    assert (o.mode, o.value_max, o.fill_radius, o.fill_min, o.empty) == (0, 1024.0, 1, 1, 0.0)
    assert rm.DEFAULTS == dict(mode=o.mode, value_max=o.value_max, fill_radius=o.fill_radius, fill_min=o.fill_min, empty=o.empty)
    assert L.mcrt_default_recon_opts(None) == INVALID and b"null" in L.mcrt_last_error()
    e = mcrt.recon_opts_struct(mode="max", value_max=2.0, fill_radius=3, fill_min=5, empty=-1.0)
    assert (e.mode, e.value_max, e.fill_radius, e.fill_min, e.empty) == (1, 2.0, 3, 5, -1.0)
    assert mcrt.RECON_MODES == {"mean": 0, "max": 1}
    with pytest.raises(TypeError):
        mcrt.recon_opts_struct(radius=3)
    src = open(os.path.join(ROOT, "include", "mcrt.h")).read()
    assert "#define MCRT_VERSION 109 " in src and L.mcrt_version() == 109
    block = src[src.index("#define MCRT_VERSION"):src.index("typedef enum")]
    added = block[block.index("mcrt_recon_opts"):]
    for name in ("mcrt_recon_opts", "mcrt_default_recon_opts", "mcrt_recon_transform", "mcrt_recon_frames", "additive"):
        assert name in added, name
    for name in ("mcrt_default_recon_opts", "mcrt_recon_transform", "mcrt_recon_frames"):
        assert re.search(r"\bint " + name + r"\(", src) and hasattr(L, name), name
    assert "MCRT_RECON_MEAN = 0, MCRT_RECON_MAX = 1" in src
    # the call without a context is refused before anything else is looked at
    assert L.mcrt_recon_frames(None, None, 1, 1, 1, None, None, 1.0, 10.0, None, None, None, None, None) == INVALID and b"null context" in L.mcrt_last_error()


# ------------------------------------------------------------------ the transform
GRIDS = {
    "unit": ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)),
    "half_mm": ((-31.75, 28.5, -12.25), (0.5, 0, 0), (0, 0.5, 0), (0, 0, 0.5)),
    "third_mm": ((-40.1, 29.7, -10.3), (1 / 3, 0, 0), (0, 1 / 3, 0), (0, 0, 1 / 3)),
    "permuted": ((3.0, 30.0, -7.0), (0, 0, 0.7), (0.9, 0, 0), (0, 1.1, 0)),
    "rotated": ((-20.0, 35.0, -9.0), (0.8, 0.6, 0.1), (-0.6, 0.8, 0.2), (0.1, -0.25, 0.95)),
    "skewed": ((12.5, 41.0, 3.25), (1.0, 0.3, 0.2), (0.25, 0.9, -0.15), (-0.35, 0.2, 1.3)),
    "left_handed": ((1.0, 2.0, 3.0), (0.5, 0.1, 0.05), (0.1, -0.6, 0.1), (0.07, 0.2, 0.4)),
}


@pytest.mark.parametrize("name", sorted(GRIDS))
@pytest.mark.parametrize("unit_mm", [10.0, 1.0, 25.4])
def test_transform_against_numpys_inverse(mcrt, name, unit_mm):
    """A = Minv * unit_mm and b = -(Minv . origin) against numpy's double inverse, every float within 1 ulp: the cofactor formula and an LU
    differ in the last places of the double, and a double next to a float rounding boundary then rounds to the neighbouring float"""
    o, du, dv, dw = GRIDS[name]
    g = mcrt.volume_grid(o, du, dv, dw, 5, 6, 7)
    A, b = mcrt.host_recon_transform(g, unit_mm)
    assert A.dtype == f32 and A.shape == (3, 3) and b.shape == (3,)
    Minv = np.linalg.inv(np.array([du, dv, dw], np.float64).T)
    want_A, want_b = Minv * unit_mm, -(Minv @ np.array(o, np.float64))
    for got, want in ((A, want_A), (b, want_b)):
        near0 = np.abs(want) < 1e-12 * np.abs(want).max()             # an exact zero of the algebra, which an LU may miss by rounding
        ulp = np.spacing(np.abs(want).astype(f32)).astype(np.float64)
        assert (np.abs(got.astype(np.float64) - want)[~near0] <= ulp[~near0]).all(), (name, got, want)
        assert (np.abs(got[near0]) <= 1e-12 * np.abs(want).max()).all()
    # the centre of voxel (i, j, l) maps onto (i, j, l)
    P = (np.array(o) + 2 * np.array(du) + 3 * np.array(dv) + 4 * np.array(dw)) / unit_mm
    assert np.allclose(b.astype(np.float64) + A.astype(np.float64) @ P, (2, 3, 4), atol=1e-3)


def test_transform_refusals(mcrt):
    L = mcrt.load_library()
    A = np.full(9, 7.0, f32); b = np.full(3, 7.0, f32)
    pa, pb = A.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)
    ok = mcrt.volume_grid((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), 2, 2, 2)
    call = lambda g, unit=10.0, a=pa, b_=pb: L.mcrt_recon_transform(C.byref(g) if g is not None else None, unit, a, b_)
    assert call(None) == INVALID and b"null grid" in L.mcrt_last_error()
    assert call(ok, a=None) == INVALID and b"null A" in L.mcrt_last_error()
    assert call(ok, b_=None) == INVALID and b"null b" in L.mcrt_last_error()
    for unit in (0.0, -1.0, np.nan, np.inf):
        assert call(ok, unit) == INVALID and b"unit_mm" in L.mcrt_last_error(), unit
    for field in ("origin_mm", "du_mm", "dv_mm", "dw_mm"):
        for bad in (np.nan, np.inf):
            for k in range(3):
                g = mcrt.volume_grid((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), 2, 2, 2)
                getattr(g, field)[k] = bad
                assert call(g) == INVALID and b"not finite" in L.mcrt_last_error(), (field, k)
    for dims in ((0, 2, 2), (2, 0, 2), (2, 2, 0)):
        assert call(mcrt.volume_grid((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), *dims)) == INVALID and b"zero size" in L.mcrt_last_error()
    for axes in (((1, 0, 0), (0, 1, 0), (0, 0, 0)), ((1, 0, 0), (2, 0, 0), (0, 0, 1)), ((1, 1, 0), (0, 1, 1), (1, 2, 1)), ((0, 0, 0), (0, 0, 0), (0, 0, 0))):
        assert call(mcrt.volume_grid((0, 0, 0), *axes, 2, 2, 2)) == INVALID and b"span space" in L.mcrt_last_error(), axes
    tiny = mcrt.volume_grid((0, 0, 0), (1e-40, 0, 0), (0, 1e-40, 0), (0, 0, 1e-40), 2, 2, 2)
    assert call(tiny) == INVALID and b"finite float" in L.mcrt_last_error()
    assert (A == 7.0).all() and (b == 7.0).all(), "a refused call wrote"
    assert call(ok) == 0 and np.array_equal(A.reshape(3, 3), 10 * np.eye(3, dtype=f32)) and not b.any()


# ------------------------------------------------------------------ the mirror's properties
@pytest.fixture(scope="module")
def case(mcrt):
    """a small sweep into a 1.5 mm grid that the sweep leaves on several sides"""
    F, E, R, row_mm = 7, 24, 90, 0.4
    pos, dirs = sweep_poses(mcrt, F, E, step_cm=0.12, fan_deg=1.0)
    g = box_grid(mcrt, (-14.0, 32.0, -3.2), (15.0, 60.0, 3.3), 1.5)
    A, b = mcrt.host_recon_transform(g)
    rng = np.random.default_rng(11)
    stack = (rng.rayleigh(1.0, (F, E, R)) * np.where(rng.random((F, E, R)) < 0.3, -1.0, 1.0)).astype(f32)
    return dict(F=F, E=E, R=R, pos=pos, dirs=dirs, A=A, b=b, row_u=f32(row_mm / 10.0), shape=(g.nw, g.nv, g.nu), stack=stack)


def _run(c, stack=None, **opts):
    return rm.recon(c["stack"] if stack is None else stack, c["pos"], c["dirs"], c["A"], c["b"], c["row_u"], c["shape"], **opts)


@pytest.mark.parametrize("mode", [rm.MEAN, rm.MAX])
def test_the_order_of_the_frames_leaves_every_bit(case, mode):
    out, count, stats = _run(case, mode=mode, fill_radius=2)
    assert count.sum() > 1000 and (count == 0).any() and stats[0] > 0
    assert count.sum() + stats.sum() == case["stack"].size
    perm = np.random.default_rng(3).permutation(case["F"])
    out2, count2, stats2 = rm.recon(case["stack"][perm], case["pos"][perm], case["dirs"][perm], case["A"], case["b"], case["row_u"], case["shape"], mode=mode,
                                    fill_radius=2)
    assert np.array_equal(out.view(np.uint32), out2.view(np.uint32)) and np.array_equal(count, count2) and np.array_equal(stats, stats2)


@pytest.mark.parametrize("mode", [rm.MEAN, rm.MAX])
@pytest.mark.parametrize("value", [0.375, -3.0, 1000.0, 1.0 + 3 * 2.0 ** -20, -2.0 ** -21])
def test_a_constant_stack_stays_that_constant(case, mode, value):
    """value_max is a power of two, 1024, so q = v * 2^21 is exact for a v that is a multiple of the fixed-point step 2^-21, and
    n * q / (n * qscale) is v again"""
    out, count, _ = _run(case, stack=np.full(case["stack"].shape, value, f32), mode=mode, fill_radius=0, empty=-5.0)
    assert (out[count > 0] == f32(value)).all() and (out[count == 0] == f32(-5.0)).all()


def test_holes_are_filled_from_sampled_voxels_only(case):
    """a block with ONE sampled voxel: radius H reaches exactly the cube of half-width H around it, with its value; a filled voxel never
    fills a further one, and a fill_min that the neighbourhood cannot hold leaves `empty`"""
    shape = (9, 9, 11)
    count = np.zeros(shape, np.uint32); acc = np.zeros(shape, np.int64)
    count[4, 4, 5] = 3; acc[4, 4, 5] = 3 * (5 << 21)                            # three samples of 5 * 2^21 / 2^21 = 5.0 at value_max = 1024
    for H in (0, 1, 2, 3):
        out = rm.resolve(acc.ravel(), count.ravel(), shape, fill_radius=H, empty=-1.0)
        want = np.full(shape, -1.0, f32)
        want[4 - H:5 + H, 4 - H:5 + H, 5 - H:6 + H] = 5.0
        assert np.array_equal(out, want), H
    assert (rm.resolve(acc.ravel(), count.ravel(), shape, fill_radius=3, fill_min=2, empty=-1.0) == np.where(count > 0, 5.0, -1.0)).all()
    # two sampled voxels three apart along u: between them the nearer ring decides (h = 1 sees one of them, never their mean)
    count[4, 4, 8] = 1; acc[4, 4, 8] = 9 << 21
    out = rm.resolve(acc.ravel(), count.ravel(), shape, fill_radius=3, empty=-1.0)
    assert out[4, 4, 6] == 5.0 and out[4, 4, 7] == 9.0 and out[4, 4, 2] == 5.0 and out[4, 4, 10] == 9.0 and out[4, 4, 1] == -1.0
    out = rm.resolve(acc.ravel(), count.ravel(), shape, fill_radius=3, fill_min=2, empty=-1.0)
    assert out[4, 4, 6] == 7.0 and out[4, 4, 7] == 7.0 and out[4, 4, 4] == -1.0 and out[4, 4, 5] == 5.0    # h = 2 holds both: (5 + 9) / 2
    # (27 neighbours at h = 1) < fill_min everywhere, and 343 at h = 3: nothing is filled
    full = np.ones(shape, np.uint32); full[4, 4, 5] = 0
    assert rm.resolve(np.zeros(shape, np.int64).ravel() + (1 << 21), full.ravel(), shape, fill_radius=3, fill_min=344, empty=-1.0)[4, 4, 5] == -1.0
    assert rm.resolve(np.zeros(shape, np.int64).ravel() + (1 << 21), full.ravel(), shape, fill_radius=1, fill_min=26, empty=-1.0)[4, 4, 5] == 1.0


def test_unusable_samples_are_counted_not_binned(case):
    stack = case["stack"].copy()
    flat = stack.reshape(-1)
    bad = np.random.default_rng(5).permutation(flat.size)[:600]
    flat[bad] = np.resize(np.array([np.nan, np.inf, -np.inf, 1024.0, -1024.0, 3e38], f32), bad.size)
    acc, count, stats, vox = rm.splat(stack, case["pos"], case["dirs"], case["A"], case["b"], case["row_u"], case["shape"])
    acc0, count0, stats0, vox0 = rm.splat(case["stack"], case["pos"], case["dirs"], case["A"], case["b"], case["row_u"], case["shape"])
    inside_bad = (vox0.reshape(-1)[bad] >= 0).sum()
    assert stats[0] == stats0[0] and stats0[1] == 0 and stats[1] == inside_bad > 0 and count.sum() == count0.sum() - inside_bad
    assert (vox.reshape(-1)[bad] == -1).all()


# ------------------------------------------------------------------ the voxels lie where the poses say
def test_every_binned_sample_lies_inside_its_voxel(mcrt):
    """an affine field c0 + g . P_mm sampled at every sample's own float position: a sampled voxel's mean lies within
    (|g_x| + |g_y| + |g_z|) p / 2 of the field at the voxel's centre, because every binned sample lies inside its voxel -- plus 1e-5 of the
    largest value for the float position and the fixed-point step.  (A numpy prototype at this size reached 0.967 of the first term.)"""
    F, E, R, p, row_mm = 24, 64, 200, 1.0, 0.3
    pos, dirs = sweep_poses(mcrt, F, E, step_cm=0.08, fan_deg=0.8)
    g = box_grid(mcrt, (-30.0, 28.0, -8.0), (31.0, 88.0, 8.5), p)
    A, b = mcrt.host_recon_transform(g)
    row_u = f32(row_mm / 10.0)
    P_mm = rm.positions(pos, dirs, R, row_u).astype(np.float64) * 10.0
    c0, grad = 100.0, np.array([1.5, -0.75, 2.25])
    stack = (c0 + P_mm @ grad).astype(f32)
    shape = (g.nw, g.nv, g.nu)
    out, count, stats = rm.recon(stack, pos, dirs, A, b, row_u, shape, fill_radius=0)
    assert (count > 0).sum() > 20000 and stats[0] > 0 and stats[1] == 0
    l, j, i = np.meshgrid(np.arange(g.nw), np.arange(g.nv), np.arange(g.nu), indexing="ij")
    centre = np.array(list(g.origin_mm))[None, None, None, :] + p * np.stack([i, j, l], -1)
    field = c0 + centre @ grad
    bound = np.abs(grad).sum() * p / 2 + 1e-5 * np.abs(stack).max()
    err = np.abs(out.astype(np.float64) - field)[count > 0]
    print("largest error %.6f of the bound %.6f (first term %.6f)" % (err.max(), bound, np.abs(grad).sum() * p / 2))
    assert err.max() <= bound
    assert err.max() > 0.5 * np.abs(grad).sum() * p / 2, "the samples do not spread over their voxels: the check is vacuous"
