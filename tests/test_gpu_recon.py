"""mcrt_recon_frames on the MI355X: k_recon_splat and k_recon_resolve against the numpy mirror of the contract (tests/recon_mirror.py) fed with
the product's own host floats, bit for bit -- voxels, counts and statistics, with the outputs pre-filled so that an unwritten voxel shows:
at the stack shapes where a wavefront's runs can go wrong, at the grids where the resolve tile and its halo can, both modes, every fill
radius, host and device pose tables; the argument errors; a traced scene through the Simulator, the C++ shim and mattausch_hip."""
import ctypes as C
import json
import os
import re
import subprocess
import numpy as np
import pytest

import image_cases as ic
import recon_mirror as rm
from test_gpu_focus import Dev

pytestmark = pytest.mark.gpu

f32 = np.float32
INVALID, LIMIT = -1, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HDR = open(os.path.join(ROOT, "mcray-tracing_amd", "csrc", "mcrt_kernels.h")).read()
TU, TV, TW = (int(re.search(r"#define RECON_%s (\d+) " % n, _HDR).group(1)) for n in ("TU", "TV", "TW"))      # k_recon_resolve's tile
FILL, CFILL = f32(-777.25), np.uint32(0xDEADBEEF)   # outputs are pre-filled: a voxel that is not written shows
ROW_MM = 0.3


def test_the_tile_is_the_kernels():
    assert (TU, TV, TW) == (32, 8, 8) and re.search(r"#define RECON_MAX_FILL 3 ", _HDR)


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


def poses(F, E, dx_cm=0.02, dz_cm=0.03, seed=0):
    """pose tables [F][E][3] in cm of no regular sweep: scan-lines dx apart along x that start near y = 3 cm and run along +y, fanned a
    little in x and in z, frames dz apart along z; every entry carries its own noise"""
    rng = np.random.default_rng(900 + 17 * F + E + seed)
    e = (np.arange(E) - (E - 1) / 2.0)[None, :]; f = (np.arange(F) - (F - 1) / 2.0)[:, None]
    pos = np.stack([dx_cm * e + 0.003 * f, 3.0 + 0.0 * e + 0.002 * f, dz_cm * f + 0.004 * np.sin(e)], -1)
    d = np.stack([0.15 * dx_cm * e + 0.0 * f, 1.0 + 0.0 * e + 0.0 * f, 0.05 * np.sin(0.5 * e) + 0.02 * f], -1)
    pos = pos + rng.normal(0, 1e-4, pos.shape)
    d = d / np.linalg.norm(d, axis=-1, keepdims=True) + rng.normal(0, 1e-4, d.shape)
    return pos.astype(f32), d.astype(f32)


def values(F, E, R, seed=0):
    """[F][E][R]: speckle with both signs and what must not be binned -- NaN, +-inf, |v| >= value_max -- beside -0.0 and exact zeros"""
    rng = np.random.default_rng(5000 + 131 * E + R + F + seed)
    x = (rng.rayleigh(1.0, (F, E, R)) * np.where(rng.random((F, E, R)) < 0.3, -1.0, 1.0) * 40.0).astype(f32)
    flat = x.reshape(-1)
    vals = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1024.0, -1024.0, 2000.0, -3e38, 1023.9999, -1023.9999, 1e-30], f32)
    k = max(len(vals), flat.size // 30) if flat.size >= 2 * len(vals) else 0
    flat[rng.permutation(flat.size)[:k]] = np.resize(vals, k)
    return x


def grid_about(mcrt, centre_mm, dims, du, dv=None, dw=None):
    """a grid of dims = (nu, nv, nw) voxels centred on centre_mm; du a pitch (axis-aligned) or three axis vectors"""
    if dv is None:
        du, dv, dw = (du, 0, 0), (0, du, 0), (0, 0, du)
    M = np.array([du, dv, dw], np.float64).T
    origin = np.asarray(centre_mm, np.float64) - M @ ((np.asarray(dims) - 1) / 2.0)
    return mcrt.volume_grid(origin, du, dv, dw, *dims)


def run(ctx, d, mcrt, x, pos, dirs, g, row_mm=ROW_MM, tables="host", want_stats=True, want_count=True, **opts):
    """one call with pre-filled outputs -> (out, count, stats) on the host"""
    F, E, R = x.shape
    shape = (g.nw, g.nv, g.nu)
    n = int(np.prod(shape))
    src = d.upload(x)
    out = d.upload(np.full(n, FILL)); cnt = d.upload(np.full(n, CFILL)) if want_count else None
    st = d.upload(np.full(2, CFILL)) if want_stats else None
    p, q = (d.upload(pos), d.upload(dirs)) if tables == "device" else (pos, dirs)
    ctx.recon_frames(src, p, q, F, E, R, g, out, count_dev=cnt, stats_dev=st, row_mm=row_mm, **opts)
    ctx.synchronize()
    return (ctx.d2h(out, shape), ctx.d2h(cnt, shape, np.uint32) if want_count else None, ctx.d2h(st, (2,), np.uint32) if want_stats else None)


def mirror(mcrt, x, pos, dirs, g, row_mm=ROW_MM, **opts):
    A, b = mcrt.host_recon_transform(g)
    o = dict(opts)
    if isinstance(o.get("mode"), str):
        o["mode"] = mcrt.RECON_MODES[o["mode"]]
    return rm.recon(x, pos, dirs, A, b, f32(row_mm / 10.0), (g.nw, g.nv, g.nu), **o)


def same(got, want, what):
    ic.assert_same_bits(got[0], want[0], what + ": out")
    assert np.array_equal(got[1], want[1]), what + ": count"
    assert np.array_equal(got[2], want[2]), (what + ": stats", got[2], want[2])


def cloud_centre(R):
    return (0.0, 30.0 + R * ROW_MM / 2.0, 0.0)


# ------------------------------------------------------------------ the splat: stack shapes and run lengths
@pytest.mark.parametrize("R", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("E", [1, 63, 64, 65, 130])
def test_stack_shapes_and_run_lengths(mcrt, ctx, E, R):
    """R and E about a wavefront's 64 lanes, F = 1 and 3, at a voxel of 20 row pitches (long runs), of 100 (a whole wavefront is one run) and
    of half a row pitch (every lane is its own run), both modes; host tables at F = 1, device tables at F = 3"""
    d = Dev(ctx)
    try:
        for F in (1, 3):
            x = values(F, E, R); pos, dirs = poses(F, E)
            for factor, dims in ((20.0, (3, 5, 2)), (100.0, (2, 2, 1)), (0.5, (37, 50, 5))):
                g = grid_about(mcrt, cloud_centre(R), dims, factor * ROW_MM)
                for mode in ("mean", "max"):
                    got = run(ctx, d, mcrt, x, pos, dirs, g, tables="host" if F == 1 else "device", mode=mode)
                    same(got, mirror(mcrt, x, pos, dirs, g, mode=mode), "F %d, voxel %g rows, %s" % (F, factor, mode))
    finally:
        d.close()


def test_samples_leave_the_block_on_all_six_sides_and_what_is_not_binned(mcrt, ctx, dev):
    """the case the shape tests rest on, looked at: samples beyond each of the six faces, every kind of unusable value inside the block, long
    and short runs"""
    F, E, R = 3, 65, 130
    x = values(F, E, R); pos, dirs = poses(F, E, dz_cm=0.5)
    for factor, dims in ((20.0, (3, 5, 1)), (0.5, (37, 50, 5))):
        g = grid_about(mcrt, cloud_centre(R), dims, factor * ROW_MM)
        A, b = mcrt.host_recon_transform(g)
        idx = rm.indices(rm.positions(pos, dirs, R, f32(ROW_MM / 10.0)), A, b)
        for c, n in enumerate(dims):
            assert (idx[..., c] < 0).any() and (idx[..., c] >= n).any(), (factor, c)
        acc, count, stats, vox = rm.splat(x, pos, dirs, A, b, f32(ROW_MM / 10.0), (g.nw, g.nv, g.nu))
        inside = np.ones(x.shape, bool)
        for c, n in enumerate(dims):
            inside &= (idx[..., c] >= 0) & (idx[..., c] < n)
        for bad in (np.isnan(x), np.isposinf(x), np.isneginf(x), np.abs(x) >= 1024):
            assert (vox[bad] == -1).all() and ((bad & inside).any() or factor < 1)           # (the fine grid holds a hundred samples: not every kind)
        assert ((inside & (x == 0) & np.signbit(x)).any() or factor < 1) and stats[0] > 0 and stats[1] > 0
        run_len = np.diff(np.flatnonzero(np.diff(vox.reshape(-1)) != 0))
        assert (run_len.max() >= 20) if factor > 1 else (np.median(run_len) == 1)
        got = run(ctx, dev, mcrt, x, pos, dirs, g)
        same(got, (rm.resolve(acc, count, (g.nw, g.nv, g.nu)), count.reshape(g.nw, g.nv, g.nu), stats), "voxel %g rows" % factor)


def test_a_nan_pose_entry_bins_nothing_of_its_scan_line(mcrt, ctx, dev):
    F, E, R = 3, 20, 70
    x = values(F, E, R); pos, dirs = poses(F, E)
    g = grid_about(mcrt, cloud_centre(R), (9, 40, 5), 0.5)
    clean = mirror(mcrt, x, pos, dirs, g)
    pos[0, 3, 2] = np.nan; dirs[2, 7, 0] = np.nan; pos[1, 0, 1] = np.inf
    want = mirror(mcrt, x, pos, dirs, g)
    assert want[2][0] > clean[2][0] and want[1].sum() < clean[1].sum()
    for tables in ("host", "device"):
        same(run(ctx, dev, mcrt, x, pos, dirs, g, tables=tables), want, tables)


# ------------------------------------------------------------------ the resolve: tiles, halos, options
TILE_GRIDS = [(1, 1, 1), (TU + 1, TV + 1, TW + 1), (2 * TU + 1, 2 * TV + 1, 2 * TW + 1)] + \
             [(n, 3, 3) for n in (TU - 1, TU, TU + 1, 2 * TU + 1)] + [(5, n, 3) for n in (TV - 1, TV, TV + 1, 2 * TV + 1)] + \
             [(5, 3, n) for n in (TW - 1, TW, TW + 1, 2 * TW + 1)]
OPTIONS = [dict(mode="mean", fill_radius=3, fill_min=1), dict(mode="max", fill_radius=1, fill_min=5, empty=-2.5), dict(mode="mean", fill_radius=0, empty=7.0),
           dict(mode="mean", fill_radius=3, fill_min=5), dict(mode="max", fill_radius=3, fill_min=1), dict(mode="max", fill_radius=0), dict(mode="mean", fill_radius=1, fill_min=1),
           dict(mode="mean", fill_radius=2, fill_min=1, value_max=100.0)]


@pytest.fixture(scope="module")
def sparse():
    """scan-lines 2.5 mm and frames 6 mm apart at a 1 mm voxel: sampled voxels, holes one to three voxels from them, and holes beyond"""
    F, E, R = 3, 24, 70
    pos, dirs = poses(F, E, dx_cm=0.25, dz_cm=0.6)
    x = values(F, E, R)
    for a in (x, pos, dirs):
        a.setflags(write=False)
    return x, pos, dirs


@pytest.mark.parametrize("dims", TILE_GRIDS)
def test_grids_about_the_resolve_tile(mcrt, ctx, sparse, dims):
    """each dimension at the tile's size - 1, + 0, + 1 and twice + 1, and 1 x 1 x 1; both modes, fill_radius 0, 1, 2, 3, fill_min 1 and 5"""
    x, pos, dirs = sparse
    d = Dev(ctx)
    try:
        centre = np.add(cloud_centre(x.shape[2]), (1.25, 0.0, 0.0) if dims == (1, 1, 1) else (0.0, 0.0, 0.0))     # (the one voxel on a scan-line)
        g = grid_about(mcrt, centre, dims, 1.0)
        seen = set()
        for o in OPTIONS:
            want = mirror(mcrt, x, pos, dirs, g, **o)
            same(run(ctx, d, mcrt, x, pos, dirs, g, **o), want, str(o))
            hole = want[1] == 0
            seen |= {"sampled"} if (~hole).any() else set()
            seen |= {"filled"} if (hole & (want[0] != f32(o.get("empty", 0.0)))).any() else set()
            seen |= {"empty"} if (hole & (want[0] == f32(o.get("empty", 0.0)))).any() else set()
        assert seen == ({"sampled"} if dims == (1, 1, 1) else {"sampled", "filled", "empty"}), seen
    finally:
        d.close()


def test_an_oblique_grid_that_is_not_orthogonal(mcrt, ctx, dev, sparse):
    x, pos, dirs = sparse
    g = grid_about(mcrt, cloud_centre(x.shape[2]), (TU + 5, TV + 3, TW + 2), (0.9, 0.3, 0.1), (-0.2, 1.0, 0.2), (0.1, -0.1, 1.2))
    for o in OPTIONS[:3]:
        want = mirror(mcrt, x, pos, dirs, g, **o)
        assert (want[1] > 0).sum() > 100 and want[2][0] > 0
        same(run(ctx, dev, mcrt, x, pos, dirs, g, tables="device", **o), want, str(o))


def test_optional_outputs_twice_the_same_and_the_scratch_only_grows(mcrt, ctx, dev, sparse):
    """count_dev and stats_dev may be null; the same call twice gives the same bits; a small grid after a large one and MAX after MEAN find
    the accumulators cleared"""
    x, pos, dirs = sparse
    big = grid_about(mcrt, cloud_centre(x.shape[2]), (2 * TU + 1, 2 * TV + 1, 2 * TW + 1), 1.0)
    small = grid_about(mcrt, cloud_centre(x.shape[2]), (7, 9, 5), 1.0)
    first = None
    for g, mode in ((small, "mean"), (big, "mean"), (small, "max"), (big, "max"), (small, "mean"), (big, "mean")):
        want = mirror(mcrt, x, pos, dirs, g, mode=mode, fill_radius=2)
        got = run(ctx, dev, mcrt, x, pos, dirs, g, mode=mode, fill_radius=2)
        same(got, want, "%s %s" % (mode, (g.nu, g.nv, g.nw)))
        if g is big and mode == "mean":
            if first is None:
                first = got
            else:
                assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(first, got)), "the same call twice"
    out, cnt, st = run(ctx, dev, mcrt, x, pos, dirs, big, want_stats=False, want_count=False, fill_radius=2)
    ic.assert_same_bits(out, first[0], "without count_dev and stats_dev")
    assert cnt is None and st is None


# ------------------------------------------------------------------ refusals
def test_refusals_leave_the_outputs_untouched(mcrt, ctx, dev, sparse):
    x, pos, dirs = sparse
    F, E, R = x.shape
    L = mcrt.load_library()
    g = grid_about(mcrt, cloud_centre(R), (9, 7, 5), 1.0)
    n = g.nu * g.nv * g.nw
    src = dev.upload(x); out = dev.upload(np.full(n, FILL)); cnt = dev.upload(np.full(n, CFILL)); st = dev.upload(np.full(2, CFILL))
    dpos = dev.upload(pos)
    P = lambda a: a.ctypes.data_as(C.c_void_p) if isinstance(a, np.ndarray) else (None if a is None else C.c_void_p(a))

    def call(c=ctx.h, s=src, F_=F, E_=E, R_=R, p=pos, q=dirs, row=ROW_MM, unit=10.0, g_=g, o=None, out_=out, cnt_=cnt, st_=st, **kw):
        opts = mcrt.recon_opts_struct(**kw) if kw else o
        return L.mcrt_recon_frames(c, P(s), F_, E_, R_, P(p), P(q), row, unit, C.byref(g_) if g_ is not None else None,
                                   C.byref(opts) if opts is not None else None, P(out_), P(cnt_), P(st_))

    def refused(code, word, **kw):
        rc = call(**kw)
        assert rc == code and word.encode() in L.mcrt_last_error(), (kw, rc, word, L.mcrt_last_error())

    refused(INVALID, "null context", c=None)
    for name, kw in (("stack_dev", dict(s=None)), ("pos", dict(p=None)), ("dir", dict(q=None)), ("grid", dict(g_=None)), ("out_dev", dict(out_=None))):
        refused(INVALID, "null " + name, **kw)
    for kw in (dict(F_=0), dict(E_=0), dict(R_=0)):
        refused(INVALID, "zero sizes", **kw)
    for bad in (0.0, -0.3, np.nan, np.inf):
        refused(INVALID, "row_mm", row=bad)
        refused(INVALID, "unit_mm", unit=bad)
    refused(INVALID, "unknown mode", mode=2)
    for bad in (0.0, -1.0, np.nan, np.inf):
        refused(INVALID, "value_max", value_max=bad)
    refused(INVALID, "fill_radius", fill_radius=4)
    refused(INVALID, "fill_min", fill_min=0)
    for bad in (np.nan, np.inf, -np.inf):
        refused(INVALID, "empty", empty=bad)
    flat = mcrt.volume_grid((0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), 3, 3, 3)
    refused(INVALID, "span space", g_=flat)
    refused(INVALID, "zero size", g_=mcrt.volume_grid((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), 3, 0, 3))
    nan_grid = mcrt.volume_grid((0, np.nan, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), 3, 3, 3)
    refused(INVALID, "not finite", g_=nan_grid)
    # overlaps: an output with the stack, an output with another output
    refused(INVALID, "stack_dev and out_dev overlap", out_=src + 4 * (x.size - 1))
    refused(INVALID, "stack_dev and count_dev overlap", cnt_=src)
    refused(INVALID, "stack_dev and stats_dev overlap", st_=src + 8)
    refused(INVALID, "out_dev and count_dev overlap", cnt_=out + 4 * (n - 1))
    refused(INVALID, "out_dev and stats_dev overlap", st_=out + 4)
    refused(INVALID, "count_dev and stats_dev overlap", st_=cnt)
    # limits
    refused(LIMIT, "rows", R_=2049)
    refused(LIMIT, "65535 frames", F_=65536, E_=1, R_=1)
    refused(LIMIT, "2^31 samples", F_=65535, E_=65535, R_=1)
    refused(LIMIT, "2^31 samples", F_=1024, E_=1024, R_=2048)
    refused(LIMIT, "2^31 voxels", g_=mcrt.volume_grid((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), 2048, 1024, 1024))
    refused(LIMIT, "2^24 tiles", g_=mcrt.volume_grid((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), 1, 1, 1 << 27))      # (2^27 voxels, and a resolve launch of 2^32 lanes)
    refused(LIMIT, "2^24 tiles", g_=mcrt.volume_grid((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), 1, 1 << 27, 1))
    ctx.synchronize()
    ic.assert_same_bits(ctx.d2h(out, (n,)), np.full(n, FILL), "out_dev after the errors")
    assert (ctx.d2h(cnt, (n,), np.uint32) == CFILL).all() and (ctx.d2h(st, (2,), np.uint32) == CFILL).all()
    ic.assert_same_bits(ctx.d2h(src, x.shape), x, "stack_dev after the errors")
    # the context still works; null options are the defaults; device tables
    assert call(p=dpos) == 0
    ctx.synchronize()
    shape = (g.nw, g.nv, g.nu)
    same((ctx.d2h(out, shape), ctx.d2h(cnt, shape, np.uint32), ctx.d2h(st, (2,), np.uint32)), mirror(mcrt, x, pos, dirs, g), "null options")


# ------------------------------------------------------------------ end to end: a traced scene
def _write_scene(mcrt, tmp_path):
    cfg, meshes = mcrt.synth.sphere_scene(3)
    cfg["workingDirectory"] = str(tmp_path) + "/"
    for f, (V, F) in meshes.items():
        mcrt.scene_io.save_obj(str(tmp_path / f), V, F)
    (tmp_path / "sphere.scene").write_text(json.dumps(cfg))
    return cfg, str(tmp_path / "sphere.scene")


def _cli_poses(mcrt, cfg, E, N, step_mm, fan_deg):
    """the poses of mattausch_hip --freehand: the scene's probe moved along its elevation axis in N steps of step_mm centred on its own pose, step
    k tilted by (k - (N-1)/2) fan_deg about the line through the arc's apex (mcrt_transducer_swept with the pivot at the radius)"""
    tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    axis = mcrt.host_elevation_axis(tr.angles)
    base = np.asarray(tr.position, f32)
    tabs = []
    for k in range(N):
        s = f32((k - (N - 1) / 2.0) * step_mm / 10.0)
        p = (base + (axis * s).astype(f32)).astype(f32)
        tilt = float(f32((k - (N - 1) / 2.0) * fan_deg * 3.14159265358979323846 / 180.0))
        tabs.append(mcrt.host_transducer_swept(E, tr.radius_cm, tr.separation_mm, p, tr.angles, tilt, float(f32(tr.radius_cm * 10.0))))
    return tr, np.stack([t[0] for t in tabs]), np.stack([t[1] for t in tabs])


def test_freehand_end_to_end(mcrt, tmp_path):
    """one run on the sphere scene: Simulator.freehand over 8 poses equals the mirror applied to the stack it binned; rf_image::reconstruct
    (tests/host/recon_driver.cpp) and mattausch_hip --freehand-out (after two frames: the sweep carries the last frame's number, 1) write the
    same bytes"""
    cfg, scene = _write_scene(mcrt, tmp_path)
    sd = mcrt.scene_io.load_scene_file(scene)
    E, S, N, step_mm, fan_deg, frame = 512, 5, 8, 1.5, 2.0, 1
    tr, pos, dirs = _cli_poses(mcrt, cfg, E, N, step_mm, fan_deg)
    # a box of 1 mm voxels about the middle of the swept cloud's first 150 rows, smaller than the cloud: samples leave it
    row_mm = float(f32(f32(100 * 1500) * f32(0.001))) / 465      # depth_mm_f / R: 100 us at 1500 m/s over 465 rows (mcrt_volume_maps' map_row)
    row_u = f32(row_mm / 10.0)
    cloud = rm.positions(pos, dirs, 150, row_u).reshape(-1, 3).astype(np.float64) * 10.0
    mid, half, p = np.round(cloud.mean(0)), 0.4 * (cloud.max(0) - cloud.min(0)), 1.0
    lo, hi = mid - np.floor(half), mid + np.floor(half)
    dims = [int(np.floor((hi[i] - lo[i]) / p)) + 1 for i in range(3)]
    g = mcrt.volume_grid(lo, (p, 0, 0), (0, p, 0), (0, 0, p), *dims)
    sim = mcrt.Simulator(sd, tr, n_samples=S)
    try:
        vox, cnt = sim.freehand(frame, pos, dirs, g, counts=True, mode="max", fill_radius=2)
        assert sim.R == 465 and sim.ctx.params.depth_cm == 15.0 and sim.ctx.params.speed_of_sound == 1500
        # the stack it binned, by hand: pose f is traced with frame id frame * N + f, then convolved and enveloped as N frames
        with sim.ctx.temp(N * E * sim.R * 4) as buf:
            sim.ctx.trace_frames_poses(frame * N, pos, dirs, buf)
            sim.ctx.convolve_frames(buf, N, E, sim.R, sim.psf.axial_kernel, sim.psf.lateral_kernel)
            sim.ctx.envelope_frames(buf, N, E, sim.R)
            stack = sim.ctx.d2h(buf, (N, E, sim.R))
        want = mirror(mcrt, stack, pos, dirs, g, row_mm=row_mm, mode="max", fill_radius=2)
        ic.assert_same_bits(vox, want[0], "Simulator.freehand")
        assert np.array_equal(cnt, want[1]) and (cnt > 0).sum() > 1000 and len(np.unique(vox)) > 100
        assert np.isfinite(stack).all() and stack.max() > 0
        # pose f is traced with frame id frame * N + f
        with sim.ctx.temp(E * sim.R * 4) as one:
            sim.ctx.trace_frames_poses(frame * N + 5, pos[5:6], dirs[5:6], one)
            sim.ctx.convolve_frames(one, 1, E, sim.R, sim.psf.axial_kernel, sim.psf.lateral_kernel)
            sim.ctx.envelope_frames(one, 1, E, sim.R)
            ic.assert_same_bits(sim.ctx.d2h(one, (E, sim.R)), stack[5], "pose 5 alone")
        for bad in (dict(compound=(0.0, 0.1)), dict(sweep=(3, 0.05)), dict(elevation=True)):
            other = mcrt.Simulator(sd, tr, n_samples=S, **bad)
            try:
                with pytest.raises(RuntimeError):
                    other.freehand(frame, pos, dirs, g)
            finally:
                other.close()
    finally:
        sim.close()
    pkg = os.path.join(ROOT, "mcray-tracing_amd")
    exe = os.path.join(pkg, "mattausch_hip")
    subprocess.check_call(["make", "-C", pkg, "mattausch_hip"])
    box = ",".join("%.17g" % v for v in list(lo) + list(hi))
    r = subprocess.run([exe, scene, str(frame + 1), str(S), str(tmp_path / "f.pgm"), str(tmp_path / "f.bin"), "--freehand", str(N), "--freehand-step-mm", str(step_mm),
                        "--freehand-fan-deg", str(fan_deg), "--freehand-box-mm", box, "--freehand-voxel-mm", str(p), "--freehand-out", str(tmp_path / "v.raw"),
                        "--freehand-mode", "max", "--freehand-fill", "2"], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "%d x %d x %d" % tuple(dims) in r.stdout, r.stdout
    assert (tmp_path / "v.raw").read_bytes() == vox.astype("<f4").tobytes(), "mattausch_hip --freehand-out"
    assert (tmp_path / "f.pgm").read_bytes().startswith(b"P5\n500 400\n255\n")
    drv = str(tmp_path / "recon_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(pkg, "host"), "-o", drv,
                           os.path.join(ROOT, "tests", "host", "recon_driver.cpp"), "-L", pkg, "-lmcrt_hip", "-Wl,-rpath," + pkg])
    r = subprocess.run([drv, scene, str(frame), str(S), str(N), str(step_mm), str(fan_deg), box, str(p), str(tmp_path / "d.raw")], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert (tmp_path / "d.raw").read_bytes() == vox.astype("<f4").tobytes(), "rf_image::reconstruct"
    for bad, word in ((["--freehand-step-mm", "1"], "need --freehand"), (["--freehand", "0", "--freehand-out", "x"], "--freehand takes"),
                      (["--freehand", "4", "--freehand-step-mm", "1", "--freehand-box-mm", "0,0,0,1,1,1", "--freehand-voxel-mm", "1"], "--freehand-out")):
        r = subprocess.run([exe, scene, "1", str(S)] + bad, capture_output=True, text=True, timeout=240)
        assert r.returncode == 1 and word in r.stdout, (bad, word, r.stdout)
