"""mcrt_recon_label_frames and mcrt_render_label_frames on the MI355X: k_recon_label_splat, k_recon_label_resolve and k_render_label against
the numpy mirror of the contracts (tests/recon_label_mirror.py) fed with the product's own host floats, exactly -- labels, counts, votes and
statistics, with the outputs pre-filled so that an unwritten voxel shows: at the stack shapes where a wavefront's runs can go wrong, at
every n_labels, at the grids where the resolve tile and its halo can, with both tie rules at work; the registration with mcrt_recon_frames;
the optional outputs; the argument errors; the label of a rendering; a traced scene through the Simulator, the C++ shim and mattausch_hip.
(No counter says whether a repeated call allocates: that point of the contract is not tested here.)"""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest

import label_mirror as lm
import recon_label_cases as rc
import recon_label_mirror as rlm
import recon_mirror as rm
import render_mirror as vm
import test_gpu_label as tgl
import test_gpu_recon as tgf
import test_gpu_render as tgr
from test_gpu_focus import Dev
from test_gpu_recon import TU, TV, TW

pytestmark = pytest.mark.gpu

f32 = np.float32
INVALID, LIMIT = -1, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LFILL, CFILL = np.uint8(254), np.uint32(0xDEADBEEF)   # outputs are pre-filled: 254 is neither a label (n_labels <= 254) nor MCRT_LABEL_NONE
ROW_MM = rc.ROW_MM
ALL = ("out", "count", "votes", "stats")


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


def run(ctx, d, x, pos, dirs, g, n_labels, tables="host", want=ALL, row_mm=ROW_MM, **opts):
    """one call with pre-filled outputs -> (labels, count, votes, stats) on the host, None where not asked for"""
    F, E, R = x.shape
    shape = (g.nw, g.nv, g.nu)
    n = int(np.prod(shape))
    src = d.upload(x)
    fill = dict(out=np.full(n, LFILL), count=np.full(n, CFILL), votes=np.full(n, CFILL), stats=np.full(2, CFILL))
    buf = {k: d.upload(fill[k]) if k in want else None for k in ALL}
    p, q = (d.upload(pos), d.upload(dirs)) if tables == "device" else (pos, dirs)
    ctx.recon_label_frames(src, p, q, F, E, R, g, n_labels, buf["out"], count_dev=buf["count"], votes_dev=buf["votes"], stats_dev=buf["stats"], row_mm=row_mm, **opts)
    ctx.synchronize()
    return tuple(None if buf[k] is None else ctx.d2h(buf[k], (2,) if k == "stats" else shape, np.uint8 if k == "out" else np.uint32) for k in ALL)


def same(got, want, what):
    for k, a, b in zip(ALL, got, want):
        if a is not None:
            assert np.array_equal(a, b), (what, k, int((a != b).sum()), a[a != b][:8], b[a != b][:8])


# ------------------------------------------------------------------ the splat: stack shapes and run lengths
@pytest.mark.parametrize("R", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("E", [1, 63, 64, 65, 130])
def test_stack_shapes_and_run_lengths(mcrt, ctx, E, R):
    """R and E about a wavefront's 64 lanes; F = 1 with host tables and F = 3 with device tables; voxels of 20 row pitches (long runs), of 100
    (a whole wavefront is one run) and of half a row pitch (every lane its own run); layered and random tissue, 1 entry in 30 not a label"""
    d = Dev(ctx)
    try:
        for F in (1, 3):
            pos, dirs = rc.poses(F, E)
            for name, x in rc.stacks(F, E, R, 5):
                for factor, dims in ((20.0, (3, 5, 2)), (100.0, (2, 2, 1)), (0.5, (37, 50, 5))):
                    g = rc.grid_about(mcrt, rc.cloud_centre(R), dims, factor * ROW_MM)
                    got = run(ctx, d, x, pos, dirs, g, 5, tables="host" if F == 1 else "device")
                    same(got, rc.mirror(mcrt, x, pos, dirs, g, 5), "F %d, %s, voxel %g rows" % (F, name, factor))
    finally:
        d.close()


def test_the_run_lengths_looked_at(mcrt, ctx, dev):
    """the case the shape tests rest on: samples beyond the block, every kind of entry that must not vote inside it, long runs of one
    (voxel, label) on the coarse grid with layered tissue, runs of one on the fine grid and with random tissue"""
    F, E, R = 3, 65, 130
    pos, dirs = rc.poses(F, E, dz_cm=0.5)
    for name, x in rc.stacks(F, E, R, 5):
        for factor, dims in ((20.0, (3, 5, 1)), (0.5, (37, 50, 5))):
            g = rc.grid_about(mcrt, rc.cloud_centre(R), dims, factor * ROW_MM)
            A, b = mcrt.host_recon_transform(g)
            votes, stats, vox = rlm.vote(x, pos, dirs, A, b, f32(ROW_MM / 10.0), (g.nw, g.nv, g.nu), 5)
            assert stats[0] > 0 and stats[1] > 0 and all((vox[x == bad] == -1).all() and (x == bad).any() for bad in (255, 5, 8))
            word = np.where(vox >= 0, vox * 5 + x, -1).reshape(-1)
            run_len = np.diff(np.flatnonzero(np.diff(word) != 0))
            assert (run_len.max() >= 20) if (factor > 1 and name == "layered") else (np.median(run_len) == 1), (name, factor, run_len.max())
            same(run(ctx, dev, x, pos, dirs, g, 5), rc.mirror(mcrt, x, pos, dirs, g, 5), "%s, voxel %g rows" % (name, factor))


@pytest.mark.parametrize("n_labels", [1, 2, 7, 254])
def test_every_n_labels(mcrt, ctx, dev, n_labels):
    """1, 2, 7 and 254 labels, the largest of which votes everywhere and wins somewhere (at 254: label 253); layered and random, the default
    fill and H = 2"""
    F, E, R = 2, 40, 90
    pos, dirs = rc.poses(F, E, dx_cm=0.05, dz_cm=0.1)
    g = rc.grid_about(mcrt, rc.cloud_centre(R), (33, 9, 9), 2.0 * ROW_MM)
    top = False
    for name, x in rc.stacks(F, E, R, n_labels):
        if name == "layered":
            x[:, :, 30:45] = n_labels - 1               # a layer of the largest label, thick enough to win its voxels
        assert x[x < n_labels].max() == n_labels - 1
        for o in (dict(), dict(fill_radius=2, fill_min=2)):
            want = rc.mirror(mcrt, x, pos, dirs, g, n_labels, **o)
            top |= bool((want[0] == n_labels - 1).any())
            assert (want[1] > 0).sum() > 100 and want[3][1] > 0
            same(run(ctx, dev, x, pos, dirs, g, n_labels, **o), want, "%s %s" % (name, o))
    assert top, "the largest label wins no voxel"


def test_a_nan_pose_entry_votes_for_nothing(mcrt, ctx, dev):
    F, E, R = 3, 20, 70
    pos, dirs = rc.poses(F, E)
    x = rc.stacks(F, E, R, 4)[0][1]
    g = rc.grid_about(mcrt, rc.cloud_centre(R), (9, 40, 5), 0.5)
    clean = rc.mirror(mcrt, x, pos, dirs, g, 4)
    pos[0, 3, 2] = np.nan; dirs[2, 7, 0] = np.nan; pos[1, 0, 1] = np.inf
    want = rc.mirror(mcrt, x, pos, dirs, g, 4)
    assert want[3][0] > clean[3][0] and want[1].sum() < clean[1].sum()
    for tables in ("host", "device"):
        same(run(ctx, dev, x, pos, dirs, g, 4, tables=tables), want, tables)


# ------------------------------------------------------------------ the resolve: tiles, halos, options, ties
TILE_GRIDS = [(1, 1, 1)] + [(u, v, w) for u in (TU - 1, TU, TU + 1) for v in (TV - 1, TV, TV + 1) for w in (TW - 1, TW, TW + 1)]
OPTIONS = [dict(fill_radius=0)] + [dict(fill_radius=H, fill_min=m) for H in (1, 2, 3) for m in (1, 3)]


@pytest.fixture(scope="module")
def sparse():
    """test_gpu_recon.py's sparse cloud -- scan-lines 2.5 mm and frames 6 mm apart at a 1 mm voxel: sampled voxels, holes one to three voxels
    from them, and holes beyond -- with layered tissue of 6 labels"""
    F, E, R = 3, 24, 70
    pos, dirs = rc.poses(F, E, dx_cm=0.25, dz_cm=0.6)
    x = rc.spoil(rc.layered(F, E, R, 6), 6)
    for a in (x, pos, dirs):
        a.setflags(write=False)
    return x, pos, dirs


@pytest.mark.parametrize("dims", TILE_GRIDS)
def test_grids_about_the_resolve_tile(mcrt, ctx, sparse, dims):
    """(31, 32, 33) x (7, 8, 9) x (7, 8, 9) voxels and 1 x 1 x 1; fill_radius 0..3, fill_min 1 and 3"""
    x, pos, dirs = sparse
    assert (TU, TV, TW) == (32, 8, 8)
    d = Dev(ctx)
    try:
        centre = np.add(rc.cloud_centre(x.shape[2]), (1.25, 0.0, 0.0) if dims == (1, 1, 1) else (0.0, 0.0, 0.0))     # (the one voxel on a scan-line)
        g = rc.grid_about(mcrt, centre, dims, 1.0)
        seen = set()
        for o in OPTIONS:
            want = rc.mirror(mcrt, x, pos, dirs, g, 6, **o)
            same(run(ctx, d, x, pos, dirs, g, 6, **o), want, str(o))
            hole = want[1] == 0
            seen |= {"sampled"} if (~hole).any() else set()
            seen |= {"filled"} if (hole & (want[0] != rlm.NONE)).any() else set()
            seen |= {"none"} if (hole & (want[0] == rlm.NONE)).any() else set()
        assert seen == ({"sampled"} if dims == (1, 1, 1) else {"sampled", "filled", "none"}), seen
    finally:
        d.close()


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_a_hole_is_filled_from_across_a_tile_edge(mcrt, ctx, dev, axis):
    """two tiles along one axis, samples placed by hand (one row per scan-line, at voxel centres) in the last two layers of the first tile
    only: the holes just beyond the edge are filled from the other tile's voxels, through the halo, and no further than H"""
    T = (TU, TV, TW)[axis]
    dims = [TU // 2, TV, TW]
    dims[axis] = 2 * T
    g = rc.grid_about(mcrt, (0.0, 30.0, 0.0), tuple(dims), 1.0)
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in dims], indexing="ij"), -1).reshape(-1, 3)
    idx = idx[(idx[:, axis] >= T - 2) & (idx[:, axis] < T)]
    idx = np.concatenate([idx, idx[::3]])                                                  # (some voxels twice: ties between two labels)
    pos = ((np.array(list(g.origin_mm)) + idx) / 10.0).astype(f32)[None]
    dirs = np.broadcast_to(np.array([0.0, 1.0, 0.0], f32), pos.shape).copy()
    x = np.random.default_rng(70 + axis).integers(0, 6, (1, len(idx), 1)).astype(np.uint8)
    for H in (1, 2, 3):
        want = rc.mirror(mcrt, x, pos, dirs, g, 6, fill_radius=H)
        count = np.moveaxis(want[1], 2 - axis, 0); labels = np.moveaxis(want[0], 2 - axis, 0)
        assert (count[T - 2:T] > 0).all() and count[T:].sum() == 0 and count[:T - 2].sum() == 0 and want[3].sum() == 0
        assert (labels[T:T + H] != rlm.NONE).all() and (labels[T + H:] == rlm.NONE).all() and (labels[T - 2 - H:T] != rlm.NONE).all()
        same(run(ctx, dev, x, pos, dirs, g, 6, fill_radius=H), want, "axis %d, H %d" % (axis, H))


@pytest.mark.parametrize("n_labels", [2, 7])
def test_the_tie_grids(mcrt, ctx, dev, n_labels):
    """the grids of tests/test_recon_label_contract.py on which sampled voxels and filled holes are decided by ties: the smallest label wins"""
    F, E, R = rc.TIE_STACK
    for name, x in rc.stacks(F, E, R, n_labels):
        for dims, factor in rc.TIE_GRIDS:
            pos, dirs, g = rc.tie_case(mcrt, dims, factor)
            for o in (dict(), dict(fill_radius=3)):
                wt, ft = rc.ties(mcrt, x, pos, dirs, g, n_labels, **o)
                assert ft > 0 and (wt > 0 or factor < 1), (name, dims, wt, ft)
                same(run(ctx, dev, x, pos, dirs, g, n_labels, **o), rc.mirror(mcrt, x, pos, dirs, g, n_labels, **o), "%s %s %s" % (name, dims, o))


def test_an_oblique_grid_and_the_scratch_only_grows(mcrt, ctx, dev, sparse):
    """a grid that is not orthogonal; a small table after a large one finds its votes cleared; the same call twice gives the same"""
    x, pos, dirs = sparse
    skew = rc.grid_about(mcrt, rc.cloud_centre(x.shape[2]), (TU + 5, TV + 3, TW + 2), (0.9, 0.3, 0.1), (-0.2, 1.0, 0.2), (0.1, -0.1, 1.2))
    small = rc.grid_about(mcrt, rc.cloud_centre(x.shape[2]), (7, 9, 5), 1.0)
    first = None
    for g, n_labels in ((small, 6), (skew, 40), (small, 6), (skew, 40), (small, 200)):
        want = rc.mirror(mcrt, x, pos, dirs, g, n_labels, fill_radius=2)
        got = run(ctx, dev, x, pos, dirs, g, n_labels, tables="device", fill_radius=2)
        same(got, want, "%s %d" % ((g.nu, g.nv, g.nw), n_labels))
        if g is skew:
            assert (want[1] > 0).sum() > 100 and want[3][0] > 0
            first = first or got
            assert all(np.array_equal(a, b) for a, b in zip(first, got)), "the same call twice"


# ------------------------------------------------------------------ registration with the float volume, optional outputs
def test_registration_with_recon_frames(mcrt, ctx, dev, sparse):
    """the same poses and grid through recon_frames and recon_label_frames, every value usable and every label valid: the counts are equal
    and the float volume is `empty` exactly where the label volume is MCRT_LABEL_NONE"""
    _, pos, dirs = sparse
    F, E, R = 3, 24, 70
    x = rc.random_labels(F, E, R, 9)
    v = (np.random.default_rng(5).rayleigh(1.0, (F, E, R)) + 0.5).astype(f32)
    g = rc.grid_about(mcrt, rc.cloud_centre(R), (2 * TU + 1, TV + 3, TW + 1), 1.0)
    shape = (g.nw, g.nv, g.nu)
    n = int(np.prod(shape))
    for o in (dict(), dict(fill_radius=3, fill_min=2), dict(fill_radius=0)):
        src = dev.upload(v); out = dev.upload(np.full(n, f32(7))); cnt = dev.upload(np.full(n, CFILL))
        ctx.recon_frames(src, pos, dirs, F, E, R, g, out, count_dev=cnt, row_mm=ROW_MM, empty=-1.0, **o)
        ctx.synchronize()
        fout, fcnt = ctx.d2h(out, shape), ctx.d2h(cnt, shape, np.uint32)
        labels, count, votes, stats = run(ctx, dev, x, pos, dirs, g, 9, **o)
        assert np.array_equal(count, fcnt) and np.array_equal(fout == f32(-1.0), labels == rlm.NONE) and stats[1] == 0, o
        assert (labels == rlm.NONE).any() and ((labels != rlm.NONE) & (count == 0)).any() == (o.get("fill_radius", 1) > 0)
        assert (votes <= count).all() and np.array_equal(votes > 0, count > 0)


def test_each_output_left_out_in_turn(mcrt, ctx, dev, sparse):
    x, pos, dirs = sparse
    g = rc.grid_about(mcrt, rc.cloud_centre(x.shape[2]), (TU + 1, TV + 1, TW + 1), 1.0)
    want = rc.mirror(mcrt, x, pos, dirs, g, 6, fill_radius=2)
    for without in ALL:
        got = run(ctx, dev, x, pos, dirs, g, 6, want=tuple(k for k in ALL if k != without), fill_radius=2)
        assert got[ALL.index(without)] is None
        same(got, want, "without " + without)
    for only in ALL:
        same(run(ctx, dev, x, pos, dirs, g, 6, want=(only,), fill_radius=2), want, "only " + only)


def test_host_pose_tables_of_changing_size_from_every_caller(mcrt):
    """Every call that takes pose tables stages host tables through one function and one pair of pinned buffers.  On ONE context, host
    (numpy) tables throughout: label_frames (F = 2: 10 lines; 465 rows, so that the beams reach the sphere), recon_label_frames (3 x 5 x 65: 15 lines; R = 65 crosses a wavefront and runs
    a scan-line's end into the next), recon_frames (1 x 130 x 7: 130 lines, the staging grows) and the first recon_label_frames again (15
    lines: it shrinks).  Each result equals the same call with DEVICE tables on a fresh context, and the two label volumes are equal."""
    cfg, sd = tgl.scene_of(mcrt, "sphere")
    E, R, LR = 5, 65, 465
    tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    lpos = np.stack([tr.pos, tr.pos + f32(0.05)]).astype(f32); ldirs = np.stack([tr.dir, tr.dir]).astype(f32)
    x = rc.spoil(rc.random_labels(3, E, R, 6), 6); pos, dirs = rc.poses(3, E)
    g = rc.grid_about(mcrt, rc.cloud_centre(R), (5, 40, 5), 0.5)
    v = tgf.values(1, 130, 7); vpos, vdirs = rc.poses(1, 130)
    gv = rc.grid_about(mcrt, rc.cloud_centre(7), (40, 6, 3), 0.7)

    def calls(tables):
        ctx = tgl.context(mcrt, sd, n_elements=E, n_rows=LR)
        d = Dev(ctx)
        try:
            lp, ld = (d.upload(lpos), d.upload(ldirs)) if tables == "device" else (lpos, ldirs)
            tissue = tgl.label(ctx, d, LR, lp, ld, n_frames=2, want=(True, False, False))[0]
            first = run(ctx, d, x, pos, dirs, g, 6, tables=tables)
            floats = tgf.run(ctx, d, mcrt, v, vpos, vdirs, gv, tables=tables)
            return tissue, first, floats, run(ctx, d, x, pos, dirs, g, 6, tables=tables)
        finally:
            tgl.done(ctx, d)

    host, want = calls("host"), calls("device")
    assert (want[0] != tgl.FILL_T).all() and len(np.unique(want[0])) > 1 and (want[0][0] != want[0][1]).any() and want[1][1].sum() > 100 and want[1][3].min() > 0 and want[2][1].sum() > 100
    assert np.array_equal(host[0], want[0]), "label_frames"
    same(host[1], want[1], "recon_label_frames, first")
    tgf.same(host[2], want[2], "recon_frames")
    same(host[3], want[3], "recon_label_frames, again")
    same(host[3], host[1], "the first and the last label volume")


# ------------------------------------------------------------------ refusals
def test_refusals_leave_the_outputs_untouched(mcrt, ctx, dev, sparse):
    x, pos, dirs = sparse
    F, E, R = x.shape
    L = mcrt.load_library()
    g = rc.grid_about(mcrt, rc.cloud_centre(R), (9, 7, 5), 1.0)
    n = g.nu * g.nv * g.nw
    src = dev.upload(x); out = dev.upload(np.full(n, LFILL)); cnt = dev.upload(np.full(n, CFILL)); win = dev.upload(np.full(n, CFILL)); st = dev.upload(np.full(2, CFILL))
    dpos = dev.upload(pos)
    P = lambda a: a.ctypes.data_as(C.c_void_p) if isinstance(a, np.ndarray) else (None if a is None else C.c_void_p(a))
    unit = lambda *dims: mcrt.volume_grid((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), *dims)

    def call(c=ctx.h, s=src, F_=F, E_=E, R_=R, p=pos, q=dirs, row=ROW_MM, unit_mm=10.0, g_=g, o="default", out_=out, cnt_=cnt, win_=win, st_=st, n_labels=6, **kw):
        opts = mcrt.recon_label_opts_struct(n_labels, **kw) if o == "default" else o
        return L.mcrt_recon_label_frames(c, P(s), F_, E_, R_, P(p), P(q), row, unit_mm, C.byref(g_) if g_ is not None else None,
                                         C.byref(opts) if opts is not None else None, P(out_), P(cnt_), P(win_), P(st_))

    def refused(code, word, **kw):
        rc_ = call(**kw)
        assert rc_ == code and word.encode() in L.mcrt_last_error(), (kw, rc_, word, L.mcrt_last_error())

    refused(INVALID, "null context", c=None)
    for name, kw in (("stack_dev", dict(s=None)), ("pos", dict(p=None)), ("dir", dict(q=None)), ("grid", dict(g_=None)), ("options", dict(o=None))):
        refused(INVALID, "null " + name, **kw)
    refused(INVALID, "all null", out_=None, cnt_=None, win_=None, st_=None)
    for kw in (dict(F_=0), dict(E_=0), dict(R_=0)):
        refused(INVALID, "zero sizes", **kw)
    for bad in (0.0, -0.3, np.nan, np.inf):
        refused(INVALID, "row_mm", row=bad)
        refused(INVALID, "unit_mm", unit_mm=bad)
    for bad in (0, 255, 256, 1 << 20):
        refused(INVALID, "n_labels", n_labels=bad)
    refused(INVALID, "fill_radius", fill_radius=4)
    refused(INVALID, "fill_min", fill_min=0)
    refused(INVALID, "span space", g_=mcrt.volume_grid((0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), 3, 3, 3))
    refused(INVALID, "zero size", g_=unit(3, 0, 3))
    refused(INVALID, "not finite", g_=mcrt.volume_grid((0, np.nan, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), 3, 3, 3))
    # overlaps: an output with the stack, an output with another output
    refused(INVALID, "stack_dev and out_dev overlap", out_=src + (x.size - 1))
    refused(INVALID, "stack_dev and count_dev overlap", cnt_=src)
    refused(INVALID, "stack_dev and votes_dev overlap", win_=src)
    refused(INVALID, "stack_dev and stats_dev overlap", st_=src + 8)
    refused(INVALID, "out_dev and count_dev overlap", cnt_=out + 4 * (n // 4 - 1))
    refused(INVALID, "out_dev and votes_dev overlap", win_=out)
    refused(INVALID, "count_dev and votes_dev overlap", win_=cnt + 4 * (n - 1))
    refused(INVALID, "out_dev and stats_dev overlap", st_=out + 4)
    refused(INVALID, "count_dev and stats_dev overlap", st_=cnt)
    refused(INVALID, "votes_dev and stats_dev overlap", st_=win + 8)
    # limits: mcrt_recon_frames' own, and the vote table's
    refused(LIMIT, "rows", R_=2049)
    refused(LIMIT, "65535 frames", F_=65536, E_=1, R_=1)
    refused(LIMIT, "2^31 samples", F_=65535, E_=65535, R_=1)
    refused(LIMIT, "2^31 samples", F_=1024, E_=1024, R_=2048)
    refused(LIMIT, "2^31 voxels", g_=unit(2048, 1024, 1024))
    refused(LIMIT, "2^24 tiles", g_=unit(1, 1, 1 << 27), n_labels=1)
    refused(LIMIT, "2^24 tiles", g_=unit(1, 1 << 27, 1), n_labels=1)
    refused(LIMIT, "vote table", g_=unit(1024, 1024, 1024), n_labels=2)          # 2^30 voxels x 2
    refused(LIMIT, "vote table", g_=unit(256, 256, 256), n_labels=128)           # 2^24 voxels x 128
    refused(LIMIT, "vote table", g_=unit(2048, 4129, 1), n_labels=254)           # 2^31 + 389120 words
    ctx.synchronize()
    assert (ctx.d2h(out, (n,), np.uint8) == LFILL).all() and all((ctx.d2h(b, (k,), np.uint32) == CFILL).all() for b, k in ((cnt, n), (win, n), (st, 2)))
    assert np.array_equal(ctx.d2h(src, x.shape, np.uint8), x), "stack_dev after the errors"
    # the context still works; device tables; one label below the limit's other side
    assert call(p=dpos) == 0
    ctx.synchronize()
    shape = (g.nw, g.nv, g.nu)
    got = (ctx.d2h(out, shape, np.uint8), ctx.d2h(cnt, shape, np.uint32), ctx.d2h(win, shape, np.uint32), ctx.d2h(st, (2,), np.uint32))
    same(got, rc.mirror(mcrt, x, pos, dirs, g, 6), "after the refusals")


# ------------------------------------------------------------------ the label of a rendering
PICTURES = [(1, 1), (7, 7), (8, 8), (9, 9), (8, 9), (33, 17)]        # (nx, ny) about k_render_label's 8 x 8 pixels per wavefront, and more than one workgroup


def wide_view(mcrt, block, direction, picture, n=24):
    """a picture 1.6 block diagonals wide: its outer rays pass the block on every side"""
    g = vm.case_grid(mcrt, block)
    L2 = 2.0 * vm.half_diagonal(g) or float(np.linalg.norm(sum(vm.grid_arrays(g)[1:4])))      # (a block of one voxel: its own diagonal, as case_view)
    return mcrt.render_view(g, direction, vm.UP, 1.6 * L2 / max(picture), L2 / n, *picture)


def render_both(ctx, d, vox, labels, view, depth=None, **opts):
    """mcrt_render_frames' depth buffer of the byte blocks vox (or the given one), then mcrt_render_label_frames -> (depth, labels picture)"""
    F, shape = vox.shape[0], vox.shape[1:]
    npix = view.nx * view.ny
    ddev = d.upload(np.full(F * npix, f32(-3.0)) if depth is None else depth)
    if depth is None:
        ctx.render_frames(d.upload(vox), F, shape, view, depth_dev=ddev, in_u8=True, **opts)
    out = d.upload(np.full(F * npix, LFILL))
    ctx.render_label_frames(d.upload(labels), F, shape, view, ddev, out)
    ctx.synchronize()
    return ctx.d2h(ddev, (F, view.ny, view.nx)), ctx.d2h(out, (F, view.ny, view.nx), np.uint8)


@pytest.mark.parametrize("mode", ["mip", "mean", "surface"])
@pytest.mark.parametrize("F", [1, 3])
def test_render_labels_match_the_mirror(mcrt, ctx, dev, mode, F):
    """a byte block and a random label block of its shape, pictures about the pixel tile, rays that pass the block on every side; MEAN's depth
    of -1 gives MCRT_LABEL_NONE everywhere"""
    seen = set()
    for bi, block in enumerate(vm.BLOCKS):
        shape = block[::-1]
        vox = np.stack([vm.byte_block(shape, seed=10 * bi + f) for f in range(F)])
        labels = np.random.default_rng(40 + bi).integers(0, 254, vox.shape, dtype=np.uint8)
        for di, direction in enumerate(vm.DIRECTIONS):
            for picture in PICTURES[(bi + di) % 2::2] + ([(33, 17)] if (bi + di) % 2 == 0 else []):
                view = wide_view(mcrt, block, direction, picture)
                depth, got = render_both(ctx, dev, vox, labels, view, mode=mode)
                want = rlm.render_labels(labels, view, depth)
                assert np.array_equal(got, want), (block, direction, picture, int((got != want).sum()))
                if mode == "mean":
                    assert (depth == -1).all() and (got == rlm.NONE).all()
                else:
                    seen |= {"label"} if (got != rlm.NONE).any() else set()
                    seen |= {"none"} if (got == rlm.NONE).any() else set()
                    if max(picture) > 8 and block != (1, 1, 1):
                        edge = np.concatenate([depth[:, 0].ravel(), depth[:, -1].ravel(), depth[:, :, 0].ravel(), depth[:, :, -1].ravel()])
                        assert (edge == -1).any() and (depth >= 0).any(), (block, direction, picture)
    assert mode == "mean" or seen == {"label", "none"}


def test_render_labels_of_a_hand_made_depth_buffer(mcrt, ctx, dev):
    """NaN, -1, n_steps, n_steps - 1, a non-integer, infinities and -0.0 in the depth buffer"""
    block = (17, 13, 11)
    shape = block[::-1]
    labels = np.random.default_rng(3).integers(0, 254, (2,) + shape, dtype=np.uint8)
    view = vm.case_view(mcrt, block, vm.DIRECTIONS[2], (9, 8))
    n = view.n_steps
    vals = np.array([np.nan, -1.0, n, n - 1, n / 2 + 0.25, n / 3 + 0.5, np.inf, -np.inf, -0.0, 0.0, n - 0.5, np.nextafter(f32(n), f32(0)), -1e-30, 1e30], f32)
    depth = np.resize(vals, (2, 8, 9)).astype(f32)
    depth[1] = np.random.default_rng(4).uniform(-2, n + 2, (8, 9)).astype(f32)
    got_depth, got = render_both(ctx, dev, np.zeros((2,) + shape, np.uint8), labels, view, depth=depth)
    assert np.array_equal(got_depth.view(np.uint32), depth.view(np.uint32))
    want = rlm.render_labels(labels, view, depth)
    assert np.array_equal(got, want) and (want != rlm.NONE).any()
    flat = depth[0].ravel()
    for bad in (np.isnan(flat), flat == -1, flat >= n, flat < 0):
        assert bad.any() and (want[0].ravel()[bad] == rlm.NONE).all()


def test_render_label_refusals(mcrt, ctx, dev):
    L = mcrt.load_library()
    nu, nv, nw = 6, 5, 4
    good = mcrt.render_view(mcrt.volume_grid((0, 0, 0), (0.5, 0, 0), (0, 0.5, 0), (0, 0, 0.5), nu, nv, nw), (0.3, 0.2, 1), vm.UP, 0.4, 0.3, 8, 7)
    lab = dev.upload(np.zeros(nu * nv * nw, np.uint8)); dep = dev.upload(np.zeros(56, f32)); out = dev.upload(np.full(56, LFILL))
    P = lambda a: None if a is None else C.c_void_p(a)

    def view(**kw):
        v = mcrt.RenderView.from_buffer_copy(good)
        for k, val in kw.items():
            if isinstance(val, tuple):
                getattr(v, k)[val[0]] = val[1]
            else:
                setattr(v, k, val)
        return v

    def refused(code, word, c=ctx.h, l=lab, F=1, u=nu, v=nv, w=nw, vw=good, d=dep, o=out):
        got = L.mcrt_render_label_frames(c, P(l), F, u, v, w, C.byref(vw) if vw is not None else None, P(d), P(o))
        assert got == code and word.encode() in L.mcrt_last_error(), (got, word, L.mcrt_last_error())

    refused(INVALID, "null context", c=None)
    for name, kw in (("label_dev", dict(l=None)), ("view", dict(vw=None)), ("depth_dev", dict(d=None)), ("out_dev", dict(o=None))):
        refused(INVALID, "null " + name, **kw)
    for kw in (dict(F=0), dict(u=0), dict(v=0), dict(w=0)):
        refused(INVALID, "zero sizes", **kw)
    refused(INVALID, "zero picture size", vw=view(nx=0))
    refused(INVALID, "zero picture size", vw=view(ny=0))
    for field in ("origin", "di", "dj", "ds"):
        for bad in (np.nan, np.inf):
            refused(INVALID, "not finite", vw=view(**{field: (1, bad)}))
    refused(INVALID, "label_dev and out_dev overlap", o=lab + 8)
    refused(INVALID, "depth_dev and out_dev overlap", o=dep + 4 * 55)
    refused(LIMIT, "n_steps", vw=view(n_steps=0))
    refused(LIMIT, "n_steps", vw=view(n_steps=4097))
    refused(LIMIT, "2^24", u=1 << 24, v=1, w=1)
    refused(LIMIT, "2^31 voxels", u=2048, v=1024, w=1024)
    refused(LIMIT, "2^31 pixels", vw=view(nx=1 << 16, ny=1 << 15))
    refused(LIMIT, "65535 frames", F=65536)
    ctx.synchronize()
    assert (ctx.d2h(out, (56,), np.uint8) == LFILL).all()
    assert L.mcrt_render_label_frames(ctx.h, P(lab), 1, nu, nv, nw, C.byref(good), P(dep), P(out)) == 0
    ctx.synchronize()
    assert np.array_equal(ctx.d2h(out, (1, 7, 8), np.uint8), rlm.render_labels(np.zeros((1, nw, nv, nu), np.uint8), good, np.zeros((1, 7, 8), f32)))


# ------------------------------------------------------------------ end to end: a traced scene
def test_freehand_labels_end_to_end(mcrt, tmp_path):
    """the spheres through Simulator.freehand_labels (geometric rule, start offset 1e-3, no filling): the mirror's bytes for the device's own
    tissue maps, the materials where the margin says, and the same bytes from rf_image::reconstruct_labels and mattausch_hip --freehand-labels"""
    sd, cfg, scene = rc.spheres_on_disk(mcrt, tmp_path)
    s = rc.SWEEP
    tr, pos, dirs = rc.sweep_poses(mcrt, cfg)
    g = rc.sweep_grid(mcrt)
    sim = mcrt.Simulator(sd, tr, n_samples=2)
    try:
        labels, count, votes = sim.freehand_labels(pos, dirs, g, rule="geometric", start_offset=1e-3, fill_radius=0, counts=True, votes=True)
        assert sim.R == 465 and sim.n_materials == len(sd.material_names)
        row_mm = mcrt.api._depth_mm_f(sim.ctx.params.depth_cm, sim.ctx.params.speed_of_sound) / sim.R
        with sim.ctx.temp(s["N"] * s["E"] * sim.R) as t:
            sim.ctx.label_frames(pos, dirs, rule="geometric", start_offset=1e-3, tissue_dev=t)
            tissue = sim.ctx.d2h(t, (s["N"], s["E"], sim.R), np.uint8)
        want = rc.mirror(mcrt, tissue, pos, dirs, g, sim.n_materials, row_mm=row_mm, fill_radius=0)
        same((labels, count, votes, None), want, "Simulator.freehand_labels")
        margin, _, _ = rc.sweep_margin_mm(sd, pos, g, row_mm, sim.row_mm)
        rc.check_the_spheres(labels, count, g, sd, margin)
        assert np.array_equal(sim.freehand_labels(pos, dirs, g, rule="geometric", start_offset=1e-3, fill_radius=0), labels)
        filled = sim.freehand_labels(pos, dirs, g, rule="geometric", start_offset=1e-3)
        assert np.array_equal(filled[count > 0], labels[count > 0]) and (filled != rlm.NONE).sum() > (labels != rlm.NONE).sum()
        for bad in (dict(compound=(0.0, 0.1)), dict(sweep=(3, 0.05)), dict(elevation=True)):
            other = mcrt.Simulator(sd, tr, n_samples=2, **bad)
            try:
                with pytest.raises(RuntimeError):
                    other.freehand_labels(pos, dirs, g)
            finally:
                other.close()
    finally:
        sim.close()
    pkg = os.path.join(ROOT, "mcray-tracing_amd")
    exe = os.path.join(pkg, "mattausch_hip")
    subprocess.check_call(["make", "-C", pkg, "mattausch_hip"])
    box = ",".join("%.17g" % v for v in s["box"])
    r = subprocess.run([exe, scene, "1", "2", str(tmp_path / "f.pgm"), "--freehand", str(s["N"]), "--freehand-step-mm", str(s["step_mm"]), "--freehand-box-mm", box,
                        "--freehand-voxel-mm", str(s["voxel"]), "--freehand-out", str(tmp_path / "v.raw"), "--freehand-fill", "0", "--freehand-labels", str(tmp_path / "l.raw"),
                        "--label-rule", "geometric", "--label-offset", "1e-3"], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert (tmp_path / "l.raw").read_bytes() == labels.tobytes(), "mattausch_hip --freehand-labels"
    assert len((tmp_path / "v.raw").read_bytes()) == 4 * labels.size
    drv = str(tmp_path / "recon_label_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(pkg, "host"), "-o", drv,
                           os.path.join(ROOT, "tests", "host", "recon_label_driver.cpp"), "-L", pkg, "-lmcrt_hip", "-Wl,-rpath," + pkg])
    r = subprocess.run([drv, scene, "2", str(s["N"]), str(s["step_mm"]), box, str(s["voxel"]), "geometric", "1e-3", "0", str(tmp_path / "d.raw")], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert (tmp_path / "d.raw").read_bytes() == labels.tobytes(), "rf_image::reconstruct_labels"
    for bad, word in ((["--freehand-labels", "x"], "needs --freehand"), (["--render-labels", "x"], "needs --render"), (["--label-rule", "geometric"], "needs --labels")):
        r = subprocess.run([exe, scene, "1", "2"] + bad, capture_output=True, text=True, timeout=240)
        assert r.returncode == 1 and word in r.stdout, (bad, word, r.stdout)


def test_render_with_labels_end_to_end(mcrt, tmp_path):
    """Simulator.render(labels=True) on test_gpu_render.py's sweep: the picture is the one without labels, and a pixel has a label exactly
    where its depth is >= 0 and the nearest voxel lies inside the grid -- then it is label_volume()'s voxel; mattausch_hip --render-labels
    writes a label picture beside the rendering"""
    cfg, scene = tgr._write_scene(mcrt, tmp_path)
    e, look = tgr.E2E, tgr.LOOK
    tr = mcrt.Transducer(e["E"], position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    g = tgr._box_grid(mcrt)
    shape = (g.nw, g.nv, g.nu)
    sim = mcrt.Simulator(mcrt.scene_io.load_scene_file(scene), tr, n_samples=e["S"], sweep=(e["K"], e["step"]), sweep_pivot_mm=e["pivot"])
    try:
        view = mcrt.render_view(g, look["direction"], (0, 0, 1), look["pixel_mm"], look["step_mm"], *look["size"])
        block = sim.label_volume(g, rule="geometric", start_offset=1e-3)
        voxels = sim.bmode_volume(e["frame"], g)
        for mode in ("mip", "surface", "mean"):
            plain = sim.render(e["frame"], g, mode=mode, **look)
            picture, labels = sim.render(e["frame"], g, mode=mode, labels=True, label_rule="geometric", label_offset=1e-3, **look)
            assert np.array_equal(picture, plain) and labels.shape == plain.shape and labels.dtype == np.uint8
            depth = vm.render(voxels, view, vm.defaults(True, mode=mode))[2]
            want = rlm.render_labels(block[None], view, depth[None])[0]
            assert np.array_equal(labels, want), mode
            inside = np.ones(depth.shape, bool)
            for x, n in zip(vm.ray_points(view, np.where(depth >= 0, depth, 0).astype(f32)), shape[::-1]):
                inside &= lm.nearest(x, n)[1]
            seen = (depth >= 0) & inside
            assert not (labels[~seen] != rlm.NONE).any() and np.array_equal(labels[seen] != rlm.NONE, block[tuple(
                lm.nearest(x, n)[0][seen] for x, n in zip(vm.ray_points(view, np.where(depth >= 0, depth, 0).astype(f32))[::-1], shape))] != rlm.NONE)
            assert (labels != rlm.NONE).any() == (mode != "mean")
    finally:
        sim.close()
    pkg = os.path.join(ROOT, "mcray-tracing_amd")
    exe = os.path.join(pkg, "mattausch_hip")
    subprocess.check_call(["make", "-C", pkg, "mattausch_hip"])
    b = tgr.BOX
    box = ",".join(repr(float(v)) for v in list(b["origin"]) + [b["origin"][i] + b["voxel"] * (b["n"][i] - 1) for i in range(3)])
    common = [exe, scene, "1", "2", str(tmp_path / "r.pgm"), "--sweep", "5", "--sweep-step-deg", "3", "--render", "0.25,1,0.15", "--render-box-mm", box, "--render-voxel-mm",
              repr(b["voxel"]), "--render-size", "40,32", "--render-mode", "mip"]
    r = subprocess.run(common, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    before = (tmp_path / "r.pgm").read_bytes()
    r = subprocess.run(common + ["--render-labels", str(tmp_path / "rl.pgm"), "--label-rule", "geometric", "--label-offset", "1e-3"], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert (tmp_path / "r.pgm").read_bytes() == before, "the rendering with and without --render-labels"
    raw = (tmp_path / "rl.pgm").read_bytes()
    head = b"P5\n40 32\n255\n"
    pic = np.frombuffer(raw[len(head):], np.uint8)
    assert raw.startswith(head) and pic.size == 40 * 32 and (pic != rlm.NONE).any() and (pic[pic != rlm.NONE] < 254).all()
