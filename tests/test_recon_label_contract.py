"""3-D ground truth without a GPU (include/mcrt.h: mcrt_recon_label_opts, mcrt_default_recon_label_opts, mcrt_recon_label_frames,
mcrt_render_label_frames): the struct and its defaults, and the properties of the numpy mirror (tests/recon_label_mirror.py) that hold
tests/test_gpu_recon_label.py honest -- the order of the samples leaves every voxel, a one-label stack gives that label wherever the float
volume has a value, the counts are the float call's, a hole is filled from sampled voxels only -- and that both tie rules do occur in the
inputs the GPU tests use."""
import ctypes as C
import os
import re
import numpy as np
import pytest

import label_mirror as lm
import recon_label_cases as rc
import recon_label_mirror as rlm
import recon_mirror as rm

f32 = np.float32
INVALID = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW_U = f32(rc.ROW_MM / 10.0)


def test_struct_defaults_and_header(mcrt):
    O = mcrt.ReconLabelOpts
    assert C.sizeof(O) == 12 and [getattr(O, n).offset for n in ("n_labels", "fill_radius", "fill_min")] == [0, 4, 8]
    L = mcrt.load_library()
    o = O()
    C.memset(C.byref(o), 0xA5, 12)
    assert L.mcrt_default_recon_label_opts(C.byref(o), 7) == 0
    assert (o.n_labels, o.fill_radius, o.fill_min) == (7, 1, 1)
    assert rlm.DEFAULTS == dict(fill_radius=o.fill_radius, fill_min=o.fill_min)
    r = mcrt.ReconOpts()
    assert L.mcrt_default_recon_opts(C.byref(r)) == 0 and (r.fill_radius, r.fill_min) == (o.fill_radius, o.fill_min), "the two volumes fill the same holes"
    assert L.mcrt_default_recon_label_opts(None, 3) == INVALID and b"null" in L.mcrt_last_error()
    e = mcrt.recon_label_opts_struct(254, fill_radius=3, fill_min=5)
    assert (e.n_labels, e.fill_radius, e.fill_min) == (254, 3, 5)
    with pytest.raises(TypeError):
        mcrt.recon_label_opts_struct(3, radius=3)
    src = open(os.path.join(ROOT, "include", "mcrt.h")).read()
    assert "#define MCRT_VERSION 109 " in src and L.mcrt_version() == 109
    block = src[src.index("#define MCRT_VERSION"):src.index("typedef enum")]
    added = block[block.index("mcrt_recon_label_opts"):]
    for name in ("mcrt_recon_label_opts", "mcrt_default_recon_label_opts", "mcrt_recon_label_frames", "mcrt_render_label_frames", "additive"):
        assert name in added, name
    for name in ("mcrt_default_recon_label_opts", "mcrt_recon_label_frames", "mcrt_render_label_frames"):
        assert re.search(r"\bint " + name + r"\(", src) and hasattr(L, name), name
    # the calls without a context are refused before anything else is looked at
    assert L.mcrt_recon_label_frames(None, None, 1, 1, 1, None, None, 1.0, 10.0, None, None, None, None, None, None) == INVALID and b"null context" in L.mcrt_last_error()
    assert L.mcrt_render_label_frames(None, None, 1, 1, 1, 1, None, None, None) == INVALID and b"null context" in L.mcrt_last_error()


@pytest.fixture(scope="module")
def cloud(mcrt):
    """three frames over a grid of one-millimetre voxels that the cloud leaves on every side, with holes between the frames"""
    F, E, R = 3, 24, 70
    pos, dirs = rc.poses(F, E, dx_cm=0.25, dz_cm=0.6)
    g = rc.grid_about(mcrt, rc.cloud_centre(R), (21, 19, 15), 1.0)
    A, b = mcrt.host_recon_transform(g)
    return (F, E, R), pos, dirs, (g.nw, g.nv, g.nu), A, b


def test_the_order_of_the_samples_leaves_every_voxel(cloud):
    (F, E, R), pos, dirs, shape, A, b = cloud
    x = rc.spoil(rc.layered(F, E, R, 5), 5)
    want = rlm.recon_labels(x, pos, dirs, A, b, ROW_U, shape, 5, fill_radius=2)
    order = np.random.default_rng(3).permutation(F * E)
    shuffled = [a.reshape(F * E, -1)[order].reshape(a.shape) for a in (x, pos, dirs)]
    got = rlm.recon_labels(shuffled[0], shuffled[1], shuffled[2], A, b, ROW_U, shape, 5, fill_radius=2)
    assert all(np.array_equal(p, q) for p, q in zip(got, want))
    assert (want[0] != rlm.NONE).sum() > 500 and (want[0] == rlm.NONE).any() and want[3][0] > 0 and want[3][1] > 0


@pytest.mark.parametrize("H, fill_min", [(0, 1), (1, 1), (3, 1), (2, 4)])
def test_one_label_everywhere_the_float_volume_has_a_value(cloud, H, fill_min):
    """a stack of one label gives that label at every reached or filled voxel, and those are the voxels where mcrt_recon_frames' mirror, run
    with an `empty` no sample can produce, has a value; the counts are its counts"""
    (F, E, R), pos, dirs, shape, A, b = cloud
    labels, count, votes, stats = rlm.recon_labels(np.full((F, E, R), 4, np.uint8), pos, dirs, A, b, ROW_U, shape, 6, fill_radius=H, fill_min=fill_min)
    out, fcount, fstats = rm.recon(np.ones((F, E, R), f32), pos, dirs, A, b, ROW_U, shape, fill_radius=H, fill_min=fill_min, empty=-5.0)
    assert np.array_equal(labels != rlm.NONE, out != f32(-5.0)) and {4} <= set(np.unique(labels).tolist()) <= {4, rlm.NONE}
    assert np.array_equal(count, fcount) and np.array_equal(votes, count) and stats[0] == fstats[0] and stats[1] == 0
    assert ((labels == 4) & (count == 0)).any() == (H > 0)


def test_counts_are_the_float_splats_with_usable_values_and_valid_labels(cloud):
    (F, E, R), pos, dirs, shape, A, b = cloud
    x = rc.random_labels(F, E, R, 7)
    votes, stats, vox = rlm.vote(x, pos, dirs, A, b, ROW_U, shape, 7)
    _, fcount, fstats, fvox = rm.splat(np.ones((F, E, R), f32), pos, dirs, A, b, ROW_U, shape)
    assert np.array_equal(votes.sum(1), fcount) and np.array_equal(vox, fvox) and np.array_equal(stats, fstats)


def brute_fill(win, n_labels, H, fill_min):
    """the header's hole rule voxel by voxel, reading `win` alone"""
    out = win.copy()
    nw, nv, nu = win.shape
    for w, v, u in zip(*np.nonzero(win == rlm.NONE)):
        for h in range(1, H + 1):
            cube = win[max(w - h, 0):w + h + 1, max(v - h, 0):v + h + 1, max(u - h, 0):u + h + 1]
            near = cube[cube != rlm.NONE]
            if near.size >= fill_min:
                out[w, v, u] = np.bincount(near, minlength=n_labels).argmax()
                break
    return out


def test_a_fill_reads_sampled_voxels_only(cloud):
    (F, E, R), pos, dirs, shape, A, b = cloud
    x = rc.spoil(rc.random_labels(F, E, R, 9), 9)
    votes, _, _ = rlm.vote(x, pos, dirs, A, b, ROW_U, shape, 9)
    win = rlm.winners(votes, shape)[0]
    for H, fill_min in ((1, 1), (3, 1), (3, 6)):
        got, filled, _ = rlm.fill(win, 9, H, fill_min)
        assert np.array_equal(got, brute_fill(win, 9, H, fill_min)) and filled.any()
        assert np.array_equal(got[win != rlm.NONE], win[win != rlm.NONE])
    # a line of holes between two sampled voxels: a hole two steps from the next sampled voxel waits for h = 2 though its neighbour was filled at
    # h = 1, and with fill_min = 2 only the holes that see BOTH ends are filled
    line = np.full((1, 1, 7), rlm.NONE, np.uint8)
    line[0, 0, 0], line[0, 0, 6] = 3, 5
    assert rlm.fill(line, 6, 3, 1)[0].reshape(-1).tolist() == [3, 3, 3, 3, 5, 5, 5]
    assert rlm.fill(line, 6, 3, 2)[0].reshape(-1).tolist() == [3, 255, 255, 3, 255, 255, 5]
    assert rlm.fill(line, 6, 2, 1)[0].reshape(-1).tolist() == [3, 3, 3, 255, 5, 5, 5]


@pytest.mark.parametrize("n_labels", [2, 7])
@pytest.mark.parametrize("kind", [0, 1])
def test_both_tie_rules_occur_on_the_tie_grids(mcrt, n_labels, kind):
    """on the 33 x 9 x 9 grid of 2-row voxels sampled voxels and filled holes are decided by ties, on the half-pitch grid filled holes are;
    tests/test_gpu_recon_label.py runs these on the device"""
    F, E, R = rc.TIE_STACK
    name, x = rc.stacks(F, E, R, n_labels)[kind]
    for (dims, factor), want_winner_ties in zip(rc.TIE_GRIDS, (True, False)):
        pos, dirs, g = rc.tie_case(mcrt, dims, factor)
        wt, ft = rc.ties(mcrt, x, pos, dirs, g, n_labels)
        assert ft > 0 and (wt > 0) == want_winner_ties, (name, dims, wt, ft)


def test_render_labels_mirror_on_a_hand_made_depth_buffer(mcrt):
    """s outside [0, n_steps), a NaN and a point outside the block are LABEL_NONE; a whole step reads the voxel nearest to the ray's point"""
    labels = np.arange(2 * 3 * 4, dtype=np.uint8).reshape(1, 2, 3, 4)
    view = mcrt.RenderView()
    view.origin[:], view.di[:], view.dj[:], view.ds[:] = (0.0, 0.0, -1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 0.5)
    view.nx, view.ny, view.n_steps = 5, 3, 6
    depth = np.array([[[2, 3, 4, 5, 2], [np.nan, -1, 6, 5.5, 0], [1, 2.25, 2.5, 7, 2]]], f32)
    got = rlm.render_labels(labels, view, depth)
    # p_w = -1 + s / 2: s = 2 -> 0, 3 -> 0.5 (rounds up to 1), 4 -> 1, 5 -> 1.5 (2: outside), 5.5 -> 1.75 (outside), 0 -> -1, 1 -> -0.5 (rounds up to 0)
    want = np.array([[[0, 12 + 1, 12 + 2, 255, 255], [255, 255, 255, 255, 255], [8, 8 + 1, 8 + 2, 255, 255]]], np.uint8)
    assert np.array_equal(got, want), got


def test_the_mirror_meets_the_margin_on_the_cpu(mcrt, orc, tmp_path):
    """the margin of tests/test_gpu_recon_label.py's end-to-end test, established without a GPU: label_mirror.label_frames through the oracle
    (every 8th scan-line of the sweep) and the vote mirror alone put the spheres' materials where the derived margin says"""
    sd, cfg, _ = rc.spheres_on_disk(mcrt, tmp_path)
    tr, pos, dirs = rc.sweep_poses(mcrt, cfg)
    pos, dirs = pos[:, ::8], dirs[:, ::8]
    g = rc.sweep_grid(mcrt)
    R, row_mm = 465, mcrt.api._depth_mm_f(15.0, 1500) / 465
    tissue, _, _ = lm.label_frames(lm.oracle_scene(orc, sd), orc, pos, dirs, R, rule=lm.GEOMETRIC, offs=1e-3)
    A, b = mcrt.host_recon_transform(g)
    labels, count, _, _ = rlm.recon_labels(tissue, pos, dirs, A, b, f32(row_mm / 10.0), (g.nw, g.nv, g.nu), len(sd.material_names), fill_radius=0)
    margin, sag, drift = rc.sweep_margin_mm(sd, pos, g, row_mm, mcrt.row_pitch_mm(4.5))
    print("margin %.3f mm (sag %.3f, drift %.3f)" % (margin, sag, drift))
    rc.check_the_spheres(labels, count, g, sd, margin)
