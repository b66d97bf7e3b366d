"""The inputs of the label-volume tests (test_recon_label_contract.py on the CPU, test_gpu_recon_label.py on the MI355X): tissue stacks, the two
grids on which the tie rules are known to occur, and the mirror call fed with the product's own host floats.  The poses, the grids' helper and
the row pitch are test_gpu_recon.py's, so that the float volume and the label volume are tested on the same clouds."""
import json
import numpy as np

import label_mirror as lm
import recon_label_mirror as rlm
from test_gpu_recon import ROW_MM, _cli_poses, cloud_centre, grid_about, poses  # noqa: F401

f32 = np.float32
TIE_STACK = (1, 64, 63)                                 # F, E, R of the tie grids
TIE_GRIDS = [((33, 9, 9), 2.0), ((37, 50, 5), 0.5)]     # (nu, nv, nw), voxel pitch in row pitches: winner and fill ties; fill ties only


def layered(F, E, R, n_labels, seed=0):
    """[F][E][R] uint8: layers a few to a few dozen rows thick whose boundaries jitter from line to line -- long runs of one label inside a
    scan-line, cut at another row in the next; the labels step through 0..n_labels-1 from layer to layer"""
    rng = np.random.default_rng(7100 + 31 * E + R + F + seed)
    n_layers = max(2, R // 9 + 2)
    thick = rng.integers(3, 24, n_layers)
    base = np.cumsum(thick)
    jitter = rng.integers(-2, 3, (F, E, n_layers))
    edges = np.sort(base[None, None, :] + jitter, axis=-1)
    layer = (np.arange(R)[None, None, :, None] >= edges[:, :, None, :]).sum(-1)
    first = rng.integers(0, n_labels)
    return ((first + layer * max(1, n_labels // 3 + 1)) % n_labels).astype(np.uint8)


def random_labels(F, E, R, n_labels, seed=0):
    """[F][E][R] uint8: every sample its own label (no run survives), the largest label present"""
    x = np.random.default_rng(7700 + 13 * E + R + F + seed).integers(0, n_labels, (F, E, R)).astype(np.uint8)
    x.reshape(-1)[0] = n_labels - 1
    return x


def spoil(x, n_labels, seed=0):
    """about 1 entry in 30 replaced by what must not vote: MCRT_LABEL_NONE, n_labels itself and another value >= n_labels"""
    x = x.copy()
    flat = x.reshape(-1)
    bad = np.array([255, n_labels, min(254, n_labels + 3)], np.uint8)
    k = max(len(bad), flat.size // 30) if flat.size >= 2 * len(bad) else 0
    rng = np.random.default_rng(8800 + flat.size + seed)
    flat[rng.permutation(flat.size)[:k]] = np.resize(bad, k)
    return x


def stacks(F, E, R, n_labels):
    """the two kinds of tissue stack, spoiled"""
    return [("layered", spoil(layered(F, E, R, n_labels), n_labels)), ("random", spoil(random_labels(F, E, R, n_labels), n_labels, 1))]


def tie_case(mcrt, dims, factor):
    """-> (pos, dirs, grid) of a tie grid"""
    F, E, R = TIE_STACK
    pos, dirs = poses(F, E)
    return pos, dirs, grid_about(mcrt, cloud_centre(R), dims, factor * ROW_MM)


def mirror(mcrt, x, pos, dirs, g, n_labels, row_mm=ROW_MM, **opts):
    """recon_label_mirror.recon_labels with the product's host floats -> (labels, count, votes, stats)"""
    A, b = mcrt.host_recon_transform(g)
    return rlm.recon_labels(x, pos, dirs, A, b, f32(row_mm / 10.0), (g.nw, g.nv, g.nu), n_labels, **opts)


def ties(mcrt, x, pos, dirs, g, n_labels, row_mm=ROW_MM, **opts):
    """-> (sampled voxels whose winner has an equal, filled holes decided by a tie), from the mirror"""
    A, b = mcrt.host_recon_transform(g)
    shape = (g.nw, g.nv, g.nu)
    votes, _, _ = rlm.vote(x, pos, dirs, A, b, f32(row_mm / 10.0), shape, n_labels)
    win, _, _, wtie = rlm.winners(votes, shape)
    _, _, ftie = rlm.fill(win, n_labels, **opts)
    return int(wtie.sum()), int(ftie.sum())


# ------------------------------------------------------------------ the traced scene of the end-to-end tests
SWEEP = dict(E=512, N=9, step_mm=2.0, voxel=2.0, box=(50.0, -40.0, -8.0, 100.0, 40.0, 8.0), position=(7.5, -7.0, 0.0))


def spheres_on_disk(mcrt, tmp_path):
    """label_mirror.spheres_scene with the probe in front of the spheres (its axis, +y, through their centre), as a scene file -> (sd, cfg, path)"""
    sd = lm.spheres_scene(mcrt)
    cfg = dict(sd.config)
    cfg["transducerPosition"] = list(SWEEP["position"])
    cfg["workingDirectory"] = str(tmp_path) + "/"
    radii = dict(zip([m["file"] for m in cfg["meshes"]], (lm.SPHERES_OUTER, lm.SPHERES_INNER)))
    for name, r in radii.items():
        V, F = mcrt.synth.icosphere(4, r, lm.SPHERES_CENTRE)
        mcrt.scene_io.save_obj(str(tmp_path / name), V, F)
    path = tmp_path / "spheres.scene"
    path.write_text(json.dumps(cfg))
    loaded = mcrt.scene_io.load_scene_file(str(path))
    assert loaded.tri.shape == sd.tri.shape and np.allclose(loaded.tri, sd.tri, rtol=0, atol=1e-5) and loaded.material_names == sd.material_names
    return loaded, cfg, str(path)


def sweep_margin_mm(sd, pos, g, row_mm, row_walk_mm):
    """how far from a sphere's surface a sampled voxel's centre may lie and still carry the other side's material: half a voxel diagonal (a
    sample lies inside its voxel), one row (the row that holds a boundary belongs to the medium behind it), the icosphere's sag r (1 - cos a)
    (the mesh lies inside the sphere by up to that), and the drift between the two row pitches over the depth of the box: the label walk puts
    row r at r * row_walk_mm of path (its row_dt times the speed of sound), the reconstruction at r * row_mm (depth_mm_f / R, the pitch of
    mcrt_volume_maps); the depth is the farthest any element is from a corner of the box"""
    o, voxel = np.array(list(g.origin_mm)), g.du_mm[0]
    corners = np.array([[o[0] + voxel * (g.nu - 1) * i, o[1] + voxel * (g.nv - 1) * j, o[2] + voxel * (g.nw - 1) * k] for i in (0, 1) for j in (0, 1) for k in (0, 1)])
    depth_mm = np.linalg.norm(corners[:, None, :] - 10.0 * np.asarray(pos, np.float64).reshape(1, -1, 3), axis=-1).max()
    tri = sd.tri.reshape(-1, 3, 3).astype(np.float64) * 10.0
    c = np.array(lm.SPHERES_CENTRE) * 10.0
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    plane = np.abs(((tri[:, 0] - c) * nrm).sum(1)) / np.linalg.norm(nrm, axis=1)            # distance of every face's plane from the centre
    r_vertex = np.linalg.norm(tri[:, 0] - c, axis=1)
    sag = (r_vertex - plane).max()
    drift = depth_mm / row_mm * abs(row_mm - row_walk_mm)
    return 0.5 * voxel * np.sqrt(3.0) + row_mm + sag + drift, sag, drift


def check_the_spheres(labels, count, g, sd, margin):
    """every SAMPLED voxel deeper inside a sphere than the margin has its material, every one farther outside the start material"""
    names = sd.material_names
    gel, liver, bone = names.index("GEL"), names.index("LIVER"), names.index("BONE")
    assert sd.start_mat == gel
    k = np.arange(g.nw)[:, None, None], np.arange(g.nv)[None, :, None], np.arange(g.nu)[None, None, :]
    o, p = np.array(list(g.origin_mm)), g.du_mm[0]
    dist = np.sqrt(sum((o[a] + p * k[2 - a] - 10.0 * lm.SPHERES_CENTRE[a]) ** 2 for a in range(3)))
    sampled = count > 0
    R1, R2 = 10.0 * lm.SPHERES_OUTER, 10.0 * lm.SPHERES_INNER
    regions = ((gel, dist > R1 + margin), (liver, (dist < R1 - margin) & (dist > R2 + margin)), (bone, dist < R2 - margin))
    for mat, where in regions:
        m = sampled & where
        assert m.sum() > 50 and (labels[m] == mat).all(), (names[mat], int(m.sum()), np.unique(labels[m], return_counts=True))
    assert set(np.unique(labels[sampled]).tolist()) == {gel, liver, bone}


def sweep_poses(mcrt, cfg, s=SWEEP):
    """a regular sweep along the probe's elevation axis, Transducer.poses of it, which is also what mattausch_hip --freehand (no fan) does"""
    tr, pos, dirs = _cli_poses(mcrt, cfg, s["E"], s["N"], s["step_mm"], 0.0)
    axis = mcrt.host_elevation_axis(tr.angles)
    where = [(np.asarray(tr.position, f32) + (axis * f32((k - (s["N"] - 1) / 2.0) * s["step_mm"] / 10.0)).astype(f32)).astype(f32) for k in range(s["N"])]
    p2, d2 = tr.poses(where, [tr.angles] * s["N"])
    assert np.array_equal(p2, pos) and np.array_equal(d2, dirs)
    return tr, pos, dirs


def sweep_grid(mcrt, s=SWEEP):
    b, p = s["box"], s["voxel"]
    dims = [int(np.floor((b[3 + i] - b[i]) / p)) + 1 for i in range(3)]
    return mcrt.volume_grid(b[:3], (p, 0, 0), (0, p, 0), (0, 0, p), *dims)
