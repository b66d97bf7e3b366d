"""The list entries of the beam stage carry what depends on the candidate's triangle alone (csrc/mcrt_beam.hip: k_beam_collect stores, beside every 64-byte
entry, the triangle's plane and padded bounds -- BeamArgs::hot --, and k_beam_test's list_tri_test reads them where packet_tri_test rebuilt them per wavefront
and entry).

  what is stored   mcrt_debug_beam_entries' words -- plane n.x n.y n.z dot(v0, n) | padded lo | padded hi -- of every entry below its list's count against a
                   numpy float32 recomputation from the vertices mcrt_debug_beam_records returns, in the operation order of tri_plane / tri_padded_bounds
                   (csrc/mcrt_device.h): every difference, product and sum rounded on its own, no fused multiply-add, pad = 2e-4f * extent + pad_abs.
                   Compared as uint32: the claim is bit for bit, so there is no tolerance.  Bounces 1 and 3; the sphere, the liver at spacing (1.0, 0.5, 2.0)
                   and a hand-made soup (below).  The begin depth and the id stored beside them -- which the list test reads in place of the list's words 7
                   and 3 -- equal those words.  Bounce 3 of the sphere meets nothing: asserted as such (beams in use, every list complete and empty)
  the read-back    of the same calls keeps its documented layout: words 12-15 of an entry are 0, word 7 (v1.w) is the depth at which the padded bounds begin --
                   recomputed exactly: beam_box's (lo_dom - xref) - m or (xref - hi_dom) - m, two float32 subtractions of stored words --, also with lists of 3
                   (the pair loop's second fetch lies past the list) and on the LAST list of the pool
  same answers     hit tables, per-bounce counts and RF images as int32 against the beams off, by tests/test_gpu_beam_order.py's method (decided + walked = the
                   bounce's rays): beam order and queue order, S = 96, capacities 1 / 3 / 4 / default, a second pass (MCRT_BEAM_NEAR=2 of 4), a table of one group,
                   a shard, the soup

The soup: six tilted sheets of 200 triangles in front of the probe, each a mesh of its own, and a mesh of hard triangles between the first two -- a
zero-area triangle (three collinear vertices: its plane is 0 0 0 | 0), a needle (one edge 2e-6 long, the others 2.8), two triangles that share vertices at
identical coordinates -- all crossing the probe's axis, and a copy of everything 300 units further along it (the scene's largest coordinate, and with it pad_abs
and the beams' margin, grows 25-fold).  E = 8, S = 256, F = 3 unless the case says otherwise."""
import numpy as np
import pytest

import test_gpu_beam_order as bo
from test_gpu_beam_deep import _context, STAGED
from test_gpu_constants import _moved

pytestmark = pytest.mark.gpu

E, S, FRAME = 8, 256, 3
N_SHEETS, SHEET_N = 6, 10
SPECIAL = ("zero-area", "needle", "shared a", "shared b")


def _soup(mcrt):
    s = mcrt.synth
    pairs = [("LIVER", "GEL"), ("FAT", "LIVER"), ("KIDNEY", "FAT"), ("LIVER", "KIDNEY"), ("FAT", "LIVER"), ("SKIN", "FAT")]
    cfg = {"transducerPosition": [-13.5, 0.0, 0.0], "transducerAngles": [0.0, 0.0, -90.0], "materials": s.materials(), "meshes": [],
           "origin": [0.0, 0.0, 0.0], "spacing": [1.0, 1.0, 1.0], "scaling": 1.0, "startingMaterial": "GEL"}
    meshes = {}
    g = np.linspace(-4.0, 4.0, SHEET_N + 1)
    Y, Z = np.meshgrid(g, g, indexing="ij")
    idx = np.arange((SHEET_N + 1) ** 2).reshape(SHEET_N + 1, SHEET_N + 1)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    F = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)]).astype(np.int32)
    for i in range(N_SHEETS):
        X = -11.0 + 1.2 * i + 0.05 * (i + 1) * Y + 0.03 * Z
        f = "sheet_%d.obj" % i
        meshes[f] = (np.stack([X.ravel(), Y.ravel(), Z.ravel()], 1).astype(np.float32), F)
        cfg["meshes"].append(s._mesh(f, *pairs[i]))
    v0 = np.array([-10.5, 1.0, -1.0], np.float32)
    V = np.array([[-10.4, -1.0, -1.0], [-10.4, 0.0, 0.0], [-10.4, 1.0, 1.0],                      # zero area: collinear, through the axis
                  v0, v0 + np.array([0.0, 2e-6, 0.0], np.float32), [-10.3, -1.0, 1.0],             # needle
                  [-10.6, -0.5, -0.5], [-10.6, 0.5, -0.5], [-10.55, 0.0, 0.5], [-10.5, 0.6, 0.6]], np.float32)
    meshes["hard.obj"] = (V, np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8], [8, 7, 9]], np.int32))
    cfg["meshes"].append(s._mesh("hard.obj", "GALLBLADDER", "FAT"))
    sd = mcrt.scene_io.build_scene(cfg, meshes)
    n = sd.n_tri
    assert n == N_SHEETS * 2 * SHEET_N * SHEET_N + 4
    t = sd.tri.reshape(-1, 3, 3)[n - 3]
    edges = np.linalg.norm(t - np.roll(t, 1, 0), axis=1)
    assert edges.min() > 0 and edges.min() < 1e-6 * edges.max()                                    # the needle survived float32
    far = _moved(mcrt, sd, (300.0, 0.0, 0.0))
    both = mcrt.scene_io.SceneData(np.concatenate([sd.tri, far.tri]), np.concatenate([sd.tri_mesh, sd.tri_mesh]), sd.meshes, sd.materials,
                                   sd.material_names, sd.start_mat, sd.spacing, sd.config)
    return cfg, both, tuple(range(n - 4, n))


_special = {}


def _scene(mcrt, name):
    if name not in bo._scenes:
        if name == "soup":
            cfg, sd, ids = _soup(mcrt)
            _special["soup"] = ids
            bo._scenes[name] = (cfg, sd)
        elif name == "liver_spaced":
            cfg, sd = bo._scene(mcrt, "liver")
            bo._scenes[name] = (cfg, _moved(mcrt, sd, spacing=(1.0, 0.5, 2.0)))
    return bo._scene(mcrt, name)


# ------------------------------------------------------------------ what is stored, and the documented read-back
def plane_and_bounds(v0, v1, v2, pad_abs):
    """tri_plane and tri_padded_bounds of csrc/mcrt_device.h on float32 arrays [n][3], one rounding per operation -> [n][10]"""
    f = np.float32
    assert v0.dtype == v1.dtype == v2.dtype == f
    a, b = v1 - v0, v2 - v0
    n = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
    w = (v0[:, 0] * n[:, 0] + v0[:, 1] * n[:, 1]) + v0[:, 2] * n[:, 2]
    lo, hi = np.minimum(v0, np.minimum(v1, v2)), np.maximum(v0, np.maximum(v1, v2))
    d = hi - lo
    ext = np.maximum(np.maximum(np.maximum(f(0.0), d[:, 0]), d[:, 1]), d[:, 2])
    pad = f(2e-4) * ext + f(pad_abs)
    out = np.concatenate([n, w[:, None], lo - pad[:, None], hi + pad[:, None]], 1)
    assert out.dtype == f
    return out


def pad_abs_of(tri):
    """the absolute part of the padding: 4e-6f x the largest |coordinate| (at least 1e-3), in float32"""
    return np.float32(4e-6) * max(np.float32(np.abs(np.asarray(tri, np.float32)).max()), np.float32(1e-3))


ENTRY_CASES = {
    "sphere": ("sphere", {}),
    "liver_spaced": ("liver_spaced", {}),
    "soup": ("soup", {}),
    # lists of 3: a list's last pair is fetched one entry past it
    "liver_cap3": ("liver", {"MCRT_BEAM_CAP": 3}),
    # a pool of two lists: the last list of the pool is in use at a bounce >= 2
    "liver_cap3_pool2": ("liver", {"MCRT_BEAM_CAP": 3, "MCRT_BEAM_GROUPS": 2}),
}


@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("name", list(ENTRY_CASES))
def test_entries_hold_plane_and_padded_bounds_bit_for_bit(mcrt, orc, name, b):
    scene, extra = ENTRY_CASES[name]
    cfg, sd = _scene(mcrt, scene)
    tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    ctx = _context(mcrt, dict(STAGED, MCRT_BEAM_B1=2, MCRT_BEAM_LAST=b, **extra))
    try:
        ctx.set_params(n_elements=E, n_samples=S, frequency=tr.frequency)
        ctx.upload_scene(sd); ctx.upload_texture(None, 256); ctx.set_transducer(tr.pos, tr.dir)
        with ctx.temp(E * ctx.params.n_rows * 4) as dev:
            ctx.trace_frame_debug(FRAME, dev, want_segs=True)
            R = ctx.debug_beam_records(b)
            ent, begin_id = ctx.debug_beam_entries(b)
            dbg = ctx.debug_beam_bounce(b)
            with pytest.raises(mcrt.McrtError):      # as the records: only the last beamed bounce is answered
                ctx.debug_beam_entries(b + 1)
    finally:
        ctx.close()
    pad_abs = pad_abs_of(sd.tri)
    assert pad_abs == np.float32(orc.OracleScene(sd.tri, sd.tri_mesh, sd.meshes, sd.materials, sd.start_mat, sd.spacing).c.pad_abs)
    recs, lists, cap, n_lists = R["records"], R["lists"], R["cap"], R["n_lists"]
    assert ent.shape == (n_lists, cap, 10) and ent.dtype == np.uint32 and lists.shape == (n_lists, cap, 16)
    if "MCRT_BEAM_CAP" in extra: assert cap == extra["MCRT_BEAM_CAP"]
    beams = np.flatnonzero(recs[:, 14] > 0)
    li, cnt = recs[beams, 15].astype(np.int64), recs[beams, 14].astype(np.int64)
    if scene == "sphere" and b == 3:      # bounce 3 of the sphere meets nothing: every list is complete and empty, and every ray is decided (as a miss) by it
        ran, decided, walked, cut, refused, used = dbg[:6]
        print("%s bounce %d: %d beams in use, %d rays decided, %d walked, %d lists cut" % (name, b, used, decided, walked, cut))
        assert len(beams) == 0 and ran and used > 0 and decided > 0 and cut == 0
        rf = recs.view(np.float32)
        live = np.flatnonzero(rf[:, 0] <= rf[:, 1])      # (records with a slope interval: beams with members, not refused)
        assert len(live) == used - refused and (rf[live, 13] == np.inf).all(), "a beam of the empty bounce has no complete list"
        return
    assert len(beams) > 0 and (cnt <= cap).all() and (li < n_lists).all() and len(np.unique(li)) == len(li)
    row_l = np.repeat(li, cnt)
    row_e = np.concatenate([np.arange(c) for c in cnt])
    row_b = np.repeat(beams, cnt)
    rows, got = lists[row_l, row_e], ent[row_l, row_e]
    v = rows.view(np.float32)
    want = plane_and_bounds(v[:, 0:3].copy(), v[:, 4:7].copy(), v[:, 8:11].copy(), pad_abs).view(np.uint32)
    bad = np.flatnonzero((got != want).any(1))
    print("%s bounce %d: %d beams with entries, %d entries in lists of %d, pad_abs %g, %d entries differ" % (name, b, len(beams), len(rows), cap, pad_abs, len(bad)))
    assert len(bad) == 0, "entry %d of list %d: stored %r, recomputed %r" % (row_e[bad[0]], row_l[bad[0]], got[bad[0]].view(np.float32), want[bad[0]].view(np.float32))
    # ---- the two words the list test takes from the stored part in place of the list's own: begin depth and id
    assert begin_id.shape == (n_lists, cap, 2) and np.array_equal(begin_id[row_l, row_e], rows[:, [7, 3]])
    # ---- the documented read-back
    assert (rows[:, 12:16] == 0).all()
    assert np.array_equal(rows[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]], np.ascontiguousarray(sd.tri, np.float32).view(np.uint32)[rows[:, 3].astype(np.int64)])
    f = np.float32
    rf = recs.view(f)
    dom, neg = (row_b % 6) // 2, (row_b % 6) % 2 == 1
    wf = want.view(f)
    k = np.arange(len(rows))
    begin = np.where(neg, rf[row_b, 12] - wf[k, 7 + dom], wf[k, 4 + dom] - rf[row_b, 12]).astype(f) - rf[row_b, 11]
    assert begin.dtype == f and np.array_equal(begin.view(np.uint32), rows[:, 7]), "v1.w is not the depth at which the padded bounds begin"
    # ---- not vacuous
    if b == 1: assert len(rows) >= E, "fewer entries at bounce 1 than scan-lines"
    if name == "liver_cap3_pool2" and b >= 2:
        assert n_lists == 2 and (li == n_lists - 1).any(), "the last list of the pool is not in use: lists %r" % li.tolist()
    if name.startswith("liver_cap3"): assert (cnt == 3).any(), "no list is full"
    if scene == "soup" and b == 1:
        ids = set(rows[:, 3].tolist())
        for what, t in zip(SPECIAL, _special["soup"]):
            assert t in ids, "the %s triangle (%d) is in no list of bounce 1" % (what, t)
        zero = want[rows[:, 3] == _special["soup"][0]][0].view(f)
        assert (zero[:4] == 0).all(), "the zero-area triangle's plane is %r" % zero[:4]


# ------------------------------------------------------------------ same answers
CASES = {
    "order": bo.Case("liver", bo.forced(4, bo.DEEP), (1, 2, 3, 4)),
    "queue_order": bo.Case("liver", bo.forced(4, 0), (1, 2, 3, 4)),
    # pad lanes
    "s96": bo.Case("liver", bo.forced(4, bo.DEEP), (1, 2, 3, 4), S=96, pads=True),
    # capacities 1 and 3: the pair loop's second fetch lies past the list
    "cap1": bo.Case("liver", bo.forced(4, bo.DEEP, MCRT_BEAM_CAP=1), (1, 2, 3, 4), expect="walked"),
    "cap3": bo.Case("liver", bo.forced(4, bo.DEEP, MCRT_BEAM_CAP=3), (1, 2, 3, 4), expect="none"),
    "cap4": bo.Case("liver", bo.forced(4, bo.DEEP, MCRT_BEAM_CAP=4), (1, 2, 3, 4), expect="none"),
    # the second pass reads the same entries from their third on
    "cap4_near2": bo.Case("liver", bo.forced(4, bo.DEEP, MCRT_BEAM_CAP=4, MCRT_BEAM_NEAR=2), (1, 2, 3, 4), expect="none"),
    # nearly every ray walked
    "one_group": bo.Case("liver", bo.forced(4, bo.DEEP, MCRT_BEAM_GROUPS=1), (1, 2, 3, 4), expect="one_group"),
    "shard": bo.Case("liver", bo.forced(4, bo.DEEP), (1, 2, 3, 4), E=12, e0=4, e1=12),
    "soup": bo.Case("soup", bo.forced(4, bo.DEEP), (1, 2, 3, 4), expect="none"),
}


@pytest.mark.parametrize("name", list(CASES))
def test_hits_and_rf_bit_identical_with_stored_planes(mcrt, name):
    case = CASES[name]
    _scene(mcrt, case.scene)
    off, on = bo._beams_off(mcrt, case), bo._run(mcrt, case, case.env)
    bo._check(case, name, off, on)
    for which in (4, 5):      # the debug call, the pass: the lists decided rays, so list_tri_test accepted hits
        decided = [on[which][b][0][1] for b in case.beamed]
        if name in ("cap1", "one_group"): assert sum(decided) > 0, (name, which, decided)
        else: assert decided[0] > 0 and sum(decided[1:]) > 0, (name, which, decided)
        if name == "cap4_near2":      # lists cut at 4 entries, and rays the first two entries left open: the second pass has tested entries
            for b in case.beamed:
                (ran, dec, walked, cut, *_), _ = on[which][b]
                print("%s %s bounce %d: decided %d walked %d cut %d" % (name, ("debug call", "pass")[which - 4], b, dec, walked, cut))
            assert all(on[which][b][0][3] > 0 for b in (1, 2)) and decided[0] > 0 and decided[1] > 0, (name, which)
