"""The trees the GPU builds, refits and walks, checked AS STRUCTURES (tests/tree_check.py): every box of the tree a context hands out must
equal, bit for bit, the outward half of the union of the padded bounds below it; every triangle is reached exactly once; the reported
stack bound is the tree's own need.  Device LBVH at leaves of 1..4, host SAH at leaves up to 4 and 8, after uploads, updates and
refits, in a group, and on the scenes where a bottom-up fit or the half rounding can go wrong (tied Morton codes, zero centroid
extent, coordinates beyond +-65504 and inside +-2^-14).  A stale or short box loses only the rays that graze it; here it fails on
the node that has it.  The ray-level companions at the end are held against the oracle's BRUTE FORCE, never against a walk of the
product's own tree."""
import time

import numpy as np
import pytest

import tree_check as tc

pytestmark = pytest.mark.gpu

TINY = np.float32(2.0 ** -14)
NATURAL = ("sphere", "liver", "soup")          # scenes on which a builder is expected to fill its largest leaf
# (builder, environment, largest leaf the builder may make)
CONFIGS = {
    "sah": ("sah", {}, 4),
    "sah_leaf8": ("sah", {"MCRT_SAH_LEAF_MAX": "8", "MCRT_SAH_COST_TRI": "0.001"}, 8),
    "lbvh_leaf1": ("lbvh", {"MCRT_LBVH_LEAF": "1"}, 1),
    "lbvh_leaf2": ("lbvh", {"MCRT_LBVH_LEAF": "2"}, 2),
    "lbvh_leaf3": ("lbvh", {"MCRT_LBVH_LEAF": "3"}, 3),
    "lbvh_leaf4": ("lbvh", {"MCRT_LBVH_LEAF": "4"}, 4),
}
KNOBS = ("MCRT_SAH_LEAF_MAX", "MCRT_SAH_COST_TRI", "MCRT_LBVH_LEAF")


@pytest.fixture(scope="module")
def scenes(mcrt):
    return tc.all_scenes(mcrt)


@pytest.fixture
def knobs(monkeypatch):
    def set_(env):
        monkeypatch.setenv("MCRT_TUNING", "1")
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
    set_({})
    return set_


def _upload(mcrt, sd, builder):
    ctx = mcrt.Context(0)
    try:
        ctx.set_bvh_builder(builder)
        ctx.upload_scene(sd)
    except Exception:
        ctx.close()
        raise
    return ctx


def _tree(ctx):
    nodes4, max_stack = ctx.get_bvh4()
    _, btri, _ = ctx.get_bvh()
    return nodes4, btri, max_stack


def _check(ctx, tri, tri_mesh, leaf_max, what):
    nodes4, btri, max_stack = _tree(ctx)
    try:
        st = tc.check_tree(tri, nodes4, btri, max_stack, True, leaf_max, tri_mesh)
    except tc.TreeError as e:
        raise tc.TreeError("%s: %s" % (what, e)) from None
    assert 0 <= max_stack <= 64, what
    return st, nodes4, btri, max_stack


def _refs(nodes4):
    return tc.slots(nodes4)["ref"].copy()


def _coords(nodes4, axes=(0, 1, 2)):
    rec = tc.slots(nodes4)
    live = rec["ref"] != tc.EMPTY
    return np.concatenate([rec["lo"][live][:, axes].ravel(), rec["hi"][live][:, axes].ravel()])


# ------------------------------------------------------------------ trees as uploaded
@pytest.mark.parametrize("config", list(CONFIGS))
def test_uploaded_trees_are_exact(mcrt, scenes, knobs, config):
    builder, env, leaf_max = CONFIGS[config]
    knobs(env)
    seen = {}
    for name, sd in scenes.items():
        ctx = _upload(mcrt, sd, builder)
        try:
            st, nodes4, _, _ = _check(ctx, sd.tri, sd.tri_mesh, leaf_max, "%s/%s" % (config, name))
        finally:
            ctx.close()
        seen[name] = (st["n_nodes"], st["max_leaf"], st["need"])
        assert st["max_leaf"] <= leaf_max, name
        if builder == "lbvh" and name in NATURAL:
            assert st["max_leaf"] == leaf_max, (name, st["leaf_hist"])          # the knob is really in force: cnt - 1 leaf encodings of k_emit4
        if config == "sah_leaf8":
            assert st["max_leaf"] >= 5, (name, st["leaf_hist"])                 # leaves of 5..8 triangles are really walked
        x = _coords(nodes4, (0,))
        if name == "up7e4":                                                     # half overflow: outwards to +inf, inwards no further than 65504
            assert set(np.unique(x).tolist()) == {65504.0, np.inf}
        if name == "down2e5":
            assert set(np.unique(x).tolist()) == {-65504.0, -np.inf}
        if name == "tiny":                                                      # no subnormal half: 0 and +-2^-14, nothing strictly between
            x = _coords(nodes4)
            assert (x == 0).any() and (x == TINY).any() and (x == -TINY).any() and not ((x != 0) & (np.abs(x) < TINY)).any()
    print("tree_stats %s (nodes, largest leaf, stack): %s" % (config, seen))


def test_device_builder_refuses_seven_triangles(mcrt, scenes, knobs):
    s = scenes["sphere"]
    ctx = mcrt.Context(0)
    try:
        ctx.set_bvh_builder("lbvh")
        with pytest.raises(mcrt.McrtError, match="needs at least 8 triangles"):
            ctx.upload_scene(tc.with_triangles(s, s.tri[-7:], s.tri_mesh[-7:]))
    finally:
        ctx.close()


@pytest.mark.parametrize("config", ["sah", "lbvh_leaf1"])
def test_headline_scene_1m(mcrt, knobs, config):
    builder, env, leaf_max = CONFIGS[config]
    knobs(env)
    cfg, meshes = mcrt.synth.random_scene(1_000_000, 8)
    sd = mcrt.scene_io.build_scene(cfg, meshes)
    ctx = _upload(mcrt, sd, builder)
    try:
        nodes4, btri, max_stack = _tree(ctx)
    finally:
        ctx.close()
    t0 = time.perf_counter()
    try:
        st = tc.check_tree(sd.tri, nodes4, btri, max_stack, True, leaf_max, sd.tri_mesh)
    except tc.TreeError as e:
        raise tc.TreeError("1M/%s: %s" % (config, e)) from None
    dt = time.perf_counter() - t0
    print("tree_stats 1M %s: %s; check_tree alone %.2f s" % (config, st, dt))
    assert st["n_tri"] == 1_000_000 and st["n_nodes"] == len(nodes4) and 1 <= max_stack <= 64
    if builder == "lbvh":
        assert st["max_leaf"] == 1 and st["leaves"] == 1_000_000          # one triangle per leaf, as the knob says
    else:                                                                 # the context walks the host builder's own tree: same nodes, same leaves
        _, hb, h4, hms = mcrt.host_build_bvh4(sd.tri, sd.tri_mesh)
        assert len(h4) == st["n_nodes"] and hms == max_stack and hb.tobytes() == btri.tobytes()
        assert np.array_equal(_refs(h4), _refs(nodes4)) and 1 < st["max_leaf"] <= 4
    assert dt < 60.0                                                      # vectorised: seconds, not a Python loop over 10^6 nodes


# ------------------------------------------------------------------ updates and refits
@pytest.mark.parametrize("config", ["sah", "lbvh_leaf1"])
def test_trees_after_updates_and_refits(mcrt, scenes, knobs, config):
    builder, env, leaf_max = CONFIGS[config]
    knobs(env)
    for name in ("soup", "sphere"):
        sd = scenes[name]
        orig, tm = sd.tri, sd.tri_mesh
        bent = tc.smooth(orig)
        ctx = _upload(mcrt, sd, builder)
        try:
            _check(ctx, orig, tm, leaf_max, "upload")
            ctx.update_triangles(bent)                                           # a rebuild: new tree over the moved vertices
            _check(ctx, bent, tm, leaf_max, "update(smooth)")
            ctx.update_triangles(tc.scaled(orig, tc.HALF_TINY))                  # rebuilt across the half range: inside +-2^-14 ...
            _, nodes, _, _ = _check(ctx, tc.scaled(orig, tc.HALF_TINY), tm, leaf_max, "%s/%s/update(x1e-5)" % (config, name))
            x = _coords(nodes)
            assert not ((x != 0) & (np.abs(x) < TINY)).any() and (x == 0).any()
            ctx.update_triangles(tc.shifted(orig, tc.HALF_BIG_UP))               # ... and beyond 65504
            _, nodes, _, _ = _check(ctx, tc.shifted(orig, tc.HALF_BIG_UP), tm, leaf_max, "%s/%s/update(+7e4)" % (config, name))
            assert set(np.unique(_coords(nodes, (0,))).tolist()) == {65504.0, np.inf}
            ctx.update_triangles(orig)
            st0, nodes0, btri0, ms0 = _check(ctx, orig, tm, leaf_max, "update(back)")
            refs0 = _refs(nodes0)

            def refit(tri, what):
                ctx.refit_triangles(tri)
                st, nodes, btri, ms = _check(ctx, tri, tm, leaf_max, "%s/%s/refit(%s)" % (config, name, what))
                assert ms == ms0 and np.array_equal(_refs(nodes), refs0), what      # a refit keeps the topology and the stack bound
                assert np.array_equal(btri[:, 3].view(np.uint32), btri0[:, 3].view(np.uint32)), what
                return nodes, btri

            refit(bent, "smooth")
            nodes, _ = refit(tc.scaled(orig, tc.HALF_TINY), "x1e-5")              # across the half range: inside +-2^-14 ...
            x = _coords(nodes)
            assert not ((x != 0) & (np.abs(x) < TINY)).any() and (x == 0).any()
            nodes, _ = refit(tc.shifted(orig, tc.HALF_BIG_UP), "+7e4")            # ... and beyond 65504
            assert set(np.unique(_coords(nodes, (0,))).tolist()) == {65504.0, np.inf}
            nodes, btri = refit(orig, "back")
            assert nodes.tobytes() == nodes0.tobytes() and btri.tobytes() == btri0.tobytes()   # back to the first tree, byte for byte
            steps = [bent, tc.smooth(bent), tc.shifted(tc.smooth(tc.smooth(bent)), 0.5)]
            for tri in steps:                                                    # three refits in a row, nothing read in between
                ctx.refit_triangles(tri)
            st, nodes, _, ms = _check(ctx, steps[-1], tm, leaf_max, "three refits in a row")
            assert ms == ms0 and np.array_equal(_refs(nodes), refs0)
        finally:
            ctx.close()


def test_device_builder_is_deterministic(mcrt, scenes, knobs):
    """the same upload twice: the fit order differs between the runs (whichever child arrives second computes the node), unions are order-free"""
    knobs(CONFIGS["lbvh_leaf1"][1])
    for name in ("soup", "twice"):
        out = []
        for run in range(2):
            ctx = _upload(mcrt, scenes[name], "lbvh")
            try:
                nodes4, btri, ms = _tree(ctx)
            finally:
                ctx.close()
            out.append((nodes4.tobytes(), btri.tobytes(), ms))
        assert out[0] == out[1], name


@pytest.mark.parametrize("config", ["sah", "lbvh_leaf1"])
def test_every_group_member_holds_the_same_exact_tree(mcrt, scenes, knobs, config):
    builder, env, leaf_max = CONFIGS[config]
    knobs(env)
    sd = scenes["soup"]
    grp = mcrt.Group([0, 0])
    try:
        grp.set_params(n_elements=8, n_samples=64, tex_n=32)
        grp.set_bvh_builder(builder)
        grp.upload_scene(sd)
        for tri, what in ((sd.tri, "upload"), (tc.smooth(sd.tri), "refit")):
            if what == "refit":
                grp.refit_triangles(tri)
            trees = []
            for r, member in enumerate(grp.members):
                _, nodes4, btri, ms = _check(member, tri, sd.tri_mesh, leaf_max, "%s rank %d after %s" % (config, r, what))
                trees.append((nodes4.tobytes(), btri.tobytes(), ms))
            assert len(trees) == 2 and trees[0] == trees[1], what
    finally:
        grp.close()


# ------------------------------------------------------------------ ray-level companions: against brute force
E, S = 32, 64


def companion_cases(mcrt, scenes, start_offset):
    """name -> (scene, transducer): each moves the PROBE with the scene, so the rays meet the geometry as they do in the plain sphere scene"""
    cfg, _ = mcrt.synth.sphere_scene(3)

    def probe(move):
        tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
        tr.pos, tr.dir = move(tr.pos.astype(np.float32), tr.dir.astype(np.float32)).astype(np.float32), tr.dir.astype(np.float32)
        return tr

    def up(pos, d):
        pos = pos.copy(); pos[:, 0] += np.float32(tc.HALF_BIG_UP)
        return pos

    return {
        "up7e4": (scenes["up7e4"], probe(up)),
        # (a ray starts ray_start_offset along its direction: the scaled probe is pulled back by it, or every ray would start beyond the scene)
        "tiny": (scenes["tiny"], probe(lambda pos, d: pos * np.float32(tc.HALF_TINY) - np.float32(start_offset) * d)),
        # flattened along x: the sphere scene's probe sits at x = -13.5 and its central scan-line runs along +x, so the rays cross the plane
        # x = 0.  Nothing else pins that assumption: if the scene's pose changes, the share >= 0.25 guard of the test is what reports it
        "flat": (scenes["flat"], probe(lambda pos, d: pos)),
        "sphere": (scenes["sphere"], probe(lambda pos, d: pos)),
    }


def oracle_frame(orc, sd, pos, d, tex):
    osc = orc.OracleScene(sd.tri, sd.tri_mesh, sd.meshes, sd.materials, sd.start_mat, sd.spacing)
    p = orc.default_params(n_elements=E, n_samples=S)
    o = osc.trace_frame(p, pos, d, tex, use_bvh=False, n_threads=8, want_segs=True, want_ref=False)      # brute force: no tree at all
    share = float((o["hits"][:, :, 0] >= 0).mean())
    return o, share


COMPANIONS = [("up7e4", "sah"), ("up7e4", "lbvh_leaf1"), ("tiny", "sah"), ("tiny", "lbvh_leaf1"), ("flat", "sah"), ("flat", "lbvh_leaf1"),
              ("sphere", "lbvh_leaf4"), ("sphere", "sah_leaf8")]


@pytest.mark.parametrize("case,config", COMPANIONS)
def test_rays_agree_with_brute_force(mcrt, orc, tex256, scenes, knobs, case, config):
    sd, tr = companion_cases(mcrt, scenes, orc.default_params().ray_start_offset)[case]
    o, share = oracle_frame(orc, sd, tr.pos, tr.dir, tex256)
    assert share >= 0.25, "only %.3f of the bounce-0 queries hit: the case would pass vacuously" % share
    builder, env, leaf_max = CONFIGS[config]
    knobs(env)
    sim = mcrt.Simulator(sd, tr, n_samples=S, texture=tex256, bvh_builder=builder)
    try:
        st, _, _, _ = _check(sim.ctx, sd.tri, sd.tri_mesh, leaf_max, "%s/%s" % (case, config))
        if config == "sah_leaf8":
            assert st["max_leaf"] >= 5
        if config == "lbvh_leaf4":
            assert st["max_leaf"] == 4
        hits, _, cnt = sim.ctx.trace_frame_debug(0, sim.rf_dev, want_segs=True)
        rf = sim.ctx.export_rf(sim.rf_dev, E, sim.R)
    finally:
        sim.close()
    assert np.array_equal(hits, o["hits"]), "hit indices differ from brute force"
    assert np.array_equal(cnt, o["seg_count"]), "segment counts differ from brute force"
    assert np.array_equal(rf.view(np.uint32), o["rf"].view(np.uint32)), "fixed-point RF differs from brute force"
