"""The beam stages (csrc/mcrt_beam.hip) at the tracer's HARD geometry, against the CPU ORACLE -- not against the library's own walk, as tests/test_gpu_beam*.py
compare.  The hard-geometry tests of tests/test_gpu_parity.py and tests/test_gpu_constants.py run passes far below MCRT_BEAM_FROM, so they exercise the lane walk,
the packets or k_path; the beams' margins scale with the largest coordinate, their tie rule goes through a sorted and possibly cut list, their traversal reads
the half-float node boxes after a refit, and none of that had met those inputs.  Here the beams are forced for bounces 1-4 and ordered (MCRT_TUNING=1
MCRT_PATH_MAX=0 MCRT_BEAM_B1=2 MCRT_BEAM_LAST=4, the default MCRT_BEAM_ORDER) in every case:

  ties        the duplicated sphere of test_duplicated_triangles_every_hit_is_a_tie, both builders; at the default capacity and with lists of 3 of which the
              first pass tests 1, so that a cut falls between two twins of equal begin; hits.max() < T
  planes      the 22 elements of test_axis_parallel_rays_and_rays_in_box_planes (zero and negative-zero components, rays in a face plane, along an edge, the face
              diagonal, clamped reciprocals), S = 64, both builders: bounce 1 starts on the box's faces and edges
  refit       test_refit_keeps_frames_exact's deformation of the 50 000-triangle soup, both builders: beams after mcrt_refit_triangles, the oracle walking the
              downloaded refitted tree on the moved triangles
  device tree liver(3) built on the GPU
  far away    sphere(3) and liver(3) moved by test_gpu_constants.py's AWAY and by (40000, 0, 0), where m is 0.16 units and a float32 ulp 0.004; at the far
              shift the counters need only say that the bounces ran by beams and decided + walked is the ray count
  wide beams  the shininess-50 sphere and the shininess-1000 soup of tests/test_gpu_beam_lists.py through whole passes: beams refused, lists cut, rays walked
              and rays decided.  (No list of the sphere's is cut at the default capacity -- its fullest beam holds 175 candidates --, so it is also run with
              lists of 64, where cut > 0 is asserted of it too.)
  fuzz        cases 0-7 of test_randomised_configurations' generator, the same draws; max_depth 1 leaves the beams off

Compared bit for bit in every case: hit indices and segment counts of a debug call, its RF words, and the RF words of the LAST frame of a pass of 3 frames (fuzz:
of its drawn 1-4).  The oracle runs brute force where the scene is small, else it walks the context's downloaded tree.  mcrt_debug_beam_bounce must say of
every case's named bounces that they ran by beams and that the lists decided rays, on the debug call and on the pass; decided + walked of the debug call is the
bounce's ray count.  E <= 24, S <= 256."""
import copy

import numpy as np
import pytest

import beam_mirror as bm
from test_gpu_beam_deep import _context
from test_gpu_constants import AWAY, _moved, _probe

pytestmark = pytest.mark.gpu

BEAMS = {"MCRT_PATH_MAX": 0, "MCRT_BEAM_B1": 2, "MCRT_BEAM_LAST": 4}
FAR = (40000.0, 0.0, 0.0)
B_LOOK = 6


class Run:
    pass


def _gpu(mcrt, sd, pos, dirs, frame, tex256, env=(), builder="sah", tex=None, F=3, first=None, prepare=None, **params):
    """beams forced: a debug call of `frame` and a pass of F frames that ends with it"""
    pos, dirs = np.ascontiguousarray(pos, np.float32), np.ascontiguousarray(dirs, np.float32)
    ctx = _context(mcrt, dict(BEAMS, **dict(env)))
    try:
        ctx.set_bvh_builder(builder)
        ctx.set_params(n_elements=pos.shape[0], **params)
        tex_n = ctx.params.tex_n
        ctx.upload_scene(sd); ctx.upload_texture(None if tex_n == 256 else tex, tex_n); ctx.set_transducer(pos, dirs)
        if prepare is not None: prepare(ctx)
        r = Run()
        r.pos, r.dirs, r.frame, r.tex = pos, dirs, frame, tex256 if tex_n == 256 else tex
        r.p = copy.copy(ctx.params)
        E, R = r.p.n_elements, r.p.n_rows
        dev = ctx.alloc(F * E * R * 4)
        r.hits, _, r.cnt = ctx.trace_frame_debug(frame, dev, want_segs=True)
        r.dbg_call = [ctx.debug_beam_bounce(b) for b in range(B_LOOK + 1)]
        r.rf_dbg = ctx.export_rf(dev, E, R)
        ctx.trace_frames(frame - F + 1 if first is None else first, F, dev); ctx.synchronize()
        r.dbg_pass = [ctx.debug_beam_bounce(b) for b in range(B_LOOK + 1)]
        r.rf_last = np.ascontiguousarray(ctx.d2h(dev, (F, E, R))[F - 1].T)
        ctx.free(dev)
        r.tree = (ctx.get_bvh4()[0], ctx.get_bvh()[1])
        return r
    finally:
        ctx.close()


def _oracle(orc, sd, r, brute):
    p = r.p
    osc = orc.OracleScene(sd.tri, sd.tri_mesh, sd.meshes, sd.materials, sd.start_mat, sd.spacing)
    if not brute: osc.set_bvh4(*r.tree)
    op = orc.default_params(n_elements=p.n_elements, n_samples=p.n_samples, max_depth=p.max_depth, n_rows=p.n_rows, frequency=p.frequency,
                            intensity_epsilon=p.intensity_epsilon, initial_intensity=p.initial_intensity, ray_start_offset=p.ray_start_offset,
                            sos=p.speed_of_sound, depth_cm=p.depth_cm, seed=p.seed, sanitize_tir=p.sanitize_tir, tex_n=p.tex_n, tex_res=p.tex_res)
    return osc.trace_frame(op, r.pos, r.dirs, r.tex, frame_id=r.frame, use_bvh=0 if brute else 2, n_threads=16, want_segs=True, want_ref=False)


def _words(a, b, what):
    x, y = a.view(np.uint32), b.view(np.uint32)
    assert x.shape == y.shape and np.array_equal(x, y), "%s: %d of %d RF words differ from the oracle's" % (what, np.count_nonzero(x != y), x.size)


def _check(r, o, what, decided=(1,), only_ran=False):
    """the counters first (no case passes without its beams), then the comparison"""
    B = r.p.max_depth
    for b in range(B_LOOK + 1):
        n = int((o["seg_count"] > b).sum())
        print("%s bounce %d: %d rays; debug call %s, pass %s" % (what, b, n, r.dbg_call[b], r.dbg_pass[b]))
        for which, d in (("debug call", r.dbg_call[b]), ("pass", r.dbg_pass[b])):
            if not (1 <= b <= 4 and b < B):
                assert d == (False, 0, 0, 0, 0, 0, 0, 0), (what, b, which)
                continue
            assert d[0], "%s: bounce %d did not run by beams in the %s" % (what, b, which)
            if which == "debug call": assert d[1] + d[2] == n, (what, b, d, n)
            if b in decided and not only_ran: assert d[1] > 0, "%s: the lists decided no ray of bounce %d in the %s" % (what, b, which)
    assert np.array_equal(r.cnt, o["seg_count"]), what
    assert np.array_equal(r.hits, o["hits"]), "%s: %d hit indices differ from the oracle's" % (what, np.count_nonzero(r.hits != o["hits"]))
    _words(r.rf_dbg, o["rf"], what + ", debug call")
    _words(r.rf_last, o["rf"], what + ", last frame of the pass")


# ------------------------------------------------------------------ ties
@pytest.mark.parametrize("env", [{}, {"MCRT_BEAM_CAP": 3, "MCRT_BEAM_NEAR": 1}], ids=["default", "cap3_near1"])
@pytest.mark.parametrize("builder", ["sah", "lbvh"])
def test_every_hit_a_tie(mcrt, orc, tex256, builder, env):
    cfg, meshes = mcrt.synth.sphere_scene(3)
    sd0 = mcrt.scene_io.build_scene(cfg, meshes)
    T = sd0.n_tri
    sd = mcrt.scene_io.SceneData(np.concatenate([sd0.tri, sd0.tri]), np.concatenate([sd0.tri_mesh, sd0.tri_mesh]), sd0.meshes, sd0.materials,
                                 sd0.material_names, sd0.start_mat, sd0.spacing, sd0.config)
    pos, dirs = _probe(mcrt, cfg, 16)
    r = _gpu(mcrt, sd, pos, dirs, 5, tex256, env=env, builder=builder, n_samples=128)
    o = _oracle(orc, sd, r, brute=True)
    assert (o["hits"] >= 0).sum() > 16 * 128 // 2 and o["hits"].max() < T, "the oracle itself must pick the smaller twin"
    _check(r, o, "ties %s %s" % (builder, env), decided=(1, 2))
    assert r.hits.max() < T
    if env:      # every list that holds a triangle holds its twin: lists of 3 are cut between twins
        assert r.dbg_call[1][3] > 0 and r.dbg_pass[1][3] > 0, "no list was cut"


# ------------------------------------------------------------------ planes and axes
@pytest.mark.parametrize("builder", ["sah", "lbvh"])
def test_axis_parallel_rays_and_rays_in_box_planes(mcrt, orc, sphere, tex256, builder):
    cfg, sd = sphere
    V = sd.tri.reshape(-1, 3)
    lo, hi = V.min(0), V.max(0)
    tiny, den = np.float32(1e-30), np.float32(1e-45)
    el = [((-13.5, 0, 0), (1, 0, 0)), ((-13.5, 0, 0), (1, -0.0, 0.0)), ((-13.5, 0, 0), (1, 0.0, -0.0)),
          ((-13.5, hi[1], 0), (1, 0, 0)), ((-13.5, hi[1], hi[2]), (1, 0, 0)), ((-13.5, lo[1], 0.5), (1, 0, 0)),
          ((0, 0, 0), (0, 1, 0)), ((0, 0, 0), (0, 0, 1)), ((0, 0, 0), (0, -1, 0)), ((0, 0, 0), (-1, 0, 0)), ((0, 0, 0), (0, 0, -1)),
          ((-13.5, 0, 0), (1, tiny, 0)), ((-13.5, 0, 0), (1, -tiny, den)), ((-13.5, 0, 0), (1, 1e-38, -1e-38)),
          ((-13.5, 2, 0), (1, 0, 0)), ((-13.5, 0, 2), (1, 0, 0)), ((-13.5, 0, 0), (-1, 0, 0)), ((0, hi[1], 0), (0, -1, 0)),
          ((lo[0], lo[1], lo[2]), (1, 1, 1)), ((hi[0], 0, 0), (-1, 0, 0)), ((0, 0, -13.5), (0, 0, 1)), ((0.25, -13.5, 0.25), (0, 1, 0))]
    pos = np.array([e[0] for e in el], np.float32)
    d = np.array([e[1] for e in el], np.float32)
    d[18] /= np.float32(np.sqrt(3.0))
    assert len(el) == 22
    r = _gpu(mcrt, sd, pos, d, 2, tex256, builder=builder, n_samples=64)
    o = _oracle(orc, sd, r, brute=True)
    assert (o["hits"][:, :, 0] >= 0).sum() >= 12 * 64, "most of these rays must hit something"
    _check(r, o, "planes " + builder, decided=(1,))


# ------------------------------------------------------------------ refit
@pytest.mark.parametrize("builder", ["sah", "lbvh"])
def test_beams_after_a_refit(mcrt, orc, tex256, builder):
    cfg, meshes = mcrt.synth.random_scene(50000, 8, seed=7)
    sd = mcrt.scene_io.build_scene(cfg, meshes)
    moved = sd.tri.reshape(-1, 3, 3).copy()
    moved[:, :, 2] += 0.25 * np.cos(0.7 * moved[:, :, 0]) + 0.1 * moved[:, :, 1]        # smooth deformation + shear
    moved = moved.reshape(-1, 9).astype(np.float32)
    pos, dirs = _probe(mcrt, cfg, 24)

    def refit(ctx):
        with ctx.temp(24 * ctx.params.n_rows * 4) as dev:
            ctx.trace_frame(0, dev); ctx.synchronize()                                  # the tree is in use before it is refitted
        ctx.refit_triangles(moved)

    r = _gpu(mcrt, sd, pos, dirs, 6, tex256, builder=builder, prepare=refit, n_samples=192)
    assert np.array_equal(r.tree[1][np.argsort(r.tree[1][:, 3].view(np.uint32))][:, [0, 1, 2, 4, 5, 6, 8, 9, 10]], moved)   # the records carry the new vertices
    sd2 = copy.copy(sd); sd2.tri = moved
    o = _oracle(orc, sd2, r, brute=False)
    assert (o["hits"] >= 0).sum() > 24 * 192 // 4
    _check(r, o, "refit " + builder, decided=(1,))


# ------------------------------------------------------------------ a tree built on the device
def test_device_built_tree(mcrt, orc, tex256):
    cfg, sd = bm.scene(mcrt, "liver")
    pos, dirs = _probe(mcrt, cfg, bm.E)
    r = _gpu(mcrt, sd, pos, dirs, 9, tex256, builder="lbvh", n_samples=bm.S)
    o = _oracle(orc, sd, r, brute=False)
    assert (o["seg_count"] > 3).sum() > 256
    _check(r, o, "liver lbvh", decided=(1, 2, 3))


# ------------------------------------------------------------------ far from the origin
@pytest.mark.parametrize("shift", [AWAY, FAR], ids=["away", "far"])
@pytest.mark.parametrize("scene", ["sphere", "liver"])
def test_scene_away_from_the_origin(mcrt, orc, tex256, scene, shift):
    cfg, sd0 = bm.scene(mcrt, scene)
    sd = _moved(mcrt, sd0, shift)
    pos, dirs = _probe(mcrt, cfg, bm.E, shift)
    r = _gpu(mcrt, sd, pos, dirs, 2, tex256, n_samples=bm.S)
    o = _oracle(orc, sd, r, brute=False)
    assert (o["hits"] >= 0).sum() > 500, "the translated scene is not hit"
    _check(r, o, "%s at %r" % (scene, shift), decided=(1, 2), only_ran=shift == FAR)


# ------------------------------------------------------------------ wide beams through whole passes
@pytest.mark.parametrize("scene,env", [("sphere_shiny50", {}), ("sphere_shiny50", {"MCRT_BEAM_CAP": 64}), ("soup_shiny1000", {})], ids=["sphere", "sphere_cap64", "soup"])
def test_wide_beams(mcrt, orc, tex256, scene, env):
    cfg, sd = bm.scene(mcrt, scene)
    pos, dirs = _probe(mcrt, cfg, bm.E)
    r = _gpu(mcrt, sd, pos, dirs, bm.FRAME, tex256, env=env, n_samples=bm.S)
    o = _oracle(orc, sd, r, brute=False)
    _check(r, o, "wide %s %s" % (scene, env), decided=(1,))
    for which, dbg in (("debug call", r.dbg_call), ("pass", r.dbg_pass)):
        decided, walked, cut, refused = (sum(dbg[b][k] for b in range(1, 5)) for k in (1, 2, 3, 4))
        assert refused > 0 and walked > 0 and decided > 0, (which, decided, walked, cut, refused)
        if scene == "soup_shiny1000" or env: assert cut > 0, (which, decided, walked, cut, refused)


# ------------------------------------------------------------------ fuzz
@pytest.mark.parametrize("case", range(8))
def test_randomised_configurations_by_beams(mcrt, orc, tex256, case):
    """test_randomised_configurations' generator (tests/test_gpu_parity.py), draw for draw, so the oracle side is that test's; every case staged, with beams"""
    rng = np.random.default_rng(1000 + case)
    env = {}
    if case % 4 == 3: env["MCRT_KSPLIT_LIMIT"] = 0
    if case == 6: env["MCRT_GROUPS"] = 2
    if case % 2 == 1:
        env["MCRT_PACKET_BOUNCES"] = hex(int(rng.integers(1, 1 << 16)) | 2); env["MCRT_PACKET_FROM"] = 0
    if case % 3 == 0:
        cfg, meshes = mcrt.synth.random_scene(int(rng.integers(2000, 30000)), 8, seed=int(rng.integers(1, 1000)))
    elif case % 3 == 1:
        cfg, meshes = mcrt.synth.liver_scene(int(rng.integers(1, 3)))
    else:
        cfg, meshes = mcrt.synth.sphere_scene(int(rng.integers(1, 4)))
    sd = mcrt.scene_io.build_scene(cfg, meshes)
    E, S = int(rng.integers(1, 40)), int(rng.integers(1, 200))
    R, B = int(rng.integers(20, 700)), int(rng.integers(1, 17))
    tex_n = int(rng.choice([4, 16, 37, 64, 256]))
    freq = float(rng.choice([2.5, 4.5, 7.0]))
    sanitize = int(rng.integers(0, 2))
    seed = int(rng.integers(0, 2 ** 31))
    F = int(rng.integers(1, 5))
    builder = "lbvh" if (case % 2 and sd.n_tri >= 8) else "sah"
    tex = tex256 if tex_n == 256 else rng.normal(size=(tex_n, tex_n, tex_n, 2)).astype(np.float32)
    tr = mcrt.Transducer(E, frequency=freq, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    frame0 = int(rng.integers(0, 1000))
    what = dict(case=case, E=E, S=S, R=R, B=B, tex_n=tex_n, freq=freq, sanitize=sanitize, F=F, builder=builder, tris=sd.n_tri)
    r = _gpu(mcrt, sd, tr.pos, tr.dir, frame0 + F - 1, tex256, env=env, builder=builder, tex=tex, F=F, first=frame0,
             n_samples=S, n_rows=R, max_depth=B, tex_n=tex_n, frequency=freq, sanitize_tir=sanitize, seed=seed)
    o = _oracle(orc, sd, r, brute=False)
    if B == 1: assert not any(d[0] for d in r.dbg_call + r.dbg_pass), "max_depth 1 must leave the beams off"
    _check(r, o, str(what), decided=())
