"""The tracer at constants that are NOT the reference's: mcrt_params is the run-time form of the reference's compile-time constants, the
scene carries a spacing and may lie anywhere, and k_march / shade_path / prepare_tables hold a stack of gates keyed on exactly those numbers
(the verified reciprocal quotient, lean_bound, the padded LDS image of the fast kernel, row_near's guess, the loop test t < max_travel, the
|echo| >= 1024 flag, the tables cached by parameter).  The image must not depend on which side of a gate a step falls; the oracle
(oracle/mcrt_oracle.c) takes every one of these parameters and does the plain thing with them: a true division x / res, a true t / row_dt.

The comparison is the same everywhere and has no tolerance: hit indices of mcrt_trace_frame_debug == the oracle's, and the RF image -- of
the debug call (every path to its end) AND of a plain mcrt_trace_frame (late paths retired, the form the knobs choose) -- == the oracle's
fixed-point image viewed as uint32, NaN pattern included.  The oracle walks the context's own BVH4 (set_bvh4, use_bvh=2).  Unless a case
says otherwise it is traced in both forms, which reach k_march through different segment hand-outs: staged (MCRT_PATH_MAX=0: a walk / shade /
march launch per bounce) and latency (the default path_max: k_path, then one k_march over all bounces).

Every "condition from the oracle" is asserted BEFORE the GPU comparison of its case, from the oracle's segments alone, so that a case cannot
pass without carrying the work it is there for; the figures observed are in each test's docstring."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32 = np.float32
FORMS = {"staged": {"MCRT_PATH_MAX": 0}, "latency": {}}
THIRD = float(F32(1.0) / F32(3.0))


def _context(mcrt, env):
    """a Context created under MCRT_TUNING=1 + `env`; the environment is restored before it is used (the knobs are read in mcrt_create)"""
    env = dict({k: str(v) for k, v in env.items()}, MCRT_TUNING="1")
    prev = {k: os.environ.get(k) for k in env}
    try:
        os.environ.update(env)
        return mcrt.Context(0)
    finally:
        for k, v in prev.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v


class Consts:
    """derive_consts (mcrt_api.cpp; main.cpp:23-37, rfimage.h:35,180) worked out here, not asked of the library"""

    def __init__(self, frequency=4.5, speed_of_sound=1500, depth_cm=15.0):
        self.sos = int(speed_of_sound)
        self.axial_res_f = F32(1.45) / F32(frequency)
        self.axial_res_mm = float(self.axial_res_f)
        self.axial_res_um = int(F32(self.axial_res_f * F32(1000.0)))
        self.time_step = (self.axial_res_mm * 1000.0) / float(speed_of_sound)
        self.row_dt = float(self.axial_res_um) / float(speed_of_sound)
        self.inv_row_dt = 1.0 / self.row_dt
        self.max_travel = (depth_cm / float(speed_of_sound)) * 10000.0
        self.max_rows = (speed_of_sound * int(self.max_travel)) // self.axial_res_um


def _lean_bound(tex_res):
    """fill_pass: 2^31 * tex_res * (1 - 2^-20) in float, capped at 1e18; the lean cell needs tex_res > 1e-16 (prepare_tables)"""
    if not tex_res > 1e-16:
        return F32(0.0)
    lim = F32(F32(2147483648.0) * F32(tex_res)) * (F32(1.0) - F32(2.0 ** -20))
    return min(lim, F32(1e18))


def _census(o, sd, k, tex_res=0.145, chunk=2048):
    """The reference's accumulation loop (main.cpp:112-140) replayed in numpy from the ORACLE's segments -- the float32 point recursion
    point += delta and the double time recursion t += time_step, both sequential sums -- and its valid steps (step < steps and
    t < max_travel) counted by the branch of k_march they take:
      a  reach < lean_bound                      (vox_cell_lean / vox_cell_lean256_v)
      b  general branch, every |q| < 2^31        (vox_index: (int)q)
      c  some 2^31 <= |q| < 2^63                 ((long long)q)
      d  some |q| beyond 2^63, or not finite     (the "indefinite" value)
    with q = coordinate / tex_res in float.  k_march's `reach` is the abs_sum of the first and the last of a lane's H points; here a step
    stands for itself: reach ~ 2 * abs_sum(its point).  Counted twice: over every valid step ("steps", a .. d, "negative"), and under "loud"
    over the steps k_march really takes -- those of segments whose medium scatters (mu0 or sigma != 0; the others it skips as exact no-ops,
    the texture being finite).  Also: the segments the loop test t < max_travel cuts short of steps_from(dist / axial_res_mm) ("cut"), and
    those of them whose first refused step would still have had a row in the derived image of max_rows rows ("cut_in_image")."""
    segs, cnt = o["segs"], o["seg_count"]
    sg = segs[np.arange(segs.shape[2])[None, None, :] < cnt[:, :, None]]
    mats = np.asarray(sd.materials, np.float32).reshape(-1, 8)
    loud = (mats[sg["media"], 2] != 0) | (mats[sg["media"], 4] != 0)
    bound, res = _lean_bound(tex_res), F32(tex_res)
    n = dict(a=0, b=0, c=0, d=0, steps=0, negative=0, segments=int(sg.shape[0]), with_steps=0, cut=0, cut_in_image=0, loud=dict(a=0, b=0, c=0, d=0, steps=0, negative=0))
    kmax = int(k.max_travel / k.time_step) + 3
    for c0 in range(0, sg.shape[0], chunk):
        s = sg[c0:c0 + chunk]
        df = s["to"] - s["from"]
        dist_f = np.sqrt(df[:, 0] * df[:, 0] + df[:, 1] * df[:, 1] + df[:, 2] * df[:, 2]) * F32(10.0)
        q = dist_f.astype(np.float64) / k.axial_res_mm
        ok = np.abs(q) < 9.2233720368547758e18
        steps = np.where(ok, np.where(ok, q, 0.0).astype(np.int64) & 0xffffffff, 0)
        K = int(min(max(int(steps.max()), 1), kmax))
        t = np.empty((s.shape[0], K), np.float64); t[:, 0] = s["distance_traveled"] * 1000.0 / float(k.sos); t[:, 1:] = k.time_step
        t = np.cumsum(t, axis=1)
        valid = (np.arange(K)[None, :] < steps[:, None]) & (t < k.max_travel)
        n["with_steps"] += int((steps > 0).sum()); nv = valid.sum(1)
        cut = (steps > 0) & (nv < steps)
        refused = t[np.arange(s.shape[0]), np.minimum(nv, K - 1)]              # the time of the first step the loop test refuses
        n["cut"] += int(cut.sum()); n["cut_in_image"] += int((cut & (refused / k.row_dt < k.max_rows)).sum())
        p = np.empty((s.shape[0], K, 3), np.float32); p[:, 0] = s["from"]; p[:, 1:] = (k.axial_res_f * s["dir"])[:, None, :]
        p = np.cumsum(p, axis=1, dtype=np.float32)
        with np.errstate(over="ignore", invalid="ignore"):
            aq = np.abs(p / res).max(axis=2)
        reach = ((np.abs(p[:, :, 0]) + np.abs(p[:, :, 1])) + np.abs(p[:, :, 2])) * F32(2.0)
        neg = (p < 0).any(axis=2)
        for out, v in ((n, valid), (n["loud"], valid & loud[c0:c0 + chunk, None])):
            a = v & (reach < bound)
            g = v & ~a
            out["a"] += int(a.sum()); out["b"] += int((g & (aq < 2.0 ** 31)).sum()); out["c"] += int((g & (aq >= 2.0 ** 31) & (aq < 2.0 ** 63)).sum())
            out["d"] += int((g & ~(aq < 2.0 ** 63)).sum()); out["steps"] += int(v.sum()); out["negative"] += int((v & neg).sum())
    return n


def _texture(orc, tex256, n):
    return tex256 if n == 256 else orc.texture(n)


class Rig:
    """a scene, a probe and a texture on a context of one form, and the oracle of the same configuration"""

    def __init__(self, mcrt, orc, sd, pos, dirs, tex, tex_n, env=(), **params):
        self.mcrt, self.orc, self.sd, self.pos, self.dirs, self.tex = mcrt, orc, sd, np.ascontiguousarray(pos, np.float32), np.ascontiguousarray(dirs, np.float32), tex
        self.ctx = _context(mcrt, dict(env))
        try:
            self.ctx.set_params(n_elements=self.pos.shape[0], tex_n=tex_n, **params)
            self.ctx.upload_scene(sd); self.ctx.upload_texture(None if tex_n == 256 else tex, tex_n); self.ctx.set_transducer(self.pos, self.dirs)
        except Exception:
            self.ctx.close()
            raise
        self.osc = None

    def close(self):
        self.ctx.close()

    def consts(self):
        p = self.ctx.params
        return Consts(p.frequency, p.speed_of_sound, p.depth_cm)

    def oracle(self, frame, want_segs=True):
        """the oracle at the context's parameters, walking the context's tree"""
        p = self.ctx.params
        if self.osc is None:
            self.osc = self.orc.OracleScene(self.sd.tri, self.sd.tri_mesh, self.sd.meshes, self.sd.materials, self.sd.start_mat, self.sd.spacing)
            self.osc.set_bvh4(self.ctx.get_bvh4()[0], self.ctx.get_bvh()[1])
        op = self.orc.default_params(n_elements=p.n_elements, n_samples=p.n_samples, max_depth=p.max_depth, n_rows=p.n_rows, frequency=p.frequency,
                                     intensity_epsilon=p.intensity_epsilon, initial_intensity=p.initial_intensity, ray_start_offset=p.ray_start_offset,
                                     sos=p.speed_of_sound, depth_cm=p.depth_cm, seed=p.seed, sanitize_tir=p.sanitize_tir, tex_n=p.tex_n, tex_res=p.tex_res)
        return self.osc.trace_frame(op, self.pos, self.dirs, self.tex, frame_id=frame, use_bvh=2, n_threads=16, want_segs=want_segs, want_ref=False)

    def gpu(self, frame):
        """-> (hit indices and RF image of a debug call, RF image of a plain mcrt_trace_frame), images [R][E]"""
        E, R = self.ctx.params.n_elements, self.ctx.params.n_rows
        dev = self.ctx.alloc(E * R * 4)                                  # (a buffer per call: E * R changes under the live-context test)
        try:
            hits, _, _ = self.ctx.trace_frame_debug(frame, dev)
            rf_dbg = self.ctx.export_rf(dev, E, R)
            self.ctx.trace_frame(frame, dev); self.ctx.synchronize()
            return hits, rf_dbg, self.ctx.export_rf(dev, E, R)
        finally:
            self.ctx.free(dev)

    def check(self, frame, o, what=""):
        hits, rf_dbg, rf = self.gpu(frame)
        assert np.array_equal(hits, o["hits"]), "%s: hit indices differ from the oracle's (%d of %d)" % (what, np.count_nonzero(hits != o["hits"]), hits.size)
        _same(rf_dbg, o["rf"], what + ": RF of the debug call")
        _same(rf, o["rf"], what + ": RF of mcrt_trace_frame")
        return rf


def _same(rf, ref, what):
    a, b = rf.view(np.uint32), ref.view(np.uint32)
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        r, e = bad[0]
        raise AssertionError("%s not bit-identical to the oracle's: %d of %d words differ, first at row %d scan-line %d: %r (0x%08x) against %r (0x%08x)"
                             % (what, bad.shape[0], a.size, r, e, rf[r, e], a[r, e], ref[r, e], b[r, e]))


SCENES = {}


def _scene(mcrt, name):
    """(config, SceneData) of the named scene, built once"""
    if name not in SCENES:
        s = mcrt.synth
        cfg, meshes = {"sphere": lambda: s.sphere_scene(5), "random": lambda: s.random_scene(20000, 8), "liver": lambda: s.liver_scene(2),
                       "sphere_loud_gel": lambda: s.sphere_scene(3, {"GEL": {"mu0": 0.3, "sigma": 0.2}})}[name]()
        SCENES[name] = (cfg, mcrt.scene_io.build_scene(cfg, meshes))
    return SCENES[name]


def _probe(mcrt, cfg, E, shift=(0.0, 0.0, 0.0)):
    tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    return (tr.pos + np.asarray(shift, np.float32)).astype(np.float32), tr.dir


def _moved(mcrt, sd, shift=(0.0, 0.0, 0.0), spacing=None):
    """the scene with every vertex translated by `shift` (in float32, as the oracle then sees it), or with another spacing"""
    tri = (sd.tri.reshape(-1, 3) + np.asarray(shift, np.float32)).astype(np.float32).reshape(-1, 9)
    return mcrt.scene_io.SceneData(tri, sd.tri_mesh, sd.meshes, sd.materials, sd.material_names, sd.start_mat, sd.spacing if spacing is None else spacing, sd.config)


def _both_forms(mcrt, orc, sd, pos, dirs, tex, tex_n, frame, before=None, after=None, env=(), **params):
    """the configuration traced in both forms against ONE oracle run; before(oracle result, rig): the case's conditions, checked before any
    GPU image is looked at; after(rig, form): what the case asserts of the context once the frame is traced"""
    o = None
    for form, fenv in FORMS.items():
        rig = Rig(mcrt, orc, sd, pos, dirs, tex, tex_n, env=dict(fenv, **dict(env)), **params)
        try:
            if o is None:
                o = rig.oracle(frame)
                if before is not None: before(o, rig)
            rig.check(frame, o, form)
            if after is not None: after(rig, form)
        finally:
            rig.close()
    return o


# ------------------------------------------------------------------ 1. texel size
# every tex_res meets a power-of-two size and 37; every value >= 0.1 also the reference's 256
TEX_RES = [0.145, 0.1, 0.25, 1.0, THIRD, 2e-8, 1e-20, 3e-30]
TEXEL_CASES = [(res, n) for res in TEX_RES for n in ((256, 64, 37) if res >= 0.1 else (64, 37))]
# tools/verify_div_cpu.c, all 2^32 floats: mismatches of the three-operation quotient against x / res inside div_res()'s gate
CPU_MISMATCHES = {0.145: 0, 0.1: 0, 0.25: 0, 1.0: 0, THIRD: 0, 2e-8: 0, 1e-20: 0, 3e-30: 500518838}


@pytest.mark.parametrize("res,tex_n", TEXEL_CASES, ids=["%g-%d" % c for c in TEXEL_CASES])
@pytest.mark.parametrize("scene", ["sphere", "random"])
def test_texel_size_takes_every_voxel_branch(mcrt, orc, tex256, scene, res, tex_n):
    """Pins div_res / k_verify_div (the gate that admits the reciprocal quotient), lean_bound (fill_pass) and both sides of
    `reach < a.lean_bound` in k_march: vox_cell_lean, vox_cell_lean256_v (256^3, k_march<.., FAST>) and vox_cell with vox_index's three
    conversion ranges and `% n` for a size that is no power of two.

    After the frame debug_fast_paths() must follow fill_pass's rule, written out below, with fast_div as tools/verify_div_cpu.c finds it on
    the CPU: ON for every value but 3e-30 (whose quotient overflows: 500 518 838 mismatches).

    Conditions from the oracle (_census: per step, with 2 * abs_sum(point) standing for k_march's reach).  Required of the frame's valid steps:
    2e-8 -- a, b and c each hold >= 1 % (lean_bound is 42.9 units there, and the reference's step of axial_res_f SCENE units carries the sample
    points ten times as far as the segment reaches); 1e-20 and 3e-30 -- d holds >= 50 %; 0.145 -- a holds all.  Observed, E 8 x S 256 x B 6,
    frame 1, (a, b, c, d):
      sphere  2e-8: (356 498, 401 957, 152 986, 0) of 911 441     1e-20, 3e-30: d = all     0.145: a = all
      random  2e-8: (174 336, 192 000, 587 776, 0) of 954 112     1e-20, 3e-30: d = all     0.145: a = all
    k_march takes only the steps of media that scatter (the others are exact no-ops).  On the sphere scene the same conditions are asserted of
    those alone: 2e-8: (189 211, 257 709, 147 897, 0) of 594 817.  On random_scene(20000, 8) they cannot be: its 20 000 triangles are hit by
    two of the eight scan-lines, 99 % of its valid steps lie in the silent GEL, and the 7 936 steps that scatter are all of class a at 2e-8 --
    that scene runs the walk and the segment hand-out at these texel sizes, the sphere scene the voxel branches."""
    cfg, sd = _scene(mcrt, scene)
    pos, dirs = _probe(mcrt, cfg, 8)
    pow2 = tex_n & (tex_n - 1) == 0

    def before(o, rig):
        n = _census(o, sd, rig.consts(), res)
        print("%s tex_res %g: %r" % (scene, res, n))
        for c in ((n, n["loud"]) if scene == "sphere" else (n,)):             # (the random scene: see the docstring)
            assert c["steps"] > 100000 and c["a"] + c["b"] + c["c"] + c["d"] == c["steps"]
            if res == 2e-8:
                assert min(c["a"], c["b"], c["c"]) >= 0.01 * c["steps"], n
            if res in (1e-20, 3e-30):
                assert c["d"] >= 0.5 * c["steps"], n
            if res == 0.145:
                assert c["a"] == c["steps"], n

    def after(rig, form):
        fast_div, lean, rows = rig.ctx.debug_fast_paths()
        assert fast_div == (CPU_MISMATCHES[res] == 0), "k_verify_div disagrees with the CPU's exhaustive check for tex_res %g" % res
        assert lean == (fast_div and res > 1e-16 and pow2 and tex_n <= 1024)
        assert (rows > 0) == (lean and tex_n == 256)

    _both_forms(mcrt, orc, sd, pos, dirs, _texture(orc, tex256, tex_n), tex_n, 1, before, after, n_samples=256, max_depth=6, tex_res=res)


# ------------------------------------------------------------------ 2. a scene that is not at the origin
AWAY = (-300.0, -200.0, 150.0)


@pytest.mark.parametrize("res,tex_n", [(0.145, 256), (0.145, 37), (0.1, 64)], ids=["0.145-256", "0.145-37", "0.1-64"])
@pytest.mark.parametrize("scene", ["sphere", "random"])
def test_scene_at_negative_coordinates(mcrt, orc, tex256, scene, res, tex_n):
    """Scene and probe translated by (-300, -200, +150): pins `(uint32_t)(int)q & mask` (vox_lean1, vox_q_v and its byte permute) and
    `(uint32_t)i % 37` (vox_index) for NEGATIVE quotients, and runs the walk, the half-float node boxes and the pad_abs scale away from
    the origin.

    Condition from the oracle: >= 90 % of the valid steps have a negative coordinate, and of those in scattering media too.  Observed (E 8 x
    S 256 x B 6, frame 2): sphere 916 181 of 916 181 (scattering: 600 764 of 600 764), random 954 112 of 954 112 (7 936 of 7 936): x starts at
    -313.5 and the 0.322-unit steps of 100 us do not reach 0."""
    cfg, sd0 = _scene(mcrt, scene)
    sd = _moved(mcrt, sd0, AWAY)
    pos, dirs = _probe(mcrt, cfg, 8, AWAY)

    def before(o, rig):
        n = _census(o, sd, rig.consts(), res)
        print("%s: %r" % (scene, n))
        assert n["steps"] > 100000 and n["negative"] >= 0.9 * n["steps"] and n["loud"]["steps"] > 0 and n["loud"]["negative"] >= 0.9 * n["loud"]["steps"], n
        assert (o["hits"] >= 0).sum() > 500, "the translated scene is not hit"

    _both_forms(mcrt, orc, sd, pos, dirs, _texture(orc, tex256, tex_n), tex_n, 2, before, n_samples=256, max_depth=6, tex_res=res)


@pytest.mark.parametrize("scene", ["sphere", "random"])
def test_scene_far_out_on_the_x_axis(mcrt, orc, tex256, scene):
    """Scene and probe translated by (+40000, 0, 0) -- inside half-float range, where a float32 coordinate has 1/256 of a unit left and the
    walk's half-float boxes 32 units: hits and RF still equal the oracle's, which sees the same float32 vertices.  Pins the conservative
    rounding of the walked node boxes and pad_abs at a large offset, and the lean voxel quotient at |q| ~ 2.8e5."""
    cfg, sd0 = _scene(mcrt, scene)
    far = (40000.0, 0.0, 0.0)
    sd = _moved(mcrt, sd0, far)
    pos, dirs = _probe(mcrt, cfg, 8, far)

    def before(o, rig):
        assert (o["hits"] >= 0).sum() > 500, "the translated scene is not hit"

    _both_forms(mcrt, orc, sd, pos, dirs, tex256, 256, 2, before, n_samples=256, max_depth=6)


# ------------------------------------------------------------------ 3. the time axis
TIME_CASES = {"sos1540": dict(speed_of_sound=1540), "sos1000": dict(speed_of_sound=1000), "sos3000": dict(speed_of_sound=3000),
              "depth3": dict(depth_cm=3.0), "depth30": dict(depth_cm=30.0), "depth60": dict(depth_cm=60.0), "depth70": dict(depth_cm=70.0),
              "7MHz_sos1540": dict(speed_of_sound=1540, frequency=7.0)}


@pytest.mark.parametrize("case", list(TIME_CASES))
@pytest.mark.parametrize("scene", ["liver", "sphere"])
def test_time_axis(mcrt, orc, tex256, scene, case):
    """speed_of_sound, depth_cm and frequency away from 1500 / 15 / 4.5, each at three image lengths: n_rows = the derived max_rows, half of
    it, and max_rows + 55, each capped at the library's 2048 rows (depth_cm 70 derives 2170).  Pins march_rows (fill_pass: the padded LDS image
    of k_march<.., FAST>, and its cut-off `g < MCRT_MAX_ROWS + 1` that sends a 256^3 texture to the generic kernel WITH the lean cell:
    depth_cm 70 at 1500 m/s gives g = 2173.9), row_near<PADDED> / row_of against mcrt_row_thresholds at other row_dt (322/1540, 322/1000,
    322/3000, 207/1540 us), and the loop test t < max_travel in k_march and shade_path's retirement at 20 .. 467 us.

    rows (debug_fast_paths) must be max(R + 1, int(max_travel * inv_row_dt) + 2) while max_travel * inv_row_dt < 2049, else 0, from this file's own
    arithmetic (Consts).

    Conditions from the oracle (_census, E 8 x S 128 x B 6, frame 3), over the segments with steps:
      depth_cm 3 -- at least 10 % are cut short of steps_from(dist / axial_res_mm) by the loop test t < max_travel.  Observed: liver 3 392 of
        5 056, sphere 2 940 of 2 940 (no step of the sphere scene scatters within 20 us: its GEL is silent as far as the box).
      depth_cm 60 -- none is cut before the image ends: no segment's first refused step would still have had a row in the derived image of
        max_rows rows.  Observed: 0 and 0.  On the liver scene no segment is cut at all (0 of 5 056: every path ends by itself before
        400 us); on the sphere scene 10 of 2 940 are, at 400 us -- paths that have left the box into GEL, whose attenuation of 1e-8 gives a
        segment of millions of steps, so "no segment is cut" cannot hold there at any depth_cm."""
    kw = TIME_CASES[case]
    cfg, sd = _scene(mcrt, scene)
    pos, dirs = _probe(mcrt, cfg, 8)
    k = Consts(kw.get("frequency", 4.5), kw.get("speed_of_sound", 1500), kw.get("depth_cm", 15.0))
    n_rows = sorted({min(2048, k.max_rows), min(2048, k.max_rows // 2), min(2048, k.max_rows + 55)})
    g = k.max_travel * k.inv_row_dt
    for form, fenv in FORMS.items():
        rig = Rig(mcrt, orc, sd, pos, dirs, tex256, 256, env=fenv, n_samples=128, max_depth=6, **kw)
        try:
            for R in n_rows:
                rig.ctx.set_params(n_rows=R)
                o = rig.oracle(3)
                if form == "staged" and R == n_rows[0]:
                    n = _census(o, sd, rig.consts())
                    print("%s %s: %r" % (scene, case, n))
                    assert n["with_steps"] >= 1000
                    if case == "depth3":
                        assert n["cut"] >= 0.1 * n["with_steps"], n
                    if case == "depth60":
                        assert n["cut_in_image"] == 0 and (n["cut"] == 0 or scene == "sphere"), n
                rig.check(3, o, "%s n_rows %d" % (form, R))
                fast_div, lean, rows = rig.ctx.debug_fast_paths()
                assert fast_div and lean
                assert rows == (max(R + 1, int(g) + 2) if g < 2049 else 0), (rows, R, g)
        finally:
            rig.close()


# ------------------------------------------------------------------ 4. intensities, start offset, spacing
def _march_launches(rig, frame):
    """k_march launches of one plain mcrt_trace_frame (mcrt_enable_timing(2))"""
    E, R = rig.ctx.params.n_elements, rig.ctx.params.n_rows
    dev = rig.ctx.alloc(E * R * 4)
    try:
        rig.ctx.enable_timing(2); rig.ctx.kernel_times(reset=True)
        rig.ctx.trace_frame(frame, dev); rig.ctx.synchronize()
        n = rig.ctx.kernel_times(reset=True)["march"][1]
        rig.ctx.enable_timing(False)
        return n
    finally:
        rig.ctx.free(dev)


LOUD = {"S8": (8, 1e6), "S256": (256, 3e7)}


@pytest.mark.parametrize("shape", list(LOUD))
@pytest.mark.parametrize("scene", ["sphere", "sphere_loud_gel"])
def test_finite_echoes_beyond_1024_flag_their_rows(mcrt, orc, tex256, scene, shape):
    """initial_intensity so large that FINITE echoes reach 1024: pins rf_add's `!(fabsf(echo) < 1024.0f)` flag in k_march, reached so far
    only by the NaN echoes of total internal reflection, and the flag words' way through k_finalize beside the bins of a k_shade that folds
    bounce 0.  S 8 with initial_intensity 1e6: the step echoes intensity * scattering pass 1024; the fold needs S % 256 == 0 and switches itself off
    there, so MCRT_FOLD_B0 must change nothing.  S 256 with 3e7 (1e6 scaled by the factor 32 that intensity / S loses, to one digit): the fold IS
    in effect on the sphere scene, whose start medium GEL is silent -- one k_march launch fewer than with MCRT_FOLD_B0=0 -- and not on the scene
    whose GEL scatters.  Staged form (the fold has no other); the fold on / off images must equal each other and the oracle's.

    What this CANNOT reach is the flag's twin in k_shade's fold (mcrt_shade.hip, `fo.refl / S`): the boundary echo is
    reflected_intensity(...) * random_angle (ray.cpp:154-164, :211), two powf of cosines times a cosine -- at most 2 whatever the ray's intensity
    is, so reflected / S is below 1024 unless it is NaN.  The oracle's segments say so: the largest |reflected_intensity| of these frames is 1.76.

    Condition from the oracle: a finite echo >= 1024 flags its row, so the image has NaN bins: >= 1 % of the bins are NaN and >= 50 % are not.
    Observed (E 16, B 6, frame 4), NaN share: S 8 / 1e6: sphere 0.1070, sphere_loud_gel 0.2722; S 256 / 3e7: sphere 0.1343, sphere_loud_gel
    0.3063 (at 3e8 the latter is 0.5755: too many) -- and no segment of these frames has a NaN echo of its own (no total internal reflection), so
    every flag is a finite echo's."""
    S, I0 = LOUD[shape]
    cfg, sd = _scene(mcrt, scene)
    pos, dirs = _probe(mcrt, cfg, 16)
    images, launches, o = {}, {}, None
    for fold in (1, 0):
        rig = Rig(mcrt, orc, sd, pos, dirs, tex256, 256, env={"MCRT_PATH_MAX": 0, "MCRT_FOLD_B0": fold}, n_samples=S, max_depth=6, initial_intensity=I0)
        try:
            if o is None:
                o = rig.oracle(4)
                nan = np.isnan(o["rf"]).mean()
                print("%s %s: NaN share %.4f" % (scene, shape, nan))
                live = np.arange(6)[None, None, :] < o["seg_count"][:, :, None]
                refl = o["segs"]["reflected_intensity"][live]
                assert not np.isnan(refl).any() and np.abs(refl).max() <= 2.0 and np.isfinite(o["segs"]["initial_intensity"][live]).all()
                assert 0.01 <= nan <= 0.5, nan
            images[fold] = rig.check(4, o, "MCRT_FOLD_B0=%d" % fold)
            launches[fold] = _march_launches(rig, 4)
        finally:
            rig.close()
    assert np.array_equal(images[1].view(np.uint32), images[0].view(np.uint32))
    assert launches[0] - launches[1] == (1 if (S % 256 == 0 and scene == "sphere") else 0), launches


@pytest.mark.parametrize("scene", ["liver", "sphere"])
def test_intensity_epsilon(mcrt, orc, tex256, scene):
    """intensity_epsilon 1e-3 and 0.0 at max_depth 16 (MCRT_MAX_BOUNCES): pins shade_path's `intensity > eps` cut and max_ray_length, whose
    log(eps / I) is -inf at 0.0 (the segment handed to the walk is then not finite, and every path ends with its first segment).

    Condition from the oracle: at 1e-3 the mean number of segments per path is below half of what it is at 1e-10.  Observed (E 8 x S 256,
    frame 5; 1e-10 / 1e-3 / 0.0): liver 5.287 / 2.247 / 1.000 -- the condition holds, and is asserted, there.  sphere 2.862 / 1.989 / 1.000:
    its paths are too short for a factor of two (a ray of intensity 1 / 256 loses a bounce, not half of them), so on the sphere scene only
    "fewer" is asserted."""
    cfg, sd = _scene(mcrt, scene)
    pos, dirs = _probe(mcrt, cfg, 8)
    mean = {}

    def before(o, rig):
        mean[len(mean)] = o["seg_count"].mean()

    for eps in (1e-10, 1e-3, 0.0):
        _both_forms(mcrt, orc, sd, pos, dirs, tex256, 256, 5, before, n_samples=256, max_depth=16, intensity_epsilon=eps)
    print("%s: mean segments per path %r" % (scene, mean))
    assert mean[1] < (0.5 if scene == "liver" else 1.0) * mean[0], mean


@pytest.mark.parametrize("offset", [0.0, 2.5])
@pytest.mark.parametrize("scene", ["sphere", "random"])
def test_ray_start_offset(mcrt, orc, tex256, scene, offset):
    """ray_start_offset 0.0 (a bounced ray starts ON the triangle it left) and 2.5 (it starts beyond thin geometry): pins FrameArgs::offs in
    k_init / shade_path against scene.cpp:112-117"""
    cfg, sd = _scene(mcrt, scene)
    pos, dirs = _probe(mcrt, cfg, 8)
    _both_forms(mcrt, orc, sd, pos, dirs, tex256, 256, 6, n_samples=256, max_depth=6, ray_start_offset=offset)


@pytest.mark.parametrize("spacing", [(1.0, 0.5, 2.0), (0.25, 0.25, 0.25)], ids=["1-0.5-2", "0.25"])
@pytest.mark.parametrize("scene", ["sphere", "random"])
def test_spacing(mcrt, orc, tex256, scene, spacing):
    """the scene's spacing (scene.cpp:281-298: distance_in_mm and enlarge), anisotropic and uniform, through SceneData into
    mcrt_upload_scene and into the oracle's scene: pins FrameArgs::sx, sy, sz in shade_path"""
    cfg, sd0 = _scene(mcrt, scene)
    sd = _moved(mcrt, sd0, spacing=spacing)
    pos, dirs = _probe(mcrt, cfg, 8)

    def before(o, rig):
        assert (o["hits"] >= 0).sum() > 500

    _both_forms(mcrt, orc, sd, pos, dirs, tex256, 256, 6, before, n_samples=256, max_depth=6)


# ------------------------------------------------------------------ 5. parameters changed on a live context
@pytest.mark.parametrize("env", [{}, {"MCRT_PATH_MAX": 0, "MCRT_GROUPS": 2}], ids=["latency", "staged_two_groups"])
def test_parameters_changed_on_a_live_context(mcrt, orc, tex256, sphere, env):
    """ONE context, never recreated, walked through a fixed sequence of parameter changes; after each step a frame is traced and compared with
    the oracle at that configuration, and the last image (defaults again) must equal the first bit for bit.  Pins the tables prepare_tables
    caches by parameter -- the row thresholds (n_rows, row_dt), verified_res / fast_div, the material table (axial_res_f, frequency) -- and
    the buffers sized by shape: accumulators and flags (ensure_acc), the work sets (ensure_work), the texture.  Once in the latency form, once
    staged as two scan-line groups.  The scene is the sphere scene with a GEL that scatters: at depth_cm 6 nothing else is in reach, and no
    image of the sequence may be empty.

    The material table's key cannot be caught by a change of frequency: its one entry that depends on it is expf(-attenuation * axial_res_f *
    0.01f * frequency) with axial_res_f = 1.45f / frequency, a product that is 1.45 up to a rounding which expf absorbs (worked out for 2 ..
    12 MHz with these materials: the same floats).  So a twelfth step pins the table through its other input: the plain sphere scene -- other
    materials (a silent GEL), another tree -- is uploaded to the same context and traced."""
    cfg, sd = _scene(mcrt, "sphere_loud_gel")
    pos, dirs = _probe(mcrt, cfg, 8)
    rng = np.random.default_rng(5)
    user = {n: orc.texture(n) * F32(1.0) for n in (37, 64)}
    user[37][..., 0] += rng.normal(size=(37, 37, 37)).astype(np.float32)          # (a user texture that is not the generator's)
    base = dict(n_samples=64, max_depth=6)
    rig = Rig(mcrt, orc, sd, pos, dirs, tex256, 256, env=env, **base)
    defaults = {f: getattr(rig.ctx.params, f) for f in ("tex_res", "speed_of_sound", "depth_cm", "frequency", "n_rows", "n_samples", "max_depth", "initial_intensity", "tex_n")}
    steps = [("defaults", {}), ("tex_res", dict(tex_res=0.25)), ("speed_of_sound", dict(speed_of_sound=1540)), ("depth_cm", dict(depth_cm=6.0)),
             ("frequency", dict(frequency=7.0)), ("n_rows 900", dict(n_rows=900)), ("n_rows 120", dict(n_rows=120)),
             ("n_samples 256", dict(n_samples=256)), ("n_samples 7", dict(n_samples=7)), ("max_depth 16", dict(max_depth=16)), ("max_depth 1", dict(max_depth=1)),
             ("texture 37", dict(tex_n=37)), ("texture 64", dict(tex_n=64)), ("initial_intensity 1e6", dict(initial_intensity=1e6)),
             ("initial_intensity 1", dict(initial_intensity=1.0)), ("defaults again", dict(defaults))]
    try:
        first = last = None
        for name, kw in steps:
            if kw: rig.ctx.set_params(**kw)
            if "tex_n" in kw:
                n = kw["tex_n"]
                rig.tex = tex256 if n == 256 else user[n]
                rig.ctx.upload_texture(None if n == 256 else rig.tex, n)
            o = rig.oracle(7, want_segs=False)
            last = rig.check(7, o, name)
            assert np.count_nonzero(last) > 0, name
            if first is None: first = last
        assert np.array_equal(first.view(np.uint32), last.view(np.uint32)), "back at the defaults the image is not the first one"
        rig.sd, rig.osc = sphere[1], None
        rig.ctx.upload_scene(rig.sd)
        other = rig.check(7, rig.oracle(7, want_segs=False), "another scene")
        assert np.count_nonzero(other) > 0 and not np.array_equal(other.view(np.uint32), first.view(np.uint32))
    finally:
        rig.close()


# ------------------------------------------------------------------ 6. the lane-pair form of k_march on the paths above
@pytest.mark.parametrize("case", ["tex_res_2e-8_n64", "depth70_256"])
def test_lane_pair_march_at_other_constants(mcrt, orc, tex256, sphere, case):
    """k_march<.., 2, ..> (lane pairs, from MCRT_MARCH_PAIRS_FROM = 2^20 paths per pass) at constants other than the reference's: a pass of
    E 16 x S 256 x F 256 = exactly 2^20 paths at tex_res 2e-8 with a 64^3 texture (the generic kernel, both sides of lean_bound and the
    (long long)q range: the census of test_texel_size_takes_every_voxel_branch), and at depth_cm 70 with the 256^3 texture (the generic
    kernel with the lean cell, n_rows 2048).  The pass's first, a middle and the last frame must equal the same frame ids traced one at a
    time (4096 paths: the quad form), and the middle one the oracle's."""
    cfg, sd = sphere
    pos, dirs = _probe(mcrt, cfg, 16)
    kw, tex_n = (dict(tex_res=2e-8), 64) if case == "tex_res_2e-8_n64" else (dict(depth_cm=70.0, n_rows=2048), 256)
    F, f0, E = 256, 11, 16
    rig = Rig(mcrt, orc, sd, pos, dirs, _texture(orc, tex256, tex_n), tex_n, n_samples=256, max_depth=6, **kw)
    try:
        R = rig.ctx.params.n_rows
        dev = rig.ctx.alloc(F * E * R * 4)
        try:
            rig.ctx.trace_frames(f0, F, dev); rig.ctx.synchronize()
            big = rig.ctx.d2h(dev, (F, E, R), np.float32).view(np.uint32)
            for f in (0, 100, F - 1):
                rig.ctx.trace_frame(f0 + f, dev); rig.ctx.synchronize()
                one = rig.ctx.d2h(dev, (E, R), np.float32).view(np.uint32)
                assert np.count_nonzero(one) > 0
                assert np.array_equal(big[f], one), "frame %d of the pass differs from the frame traced alone (%d words)" % (f, np.count_nonzero(big[f] != one))
        finally:
            rig.ctx.free(dev)
        o = rig.oracle(f0 + 100, want_segs=False)
        assert np.array_equal(big[100].T, o["rf"].view(np.uint32)), "frame 100 of the pass differs from the oracle's"
    finally:
        rig.close()
