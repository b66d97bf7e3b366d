"""Retiring paths that have left the image (FrameArgs::retire_late) and folding bounce 0 of a silent start medium into k_shade
(FrameArgs::fold_b0) leave every RF image BIT-identical: mcrt_trace_frames with both on, each alone and both off (MCRT_TUNING=1
MCRT_RETIRE_LATE=0|1 MCRT_FOLD_B0=0|1, read in mcrt_create; the library's defaults are retirement on, fold off), viewed as int32.

No case can pass vacuously.  A debug call of the same frame (hit / segment tables asked for: retirement and fold are off there by
construction) must show a live segment whose start time distance_traveled * 1000 / sos is past BOTH limits -- max_travel and the image's
end row_thr[n_rows] -- i.e. a path the retirement ends early, and a bounce-0 segment with a non-zero reflected_intensity, i.e. an echo the
fold adds.  Whether the fold really ran is read from the launch counts (mcrt_enable_timing(2)): a staged pass with the fold has one k_march
launch per scan-line group fewer than without; where the fold must switch itself off (the latency form, a start material that is not silent,
S not a multiple of 256) the counts are equal.

n_rows: mcrt_set_params accepts 1 .. 2048 (MCRT_MAX_ROWS) whatever max_rows = sos * max_travel / axial_res_um is (465 at the defaults), so
the image may end before max_travel (n_rows 300: 64.4 us against 100) or after it (n_rows 520: 111.6 us) -- the case the second limit of
the retirement exists for."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COMBOS = {"both": (1, 1), "retire_only": (1, 0), "fold_only": (0, 1)}       # (MCRT_RETIRE_LATE, MCRT_FOLD_B0), each against (0, 0)
STAGED = {"MCRT_PATH_MAX": 0}                                                  # no pass takes the latency form


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


def _limits(mcrt, p):
    """(max_travel, the image's end) in us, as the library derives them (mcrt_api.cpp derive_consts, mcrt_row_thresholds)"""
    axial_um = int(np.float32(np.float32(np.float32(1.45) / np.float32(p.frequency)) * np.float32(1000.0)))
    row_dt = float(axial_um) / float(p.speed_of_sound)
    return (p.depth_cm / float(p.speed_of_sound)) * 10000.0, float(mcrt.host_row_thresholds(row_dt, p.n_rows)[-1])


class Case:
    def __init__(self, scene, E=8, S=256, F=2, frame=3, e0=0, e1=None, env=STAGED, fold=True, groups=1, poses=False, combos=tuple(COMBOS), nan_b0=False,
                 late_share=None, **params):
        self.scene, self.E, self.S, self.F, self.frame, self.e0, self.e1 = scene, E, S, F, frame, e0, E if e1 is None else e1
        self.env, self.fold, self.groups, self.poses, self.combos, self.nan_b0, self.late_share, self.params = env, fold, groups, poses, combos, nan_b0, late_share, params


def _scene(mcrt, name):
    s = mcrt.synth
    cfg, meshes = {"sphere": lambda: s.sphere_scene(3), "liver": lambda: s.liver_scene(3), "random": lambda: s.random_scene(100000, 8, seed=99),
                   "random1m": lambda: s.random_scene(1_000_000, 8, 12345),
                   "sphere_loud_gel": lambda: s.sphere_scene(3, {"GEL": {"mu0": 0.3, "sigma": 0.2}})}[name]()
    return cfg, mcrt.scene_io.build_scene(cfg, meshes)


CASES = {
    # the three workloads at test size, staged form (the sphere scene is 19.5 cm deep: its paths go late once the image ends at 10 cm)
    "sphere": Case("sphere", depth_cm=10.0, n_rows=300),
    "liver": Case("liver"),
    "random": Case("random"),
    # pass sizes either side of path_max: 2048 paths take the latency form (k_path: retirement only, the fold switches itself off), 6144 the staged one
    "latency_form": Case("random", F=1, env={"MCRT_PATH_MAX": 4096}, fold=False),
    "staged_above_path_max": Case("random", F=3, env={"MCRT_PATH_MAX": 4096}),
    "latency_form_liver_groups": Case("liver", F=2, env={"MCRT_PATH_MAX": 1 << 20}, fold=False),
    # a pose per frame
    "poses": Case("liver", F=3, poses=True),
    # a scan-line shard (e0 > 0) traced as two scan-line groups, two k_shade workgroups per scan-line
    "shard_two_groups": Case("liver", E=12, S=512, e0=4, e1=12, env=dict(STAGED, MCRT_GROUPS=2), groups=2),
    # the image ends before / after max_travel
    "rows_below_max_rows": Case("liver", n_rows=300),
    "rows_above_max_rows": Case("liver", n_rows=520),
    # many late paths: the headline scene (4.1 % of the whole frame's queries are late), bounce 1 walked as ray packets
    "headline_many_late": Case("random1m", E=16, env=dict(STAGED, MCRT_PACKET_FROM=0), combos=("both",), late_share=0.01, nan_b0=True),
    # the fold must switch itself off: a start material that scatters; S not a multiple of 256
    "start_not_silent": Case("sphere_loud_gel", fold=False, depth_cm=10.0, n_rows=300),
    "samples_not_256": Case("liver", S=192, fold=False),
    # NaN echoes (total internal reflection at bounce 0) and their flags through the fold, and sanitize_tir removing them
    "tir_nan": Case("random", E=32, sanitize_tir=0, nan_b0=True),
    "tir_sanitized": Case("random", E=32, sanitize_tir=1),
}


def _setup(mcrt, case, cfg, sd, tr, env):
    ctx = _context(mcrt, dict(case.env, **env))
    ctx.set_params(n_elements=case.E, n_samples=case.S, frequency=tr.frequency, **case.params)
    ctx.upload_scene(sd); ctx.upload_texture(None, 256); ctx.set_transducer(tr.pos, tr.dir)
    return ctx


def _trace(mcrt, case, ctx, poses):
    """-> (the pass's RF images [F][ne][R] as int32, k_march launches of one more, timed, pass)"""
    ne, R = case.e1 - case.e0, ctx.params.n_rows
    dev = ctx.alloc(case.F * ne * R * 4)
    try:
        def go():
            if poses is not None: ctx.trace_frames_poses(case.frame, poses[0], poses[1], dev, case.e0, case.e1)
            else: ctx.trace_frames(case.frame, case.F, dev, case.e0, case.e1)
            ctx.synchronize()
        go()
        img = ctx.d2h(dev, (case.F, ne, R), np.float32).view(np.int32).copy()
        ctx.enable_timing(2); ctx.kernel_times(reset=True)
        go()
        n_march = ctx.kernel_times(reset=True)["march"][1]
        ctx.enable_timing(False)
        again = ctx.d2h(dev, (case.F, ne, R), np.float32).view(np.int32)
        assert np.array_equal(img, again), "the timed pass differs from the plain one"
        return img, n_march
    finally:
        ctx.free(dev)


def _debug(case, ctx):
    ne, R = case.e1 - case.e0, ctx.params.n_rows
    dev = ctx.alloc(ne * R * 4)
    try:
        hits, segs, cnt = ctx.trace_frame_debug(case.frame, dev, case.e0, case.e1, want_segs=True)
        return hits, segs, cnt, ctx.d2h(dev, (ne, R), np.float32).view(np.int32).copy()
    finally:
        ctx.free(dev)


@pytest.mark.parametrize("name", list(CASES))
def test_rf_bit_identical_with_retirement_and_fold(mcrt, name):
    case = CASES[name]
    cfg, sd = _scene(mcrt, case.scene)
    tr = mcrt.Transducer(case.E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    poses = None
    if case.poses:
        sweep = [mcrt.Transducer(case.E, position=cfg["transducerPosition"], angles_deg=np.asarray(cfg["transducerAngles"], np.float64) + np.array([4.0 * f - 4.0, 0.0, 0.0]))
                 for f in range(case.F)]
        poses = (np.stack([t.pos for t in sweep]), np.stack([t.dir for t in sweep]))
        tr.pos, tr.dir = sweep[0].pos, sweep[0].dir                       # the debug call below traces frame `frame` with the first pose
    off = _setup(mcrt, case, cfg, sd, tr, {"MCRT_RETIRE_LATE": 0, "MCRT_FOLD_B0": 0})
    try:
        # ---- the case is not vacuous: from the tables of a debug call (every path to its end) ----
        hits, segs, cnt, rf_dbg = _debug(case, off)
        B = segs.shape[2]
        live = np.arange(B)[None, None, :] < cnt[:, :, None]
        max_travel, image_end = _limits(mcrt, off.params)
        t_start = segs["distance_traveled"] * 1000.0 / float(off.params.speed_of_sound)
        late = live & (t_start >= max_travel) & (t_start >= image_end)
        assert not late[:, :, 0].any()
        assert late.any(), "no path of this case is ever retired"
        if case.late_share is not None:
            share = late.sum() / live.sum()
            print("late share of the closest-hit queries: %.4f (%d of %d)" % (share, late.sum(), live.sum()))
            assert share >= case.late_share
        refl0 = segs["reflected_intensity"][:, :, 0]
        assert (live[:, :, 0] & (refl0 != 0)).any(), "no bounce-0 boundary echo in this case"
        if case.nan_b0:
            assert np.isnan(refl0[live[:, :, 0]]).any(), "no NaN boundary echo at bounce 0 in this case"
        mats = np.asarray(sd.materials, np.float32).reshape(-1, 8)
        assert (mats[sd.start_mat, 2] == 0 and mats[sd.start_mat, 4] == 0) == (case.scene != "sphere_loud_gel")
        ref, march_off = _trace(mcrt, case, off, poses)
        assert np.count_nonzero(ref) > 0
        if not case.poses:
            assert np.array_equal(ref[0], rf_dbg), "the debug call's image of the first frame differs from the pass's"
        for combo in case.combos:
            retire, fold = COMBOS[combo]
            on = _setup(mcrt, case, cfg, sd, tr, {"MCRT_RETIRE_LATE": retire, "MCRT_FOLD_B0": fold})
            try:
                img, march_on = _trace(mcrt, case, on, poses)
                assert np.array_equal(img, ref), "%s: RF image not bit-identical (%d of %d words differ)" % (combo, np.count_nonzero(img != ref), ref.size)
                assert march_off - march_on == (case.groups if (fold and case.fold) else 0), (combo, march_off, march_on)
                # hit and segment tables are asked for: every path is shown to its end whatever the knobs say
                h2, s2, c2, rf2 = _debug(case, on)
                assert np.array_equal(c2, cnt) and np.array_equal(h2, hits) and s2.tobytes() == segs.tobytes() and np.array_equal(rf2, rf_dbg), combo
                # ... and so does a counting pass
                on.enable_stats(True); on.get_stats(reset=True); off.enable_stats(True); off.get_stats(reset=True)
                i_on, _ = _trace(mcrt, case, on, poses); i_off, _ = _trace(mcrt, case, off, poses)
                st_on, st_off = on.get_stats(reset=True), off.get_stats(reset=True)
                on.enable_stats(False); off.enable_stats(False)
                assert st_on == st_off and st_on["segments"] > 0 and np.array_equal(i_on, ref) and np.array_equal(i_off, ref), (combo, st_on, st_off)
            finally:
                on.close()
    finally:
        off.close()
