"""Bounce 1 by beams (csrc/mcrt_beam.hip: a scan-line's bounce-1 rays tested against the triangles collected once per beam) leaves every
closest hit and every RF image BIT-identical: the beam forced on in every staged pass (MCRT_TUNING=1 MCRT_BEAM_B1=2, read in mcrt_create)
against the beam off (MCRT_BEAM_B1=0) on two contexts -- the hit table of a debug call (every bounce's triangle per path, bounce 1's among
them) and the RF images of a pass of several frames, viewed as int32.

No case passes vacuously: mcrt_debug_beam says whether bounce 1 ran by beams, how many rays the beams' lists decided, how many leftover rays
were walked through the tree, how many beams were cut at their capacity, how many were refused for their spread and how many have rays at
all; each case states what it expects of them.

TIR: a path that meets total internal reflection always reflects (the reflected share of its intensity is 1), so the NaN refraction
direction is never a ray's direction; the case (a start medium of four times the box's impedance) keeps the NaN boundary echoes of
sanitize_tir = 0 beside the beams.  The guard of beam_ray that refuses a ray with a coordinate that is no number ("a NaN proves nothing") is
therefore reached by no scene a host can upload and by no case here: it stands against state that only an error elsewhere could produce."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STAGED = {"MCRT_PATH_MAX": 0}                                                  # no pass takes the latency form (k_path), which has no bounce-1 launch


def _context(mcrt, env):
    env = dict({k: str(v) for k, v in env.items()}, MCRT_TUNING="1")
    prev = {k: os.environ.get(k) for k in env}
    try:
        os.environ.update(env)
        return mcrt.Context(0)
    finally:
        for k, v in prev.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v


_scenes = {}


def _scene(mcrt, name):
    if name not in _scenes:
        s = mcrt.synth
        cfg, meshes = {"sphere": lambda: s.sphere_scene(3), "liver": lambda: s.liver_scene(3), "soup": lambda: s.random_scene(20000, 8, seed=99),
                       "sphere_tir": lambda: s.sphere_scene(3, {"GEL": {"impedance": 8.0}})}[name]()
        _scenes[name] = (cfg, mcrt.scene_io.build_scene(cfg, meshes))
    return _scenes[name]


class Case:
    def __init__(self, scene, E=8, S=256, F=3, frame=3, e0=0, e1=None, env=None, probe=None, poses=False, expect="resolved", nan_b0=False, **params):
        self.scene, self.E, self.S, self.F, self.frame, self.e0, self.e1 = scene, E, S, F, frame, e0, E if e1 is None else e1
        self.env, self.probe, self.poses, self.expect, self.nan_b0, self.params = env or {}, probe, poses, expect, nan_b0, params


CASES = {
    "sphere": Case("sphere"),
    "soup": Case("soup"),
    "liver": Case("liver"),
    # wavefronts straddle scan-lines and histories
    "sphere_s96": Case("sphere", S=96),
    "soup_s96": Case("soup", S=96),
    "liver_s96": Case("liver", S=96),
    # scan-line 2 looks away from the scene: nothing of it reaches bounce 1
    "miss_at_bounce_0": Case("liver", probe="miss"),
    # lists of ONE triangle: a beam that meets a second triangle is incomplete from that triangle's depth on, and the first one begins at the rays' origin, where
    # no ray hits it -- the incomplete-beam and leftover paths (the hand-over between the two passes, gather, the lane walk on counts and cursors of its own,
    # scatter) carry nearly every ray
    "one_entry_sphere": Case("sphere", env={"MCRT_BEAM_CAP": 1, "MCRT_BEAM_NEAR": 1}, expect="leftovers"),
    "one_entry_soup": Case("soup", env={"MCRT_BEAM_CAP": 1, "MCRT_BEAM_NEAR": 1}, expect="leftovers"),
    "one_entry_liver": Case("liver", env={"MCRT_BEAM_CAP": 1, "MCRT_BEAM_NEAR": 1}, expect="leftovers"),
    "one_entry_liver_s96": Case("liver", S=96, env={"MCRT_BEAM_CAP": 1, "MCRT_BEAM_NEAR": 1}, expect="leftovers"),
    # lists of four triangles of which the first pass tests one, the second pass the other three: a cut list still decides the rays that hit before its cut, so
    # here both ways carry rays
    "tiny_lists": Case("liver", env={"MCRT_BEAM_CAP": 4, "MCRT_BEAM_NEAR": 1}, expect="both"),
    "tiny_lists_s96": Case("liver", S=96, env={"MCRT_BEAM_CAP": 4, "MCRT_BEAM_NEAR": 1}, expect="both"),
    # every scan-line exactly along an axis: bounce 0's slopes are 0
    "along_an_axis": Case("soup", probe="axis"),
    # total internal reflection with sanitize_tir off: NaN boundary echoes
    "tir_nan": Case("sphere_tir", sanitize_tir=0, nan_b0=True),
    # a pose per frame: the origins differ from frame to frame, the beam stays off
    "poses": Case("liver", poses=True, expect="off"),
    # a scan-line shard
    "shard": Case("liver", E=12, e0=4, e1=12),
    # where bounce 1 runs as packets by default (MCRT_BEAM_B1=1 is the default; here: packets from the first path), against packets
    "default_where_packets": Case("soup", env={"MCRT_PACKET_FROM": 0, "MCRT_BEAM_FROM": 0}, expect="default"),
    # ... and below the pass size from which the beams are the default (MCRT_BEAM_FROM), packets run
    "default_small_pass": Case("soup", env={"MCRT_PACKET_FROM": 0}, expect="default_off"),
}


def _probe(mcrt, case, cfg):
    tr = mcrt.Transducer(case.E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    if case.probe == "miss":
        tr.dir = tr.dir.copy(); tr.dir[2] = -tr.dir[2]
    if case.probe == "axis":
        mid = tr.dir[case.E // 2]
        k = int(np.argmax(np.abs(mid)))
        d = np.zeros(3, tr.dir.dtype); d[k] = np.sign(mid[k])
        tr.dir = np.tile(d, (case.E, 1))
        assert np.count_nonzero(tr.dir[0]) == 1
    return tr


def _setup(mcrt, case, sd, tr, env):
    ctx = _context(mcrt, dict(STAGED, **dict(case.env, **env)))
    ctx.set_params(n_elements=case.E, n_samples=case.S, frequency=tr.frequency, **case.params)
    ctx.upload_scene(sd); ctx.upload_texture(None, 256); ctx.set_transducer(tr.pos, tr.dir)
    return ctx


def _run(mcrt, case, ctx, poses):
    """-> (hit table of a debug call [ne][S][B], its RF image, the pass's RF images [F][ne][R], mcrt_debug_beam after the pass and after the debug call)"""
    ne, R = case.e1 - case.e0, ctx.params.n_rows
    dev = ctx.alloc(case.F * ne * R * 4)
    try:
        hits, segs, cnt = ctx.trace_frame_debug(case.frame, dev, case.e0, case.e1, want_segs=True)
        beam_dbg = ctx.debug_beam()
        rf_dbg = ctx.d2h(dev, (ne, R), np.float32).view(np.int32).copy()
        if poses is not None: ctx.trace_frames_poses(case.frame, poses[0], poses[1], dev, case.e0, case.e1)
        else: ctx.trace_frames(case.frame, case.F, dev, case.e0, case.e1)
        ctx.synchronize()
        beam = ctx.debug_beam()
        return hits, segs, cnt, rf_dbg, ctx.d2h(dev, (case.F, ne, R), np.float32).view(np.int32).copy(), beam, beam_dbg
    finally:
        ctx.free(dev)


@pytest.mark.parametrize("name", list(CASES))
def test_hits_and_rf_bit_identical_with_beams(mcrt, name):
    case = CASES[name]
    cfg, sd = _scene(mcrt, case.scene)
    tr = _probe(mcrt, case, cfg)
    poses = None
    if case.poses:
        sweep = [mcrt.Transducer(case.E, position=cfg["transducerPosition"], angles_deg=np.asarray(cfg["transducerAngles"], np.float64) + np.array([4.0 * f - 4.0, 0.0, 0.0]))
                 for f in range(case.F)]
        poses = (np.stack([t.pos for t in sweep]), np.stack([t.dir for t in sweep]))
        tr.pos, tr.dir = sweep[0].pos, sweep[0].dir
    off = _setup(mcrt, case, sd, tr, {"MCRT_BEAM_B1": 0})
    on = _setup(mcrt, case, sd, tr, {} if case.expect.startswith("default") else {"MCRT_BEAM_B1": 2})
    try:
        h0, s0, c0, d0, rf0, b0, g0 = _run(mcrt, case, off, poses)
        h1, s1, c1, d1, rf1, b1, g1 = _run(mcrt, case, on, poses)
        print("%s: beam off %s, on %s (debug call %s)" % (name, b0, b1, g1))
        # the case is what it says
        assert b0 == (False, 0, 0, 0, 0, 0) and g0 == b0
        n1 = case.F * int((c0 > 1).sum()) if poses is None else None      # rays of bounce 1 in the pass, if every frame were frame `frame`: an order of magnitude
        assert (h0[:, :, 0] >= 0).any() and (c0 > 1).any(), "no ray reaches bounce 1"
        if case.probe == "miss":
            assert (h0[2, :, 0] == -1).all() and (h0[3, :, 0] >= 0).all()
        if case.nan_b0:
            live0 = c0 > 0
            assert np.isnan(s0["reflected_intensity"][:, :, 0][live0]).any(), "no total internal reflection at bounce 0"
        if case.expect in ("off", "default_off"):
            assert b1 == (False, 0, 0, 0, 0, 0) and (g1 == b1 or case.poses)      # (the debug call traces with the context's one pose)
        else:
            for ran, resolved, walked, cut, refused, used in (b1, g1):      # the pass, and the debug call whose hit table is compared
                assert ran and resolved + walked > 0
                assert 0 < used <= 12 * (case.e1 - case.e0) and cut + refused <= used
                if case.expect == "leftovers":
                    # nearly every ray: nine in ten at least.  Half the beams at least are cut: a scan-line's refracted beam meets what it entered and more, its
                    # reflected beam may leave the scene and meet nothing
                    assert walked >= 0.9 * (resolved + walked) and 2 * cut >= used, (b1, g1)
                elif case.expect == "both":
                    assert cut > 0 and walked > 0 and resolved > 0, (b1, g1)
                else:
                    assert resolved > 0, (b1, g1)
            assert b1[1] + b1[2] > n1 // 2
        # ... and bit-identical
        assert np.array_equal(c1, c0) and np.array_equal(h1, h0), "hit tables differ: %d entries" % np.count_nonzero(h1 != h0)
        assert s1.tobytes() == s0.tobytes() and np.array_equal(d1, d0)
        assert np.count_nonzero(rf0) > 0
        assert np.array_equal(rf1, rf0), "RF images not bit-identical (%d of %d words differ)" % (np.count_nonzero(rf1 != rf0), rf0.size)
    finally:
        on.close(); off.close()
