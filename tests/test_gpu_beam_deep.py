"""Bounces 2 .. MCRT_BEAM_LAST by beams (csrc/mcrt_beam.hip: the rays that left one triangle of a scan-line in one medium, tested against the
triangles collected once per beam) leave every closest hit and every RF image BIT-identical: the beams forced on in every staged pass
(MCRT_TUNING=1 MCRT_BEAM_B1=2 MCRT_BEAM_LAST=..., read in mcrt_create) against the beams off (MCRT_BEAM_B1=0) on two contexts -- the hit table
of a debug call (every bounce's triangle per path) and the RF images of a pass of several frames, viewed as int32.  The method is
tests/test_gpu_beam.py's; the beams-off side of a shape is traced once and shared by the cases of that shape.

No case passes vacuously.  mcrt_debug_beam_bounce says per bounce whether it ran by beams, how many rays the lists decided, how many were
walked, how many beams were cut, refused and in use, how many sampled rays found no slot of the group table and how many slots were claimed:
  - decided + walked of the debug call is that bounce's ray count in the hit table;
  - plain cases: at least half of a beamed bounce's rays are decided by lists where the bounce has >= 256 rays;
  - lists of one triangle (capacity 1) and a table of one group: at least half are walked (one group: at the bounces >= 2, whose beams go
    through the table).

Scenes at E = 8, S = 256 / 96, F = 3: liver(3) carries nearly every path into bounces 2 and 3 in a few groups per scan-line; sphere(3)'s
bounce 3 hits nothing, so its lists are complete and empty; the soup of 400 000 triangles carries 3 298 of the 6 144 paths of three frames
into bounce 3 (counted on the CPU oracle, tools/beam_count.py's trace; the 20 000-triangle soup of test_gpu_beam.py leaves 225 at bounce 2)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STAGED = {"MCRT_PATH_MAX": 0}                                                  # no pass takes the latency form (k_path), which has no per-bounce launches
OFF = {"MCRT_BEAM_B1": 0}


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


_scenes, _off = {}, {}


def _scene(mcrt, name):
    if name not in _scenes:
        s = mcrt.synth
        cfg, meshes = {"sphere": lambda: s.sphere_scene(3), "liver": lambda: s.liver_scene(3), "soup": lambda: s.random_scene(400000, 8, seed=99),
                       "sphere_tir": lambda: s.sphere_scene(3, {"GEL": {"impedance": 8.0}})}[name]()
        _scenes[name] = (cfg, mcrt.scene_io.build_scene(cfg, meshes))
    return _scenes[name]


def forced(last, **more):
    return dict({"MCRT_BEAM_B1": 2, "MCRT_BEAM_LAST": last}, **more)


class Case:
    def __init__(self, scene, env, beamed, E=8, S=256, F=3, frame=3, e0=0, e1=None, poses=False, expect="decided", nan_b0=False, **params):
        self.scene, self.env, self.beamed, self.E, self.S, self.F, self.frame, self.e0, self.e1 = scene, env, beamed, E, S, F, frame, e0, E if e1 is None else e1
        self.poses, self.expect, self.nan_b0, self.params = poses, expect, nan_b0, params

    def shape(self):
        return (self.scene, self.E, self.S, self.F, self.frame, self.e0, self.e1, self.poses, tuple(sorted(self.params.items())))


CASES = {
    # each depth on its own
    "liver_last2": Case("liver", forced(2), (1, 2)),
    "liver_last3": Case("liver", forced(3), (1, 2, 3)),
    "liver_last4": Case("liver", forced(4), (1, 2, 3, 4)),
    # bounce 3 hits nothing: complete, empty lists
    "sphere_last4": Case("sphere", forced(4), (1, 2, 3, 4)),
    "soup_last4": Case("soup", forced(4), (1, 2, 3, 4)),
    # wavefronts straddle scan-lines and groups
    "liver_s96": Case("liver", forced(4), (1, 2, 3, 4), S=96),
    # lists of ONE triangle: nearly every ray is a leftover at every beamed bounce -- gathered into the even halves at the odd bounces, into the odd halves at the even ones
    "one_entry_liver": Case("liver", forced(4, MCRT_BEAM_CAP=1, MCRT_BEAM_NEAR=1), (1, 2, 3, 4), expect="walked"),
    # ... in the soup a beam that leaves the scene has at most one candidate and is complete with one entry: its rays are decided; the cut beams' rays are walked
    "one_entry_soup": Case("soup", forced(3, MCRT_BEAM_CAP=1, MCRT_BEAM_NEAR=1), (1, 2, 3), expect="cut"),
    # lists of four triangles, the first pass over one of them: both passes and both ways carry rays
    "tiny_lists": Case("liver", forced(3, MCRT_BEAM_CAP=4, MCRT_BEAM_NEAR=1), (1, 2, 3), expect="any"),
    # a table of ONE group: every other group finds no slot and is walked
    "one_group": Case("liver", forced(4, MCRT_BEAM_GROUPS=1), (1, 2, 3, 4), expect="one_group"),
    # a scan-line shard
    "shard": Case("liver", forced(3), (1, 2, 3), E=12, e0=4, e1=12),
    # a pose per frame: the beams stay off at every bounce
    "poses": Case("liver", forced(4), (), poses=True),
    # total internal reflection with sanitize_tir off: NaN boundary echoes
    "tir_nan": Case("sphere_tir", forced(4), (1, 2, 3, 4), sanitize_tir=0, nan_b0=True),
    # default knobs (MCRT_BEAM_B1 = 1, the default MCRT_BEAM_LAST), either side of the pass size from which the deeper bounces take beams: from the first path ...
    "default_from_0": Case("liver", {"MCRT_PACKET_FROM": 0, "MCRT_BEAM_FROM": 0, "MCRT_BEAM_DEEP_FROM": 0}, "default"),
    # ... and a pass below the default MCRT_BEAM_DEEP_FROM: no bounce >= 2 by beams
    "default_small_pass": Case("liver", {"MCRT_PACKET_FROM": 0, "MCRT_BEAM_FROM": 0}, (1,)),
}
B_MAX = 6      # bounces whose counters are looked at


def _poses(mcrt, case, cfg):
    sweep = [mcrt.Transducer(case.E, position=cfg["transducerPosition"], angles_deg=np.asarray(cfg["transducerAngles"], np.float64) + np.array([4.0 * f - 4.0, 0.0, 0.0]))
             for f in range(case.F)]
    return (np.stack([t.pos for t in sweep]), np.stack([t.dir for t in sweep])), sweep[0]


def _run(mcrt, case, sd, tr, poses, env):
    """-> (hit table of a debug call [ne][S][B], its segments and counts, its RF image, the pass's RF images [F][ne][R],
           mcrt_debug_beam_bounce of bounces 0 .. B_MAX after the debug call and after the pass)"""
    ctx = _context(mcrt, dict(STAGED, **env))
    try:
        ctx.set_params(n_elements=case.E, n_samples=case.S, frequency=tr.frequency, **case.params)
        ctx.upload_scene(sd); ctx.upload_texture(None, 256); ctx.set_transducer(tr.pos, tr.dir)
        ne, R = case.e1 - case.e0, ctx.params.n_rows
        dev = ctx.alloc(case.F * ne * R * 4)
        hits, segs, cnt = ctx.trace_frame_debug(case.frame, dev, case.e0, case.e1, want_segs=True)
        dbg_call = [ctx.debug_beam_bounce(b) for b in range(B_MAX + 1)]
        rf_dbg = ctx.d2h(dev, (ne, R), np.float32).view(np.int32).copy()
        if poses is not None: ctx.trace_frames_poses(case.frame, poses[0], poses[1], dev, case.e0, case.e1)
        else: ctx.trace_frames(case.frame, case.F, dev, case.e0, case.e1)
        ctx.synchronize()
        dbg_pass = [ctx.debug_beam_bounce(b) for b in range(B_MAX + 1)]
        rf = ctx.d2h(dev, (case.F, ne, R), np.float32).view(np.int32).copy()
        ctx.free(dev)
        return hits, segs, cnt, rf_dbg, rf, dbg_call, dbg_pass
    finally:
        ctx.close()


@pytest.mark.parametrize("name", list(CASES))
def test_hits_and_rf_bit_identical_with_deep_beams(mcrt, name):
    case = CASES[name]
    cfg, sd = _scene(mcrt, case.scene)
    tr = mcrt.Transducer(case.E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    poses = None
    if case.poses:
        poses, first = _poses(mcrt, case, cfg)
        tr.pos, tr.dir = first.pos, first.dir
    if case.shape() not in _off:
        _off[case.shape()] = _run(mcrt, case, sd, tr, poses, OFF)
    h0, s0, c0, d0, rf0, g0, b0 = _off[case.shape()]
    h1, s1, c1, d1, rf1, g1, b1 = _run(mcrt, case, sd, tr, poses, case.env)
    nothing = (False, 0, 0, 0, 0, 0, 0, 0)
    beamed = case.beamed
    if beamed == "default":      # bounce 1, and 2 .. the library's default MCRT_BEAM_LAST: read off the context, at least bounce 2
        beamed = tuple(b for b in range(B_MAX + 1) if b1[b][0])
        assert beamed[:2] == (1, 2) and beamed == tuple(range(1, len(beamed) + 1)), beamed
    for b in range(B_MAX + 1): print("%s bounce %d: rays of the debug call %d, debug call %s, pass %s" % (name, b, int((c0 > b).sum()), g1[b], b1[b]))
    # the case is what it says
    assert all(x == nothing for x in g0 + b0)
    assert (c0 > 3).any() or case.scene.startswith("sphere"), "no ray reaches bounce 3"
    if case.nan_b0:
        assert np.isnan(s0["reflected_intensity"][:, :, 0][c0 > 0]).any(), "no total internal reflection at bounce 0"
    for b in range(B_MAX + 1):
        n_dbg = int((c0 > b).sum())
        for which, (ran, decided, walked, cut, refused, used, lost, claimed) in (("debug call", g1[b]), ("pass", b1[b])):
            if case.poses and which == "debug call": continue      # (the debug call traces with the context's one pose)
            if b not in beamed:
                assert (ran, decided, walked) == (False, 0, 0), (b, which)
                continue
            n = decided + walked
            assert ran, (b, which)
            if which == "debug call": assert n == n_dbg, (b, n, n_dbg)
            else: assert 0 < n <= case.F * (case.e1 - case.e0) * case.S or n_dbg < 16, (b, n, n_dbg)      # (an image-only pass ends paths past the image early: not F x the debug call's)
            assert cut + refused <= used and (used > 0 or n == 0)
            if b >= 2: assert (claimed > 0 or n == 0) and used <= 6 * claimed
            if n < 256: continue
            if case.expect == "decided": assert 2 * decided >= n, (b, which, decided, walked)
            elif case.expect == "walked": assert 2 * walked >= n, (b, which, decided, walked)
            elif case.expect == "one_group" and b >= 2: assert 2 * walked >= n and claimed == 1 and lost > 0, (b, which, decided, walked, claimed, lost)
            elif case.expect == "cut": assert walked > 0 and cut > 0, (b, which, decided, walked, cut)
            elif case.expect == "any": assert decided > 0 and walked > 0 and cut > 0, (b, which, decided, walked, cut)
    # ... and bit-identical
    assert np.array_equal(c1, c0) and np.array_equal(h1, h0), "hit tables differ: %d entries" % np.count_nonzero(h1 != h0)
    assert s1.tobytes() == s0.tobytes() and np.array_equal(d1, d0)
    assert np.count_nonzero(rf0) > 0
    assert np.array_equal(rf1, rf0), "RF images not bit-identical (%d of %d words differ)" % (np.count_nonzero(rf1 != rf0), rf0.size)
