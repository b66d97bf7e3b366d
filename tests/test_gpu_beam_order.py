"""The beam order (csrc/mcrt_beam.hip: k_beam_rank / k_beam_scan / k_beam_place -- a permutation of a beamed bounce's queue grouped by beam, through which
k_beam_test's first pass reads its rays, one beam per wavefront; MCRT_BEAM_ORDER is the mask of ordered bounces) leaves every closest hit and every RF
image BIT-identical.  The method is tests/test_gpu_beam_deep.py's: the beams forced on in every staged pass (MCRT_TUNING=1 MCRT_BEAM_B1=2 MCRT_BEAM_LAST=...,
read in mcrt_create) against the beams off (MCRT_BEAM_B1=0) on two contexts -- the hit table of a debug call and the RF images of a pass of several frames,
viewed as int32; the beams-off side of a shape is traced once and shared by the cases of that shape.

No case passes vacuously.  Per beamed bounce mcrt_debug_beam_bounce's decided + walked is the bounce's ray count, and mcrt_debug_beam_order says whether the
bounce was ordered, how many rays were placed (= the ray count), in how many segments, with how many pad lanes (<= 63 per segment, rays + pads a whole
number of wavefronts), and -- with MCRT_BEAM_PAIRS=1 -- how many (wavefront, beam) pairs k_beam_test's first pass met.

Shapes: E = 8, S = 256, F = 3 on liver(3) unless the case says otherwise (tests/test_gpu_beam_deep.py's docstring says what these scenes carry into which
bounce)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STAGED = {"MCRT_PATH_MAX": 0}                                                  # no pass takes the latency form (k_path), which has no per-bounce launches
OFF = {"MCRT_BEAM_B1": 0}
DEEP = 0x1c                                                                    # bounces 2, 3, 4 ordered
B_MAX = 6                                                                      # bounces whose counters are looked at


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
        cfg, meshes = {"sphere": lambda: s.sphere_scene(3), "liver": lambda: s.liver_scene(3)}[name]()
        _scenes[name] = (cfg, mcrt.scene_io.build_scene(cfg, meshes))
    return _scenes[name]


def forced(last, order, **more):
    return dict({"MCRT_BEAM_B1": 2, "MCRT_BEAM_LAST": last, "MCRT_BEAM_ORDER": order}, **more)


class Case:
    def __init__(self, scene, env, beamed, E=8, S=256, F=3, frame=3, e0=0, e1=None, poses=False, expect="decided", pads=False):
        self.scene, self.env, self.beamed, self.E, self.S, self.F, self.frame, self.e0, self.e1 = scene, env, beamed, E, S, F, frame, e0, E if e1 is None else e1
        self.poses, self.expect, self.pads = poses, expect, pads
        self.ordered = tuple(b for b in beamed if (int(env.get("MCRT_BEAM_ORDER", 0)) >> b) & 1)

    def shape(self):
        return (self.scene, self.E, self.S, self.F, self.frame, self.e0, self.e1, self.poses)


CASES = {
    "liver_deep": Case("liver", forced(4, DEEP), (1, 2, 3, 4)),
    # segments that are no multiples of 64; wavefronts that straddled scan-lines before
    "liver_s96": Case("liver", forced(4, DEEP), (1, 2, 3, 4), S=96, pads=True),
    # bounce 3 hits nothing: complete, empty lists; then a bounce without rays: empty counters, a length of 0, a worst-case grid that does nothing
    "sphere": Case("sphere", forced(4, DEEP), (1, 2, 3, 4)),
    # a table of ONE group: nearly every ray is in the pseudo-beam and is walked
    "one_group": Case("liver", forced(4, DEEP, MCRT_BEAM_GROUPS=1), (1, 2, 3, 4), expect="one_group"),
    # lists of ONE triangle
    "one_entry": Case("liver", forced(4, DEEP, MCRT_BEAM_CAP=1, MCRT_BEAM_NEAR=1), (1, 2, 3, 4), expect="walked"),
    # lists of four, the first pass over one: the ordered first pass hands over to the second pass over its leftover queue
    "tiny_lists": Case("liver", forced(3, DEEP, MCRT_BEAM_CAP=4, MCRT_BEAM_NEAR=1), (1, 2, 3), expect="any"),
    # a scan-line shard
    "shard": Case("liver", forced(3, DEEP), (1, 2, 3), E=12, e0=4, e1=12),
    # a pose per frame: the beams stay off, and nothing of the order runs
    "poses": Case("liver", forced(4, DEEP), (), poses=True),
    # bounce 1 ordered as well (direct addressing, no group table)
    "bounce1": Case("liver", forced(4, 0x1e), (1, 2, 3, 4)),
}


def _poses(mcrt, case, cfg):
    sweep = [mcrt.Transducer(case.E, position=cfg["transducerPosition"], angles_deg=np.asarray(cfg["transducerAngles"], np.float64) + np.array([4.0 * f - 4.0, 0.0, 0.0]))
             for f in range(case.F)]
    return (np.stack([t.pos for t in sweep]), np.stack([t.dir for t in sweep])), sweep[0]


def _run(mcrt, case, env):
    """-> (hit table of a debug call [ne][S][B], its counts, its RF image, the pass's RF images [F][ne][R],
           (mcrt_debug_beam_bounce, mcrt_debug_beam_order) of bounces 0 .. B_MAX after the debug call and after the pass)"""
    cfg, sd = _scene(mcrt, case.scene)
    tr = mcrt.Transducer(case.E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    poses = None
    if case.poses:
        poses, first = _poses(mcrt, case, cfg)
        tr.pos, tr.dir = first.pos, first.dir
    ctx = _context(mcrt, dict(STAGED, **env))
    try:
        ctx.set_params(n_elements=case.E, n_samples=case.S, frequency=tr.frequency)
        ctx.upload_scene(sd); ctx.upload_texture(None, 256); ctx.set_transducer(tr.pos, tr.dir)
        ne, R = case.e1 - case.e0, ctx.params.n_rows
        dev = ctx.alloc(case.F * ne * R * 4)
        hits, _, cnt = ctx.trace_frame_debug(case.frame, dev, case.e0, case.e1, want_segs=True)
        dbg_call = [(ctx.debug_beam_bounce(b), ctx.debug_beam_order(b)) for b in range(B_MAX + 1)]
        rf_dbg = ctx.d2h(dev, (ne, R), np.float32).view(np.int32).copy()
        if poses is not None: ctx.trace_frames_poses(case.frame, poses[0], poses[1], dev, case.e0, case.e1)
        else: ctx.trace_frames(case.frame, case.F, dev, case.e0, case.e1)
        ctx.synchronize()
        dbg_pass = [(ctx.debug_beam_bounce(b), ctx.debug_beam_order(b)) for b in range(B_MAX + 1)]
        rf = ctx.d2h(dev, (case.F, ne, R), np.float32).view(np.int32).copy()
        ctx.free(dev)
        return hits, cnt, rf_dbg, rf, dbg_call, dbg_pass
    finally:
        ctx.close()


def _beams_off(mcrt, case):
    if case.shape() not in _off:
        _off[case.shape()] = _run(mcrt, case, OFF)
        h0, c0, d0, rf0, g0, b0 = _off[case.shape()]
        assert all(x == ((False, 0, 0, 0, 0, 0, 0, 0), (False, 0, 0, 0, 0)) for x in g0 + b0)
        assert (c0 > 3).any() or case.scene == "sphere", "no ray reaches bounce 3"
        assert np.count_nonzero(rf0) > 0
    return _off[case.shape()]


def _check(case, name, off, on, pairs=False):
    """bit-identical to the beams off; decided + walked = the bounce's rays; the order's own counters"""
    h0, c0, d0, rf0, _, _ = off
    h1, c1, d1, rf1, g1, b1 = on
    for b in range(B_MAX + 1): print("%s bounce %d: rays of the debug call %d, debug call %s, pass %s" % (name, b, int((c0 > b).sum()), g1[b], b1[b]))
    for b in range(B_MAX + 1):
        n_dbg = int((c0 > b).sum())
        for which, ((ran, decided, walked, cut, refused, used, lost, claimed), (ordered, placed, segments, pads, met)) in (("debug call", g1[b]), ("pass", b1[b])):
            if case.poses and which == "debug call": continue      # (the debug call traces with the context's one pose)
            where = (name, b, which)
            if b not in case.beamed:
                assert (ran, decided, walked) == (False, 0, 0) and (ordered, placed, segments, pads, met) == (False, 0, 0, 0, 0), where
                continue
            n = decided + walked
            assert ran, where
            if which == "debug call": assert n == n_dbg, (where, n, n_dbg)
            else: assert 0 < n <= case.F * (case.e1 - case.e0) * case.S or n_dbg < 16, (where, n, n_dbg)
            if b not in case.ordered:
                assert (ordered, placed, segments, pads) == (False, 0, 0, 0), where
            else:
                assert ordered and placed == n, (where, placed, n)
                assert pads <= 63 * segments and (placed + pads) % 64 == 0 and (segments > 0) == (n > 0), (where, placed, segments, pads)
                if case.pads and n >= 256: assert pads > 0, where
                if pairs: assert met <= (placed + pads) // 64 and (met > 0 or decided == 0), (where, met, placed, pads)      # one beam per wavefront
            if not pairs: assert met == 0, where
            if n < 256: continue
            if case.expect == "decided": assert 2 * decided >= n, (where, decided, walked)
            elif case.expect == "walked": assert 2 * walked >= n, (where, decided, walked)
            elif case.expect == "one_group" and b >= 2: assert 2 * walked >= n and claimed == 1 and lost > 0, (where, decided, walked, claimed, lost)
            elif case.expect == "any": assert decided > 0 and walked > 0 and cut > 0, (where, decided, walked, cut)
    assert np.array_equal(c1, c0) and np.array_equal(h1, h0), "hit tables differ: %d entries" % np.count_nonzero(h1 != h0)
    assert np.array_equal(d1, d0)
    assert np.array_equal(rf1, rf0), "RF images not bit-identical (%d of %d words differ)" % (np.count_nonzero(rf1 != rf0), rf0.size)


@pytest.mark.parametrize("name", list(CASES))
def test_hits_and_rf_bit_identical_with_beam_order(mcrt, name):
    case = CASES[name]
    _check(case, name, _beams_off(mcrt, case), _run(mcrt, case, case.env))


def test_order_moves_no_ray_between_lists_and_walk(mcrt):
    """bounces 2-4 ordered against MCRT_BEAM_ORDER=0: where no beam is refused and no sampled ray is without a slot, decided and walked are equal per bounce"""
    case = CASES["liver_deep"]
    plain = Case("liver", forced(4, 0), (1, 2, 3, 4))
    off = _beams_off(mcrt, case)
    on, un = _run(mcrt, case, case.env), _run(mcrt, plain, plain.env)
    _check(case, "ordered", off, on)
    _check(plain, "unordered", off, un)
    for b in (2, 3, 4):
        for k in (4, 5):      # the debug call, the pass
            x, y = on[k][b][0], un[k][b][0]
            assert x[4] == 0 and y[4] == 0 and x[6] == 0 and y[6] == 0, (b, k, x, y)      # none refused, none without a slot
            assert x[1:3] == y[1:3], (b, k, x, y)


def test_one_beam_per_wavefront(mcrt):
    """MCRT_BEAM_PAIRS=1: an ordered bounce's first pass meets at most one beam per wavefront of its segments; in queue order bounce 3 on the liver meets more
    pairs than it has wavefronts"""
    case = Case("liver", forced(4, DEEP, MCRT_BEAM_PAIRS=1), (1, 2, 3, 4))
    plain = Case("liver", forced(4, 0, MCRT_BEAM_PAIRS=1), (1, 2, 3, 4))
    off = _beams_off(mcrt, case)
    on, un = _run(mcrt, case, case.env), _run(mcrt, plain, plain.env)
    _check(case, "ordered", off, on, pairs=True)
    _check(plain, "unordered", off, un, pairs=True)
    for b in (2, 3, 4):
        (_, decided, walked, *_), (_, placed, segments, pads, met) = on[5][b]
        (_, d_un, w_un, *_), (_, _, _, _, met_un) = un[5][b]
        print("bounce %d of the pass: %d rays; ordered %d pairs in %d wavefronts of %d segments, in queue order %d pairs in %d wavefronts"
              % (b, placed, met, (placed + pads) // 64, segments, met_un, (d_un + w_un + 63) // 64))
    (_, d_un, w_un, *_), (_, _, _, _, met_un) = un[5][3]
    assert met_un > (d_un + w_un + 63) // 64, (met_un, d_un + w_un)
