"""Spatial compounding on the MI355X: mcrt_compound_frames and mcrt_bmode_compound_frames (k_compound) against the numpy mirror
(tests/compound_mirror.py, fed with the product's own maps) -- bit for bit in the float form, within bmode_mirror.assert_close in the 8-bit
form --, their invariances, the device maps between back-to-back calls, the argument errors, a traced scene end to end against the CPU
oracle, the Simulator, a two-rank group, the C++ shim and the CLI."""
import ctypes as C
import json
import math
import os
import subprocess
import numpy as np
import pytest

import bmode_mirror as bm
import compound_mirror as cm
import image_cases as ic
from test_gpu_focus import Dev

pytestmark = pytest.mark.gpu

f32 = np.float32
INVALID, LIMIT = -1, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = ic.SCAN_GEOMETRIES[0]
# the scan geometries of the image-stage tests, and one whose picture is no multiple of 4 pixels (33 x 35 = 1155: the tail lane owns 3)
GEOMETRIES = ic.SCAN_GEOMETRIES + [(30.0, 1.0471975511965976, 33, 35)]
# steer lists per N: a single tilted look, a duplicate, an unsorted list with the unsteered view last, 16 looks in no order with a duplicate
STEERS = {1: (0.2,), 2: (0.3, 0.3), 3: (0.15, -0.15, 0.0),
          16: (0.5, -0.5, 0.1, -0.1, 0.3, -0.3, 0.0, 0.45, -0.45, 0.2, -0.2, 0.05, -0.05, 0.35, -0.35, 0.1)}
# (F, N) handed out in turn to the (geometry, shape) pairs: every pair of F in {1, 3} and N in {1, 2, 3, 16} meets several shapes, and the
# six shapes of a geometry meet six different pairs
COMBOS = [(1, 1), (3, 2), (1, 3), (3, 16), (1, 16), (3, 1), (1, 2), (3, 3)]


@pytest.fixture(scope="module")
def ctx(mcrt):
    c = mcrt.Context(0)
    yield c
    c.close()


@pytest.fixture
def dev(ctx):
    d = Dev(ctx)
    yield d
    d.close()


def views(F, N, E, R, seed=0):
    """[F][N][E][R]: ic.scan_image per view (noise with NaN and +-inf taps), a few taps set to -0.0"""
    st = np.stack([np.stack([ic.scan_image(E, R, seed=seed + 100 * f + n) for n in range(N)]) for f in range(F)])
    flat = st.reshape(-1)
    flat[np.random.default_rng(seed + E + R).integers(0, flat.size, max(1, flat.size // 61))] = -0.0
    return st


def maps_of(mcrt, E, R, steers, geom):
    radius, angle, rows, cols = geom
    return [mcrt.host_compound_maps(E, R, s, radius, angle, out_rows=rows, out_cols=cols) for s in steers]


def compound(ctx, dev, st, steers, geom, fill=None):
    F, N, E, R = st.shape
    radius, angle, rows, cols = geom
    p = dev.upload(st); q = dev(F * rows * cols * 4)
    if fill is not None:
        ctx.h2d(q, np.full(F * rows * cols, fill, f32))
    ctx.compound_frames(p, F, E, R, steers, q, radius_mm=radius, total_angle=angle, out_rows=rows, out_cols=cols)
    return ctx.d2h(q, (F, rows, cols))


# ------------------------------------------------------------------ the float form
@pytest.mark.parametrize("gi", range(len(GEOMETRIES)))
def test_compound_frames_match_the_mirror(mcrt, ctx, dev, gi):
    """every pixel, bit for bit, with NaN / inf / -0.0 taps"""
    geom = GEOMETRIES[gi]
    for si, (E, R) in enumerate(ic.SCAN_SHAPES):
        F, N = COMBOS[(gi * len(ic.SCAN_SHAPES) + si + gi) % len(COMBOS)]
        st = views(F, N, E, R, seed=gi)
        got = compound(ctx, dev, st, STEERS[N], geom, fill=-7.25)
        want = cm.compound_frames(st, maps_of(mcrt, E, R, STEERS[N], geom))
        ic.assert_same_bits(got, want, "geometry %s shape %s F %d N %d" % (geom, (E, R), F, N))


def test_every_f_and_n_at_the_default_geometry(mcrt, ctx, dev):
    E, R = 37, 211
    for N in (1, 2, 3, 16):
        maps = maps_of(mcrt, E, R, STEERS[N], DEFAULT)
        for F in (1, 3):
            st = views(F, N, E, R, seed=N)
            ic.assert_same_bits(compound(ctx, dev, st, STEERS[N], DEFAULT), cm.compound_frames(st, maps), "F %d N %d" % (F, N))


@pytest.mark.parametrize("geom", GEOMETRIES)
def test_one_unsteered_view_is_scan_convert(ctx, dev, geom):
    radius, angle, rows, cols = geom
    E, R, F = 128, 465, 3
    st = views(F, 1, E, R, seed=4)
    p = dev.upload(st); q = dev(F * rows * cols * 4)
    ctx.scan_convert_frames(p, F, E, R, q, radius_mm=radius, total_angle=angle, out_rows=rows, out_cols=cols)
    plain = ctx.d2h(q, (F, rows, cols))
    got = compound(ctx, dev, st, (0.0,), geom)
    ic.assert_same_bits(got, plain + f32(0.0), "N = 1, steer 0")           # (a -0.0 becomes +0.0)
    assert not np.signbit(got[got == 0]).any()


def test_a_pass_equals_single_calls(ctx, dev):
    E, R, F, N = 128, 465, 11, 3                  # 11 frames: a chunk of the pass holds a group of 8 and one of 3 where frames are not cut apart
    for geom in (DEFAULT, GEOMETRIES[2], GEOMETRIES[5]):
        st = views(F, N, E, R, seed=5)
        got = compound(ctx, dev, st, STEERS[N], geom)
        for f in range(F):
            one = compound(ctx, dev, st[f:f + 1], STEERS[N], geom)
            assert np.array_equal(got[f].view(np.uint32), one[0].view(np.uint32)), (geom, f)


def test_n_views_equal_the_combination_of_single_views(mcrt, ctx, dev):
    """each view compounded alone on the GPU, combined by the mirror's rule (sum in view order over the covering views, one division)"""
    E, R, N = 128, 465, 3
    for geom, steers in ((DEFAULT, STEERS[3]), (GEOMETRIES[3], (0.5, 0.0, -0.5))):
        st = views(1, N, E, R, seed=6)
        maps = maps_of(mcrt, E, R, steers, geom)
        singles = [compound(ctx, dev, st[:, n:n + 1], (steers[n],), geom)[0] for n in range(N)]
        covs = [cm.covered(cm.remap_point(mc, mr), E, R) for mr, mc in maps]
        ic.assert_same_bits(compound(ctx, dev, st, steers, geom)[0], cm.combine(singles, covs), str(geom))


def test_pixels_no_beam_passes_take_the_other_views_mean(mcrt, ctx, dev):
    """(20 mm, 3.6 rad, 96 x 160) at steer 0.5 has pixels with NaN maps: that view does not cover them"""
    geom = GEOMETRIES[3]
    E, R = 128, 465
    steers = (0.5, 0.0, 0.1)
    maps = maps_of(mcrt, E, R, steers, geom)
    hole = np.isnan(maps[0][0])
    assert hole.any() and np.array_equal(hole, np.isnan(maps[0][1])) and not np.isnan(maps[1][0]).any()
    assert (hole & ~np.isnan(maps[2][0])).any()                 # (the third view has a smaller hole of its own)
    st = np.random.default_rng(8).standard_normal((1, 3, E, R)).astype(f32)
    got = compound(ctx, dev, st, steers, geom)[0]
    others = compound(ctx, dev, st[:, 1:], steers[1:], geom)[0]
    assert np.array_equal(got[hole].view(np.uint32), others[hole].view(np.uint32))
    ic.assert_same_bits(got, cm.compound(st[0], maps)[0], "with holes")
    # and with that view alone they are uncovered: 0
    alone = compound(ctx, dev, st[:, :1], steers[:1], geom, fill=-7.25)[0]
    assert np.all(alone[hole] == 0) and not np.signbit(alone[hole]).any()


# ------------------------------------------------------------------ the 8-bit form
E8, R8 = 128, 465
TGC = (0.02 * np.arange(R8)).astype(f32)


def envelopes(F, N, seed=0):
    """[F][N][E8][R8]: positive speckle falling off with depth, brighter in later views, with NaN and inf scan-lines"""
    rng = np.random.default_rng(50 + seed)
    st = np.abs(rng.standard_normal((F, N, E8, R8))).astype(f32) * np.exp(-np.arange(R8, dtype=f32) / f32(150.0))[None, None, None, :]
    st *= (1.0 + 0.5 * np.arange(N, dtype=f32))[None, :, None, None]
    st[:, :, 1::2] *= -1
    st[0, 0, 40] = np.nan; st[0, N - 1, 41] = np.inf; st[F - 1, 0, 90, 100:200] = -np.inf
    return st.astype(f32)


def bmode(ctx, dev, st, steers, geom=DEFAULT, state=None, **kw):
    F, N, E, R = st.shape
    radius, angle, rows, cols = geom
    p = dev.upload(st); out = dev.upload(np.full(F * rows * cols, 0xA5, np.uint8)); peak = dev.upload(np.full(F, -7.25, f32))
    ctx.bmode_compound_frames(p, F, E, R, steers, out, peak_dev=peak, state_dev=state, radius_mm=radius, total_angle=angle, out_rows=rows, out_cols=cols, **kw)
    ctx.synchronize()
    return ctx.d2h(out, (F, rows, cols), np.uint8), ctx.d2h(peak, (F,), f32)


@pytest.mark.parametrize("mode", ["db", "ref_log"])
@pytest.mark.parametrize("ref,gain,tgc", [(None, 0.0, None), (None, 6.0, TGC), (0.75, -3.0, TGC)])
def test_bmode_compound_matches_the_mirror(mcrt, ctx, dev, mode, ref, gain, tgc):
    """within one grey level, exact on 99.9 % (the device's log10f is not numpy's); the reference each frame used bit for bit: with the
    automatic one the largest amplitude over ALL views of the frame, a fixed one as given; the TGC curve applied"""
    F, N = 3, 3
    st = envelopes(F, N)
    maps = maps_of(mcrt, E8, R8, STEERS[N], DEFAULT)
    kw = dict(mode=mode, ref=ref, gain_db=gain, tgc_db=tgc, dynamic_range_db=48.0)
    got, peak = bmode(ctx, dev, st, STEERS[N], **kw)
    want, refs, _ = cm.bmode_compound(st, maps, **kw)
    for f in range(F):
        bm.assert_close(got[f], want[f])
    assert np.array_equal(peak.view(np.uint32), refs.view(np.uint32))
    if ref is None:
        k = bm.tgc_factors(tgc, R8)
        per_view = np.array([[bm.amplitude(st[f, n], k).max() for n in range(N)] for f in range(F)])
        assert np.array_equal(refs, per_view.max(axis=1)) and (per_view.argmax(axis=1) == N - 1).all()     # the brightest view sets it
    else:
        assert np.all(refs == f32(ref))
    if tgc is not None:
        flat, _ = bmode(ctx, dev, st, STEERS[N], **dict(kw, tgc_db=None))
        assert not np.array_equal(flat, got)
    assert got.max() > 100 and (got == 0).any()                     # (a picture, not a blank)


@pytest.mark.parametrize("geom", [GEOMETRIES[1], GEOMETRIES[3], GEOMETRIES[4], GEOMETRIES[5]])
def test_bmode_compound_at_other_geometries(mcrt, ctx, dev, geom):
    F, N = 2, 16
    st = envelopes(F, N, seed=1)
    got, peak = bmode(ctx, dev, st, STEERS[N], geom)
    want, refs, _ = cm.bmode_compound(st, maps_of(mcrt, E8, R8, STEERS[N], geom))
    for f in range(F):
        bm.assert_close(got[f], want[f])
    assert np.array_equal(peak.view(np.uint32), refs.view(np.uint32))


@pytest.mark.parametrize("geom", GEOMETRIES)
def test_one_unsteered_view_gives_bmode_frames_bytes(ctx, dev, geom):
    radius, angle, rows, cols = geom
    F = 3
    st = envelopes(F, 1, seed=2)
    for kw in (dict(), dict(mode="ref_log", tgc_db=TGC), dict(persistence=0.6, ref=0.5)):
        p = dev.upload(st); out = dev(F * rows * cols); peak = dev(4 * F)
        ctx.bmode_frames(p, F, E8, R8, out, peak_dev=peak, radius_mm=radius, total_angle=angle, out_rows=rows, out_cols=cols, **kw)
        plain, ppeak = ctx.d2h(out, (F, rows, cols), np.uint8), ctx.d2h(peak, (F,), f32)
        got, gpeak = bmode(ctx, dev, st, (0.0,), geom, **kw)
        assert np.array_equal(got, plain) and np.array_equal(gpeak.view(np.uint32), ppeak.view(np.uint32)), kw


@pytest.mark.parametrize("geom", [DEFAULT, GEOMETRIES[5]])
def test_persistence_two_calls_of_two_equal_one_of_four(mcrt, ctx, dev, geom):
    radius, angle, rows, cols = geom
    N = 3
    st = envelopes(4, N, seed=3)
    maps = maps_of(mcrt, E8, R8, STEERS[N], geom)
    s4 = dev.upload(np.full(rows * cols, 0.25, f32))
    whole, _ = bmode(ctx, dev, st, STEERS[N], geom, state=s4, persistence=0.7, reset_state=True)
    s2 = dev.upload(np.full(rows * cols, 0.75, f32))
    a, _ = bmode(ctx, dev, st[:2], STEERS[N], geom, state=s2, persistence=0.7, reset_state=True)
    b, _ = bmode(ctx, dev, st[2:], STEERS[N], geom, state=s2, persistence=0.7, reset_state=False)
    assert np.array_equal(np.concatenate([a, b]), whole)
    assert np.array_equal(ctx.d2h(s2, (rows * cols,)).view(np.uint32), ctx.d2h(s4, (rows * cols,)).view(np.uint32))
    want, _, y = cm.bmode_compound(st, maps, persistence=0.7)
    for f in range(4):
        bm.assert_close(whole[f], want[f])
    assert np.abs(ctx.d2h(s4, (rows, cols)) - y).max() < 1e-5
    plain, _ = bmode(ctx, dev, st, STEERS[N], geom)
    assert np.array_equal(plain[0], whole[0]) and not np.array_equal(plain[3], whole[3])


# ------------------------------------------------------------------ the maps on the device
def test_back_to_back_calls_each_get_their_own_maps(mcrt, ctx, dev):
    """different steer lists and geometries without a synchronisation in between; scan_convert_frames in turn keeps its own maps"""
    E, R = 64, 465
    calls = [(DEFAULT, (0.1, -0.1)), (DEFAULT, (0.1, 0.1)), (GEOMETRIES[1], (0.1, 0.1)), (DEFAULT, (-0.1, 0.1)), (DEFAULT, (0.1, -0.1)),
             (GEOMETRIES[5], (0.1, -0.1, 0.0)), (DEFAULT, (0.1,))]
    sts = [views(1, len(s), E, R, seed=30 + i) for i, (_, s) in enumerate(calls)]
    ps = [dev.upload(s) for s in sts]
    qs = [dev(g[2] * g[3] * 4) for g, _ in calls]
    plain = [dev(g[2] * g[3] * 4) for g, _ in calls]
    ctx.synchronize()
    for (g, s), p, q, pq in zip(calls, ps, qs, plain):
        ctx.compound_frames(p, 1, E, R, s, q, radius_mm=g[0], total_angle=g[1], out_rows=g[2], out_cols=g[3])
        ctx.scan_convert_frames(p, 1, E, R, pq, radius_mm=g[0], total_angle=g[1], out_rows=g[2], out_cols=g[3])
    ctx.synchronize()
    for i, ((g, s), st, q, pq) in enumerate(zip(calls, sts, qs, plain)):
        ic.assert_same_bits(ctx.d2h(q, (g[2], g[3])), cm.compound(st[0], maps_of(mcrt, E, R, s, g))[0], "call %d" % i)
        mr, mc = mcrt.host_scan_maps(E, R, g[0], g[1], out_rows=g[2], out_cols=g[3])
        ic.assert_same_bits(ctx.d2h(pq, (g[2], g[3])), cm.convert(st[0, 0], mr, mc), "plain call %d" % i)


# ------------------------------------------------------------------ errors
def test_errors_leave_the_outputs_untouched(mcrt, ctx, dev):
    E, R, N, rows, cols = 16, 40, 2, 20, 24
    st = views(1, N, E, R)
    p = dev.upload(st)
    img = np.full(rows * cols, -7.25, f32); q = dev.upload(img)
    bytes_ = np.full(rows * cols, 0xA5, np.uint8); o8 = dev.upload(bytes_)
    state0 = np.full(rows * cols, 0.5, f32); state = dev.upload(state0)
    peak0 = np.full(1, -7.25, f32); peak = dev.upload(peak0)
    big = dev(2 * 2049 * 4)
    L = ctx.L
    vp = C.c_void_p
    good = mcrt.compound_struct((0.1, -0.1))

    def cf(h=ctx.h, rf=p, F=1, e=E, r=R, radius=30.0, angle=1.0, cp=good, out=q, orows=rows, ocols=cols):
        return L.mcrt_compound_frames(h, vp(rf) if rf else None, F, e, r, radius, angle, C.byref(cp) if cp is not None else None, vp(out) if out else None, orows, ocols)

    def bf(h=ctx.h, rf=p, F=1, e=E, r=R, cp=good, out=o8, par=None, tgc=None):
        par = par if par is not None else mcrt.bmode_params(radius_mm=30.0, total_angle=1.0, out_rows=rows, out_cols=cols, persistence=0.5, reset_state=False)
        return L.mcrt_bmode_compound_frames(h, vp(rf) if rf else None, F, e, r, C.byref(par) if par is not False else None, C.byref(cp) if cp is not None else None,
                                            tgc.ctypes.data_as(vp) if tgc is not None else None, vp(state), vp(peak), vp(out) if out else None)

    def steers(*s):
        return mcrt.compound_struct(s)

    empty = mcrt.Compound(); seventeen = mcrt.compound_struct([0.01 * i for i in range(17)])
    assert seventeen.n_views == 17
    for call in (cf, bf):
        assert call(h=None) == INVALID
        assert call(rf=None) == INVALID and call(out=None) == INVALID and call(cp=None) == INVALID
        for kw in (dict(F=0), dict(e=0), dict(r=0)):
            assert call(**kw) == INVALID, kw
        assert call(cp=empty) == INVALID and call(cp=seventeen) == INVALID
        for s in (math.nan, math.inf, -math.inf, math.pi / 2, -math.pi / 2, 1.6):
            assert call(cp=steers(0.0, s)) == INVALID, s
            assert b"steer" in L.mcrt_last_error()
        assert call(rf=big, e=2, r=2049) == LIMIT
        assert call(F=32768) == LIMIT and call(F=65535 // 16 + 1, cp=steers(*STEERS[16])) == LIMIT       # F * N > 65535
        # overlap: the output inside the stack, on its last bytes, ending just inside its start
        for out in (p, p + N * E * R * 4 - 4, p - 4):
            assert call(out=out) == INVALID and b"overlap" in L.mcrt_last_error()
    assert cf(orows=0) == INVALID and cf(ocols=0) == INVALID
    for angle in (0.0, -1.0, math.nan):
        assert cf(angle=angle) == INVALID
        assert bf(par=mcrt.bmode_params(radius_mm=30.0, total_angle=angle, out_rows=rows, out_cols=cols)) == INVALID
    assert bf(par=False) == INVALID
    assert bf(e=1 << 28, r=2, cp=steers(*STEERS[16])) == LIMIT and b"scan-lines" in L.mcrt_last_error()      # N * E does not fit 32 bits
    assert bf(par=mcrt.bmode_params(out_rows=0, out_cols=cols)) == INVALID
    for kw in (dict(mode=7), dict(dynamic_range_db=0.0), dict(dynamic_range_db=math.nan), dict(gain_db=math.inf), dict(ref=math.nan), dict(persistence=1.0),
               dict(persistence=-0.1)):
        assert bf(par=mcrt.bmode_params(radius_mm=30.0, total_angle=1.0, out_rows=rows, out_cols=cols, **kw)) == INVALID, kw
    bad_tgc = np.zeros(R, f32); bad_tgc[7] = np.nan
    assert bf(tgc=bad_tgc) == INVALID
    ctx.synchronize()
    assert np.array_equal(ctx.d2h(q, (rows * cols,)).view(np.uint32), img.view(np.uint32))
    assert np.array_equal(ctx.d2h(o8, (rows * cols,), np.uint8), bytes_)
    assert np.array_equal(ctx.d2h(state, (rows * cols,)), state0) and np.array_equal(ctx.d2h(peak, (1,)), peak0)
    assert np.array_equal(ctx.d2h(p, st.shape).view(np.uint32), st.view(np.uint32))
    # the context still works
    assert cf() == 0 and bf() == 0
    ctx.synchronize()
    maps = maps_of(mcrt, E, R, (0.1, -0.1), (30.0, 1.0, rows, cols))
    ic.assert_same_bits(ctx.d2h(q, (rows, cols)), cm.compound(st[0], maps)[0], "after the errors")
    assert ctx.d2h(peak, (1,))[0] > 0


# ------------------------------------------------------------------ end to end: a traced scene
STEER3 = (-0.15, 0.0, 0.15)


def _oracle(orc, sd):
    return orc.OracleScene(sd.tri, sd.tri_mesh, sd.meshes, sd.materials, sd.start_mat, sd.spacing)


def _setup(obj, sd, tr, S, tex):
    obj.set_params(n_elements=tr.n_elements, n_samples=S, frequency=tr.frequency)
    obj.upload_scene(sd)
    obj.upload_texture(tex, 256)
    obj.set_transducer(tr.pos, tr.dir)


def test_a_traced_scene_end_to_end(mcrt, orc, tex256):
    """every view of the pose pass is the CPU oracle's frame from the steered table with frame id f * N + n, bit for bit; their compound is
    the mirror's; and it is another picture than the unsteered view's own conversion, on the pixels the mirror names"""
    cfg, meshes = mcrt.synth.sphere_scene(3)
    sd = mcrt.scene_io.build_scene(cfg, meshes)
    E, S, F, N = 32, 16, 2, 3
    tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    pos, dirs = tr.steered(STEER3)
    assert pos[1].tobytes() == tr.pos.tobytes() and dirs[1].tobytes() == tr.dir.tobytes()
    p = orc.default_params(n_elements=E, n_samples=S)
    R = p.n_rows
    osc = _oracle(orc, sd)
    want = np.stack([np.stack([osc.trace_frame(p, pos[n], dirs[n], tex256, frame_id=f * N + n, use_bvh=False)["rf"].T for n in range(N)]) for f in range(F)])
    # facts of the input, from the oracle: the looks are different images, and so are the frames
    for f in range(F):
        assert np.count_nonzero(np.nan_to_num(want[f, 1])) > 1000
        assert not np.array_equal(want[f, 0], want[f, 1], equal_nan=True) and not np.array_equal(want[f, 2], want[f, 1], equal_nan=True)
    assert not np.array_equal(want[0], want[1], equal_nan=True)
    c = mcrt.Context(0)
    try:
        _setup(c, sd, tr, S, tex256)
        st_dev, out_dev, plain_dev = c.alloc(F * N * E * R * 4), c.alloc(F * 400 * 500 * 4), c.alloc(400 * 500 * 4)
        c.trace_frames_poses(0, np.tile(pos, (F, 1, 1)), np.tile(dirs, (F, 1, 1)), st_dev)
        c.compound_frames(st_dev, F, E, R, STEER3, out_dev)
        c.synchronize()
        st = c.d2h(st_dev, (F, N, E, R))
        for f in range(F):
            for n in range(N):
                ic.assert_same_bits(st[f, n], want[f, n], "frame %d view %d vs the oracle" % (f, n))
        maps = maps_of(mcrt, E, R, STEER3, DEFAULT)
        got = c.d2h(out_dev, (F, 400, 500))
        mirror = cm.compound_frames(st, maps)
        ic.assert_same_bits(got, mirror, "compound vs the mirror")
        for f in range(F):
            c.scan_convert_frames(st_dev + (f * N + 1) * E * R * 4, 1, E, R, plain_dev)
            plain = c.d2h(plain_dev, (400, 500))
            named = cm.convert(st[f, 1], *maps[1]).view(np.uint32) != mirror[f].view(np.uint32)
            differs = plain.view(np.uint32) != got[f].view(np.uint32)
            assert named.sum() > 1000 and np.array_equal(differs, named), f
        for d in (st_dev, out_dev, plain_dev):
            c.free(d)
    finally:
        c.close()


def _pipeline(ctx, psf, views_dev, F, N, E, R, steers, row_mm):
    """convolve and envelope over the F * N views, then both compound forms -> (float [F][400][500], bytes [F][400][500])"""
    if psf.has_focus:
        ctx.convolve_frames_depth(views_dev, F * N, E, R, psf.axial_kernel, psf.lateral_rows(R, row_mm))
    else:
        ctx.convolve_frames(views_dev, F * N, E, R, psf.axial_kernel, psf.lateral_kernel)
    ctx.envelope_frames(views_dev, F * N, E, R)
    a, b = ctx.alloc(F * 400 * 500 * 4), ctx.alloc(F * 400 * 500)
    ctx.compound_frames(views_dev, F, E, R, steers, a)
    ctx.bmode_compound_frames(views_dev, F, E, R, steers, b, dynamic_range_db=50.0)
    out = ctx.d2h(a, (F, 400, 500)), ctx.d2h(b, (F, 400, 500), np.uint8)
    ctx.free(a); ctx.free(b)
    return out


@pytest.mark.parametrize("elevation", [False, True])
def test_simulator(mcrt, tex256, elevation):
    """Simulator(compound=...) alone and with elevation=True: frame f traced alone is frame f of a hand-made pass by the frame-id rule"""
    cfg, meshes = mcrt.synth.sphere_scene(3)
    sd = mcrt.scene_io.build_scene(cfg, meshes)
    E, S, K, F = 16, 16, 3, 3
    N = len(STEER3)
    tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    psf = mcrt.Psf(freq=tr.frequency, var_z=9.0, elevation_size=K, elevation_pitch_um=1500, focus_mm=(40.0,) if elevation else None)
    sim = mcrt.Simulator(sd, tr, n_samples=S, texture=tex256, psf=psf, elevation=elevation, compound=STEER3)
    try:
        R, ctx = sim.R, sim.ctx
        assert sim.N == N and sim.steers == STEER3
        with pytest.raises(RuntimeError):
            sim.frame(0)
        pos, dirs = tr.steered(STEER3)
        views_dev = ctx.alloc(F * N * E * R * 4)
        if elevation:                                       # views outer, planes inner: ((f0 + f) * N + n) * K + k
            axis = mcrt.host_elevation_axis(tr.angles)
            tabs = [mcrt.host_elevation_planes(pos[n], dirs[n], axis, K, 1500) for n in range(N)]
            ppos = np.concatenate([t[0] for t in tabs]); pdir = np.concatenate([t[1] for t in tabs])
            planes_dev = ctx.alloc(F * N * K * E * R * 4)
            ctx.trace_frames_poses(0, np.tile(ppos, (F, 1, 1)), np.tile(pdir, (F, 1, 1)), planes_dev)
            ctx.elevation_frames(planes_dev, F * N, K, E, R, psf.elevation_rows(R, sim.row_mm), views_dev)
            ctx.synchronize(); ctx.free(planes_dev)
        else:
            ctx.trace_frames_poses(0, np.tile(pos, (F, 1, 1)), np.tile(dirs, (F, 1, 1)), views_dev)
        raw = ctx.d2h(views_dev, (F, N, E, R))
        assert not np.array_equal(raw[0], raw[2], equal_nan=True) and not np.array_equal(raw[0, 0], raw[0, 1], equal_nan=True)
        pictures, bytes_ = _pipeline(ctx, psf, views_dev, F, N, E, R, STEER3, sim.row_mm)
        ctx.free(views_dev)
        for f in (0, 2):
            sim.trace(f)
            ic.assert_same_bits(ctx.d2h(sim.views_dev, (N, E, R)), raw[f], "frame %d alone vs in the pass" % f)
            ic.assert_same_bits(sim.compound_image(f), pictures[f], "compound_image(%d)" % f)
            assert np.array_equal(sim.bmode(f, dynamic_range_db=50.0), bytes_[f])
        assert bytes_.max() > 200 and np.count_nonzero(pictures[0]) > 1000
    finally:
        sim.close()
    plain = mcrt.Simulator(sd, tr, n_samples=S, texture=tex256)
    try:
        assert plain.steers is None
        with pytest.raises(RuntimeError):
            plain.compound_image(0)
        assert plain.frame(0).shape == (plain.R, E)
    finally:
        plain.close()
    with pytest.raises(ValueError):
        mcrt.Simulator(sd, tr, n_samples=S, texture=tex256, compound=[0.01 * i for i in range(17)])


def test_a_two_rank_group_equals_one_context(mcrt, sphere, tex256):
    cfg, sd = sphere
    E, S, F = 16, 32, 2
    N = len(STEER3)
    tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    pos, dirs = tr.steered(STEER3)
    pos, dirs = np.tile(pos, (F, 1, 1)), np.tile(dirs, (F, 1, 1))
    psf = mcrt.Psf(freq=tr.frequency)
    one = mcrt.Context(0); _setup(one, sd, tr, S, tex256)
    grp = mcrt.Group([0, 0]); _setup(grp, sd, tr, S, tex256)
    try:
        R = one.params.n_rows
        out = []
        for tracer, c in ((one, one), (grp, grp.root)):
            st_dev = c.alloc(F * N * E * R * 4)
            tracer.trace_frames_poses(5 * N, pos, dirs, st_dev)
            tracer.synchronize()
            raw = c.d2h(st_dev, (F, N, E, R))
            out.append((raw,) + _pipeline(c, psf, st_dev, F, N, E, R, STEER3, mcrt.row_pitch_mm(tr.frequency)))
            c.free(st_dev)
        for a, b in zip(out[0], out[1]):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
        assert np.count_nonzero(out[1][1]) > 1000 and out[1][2].max() > 200
    finally:
        grp.close(); one.close()


# ------------------------------------------------------------------ the C++ shim and the CLI
def _write_scene(mcrt, tmp_path):
    cfg, meshes = mcrt.synth.sphere_scene(3)
    cfg["workingDirectory"] = str(tmp_path) + "/"
    for f, (V, F) in meshes.items():
        mcrt.scene_io.save_obj(str(tmp_path / f), V, F)
    (tmp_path / "sphere.scene").write_text(json.dumps(cfg))
    return cfg, str(tmp_path / "sphere.scene")


@pytest.mark.parametrize("devices", [None, "0,0"])
def test_host_shim(mcrt, tmp_path, devices):
    """transducer<N>::steered and rf_image::trace / convolve / envelope / postprocess with a steer list write the tables and the pictures
    Python's Simulator produces, bit for bit -- on one context and on a two-rank group"""
    pkg = os.path.join(ROOT, "mcray-tracing_amd")
    exe = str(tmp_path / "compound_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(pkg, "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "compound_driver.cpp"), "-L", pkg, "-lmcrt_hip", "-Wl,-rpath," + pkg])
    cfg, scene = _write_scene(mcrt, tmp_path)
    out = tmp_path / "compound.bin"
    E, S, frame, N = 64, 8, 3, len(STEER3)
    r = subprocess.run([exe, scene, str(out), str(frame), str(S), ",".join(repr(s) for s in STEER3)] + (["--devices", devices] if devices else []),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = out.read_bytes()
    tab = N * E * 3 * 4
    assert len(raw) == 2 * tab + 400 * 500 * 5
    tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    pos, dirs = tr.steered(STEER3)
    assert raw[:tab] == pos.tobytes() and raw[tab:2 * tab] == dirs.tobytes()
    picture = np.frombuffer(raw, f32, 400 * 500, 2 * tab).reshape(400, 500)
    bytes_ = np.frombuffer(raw, np.uint8, 400 * 500, 2 * tab + 400 * 500 * 4).reshape(400, 500)
    sim = mcrt.Simulator(mcrt.scene_io.load_scene_file(scene), tr, n_samples=S, compound=STEER3)
    try:
        ic.assert_same_bits(picture, sim.compound_image(frame), "shim vs python, float")
        assert np.array_equal(bytes_, sim.bmode(frame))
    finally:
        sim.close()
    assert np.count_nonzero(picture) > 1000 and bytes_.max() > 200


def test_cli_compound_options(mcrt, tmp_path):
    exe = os.path.join(ROOT, "mcray-tracing_amd", "mattausch_hip")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "mcray-tracing_amd"), "mattausch_hip"])
    _, scene = _write_scene(mcrt, tmp_path)

    def run(name, *opts):
        r = subprocess.run([exe, scene, "2", "5", str(tmp_path / (name + ".pgm")), str(tmp_path / (name + ".bin"))] + list(opts),
                           capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout + r.stderr
        return (tmp_path / (name + ".pgm")).read_bytes(), (tmp_path / (name + ".bin")).read_bytes()

    plain = run("plain")
    assert run("unused", "--compound-step-deg", "8") == plain                  # without --compound: byte for byte
    assert run("one", "--compound", "1") == plain                              # the unsteered view alone, frame id f
    assert run("one_step", "--compound", "1", "--compound-step-deg", "8") == plain
    three = run("three", "--compound", "3")
    assert len(three[0]) == len(plain[0]) and three[0] != plain[0]
    assert len(three[1]) == len(plain[1]) and three[1] != plain[1]             # rf.bin: the unsteered view, traced with another frame id
    assert run("three_wide", "--compound", "3", "--compound-step-deg", "10")[0] != three[0]
    db = run("db", "--db", "60")
    assert run("one_db", "--compound", "1", "--db", "60") == db
    assert run("five_db", "--compound", "5", "--db", "60")[0] != db[0]
    for bad in (["--compound", "2"], ["--compound", "0"], ["--compound", "17"], ["--compound", "-3"], ["--compound", "3", "--compound-step-deg", "90"],
                ["--compound", "3", "--elevation", "3"]):
        r = subprocess.run([exe, scene, "1", "5"] + bad, capture_output=True, text=True, timeout=240)
        assert r.returncode == 1 and "--compound" in r.stdout, (bad, r.stdout)
