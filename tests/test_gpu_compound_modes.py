"""The compounding modes on the MI355X: mcrt_compound_frames_opts and mcrt_bmode_compound_frames_opts (k_compound's weighted, max and median
forms) against the numpy mirror (tests/compound_modes_mirror.py, fed with the product's own maps) -- bit for bit in the float form, within
bmode_mirror.assert_close in the 8-bit form --, the defaults against the calls without options, holes, invariances, persistence, the
argument errors, the Simulator, the C++ shim and the CLI."""
import ctypes as C
import math
import os
import subprocess
import numpy as np
import pytest

import bmode_mirror as bm
import compound_mirror as cm
import compound_modes_mirror as mm
import image_cases as ic
import test_gpu_compound as tg
from test_gpu_focus import Dev

pytestmark = pytest.mark.gpu

f32 = np.float32
INVALID = -1
ROOT = tg.ROOT
DEFAULT = tg.DEFAULT
GEOMETRIES = tg.GEOMETRIES
STEERS = dict(tg.STEERS)
STEERS[5] = (0.25, -0.25, 0.0, 0.4, -0.1)
MODES = mm.MODES
# (F, N): F = 11 is a group of 8 and one of 3 where the frames are not cut apart; N = 5 and 16 cross the median's sort buckets (4, 8, 16)
COMBOS = [(F, N) for F in (1, 3, 11) for N in (1, 2, 3, 5, 16)]
LIGHT = [c for c in COMBOS if c[0] * c[1] <= 33]        # for the pictures of 50000 pixels and more (the mirror's time)
UNEQUAL = (0.5, 0.0, 2.0, 1.0, 0.25, 3.0, 0.0, 1.5)


def weights_of(N, unequal):
    """None (every view 1), or unequal weights with a 0 among them (one view alone cannot have weight 0: that is refused)"""
    if not unequal:
        return None
    return (0.5,) if N == 1 else tuple(UNEQUAL[n % len(UNEQUAL)] for n in range(N))


OPTIONS = [(0.0, False), (2.5, False), (0.0, True), (2.5, True)]       # (feather_lines, unequal weights)


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


_views = {}


def views(F, N, E, R, seed=0):
    """tg.views (NaN, +-inf and -0.0 taps), made once per shape and shared: nothing writes to it"""
    key = (F, N, E, R, seed)
    if key not in _views:
        _views[key] = tg.views(F, N, E, R, seed)
        _views[key].setflags(write=False)
    return _views[key]


def compound(ctx, dev, st, steers, geom, mode="mean", weights=None, feather=0.0, fill=-7.25):
    F, N, E, R = st.shape
    radius, angle, rows, cols = geom
    p = dev.upload(st); q = dev.upload(np.full(F * rows * cols, fill, f32))
    ctx.compound_frames(p, F, E, R, steers, q, radius_mm=radius, total_angle=angle, out_rows=rows, out_cols=cols, mode=mode, view_weights=weights,
                        feather_lines=feather)
    return ctx.d2h(q, (F, rows, cols))


# ------------------------------------------------------------------ the float form
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("gi", range(len(GEOMETRIES)))
def test_modes_match_the_mirror(mcrt, ctx, dev, gi, mode):
    """every pixel, bit for bit, over the scan shapes and geometries (the 33 x 35 picture's tail wavefront is partial)"""
    geom = GEOMETRIES[gi]
    combos = LIGHT if geom[2] * geom[3] >= 50000 else COMBOS
    mi = MODES.index(mode)
    for si, (E, R) in enumerate(ic.SCAN_SHAPES):
        k = gi * len(ic.SCAN_SHAPES) + si
        F, N = combos[(k + 4 * mi) % len(combos)]
        feather, unequal = OPTIONS[(k + mi) % len(OPTIONS)]
        w = weights_of(N, unequal)
        st = views(F, N, E, R, seed=gi)
        got = compound(ctx, dev, st, STEERS[N], geom, mode, w, feather)
        want = mm.compound_frames(st, tg.maps_of(mcrt, E, R, STEERS[N], geom), mode, w, feather)
        ic.assert_same_bits(got, want, "%s geometry %s shape %s F %d N %d feather %g weights %s" % (mode, geom, (E, R), F, N, feather, w))


@pytest.mark.parametrize("mode", MODES)
def test_every_option_f_and_n(mcrt, ctx, dev, mode):
    """{no feather, 2.5 lines} x {weights 1, unequal with a 0} x every (F, N) on the 33 x 35 picture (two workgroups, a partial tail)"""
    E, R = 37, 211
    geom = GEOMETRIES[5]
    for F, N in COMBOS:
        maps = tg.maps_of(mcrt, E, R, STEERS[N], geom)
        st = views(F, N, E, R, seed=N)
        for feather, unequal in OPTIONS:
            w = weights_of(N, unequal)
            got = compound(ctx, dev, st, STEERS[N], geom, mode, w, feather)
            ic.assert_same_bits(got, mm.compound_frames(st, maps, mode, w, feather), "%s F %d N %d feather %g weights %s" % (mode, F, N, feather, w))


def _opts_call(ctx, mcrt, p, F, E, R, steers, q, geom, o):
    radius, angle, rows, cols = geom
    cp = mcrt.compound_struct(steers)
    vp = C.c_void_p
    return ctx.L.mcrt_compound_frames_opts(ctx.h, vp(p), F, E, R, radius, angle, C.byref(cp), vp(q), rows, cols, C.byref(o) if o is not None else None)


def test_defaults_are_the_calls_without_options(mcrt, ctx, dev):
    """NULL options, default options, and weights 1 on the views in use with other weights past them: the old entry points' output"""
    E, R = 128, 465
    for geom, (F, N) in ((DEFAULT, (3, 3)), (GEOMETRIES[5], (11, 16)), (GEOMETRIES[3], (1, 5))):
        radius, angle, rows, cols = geom
        st = views(F, N, E, R, seed=9)
        old = tg.compound(ctx, dev, st, STEERS[N], geom)
        past = mcrt.compound_opts_struct()
        for n in range(N, 16):
            past.view_weight[n] = -3.0                         # not read
        for o in (None, mcrt.compound_opts_struct(), past):
            p = dev.upload(st); q = dev.upload(np.full(F * rows * cols, -7.25, f32))
            assert _opts_call(ctx, mcrt, p, F, E, R, STEERS[N], q, geom, o) == 0
            ic.assert_same_bits(ctx.d2h(q, (F, rows, cols)), old, "float, %s" % (geom,))
        env = tg.envelopes(2, N, seed=4)
        for kw in (dict(), dict(persistence=0.6, ref=0.5, tgc_db=tg.TGC)):
            want, wpeak = tg.bmode(ctx, dev, env, STEERS[N], geom, **kw)
            for o in (None, mcrt.compound_opts_struct()):
                par = mcrt.bmode_params(radius_mm=radius, total_angle=angle, out_rows=rows, out_cols=cols, **{k: v for k, v in kw.items() if k != "tgc_db"})
                cp = mcrt.compound_struct(STEERS[N])
                p = dev.upload(env); out = dev.upload(np.full(2 * rows * cols, 0xA5, np.uint8)); peak = dev(8)
                tgc = kw.get("tgc_db")
                vp = C.c_void_p
                assert ctx.L.mcrt_bmode_compound_frames_opts(ctx.h, vp(p), 2, tg.E8, tg.R8, C.byref(par), C.byref(cp), tgc.ctypes.data_as(vp) if tgc is not None else None,
                                                             None, vp(peak), vp(out), C.byref(o) if o is not None else None) == 0
                assert np.array_equal(ctx.d2h(out, (2, rows, cols), np.uint8), want)
                assert np.array_equal(ctx.d2h(peak, (2,)).view(np.uint32), wpeak.view(np.uint32))


@pytest.mark.parametrize("mode", MODES)
def test_hole_pixels_take_the_other_views(mcrt, ctx, dev, mode):
    """(20 mm, 3.6 rad, 96 x 160) at steer 0.5 has pixels with NaN maps: that view does not contribute there, in any mode"""
    geom = GEOMETRIES[3]
    E, R = 128, 465
    steers = (0.5, 0.0, 0.1)
    maps = tg.maps_of(mcrt, E, R, steers, geom)
    hole = np.isnan(maps[0][0])
    assert hole.any()
    st = np.random.default_rng(8).standard_normal((1, 3, E, R)).astype(f32)
    for feather in (0.0, 2.5):
        got = compound(ctx, dev, st, steers, geom, mode, None, feather)[0]
        others = compound(ctx, dev, st[:, 1:], steers[1:], geom, mode, None, feather)[0]
        assert np.array_equal(got[hole].view(np.uint32), others[hole].view(np.uint32))
        ic.assert_same_bits(got, mm.compound(st[0], maps, mode, None, feather)[0], mode + " with holes")
        alone = compound(ctx, dev, st[:, :1], steers[:1], geom, mode, None, feather)[0]
        assert np.all(alone[hole] == 0) and not np.signbit(alone[hole]).any()


def test_invariances(mcrt, ctx, dev):
    E, R = 128, 465
    # a permutation of the views and their stack leaves max and median as they are
    N = 5
    perm = [3, 0, 4, 2, 1]
    st = views(3, N, E, R, seed=5)
    w = weights_of(N, True)
    for geom in (DEFAULT, GEOMETRIES[5]):
        for mode in ("max", "median"):
            a = compound(ctx, dev, st, STEERS[N], geom, mode, w, 2.5)
            b = compound(ctx, dev, st[:, perm], [STEERS[N][i] for i in perm], geom, mode, [w[i] for i in perm], 2.5)
            ic.assert_same_bits(a, b, "%s under a permutation, %s" % (mode, geom))
    # a pass equals single calls
    F, N = 11, 3
    st = views(F, N, E, R, seed=6)
    for mode in MODES:
        got = compound(ctx, dev, st, STEERS[N], GEOMETRIES[2], mode, weights_of(N, True), 2.5)
        for f in (0, 7, 8, 10):
            one = compound(ctx, dev, st[f:f + 1], STEERS[N], GEOMETRIES[2], mode, weights_of(N, True), 2.5)
            ic.assert_same_bits(got[f], one[0], "%s frame %d alone" % (mode, f))
    # one view: max == median == mean, bit for bit
    st = views(3, 1, E, R, seed=7)
    for feather in (0.0, 2.5):
        mean, mx, med = (compound(ctx, dev, st, STEERS[1], DEFAULT, mode, (0.5,), feather) for mode in MODES)
        ic.assert_same_bits(mx, med, "max vs median, one view")
        # (w s) / w is s where w is a power of two -- off the ramp, w = 0.5 -- and w s is not subnormal
        w = mcrt.host_compound_weights(E, R, STEERS[1][0], 0.5, feather)
        ok = ((w == 0.5) | (w == 0))[None] & ~(np.isfinite(mean) & (np.abs(mean) < 1e-30) & (mean != 0))
        assert ok.mean() > 0.9
        ic.assert_same_bits(mean[ok], med[ok], "mean vs median, one view")


# ------------------------------------------------------------------ the 8-bit form
def bmode(ctx, dev, st, steers, geom=DEFAULT, state=None, **kw):
    F, N, E, R = st.shape
    radius, angle, rows, cols = geom
    p = dev.upload(st); out = dev.upload(np.full(F * rows * cols, 0xA5, np.uint8)); peak = dev.upload(np.full(F, -7.25, f32))
    ctx.bmode_compound_frames(p, F, E, R, steers, out, peak_dev=peak, state_dev=state, radius_mm=radius, total_angle=angle, out_rows=rows, out_cols=cols, **kw)
    ctx.synchronize()
    return ctx.d2h(out, (F, rows, cols), np.uint8), ctx.d2h(peak, (F,), f32)


def _mirror_kw(kw):
    kw = dict(kw)
    return dict(compound_mode=kw.pop("compound_mode", "mean"), weights=kw.pop("view_weights", None), **kw)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("F,N", [(3, 3), (2, 16)])
def test_bmode_modes_match_the_mirror(mcrt, ctx, dev, mode, F, N):
    """within one grey level, exact on 99.9 %; the reference of each frame bit for bit; automatic and fixed reference, TGC"""
    st = tg.envelopes(F, N, seed=N)
    maps = tg.maps_of(mcrt, tg.E8, tg.R8, STEERS[N], DEFAULT)
    plain, _ = tg.bmode(ctx, dev, st, STEERS[N], dynamic_range_db=48.0)
    for ref, gain, tgc, feather, unequal in ((None, 0.0, None, 2.5, True), (0.75, -3.0, tg.TGC, 0.0 if mode != "mean" else 8.0, False)):
        kw = dict(compound_mode=mode, view_weights=weights_of(N, unequal), feather_lines=feather, ref=ref, gain_db=gain, tgc_db=tgc, dynamic_range_db=48.0)
        got, peak = bmode(ctx, dev, st, STEERS[N], **kw)
        want, refs, _ = mm.bmode_compound(st, maps, **_mirror_kw(kw))
        for f in range(F):
            bm.assert_close(got[f], want[f])
        assert np.array_equal(peak.view(np.uint32), refs.view(np.uint32))
        assert got.max() > 100 and (got == 0).any()
        if ref is None:
            assert not np.array_equal(got, plain)


@pytest.mark.parametrize("mode", ["max", "median", "mean"])
def test_persistence_carries_across_calls(mcrt, ctx, dev, mode):
    """two calls of two frames equal one call of four; eleven frames in one lane's walk (a group of 8 and one of 3) match the mirror"""
    N = 3
    for geom in (DEFAULT, GEOMETRIES[5]):
        radius, angle, rows, cols = geom
        st = tg.envelopes(4, N, seed=3)
        kw = dict(compound_mode=mode, view_weights=weights_of(N, True), feather_lines=2.5, persistence=0.7)
        s4 = dev.upload(np.full(rows * cols, 0.25, f32))
        whole, _ = bmode(ctx, dev, st, STEERS[N], geom, state=s4, reset_state=True, **kw)
        s2 = dev.upload(np.full(rows * cols, 0.75, f32))
        a, _ = bmode(ctx, dev, st[:2], STEERS[N], geom, state=s2, reset_state=True, **kw)
        b, _ = bmode(ctx, dev, st[2:], STEERS[N], geom, state=s2, reset_state=False, **kw)
        assert np.array_equal(np.concatenate([a, b]), whole)
        assert np.array_equal(ctx.d2h(s2, (rows * cols,)).view(np.uint32), ctx.d2h(s4, (rows * cols,)).view(np.uint32))
        want, _, y = mm.bmode_compound(st, tg.maps_of(mcrt, tg.E8, tg.R8, STEERS[N], geom), **_mirror_kw(kw))
        for f in range(4):
            bm.assert_close(whole[f], want[f])
        assert np.abs(ctx.d2h(s4, (rows, cols)) - y).max() < 1e-5
    geom = GEOMETRIES[5]
    st = tg.envelopes(11, N, seed=5)
    got, _ = bmode(ctx, dev, st, STEERS[N], geom, **kw)
    want, _, _ = mm.bmode_compound(st, tg.maps_of(mcrt, tg.E8, tg.R8, STEERS[N], geom), **_mirror_kw(kw))
    for f in range(11):
        bm.assert_close(got[f], want[f])


# ------------------------------------------------------------------ errors
def test_new_refusals_leave_the_outputs_untouched(mcrt, ctx, dev):
    E, R, N, rows, cols = 16, 40, 2, 20, 24
    st = tg.views(1, N, E, R)
    p = dev.upload(st)
    img = np.full(rows * cols, -7.25, f32); q = dev.upload(img)
    bytes_ = np.full(rows * cols, 0xA5, np.uint8); o8 = dev.upload(bytes_)
    state0 = np.full(rows * cols, 0.5, f32); state = dev.upload(state0)
    peak0 = np.full(1, -7.25, f32); peak = dev.upload(peak0)
    L = ctx.L
    vp = C.c_void_p
    cp = mcrt.compound_struct((0.1, -0.1))
    par = mcrt.bmode_params(radius_mm=30.0, total_angle=1.0, out_rows=rows, out_cols=cols, persistence=0.5, reset_state=False)

    def cf(o, cp=cp, F=1):
        return L.mcrt_compound_frames_opts(ctx.h, vp(p), F, E, R, 30.0, 1.0, C.byref(cp), vp(q), rows, cols, C.byref(o) if o is not None else None)

    def bf(o, cp=cp, F=1):
        return L.mcrt_bmode_compound_frames_opts(ctx.h, vp(p), F, E, R, C.byref(par), C.byref(cp), None, vp(state), vp(peak), vp(o8), C.byref(o) if o is not None else None)

    S = mcrt.compound_opts_struct
    bad = [(S(mode=3), b"mode"), (S(mode=0xffffffff), b"mode")]
    bad += [(S(feather_lines=x), b"feather_lines") for x in (-1.0, math.nan, math.inf, -math.inf)]
    bad += [(S(view_weights=w), b"view_weight") for w in ((1.0, -0.5), (math.nan, 1.0), (1.0, math.inf), (0.0, 0.0), (-0.0, 0.0))]
    bad += [(S(mode=m, view_weights=(0.0, 0.0)), b"view_weight") for m in ("max", "median")]
    for call in (cf, bf):
        for o, word in bad:
            assert call(o) == INVALID, (o.mode, o.feather_lines, list(o.view_weight)[:2])
            assert word in L.mcrt_last_error(), L.mcrt_last_error()
        # what the calls without options refuse is still refused
        assert call(S("median"), cp=mcrt.compound_struct((0.0, math.nan))) == INVALID and b"steer" in L.mcrt_last_error()
        assert call(S("max"), F=0) == INVALID and call(S("max"), cp=mcrt.Compound()) == INVALID
        assert call(S("max"), F=32768) == -5
    ctx.synchronize()
    assert np.array_equal(ctx.d2h(q, (rows * cols,)).view(np.uint32), img.view(np.uint32))
    assert np.array_equal(ctx.d2h(o8, (rows * cols,), np.uint8), bytes_)
    assert np.array_equal(ctx.d2h(state, (rows * cols,)), state0) and np.array_equal(ctx.d2h(peak, (1,)), peak0)
    # a weight past n_views is not read; the context still works
    ok = S("median", (1.0, 0.5), 2.5); ok.view_weight[2] = math.nan
    assert cf(ok) == 0 and bf(ok) == 0
    ctx.synchronize()
    maps = tg.maps_of(mcrt, E, R, (0.1, -0.1), (30.0, 1.0, rows, cols))
    ic.assert_same_bits(ctx.d2h(q, (rows, cols)), mm.compound(st[0], maps, "median", (1.0, 0.5), 2.5)[0], "after the errors")
    assert ctx.d2h(peak, (1,))[0] > 0
    with pytest.raises(KeyError):
        ctx.compound_frames(p, 1, E, R, (0.1, -0.1), q, mode="mode")


# ------------------------------------------------------------------ the wrappers
def test_simulator(mcrt, tex256):
    """Simulator(compound=, compound_mode="median", compound_feather=8): compound_image and bmode equal the hand-made pipeline"""
    cfg, meshes = mcrt.synth.sphere_scene(3)
    sd = mcrt.scene_io.build_scene(cfg, meshes)
    E, S = 16, 16
    tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    sim = mcrt.Simulator(sd, tr, n_samples=S, texture=tex256, compound=tg.STEER3, compound_mode="median", compound_feather=8)
    plain = mcrt.Simulator(sd, tr, n_samples=S, texture=tex256, compound=tg.STEER3)
    try:
        ctx, R, N = sim.ctx, sim.R, sim.N
        picture = sim.compound_image(2)
        views_dev = ctx.alloc(N * E * R * 4)
        ctx.trace_frames_poses(2 * N, sim.view_pos, sim.view_dir, views_dev)
        ctx.convolve_frames(views_dev, N, E, R, sim.psf.axial_kernel, sim.psf.lateral_kernel)
        ctx.envelope_frames(views_dev, N, E, R)
        a, b = ctx.alloc(400 * 500 * 4), ctx.alloc(400 * 500)
        ctx.compound_frames(views_dev, 1, E, R, tg.STEER3, a, mode="median", feather_lines=8.0)
        ctx.bmode_compound_frames(views_dev, 1, E, R, tg.STEER3, b, dynamic_range_db=50.0, compound_mode="median", feather_lines=8.0)
        ic.assert_same_bits(picture, ctx.d2h(a, (400, 500)), "compound_image")
        assert np.array_equal(sim.bmode(2, dynamic_range_db=50.0), ctx.d2h(b, (400, 500), np.uint8))
        env = ctx.d2h(views_dev, (N, E, R))
        ic.assert_same_bits(picture, mm.compound(env, tg.maps_of(mcrt, E, R, tg.STEER3, DEFAULT), "median", None, 8.0)[0], "vs the mirror")
        for d in (views_dev, a, b):
            ctx.free(d)
        other = plain.compound_image(2)
        assert np.count_nonzero(picture) > 1000 and not np.array_equal(other, picture)
    finally:
        sim.close(); plain.close()
    for kw in (dict(compound_mode="max"), dict(compound_feather=2.0), dict(compound=tg.STEER3, compound_weights=(1.0, 2.0))):
        with pytest.raises(ValueError):
            mcrt.Simulator(sd, tr, n_samples=S, texture=tex256, **kw)


def test_host_shim(mcrt, tmp_path):
    """rf_image::postprocess with an mcrt_compound_opts writes the pictures Python's Simulator produces, bit for bit"""
    pkg = os.path.join(ROOT, "mcray-tracing_amd")
    exe = str(tmp_path / "compound_modes_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(pkg, "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "compound_modes_driver.cpp"), "-L", pkg, "-lmcrt_hip", "-Wl,-rpath," + pkg])
    cfg, scene = tg._write_scene(mcrt, tmp_path)
    E, S, frame = 64, 8, 3
    tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    for mode, feather, weights in (("median", 8.0, (1.0, 1.0, 1.0)), ("mean", 4.0, (1.0, 0.5, 2.0))):
        out = tmp_path / (mode + ".bin")
        r = subprocess.run([exe, scene, str(out), str(frame), str(S), ",".join(repr(s) for s in tg.STEER3), mode, repr(feather), ",".join(repr(w) for w in weights)],
                           capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout + r.stderr
        raw = out.read_bytes()
        assert len(raw) == 400 * 500 * 5
        picture = np.frombuffer(raw, f32, 400 * 500).reshape(400, 500)
        bytes_ = np.frombuffer(raw, np.uint8, 400 * 500, 400 * 500 * 4).reshape(400, 500)
        sim = mcrt.Simulator(mcrt.scene_io.load_scene_file(scene), tr, n_samples=S, compound=tg.STEER3, compound_mode=mode, compound_feather=feather,
                             compound_weights=weights)
        try:
            ic.assert_same_bits(picture, sim.compound_image(frame), "shim vs python, float, " + mode)
            assert np.array_equal(bytes_, sim.bmode(frame))
        finally:
            sim.close()
        assert np.count_nonzero(picture) > 1000 and bytes_.max() > 200


def test_cli_options(mcrt, tmp_path):
    exe = os.path.join(ROOT, "mcray-tracing_amd", "mattausch_hip")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "mcray-tracing_amd"), "mattausch_hip"])
    _, scene = tg._write_scene(mcrt, tmp_path)

    def run(name, *opts):
        r = subprocess.run([exe, scene, "2", "5", str(tmp_path / (name + ".pgm")), str(tmp_path / (name + ".bin"))] + list(opts),
                           capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout + r.stderr
        return (tmp_path / (name + ".pgm")).read_bytes(), (tmp_path / (name + ".bin")).read_bytes()

    three = run("three", "--compound", "3")
    assert run("defaults", "--compound", "3", "--compound-mode", "mean", "--compound-feather", "0", "--compound-weights", "1,1,1") == three
    pictures = {three[0]}
    for name, opts in (("max", ["--compound-mode", "max"]), ("median", ["--compound-mode", "median"]), ("feather", ["--compound-feather", "16"]),
                       ("weights", ["--compound-weights", "1,0.25,2"])):
        got = run(name, "--compound", "3", *opts)
        assert len(got[0]) == len(three[0]) and got[0] not in pictures, name
        assert got[1] == three[1]                               # rf.bin, the unsteered view, is as it was
        pictures.add(got[0])
    db = run("db", "--compound", "3", "--db", "60")
    assert run("db_defaults", "--compound", "3", "--db", "60", "--compound-mode", "mean") == db
    assert run("db_median", "--compound", "3", "--db", "60", "--compound-mode", "median", "--compound-feather", "8")[0] != db[0]
    for bad, word in ((["--compound-mode", "max"], "--compound-mode"), (["--compound-feather", "4"], "--compound-feather"), (["--compound-weights", "1,1,1"], "--compound-weights"),
                      (["--compound", "3", "--compound-weights", "1,1"], "--compound-weights"), (["--compound", "3", "--compound-weights", "1,1,1,1"], "--compound-weights"),
                      (["--compound", "3", "--compound-mode", "mode"], "--compound-mode"), (["--compound", "3", "--compound-feather", "-1"], "--compound-feather"),
                      (["--compound", "3", "--compound-weights", "0,0,0"], "view_weight"), (["--compound", "3", "--elevation", "3", "--compound-mode", "max"], "--compound")):
        r = subprocess.run([exe, scene, "1", "5"] + bad, capture_output=True, text=True, timeout=240)
        assert r.returncode == 1 and word in r.stdout, (bad, r.stdout)
