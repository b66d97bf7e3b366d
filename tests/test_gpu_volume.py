"""Volume imaging on the MI355X: mcrt_volume_frames and mcrt_bmode_volume_frames (k_volume) against the numpy mirror (tests/volume_mirror.py,
fed with the product's own maps) -- bit for bit in the float form, within bmode_mirror.assert_close in the 8-bit form --, a pass against
single calls, a cut against its layer, the four cached grids, the argument errors, a traced scene end to end against the CPU oracle, the
Simulator, a two-rank group, the C++ shim and the CLI."""
import ctypes as C
import json
import math
import os
import subprocess
import numpy as np
import pytest

import bmode_mirror as bm
import image_cases as ic
import volume_mirror as vm
from test_gpu_focus import Dev

pytestmark = pytest.mark.gpu

f32 = np.float32
INVALID, LIMIT = -1, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIVOTS = (-20.0, 0.0, 10.0)
# (K, F) handed out in turn to the (grid, shape) pairs: every pair of K in {1, 2, 3, 8} and F in {1, 3} meets several shapes and grids
COMBOS = [(1, 1), (2, 3), (3, 1), (8, 3), (8, 1), (1, 3), (2, 1), (3, 3)]


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


def planes(F, K, E, R, seed=0):
    """[F][K][E][R]: ic.scan_image per plane (noise with NaN and +-inf taps), a few taps set to -0.0"""
    st = np.stack([np.stack([ic.scan_image(E, R, seed=seed + 100 * f + k) for k in range(K)]) for f in range(F)])
    flat = st.reshape(-1)
    flat[np.random.default_rng(seed + E + R).integers(0, flat.size, max(1, flat.size // 61))] = -0.0
    return st


def shape_of(g):
    return (g.nw, g.nv, g.nu)


def gather(ctx, dev, st, sweep, g, fill=None, p=None):
    F, K, E, R = st.shape
    n = g.nu * g.nv * g.nw
    p = p or dev.upload(st); q = dev(F * n * 4)
    if fill is not None:
        ctx.h2d(q, np.full(F * n, fill, f32))
    ctx.volume_frames(p, F, E, R, sweep, g, q)
    return ctx.d2h(q, (F,) + shape_of(g))


# ------------------------------------------------------------------ the float form
@pytest.mark.parametrize("gi", range(len(vm.GRID_SHAPES)))
def test_volume_frames_match_the_mirror(mcrt, ctx, dev, gi):
    """every point, bit for bit, with NaN / inf / -0.0 taps; the output is pre-filled so that an unwritten point shows"""
    which = vm.GRID_SHAPES[gi]
    for si, (E, R) in enumerate(ic.SCAN_SHAPES):
        K, F = COMBOS[(gi * len(ic.SCAN_SHAPES) + si + gi) % len(COMBOS)]
        pivot = PIVOTS[(gi + si) % len(PIVOTS)]
        g = vm.grid_for(mcrt, which, E, R, K, pivot)
        sweep = (K, vm.STEP, pivot)
        st = planes(F, K, E, R, seed=gi)
        got = gather(ctx, dev, st, sweep, g, fill=-7.25)
        want = vm.volume_frames(st, mcrt.host_volume_maps(E, R, sweep, g))
        ic.assert_same_bits(got, want, "grid %s shape %s K %d F %d pivot %g" % (which, (E, R), K, F, pivot))


def test_every_k_f_and_pivot_at_one_shape(mcrt, ctx, dev):
    E, R = 37, 211
    for K in (1, 2, 3, 8):
        for pivot in PIVOTS:
            g = vm.grid_for(mcrt, (33, 35, 5), E, R, K, pivot)
            maps = mcrt.host_volume_maps(E, R, (K, vm.STEP, pivot), g)
            for F in (1, 3):
                st = planes(F, K, E, R, seed=K)
                ic.assert_same_bits(gather(ctx, dev, st, (K, vm.STEP, pivot), g, fill=-7.25), vm.volume_frames(st, maps), "K %d F %d pivot %g" % (K, F, pivot))


def test_points_beside_the_sweep(mcrt, ctx, dev):
    """a grid twice as large as the swept region in every direction: planes -1 and K, rows and scan-lines outside, points behind the pivot --
    zeros where nothing is inside, the half-weighted edge plane where one plane is"""
    E, R, K, pivot = 37, 211, 3, 10.0
    c, h = vm.box(E, R, K, pivot)
    g = mcrt.volume_grid((c[0] - 6 * h[0], -20.0, c[2] - 6 * h[2]), (12 * h[0] / 40, 0, 0), (0, 220.0 / 44, 0), (0, 0, 12 * h[2] / 12), 41, 45, 13)
    maps = mcrt.host_volume_maps(E, R, (K, vm.STEP, pivot), g)
    mz = maps[0]
    assert (mz < -1).any() and (mz >= K).any() and ((mz >= -1) & (mz < 0)).any() and ((mz >= K - 1) & (mz < K)).any() and ((mz >= 0) & (mz < K - 1)).any()
    st = np.random.default_rng(3).standard_normal((2, K, E, R)).astype(f32)
    got = gather(ctx, dev, st, (K, vm.STEP, pivot), g, fill=-7.25)
    ic.assert_same_bits(got, vm.volume_frames(st, maps), "beside the sweep")
    assert np.all(got[:, (mz < -1) | (mz >= K)] == 0) and (got != 0).sum() > 100


def test_a_pass_equals_single_calls(mcrt, ctx, dev):
    """11 frames.  At 160 x 200 x 14 points the pass is cut into chunks of 2 frames (a lane walks two frames and, in the last chunk, one); at
    33 x 35 x 5 a chunk is one frame"""
    E, R, K, F, pivot = 128, 465, 3, 11, 10.0
    st = planes(F, K, E, R, seed=5)
    p = dev.upload(st)
    for which in ((160, 200, 14), (33, 35, 5)):
        g = vm.grid_for(mcrt, which, E, R, K, pivot)
        got = gather(ctx, dev, st, (K, vm.STEP, pivot), g, p=p)
        for f in range(F):
            one = gather(ctx, dev, st[f:f + 1], (K, vm.STEP, pivot), g, p=p + f * K * E * R * 4)
            assert np.array_equal(got[f].view(np.uint32), one[0].view(np.uint32)), (which, f)
        assert np.count_nonzero(np.nan_to_num(got)) > got.size // 2


def test_a_cut_is_its_layer_of_the_volume(mcrt, ctx, dev):
    E, R, K, pivot = 128, 465, 8, 0.0
    g = vm.grid_for(mcrt, (33, 35, 5), E, R, K, pivot)
    st = planes(2, K, E, R, seed=6)
    whole = gather(ctx, dev, st, (K, vm.STEP, pivot), g)
    for l in range(5):
        cut = gather(ctx, dev, st, (K, vm.STEP, pivot), vm.layer_cut(mcrt, g, l), fill=-7.25)
        ic.assert_same_bits(cut[:, 0], whole[:, l], "layer %d" % l)


def test_a_volume_and_three_cuts_in_turn(mcrt, ctx, dev):
    """the four grids a display asks for per frame -- the volume, a C-plane, a sagittal cut, an oblique cut -- alternate without a
    synchronisation in between; the second round gives the first round's bits (its maps are the cached ones), and a fifth grid, which evicts
    one of the four, and the evicted one after it are right too"""
    E, R, K, pivot = 64, 465, 8, 10.0
    sweep = (K, vm.STEP, pivot)
    c, h = vm.box(E, R, K, pivot)
    grids = [vm.grid_for(mcrt, (33, 35, 5), E, R, K, pivot), mcrt.cplane_grid(c[1], 48, 40, 2 * h[0] / 48), mcrt.sagittal_grid(0.5, 40, 36, 2 * h[2] / 40, c[1] - h[1]),
             vm.grid_for(mcrt, "oblique", E, R, K, pivot), vm.grid_for(mcrt, (257, 3, 2), E, R, K, pivot)]
    st = planes(1, K, E, R, seed=7)
    p = dev.upload(st)
    outs = [[dev(g.nu * g.nv * g.nw * 4) for g in grids[:4]] for _ in range(2)]
    ctx.synchronize()
    for rnd in range(2):
        for g, q in zip(grids[:4], outs[rnd]):
            ctx.volume_frames(p, 1, E, R, sweep, g, q)
    ctx.synchronize()
    for i, g in enumerate(grids[:4]):
        first = ctx.d2h(outs[0][i], shape_of(g)); second = ctx.d2h(outs[1][i], shape_of(g))
        ic.assert_same_bits(first, vm.volume(st[0], mcrt.host_volume_maps(E, R, sweep, g)), "grid %d" % i)
        ic.assert_same_bits(second, first, "grid %d, second round" % i)
    for i in (4, 0, 1, 4, 2, 3):
        g = grids[i]
        ic.assert_same_bits(gather(ctx, dev, st, sweep, g, p=p)[0], vm.volume(st[0], mcrt.host_volume_maps(E, R, sweep, g)), "after eviction, grid %d" % i)
    # the key holds the sweep as well: the same grid under another step or pivot is another set of maps
    for other in ((K, 0.04, pivot), (K, vm.STEP, 0.0), (K - 1, vm.STEP, pivot)):
        ic.assert_same_bits(gather(ctx, dev, st[:, :other[0]], other, grids[0])[0], vm.volume(st[0, :other[0]], mcrt.host_volume_maps(E, R, other, grids[0])), str(other))


# ------------------------------------------------------------------ the 8-bit form
E8, R8, K8 = 128, 465, 3
TGC = (0.02 * np.arange(R8)).astype(f32)


def envelopes(F, K, seed=0):
    """[F][K][E8][R8]: positive speckle falling off with depth, brighter in later planes, with NaN and inf scan-lines"""
    rng = np.random.default_rng(50 + seed)
    st = np.abs(rng.standard_normal((F, K, E8, R8))).astype(f32) * np.exp(-np.arange(R8, dtype=f32) / f32(150.0))[None, None, None, :]
    st *= (1.0 + 0.5 * np.arange(K, dtype=f32))[None, :, None, None]
    st[:, :, 1::2] *= -1
    st[0, 0, 40] = np.nan; st[0, K - 1, 41] = np.inf; st[F - 1, 0, 90, 100:200] = -np.inf
    return st.astype(f32)


def bmode(ctx, dev, st, sweep, g, **kw):
    F, K, E, R = st.shape
    n = g.nu * g.nv * g.nw
    p = dev.upload(st); out = dev.upload(np.full(F * n, 0xA5, np.uint8)); peak = dev.upload(np.full(F, -7.25, f32))
    ctx.bmode_volume_frames(p, F, E, R, sweep, g, out, peak_dev=peak, **kw)
    ctx.synchronize()
    return ctx.d2h(out, (F,) + shape_of(g), np.uint8), ctx.d2h(peak, (F,), f32)


@pytest.mark.parametrize("mode", ["db", "ref_log"])
@pytest.mark.parametrize("ref,gain,tgc", [(None, 0.0, None), (None, 6.0, TGC), (0.75, -3.0, TGC)])
def test_bmode_volume_matches_the_mirror(mcrt, ctx, dev, mode, ref, gain, tgc):
    """test_gpu_bmode.py's tolerance: within one grey level, exact on 99.9 % (the device's log10f is not numpy's); the reference each frame used
    bit for bit: with the automatic one the largest amplitude over the WHOLE sweep of the frame, a fixed one as given"""
    F, pivot = 3, 10.0
    sweep = (K8, vm.STEP, pivot)
    st = envelopes(F, K8)
    kw = dict(mode=mode, ref=ref, gain_db=gain, tgc_db=tgc, dynamic_range_db=48.0)
    for which in ((33, 35, 5), "oblique"):                  # 5775 points: byte stores at the end and an odd size; 3072: word stores throughout
        g = vm.grid_for(mcrt, which, E8, R8, K8, pivot)
        got, peak = bmode(ctx, dev, st, sweep, g, **kw)
        want, refs = vm.bmode_volume(st, mcrt.host_volume_maps(E8, R8, sweep, g), **kw)
        for f in range(F):
            bm.assert_close(got[f], want[f])
        assert np.array_equal(peak.view(np.uint32), refs.view(np.uint32))
        if ref is None:
            k = bm.tgc_factors(tgc, R8)
            per_plane = np.array([[bm.amplitude(st[f, n], k).max() for n in range(K8)] for f in range(F)])
            assert np.array_equal(refs, per_plane.max(axis=1)) and (per_plane.argmax(axis=1) == K8 - 1).all()     # the brightest plane sets it
        else:
            assert np.all(refs == f32(ref))
        assert len(np.unique(got)) > 50                                     # (a picture, not a blank: the mirror has 78 to 247 grey levels here)


@pytest.mark.parametrize("which", [(1, 1, 1), (257, 3, 2), (160, 200, 14)])
def test_bmode_volume_at_other_grids(mcrt, ctx, dev, which):
    """one point; 1542 points (no multiple of 4: bytes); 448 000 points (chunks of more than one frame) -- and an output that is not
    word-aligned"""
    F, pivot = 5, 0.0
    sweep = (K8, vm.STEP, pivot)
    st = envelopes(F, K8, seed=1)
    g = vm.grid_for(mcrt, which, E8, R8, K8, pivot)
    got, peak = bmode(ctx, dev, st, sweep, g, dynamic_range_db=50.0)
    want, refs = vm.bmode_volume(st, mcrt.host_volume_maps(E8, R8, sweep, g), dynamic_range_db=50.0)
    for f in range(F):
        bm.assert_close(got[f], want[f])
    assert np.array_equal(peak.view(np.uint32), refs.view(np.uint32))
    if which == (160, 200, 14):
        n = g.nu * g.nv * g.nw
        p = dev.upload(st[:1]); out = dev.upload(np.full(n + 8, 0xA5, np.uint8))
        ctx.bmode_volume_frames(p, 1, E8, R8, sweep, g, out + 1, dynamic_range_db=50.0)
        ctx.synchronize()
        raw = ctx.d2h(out, (n + 8,), np.uint8)
        assert raw[0] == 0xA5 and np.all(raw[n + 1:] == 0xA5) and np.array_equal(raw[1:n + 1].reshape(shape_of(g)), got[0])


# ------------------------------------------------------------------ errors
def test_errors_leave_the_outputs_untouched(mcrt, ctx, dev):
    E, R, K = 16, 40, 2
    st = planes(1, K, E, R)
    p = dev.upload(st)
    good_g = mcrt.volume_grid((-5, 60, -1), (0.5, 0, 0), (0, 0.5, 0), (0, 0, 0.5), 6, 5, 4)
    n = 120
    img = np.full(n, -7.25, f32); q = dev.upload(img)
    bytes_ = np.full(n, 0xA5, np.uint8); o8 = dev.upload(bytes_)
    peak0 = np.full(1, -7.25, f32); peak = dev.upload(peak0)
    big = dev(2 * 2049 * 4)
    L = ctx.L
    vp = C.c_void_p
    good_s = mcrt.sweep_struct(K, 0.05, 10.0)

    def vf(h=ctx.h, rf=p, F=1, e=E, r=R, radius=30.0, angle=1.0, sw=good_s, g=good_g, out=q):
        return L.mcrt_volume_frames(h, vp(rf) if rf else None, F, e, r, radius, angle, C.byref(sw) if sw is not None else None, C.byref(g) if g is not None else None,
                                    vp(out) if out else None)

    def bf(h=ctx.h, rf=p, F=1, e=E, r=R, sw=good_s, g=good_g, out=o8, par=None, tgc=None, angle=1.0):
        par = par if par is not None else mcrt.bmode_params(radius_mm=30.0, total_angle=angle, out_rows=0, out_cols=0)
        return L.mcrt_bmode_volume_frames(h, vp(rf) if rf else None, F, e, r, C.byref(par) if par is not False else None, C.byref(sw) if sw is not None else None,
                                          C.byref(g) if g is not None else None, tgc.ctypes.data_as(vp) if tgc is not None else None, vp(peak), vp(out) if out else None)

    def grid(**kw):
        g = mcrt.volume_grid((-5, 60, -1), (0.5, 0, 0), (0, 0.5, 0), (0, 0, 0.5), 6, 5, 4)
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(g, k)[v[0]] = v[1]
            else:
                setattr(g, k, v)
        return g

    for call in (vf, bf):
        assert call(h=None) == INVALID
        assert call(rf=None) == INVALID and call(out=None) == INVALID and call(sw=None) == INVALID and call(g=None) == INVALID
        for kw in (dict(F=0), dict(e=0), dict(r=0)):
            assert call(**kw) == INVALID, kw
        for s in ((0, 0.05, 0.0), (257, 0.001, 0.0), (K, 0.0, 0.0), (K, -0.1, 0.0), (K, math.nan, 0.0), (K, math.inf, 0.0), (K, 3.2, 0.0), (K, 0.05, math.nan),
                  (K, 0.05, math.inf)):
            assert call(sw=mcrt.sweep_struct(*s)) == INVALID, s
        for kw in (dict(nu=0), dict(nv=0), dict(nw=0), dict(origin_mm=(1, math.nan)), dict(du_mm=(0, math.inf)), dict(dv_mm=(2, -math.inf)), dict(dw_mm=(1, math.nan))):
            assert call(g=grid(**kw)) == INVALID, kw
        assert call(g=grid(nu=1 << 16, nv=1 << 15, nw=1)) == LIMIT and call(g=grid(nu=0xFFFFFFFF, nv=0xFFFFFFFF, nw=0xFFFFFFFF)) == LIMIT
        assert call(rf=big, e=2, r=2049) == LIMIT
        assert call(F=32768) == LIMIT and call(F=256, sw=mcrt.sweep_struct(256, 0.001, 0.0)) == LIMIT       # F * K > 65535
        for angle in (0.0, -1.0, math.nan):
            assert call(angle=angle) == INVALID
        # overlap: the output inside the stack, on its last bytes, ending just inside its start
        for out in (p, p + K * E * R * 4 - 4, p - 4):
            assert call(out=out) == INVALID and b"overlap" in L.mcrt_last_error()
    assert bf(par=False) == INVALID
    assert bf(e=1 << 28, r=2, sw=mcrt.sweep_struct(16, 0.05, 0.0)) == LIMIT and b"scan-lines" in L.mcrt_last_error()      # K * E does not fit 32 bits
    for kw in (dict(mode=7), dict(dynamic_range_db=0.0), dict(dynamic_range_db=math.nan), dict(gain_db=math.inf), dict(ref=math.nan), dict(persistence=1.0),
               dict(persistence=-0.1), dict(persistence=0.5)):
        assert bf(par=mcrt.bmode_params(radius_mm=30.0, total_angle=1.0, out_rows=0, out_cols=0, **kw)) == INVALID, kw
    assert b"persistence" in L.mcrt_last_error()
    bad_tgc = np.zeros(R, f32); bad_tgc[7] = np.nan
    assert bf(tgc=bad_tgc) == INVALID
    ctx.synchronize()
    assert np.array_equal(ctx.d2h(q, (n,)).view(np.uint32), img.view(np.uint32))
    assert np.array_equal(ctx.d2h(o8, (n,), np.uint8), bytes_)
    assert np.array_equal(ctx.d2h(peak, (1,)), peak0)
    assert np.array_equal(ctx.d2h(p, st.shape).view(np.uint32), st.view(np.uint32))
    # the context still works; p's own picture size is ignored, whatever it says
    assert vf() == 0 and bf(par=mcrt.bmode_params(radius_mm=30.0, total_angle=1.0, out_rows=7, out_cols=1 << 31)) == 0
    ctx.synchronize()
    maps = mcrt.host_volume_maps(E, R, (K, 0.05, 10.0), good_g, radius_mm=30.0, total_angle=1.0)
    ic.assert_same_bits(ctx.d2h(q, (4, 5, 6)), vm.volume(st[0], maps), "after the errors")
    assert ctx.d2h(peak, (1,))[0] > 0


# ------------------------------------------------------------------ end to end: a traced scene
SWEEP3 = (3, 0.06)
PIVOT3 = 10.0


def _oracle(orc, sd):
    return orc.OracleScene(sd.tri, sd.tri_mesh, sd.meshes, sd.materials, sd.start_mat, sd.spacing)


def _setup(obj, sd, tr, S, tex):
    obj.set_params(n_elements=tr.n_elements, n_samples=S, frequency=tr.frequency)
    obj.upload_scene(sd)
    obj.upload_texture(tex, 256)
    obj.set_transducer(tr.pos, tr.dir)


def _cut_for(mcrt, E, R):
    """a sagittal cut and a small volume inside the 3-plane sweep"""
    c, h = vm.box(E, R, SWEEP3[0], PIVOT3)
    s = SWEEP3[1] / vm.STEP
    return (mcrt.sagittal_grid(c[0], 40, 48, 2 * h[2] * s / 40, c[1] - h[1], z0_mm=-h[2] * s), mcrt.volume_grid((c[0] - h[0], c[1] - h[1], -h[2] * s), (2 * h[0] / 32, 0, 0),
            (0, 2 * h[1] / 24, 0), (0, 0, 2 * h[2] * s / 4), 33, 25, 5))


def _rotate(v, axis, ang):
    k = np.asarray(axis, np.float64)
    return v * math.cos(ang) + np.cross(k, v) * math.sin(ang) + k * (v @ k) * (1 - math.cos(ang))


def test_a_traced_scene_end_to_end(mcrt, orc, tex256):
    """the planes the Simulator traces are the CPU oracle's frames from the same swept tables with frame id f * K + k, bit for bit; the
    volume after PSF and envelope is the mirror's, fed with the oracle's planes; and the first segment of every path of plane k ends in
    that plane's tilted plane"""
    cfg, meshes = mcrt.synth.sphere_scene(3)
    sd = mcrt.scene_io.build_scene(cfg, meshes)
    E, S, K = 32, 16, SWEEP3[0]
    tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    pos, dirs = tr.swept(K, SWEEP3[1], PIVOT3)
    assert pos[1].tobytes() == tr.pos.tobytes() and dirs[1].tobytes() == tr.dir.tobytes() and pos[0].tobytes() != tr.pos.tobytes()
    p = orc.default_params(n_elements=E, n_samples=S)
    R = p.n_rows
    osc = _oracle(orc, sd)
    frames = (0, 2)
    want = {f: np.stack([osc.trace_frame(p, pos[k], dirs[k], tex256, frame_id=f * K + k, use_bvh=False)["rf"].T for k in range(K)]) for f in frames}
    for f in frames:
        assert np.count_nonzero(np.nan_to_num(want[f][1])) > 1000
        assert not np.array_equal(want[f][0], want[f][1], equal_nan=True) and not np.array_equal(want[f][2], want[f][1], equal_nan=True)
    sim = mcrt.Simulator(sd, tr, n_samples=S, texture=tex256, sweep=SWEEP3, sweep_pivot_mm=PIVOT3)
    try:
        assert sim.R == R
        with pytest.raises(RuntimeError):
            sim.frame(0)
        with pytest.raises(RuntimeError):
            sim.bmode(0)
        sw = (K, SWEEP3[1], PIVOT3)
        for f in frames:
            sim.trace(f)
            sim.ctx.synchronize()
            ic.assert_same_bits(sim.ctx.d2h(sim.sweep_dev, (K, E, R)), want[f], "volume %d vs the oracle" % f)
            env = np.stack([orc.envelope(orc.convolve(np.ascontiguousarray(want[f][k].T), sim.psf.axial_kernel, sim.psf.lateral_kernel)).T for k in range(K)])
            for g in _cut_for(mcrt, E, R):
                maps = mcrt.host_volume_maps(E, R, sw, g)
                assert vm.taps_inside(maps, E, R, K).mean() > 0.5
                got = sim.volume(f, g)
                ic.assert_same_bits(got, vm.volume(env, maps), "volume(%d)" % f)
                assert np.count_nonzero(np.nan_to_num(got)) > 1000
                raw = sim.volume(f, g, convolve=False, envelope=False)
                ic.assert_same_bits(raw, vm.volume(want[f], maps), "raw volume(%d)" % f)
                b = sim.bmode_volume(f, g, dynamic_range_db=50.0)
                bm.assert_close(b, vm.bmode_volume(env[None], maps, dynamic_range_db=50.0)[0][0])
                assert len(np.unique(b)) > 20                                   # (a picture, not a blank)
        # the rays of plane k stay in plane k: normal (0, -sin, cos) of the probe-local frame through (0, pivot, 0), rotated and moved with the probe
        tilts = mcrt.sweep_tilts(K, SWEEP3[1])
        for k in range(K):
            sim.ctx.set_transducer(pos[k], dirs[k])
            segs, cnt, _ = sim.ctx.cast_rays(k)
            nrm = np.array([0.0, -math.sin(float(tilts[k])), math.cos(float(tilts[k]))]); p0 = np.array([0.0, PIVOT3 / 10.0, 0.0])
            for axis, a in (((0, 0, 1), tr.angles[2]), ((1, 0, 0), tr.angles[0]), ((0, 1, 0), tr.angles[1])):
                nrm = _rotate(nrm, axis, float(f32(a)) * math.pi / 180.0); p0 = _rotate(p0, axis, float(f32(a)) * math.pi / 180.0)
            p0 = p0 + np.asarray(tr.position, np.float64)
            ends = segs["to"][:, :, 0][cnt > 0].astype(np.float64)
            off = np.abs((ends - p0) @ nrm)
            print("plane %d: %d first segments, at most %.3g cm off the tilted plane" % (k, len(ends), off.max()))
            assert len(ends) > E * S // 2 and off.max() < 1e-4
            if k != 1:                                          # ... and not in the probe's own
                n0 = np.array([0.0, 0.0, 1.0])
                for axis, a in (((0, 0, 1), tr.angles[2]), ((1, 0, 0), tr.angles[0]), ((0, 1, 0), tr.angles[1])):
                    n0 = _rotate(n0, axis, float(f32(a)) * math.pi / 180.0)
                assert np.abs((ends - p0) @ n0).max() > 0.05
    finally:
        sim.close()
    plain = mcrt.Simulator(sd, tr, n_samples=S, texture=tex256)
    try:
        with pytest.raises(RuntimeError):
            plain.volume(0, _cut_for(mcrt, E, R)[0])
    finally:
        plain.close()


def test_a_two_rank_group_equals_one_context(mcrt, sphere, tex256):
    cfg, sd = sphere
    E, S, F, K = 16, 32, 2, SWEEP3[0]
    tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    pos, dirs = tr.swept(K, SWEEP3[1], PIVOT3)
    pos, dirs = np.tile(pos, (F, 1, 1)), np.tile(dirs, (F, 1, 1))
    psf = mcrt.Psf(freq=tr.frequency)
    sw = (K, SWEEP3[1], PIVOT3)
    one = mcrt.Context(0); _setup(one, sd, tr, S, tex256)
    grp = mcrt.Group([0, 0]); _setup(grp, sd, tr, S, tex256)
    try:
        R = one.params.n_rows
        g = _cut_for(mcrt, E, R)[1]
        n = g.nu * g.nv * g.nw
        out = []
        for tracer, c in ((one, one), (grp, grp.root)):
            st_dev = c.alloc(F * K * E * R * 4)
            tracer.trace_frames_poses(5 * K, pos, dirs, st_dev)
            tracer.synchronize()
            raw = c.d2h(st_dev, (F, K, E, R))
            c.convolve_frames(st_dev, F * K, E, R, psf.axial_kernel, psf.lateral_kernel)
            c.envelope_frames(st_dev, F * K, E, R)
            a, b = c.alloc(F * n * 4), c.alloc(F * n)
            c.volume_frames(st_dev, F, E, R, sw, g, a)
            c.bmode_volume_frames(st_dev, F, E, R, sw, g, b, dynamic_range_db=50.0)
            out.append((raw, c.d2h(a, (F,) + shape_of(g)), c.d2h(b, (F,) + shape_of(g), np.uint8)))
            for d in (st_dev, a, b):
                c.free(d)
        for a, b in zip(out[0], out[1]):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
        assert np.count_nonzero(out[1][1]) > 1000 and len(np.unique(out[1][2])) > 20
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


def test_host_shim(mcrt, tmp_path):
    """transducer<N>::swept and rf_image::trace / convolve / envelope / volume with a sweep write the tables and the cuts Python's Simulator
    produces, bit for bit"""
    pkg = os.path.join(ROOT, "mcray-tracing_amd")
    exe = str(tmp_path / "volume_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(pkg, "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "volume_driver.cpp"), "-L", pkg, "-lmcrt_hip", "-Wl,-rpath," + pkg])
    cfg, scene = _write_scene(mcrt, tmp_path)
    out = tmp_path / "volume.bin"
    E, S, frame, K, step, pivot = 64, 8, 3, 4, 0.05, 10.0          # an even sweep: no plane at tilt 0
    depth, nu, nv, pitch = 90.0, 96, 40, 0.25
    r = subprocess.run([exe, scene, str(out), str(frame), str(S), str(K), repr(step), repr(pivot), repr(depth), str(nu), str(nv), repr(pitch)],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = out.read_bytes()
    tab = K * E * 3 * 4
    assert len(raw) == 2 * tab + nu * nv * 5
    tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    pos, dirs = tr.swept(K, step, pivot)
    assert raw[:tab] == pos.tobytes() and raw[tab:2 * tab] == dirs.tobytes()
    cut = np.frombuffer(raw, f32, nu * nv, 2 * tab).reshape(1, nv, nu)
    bytes_ = np.frombuffer(raw, np.uint8, nu * nv, 2 * tab + nu * nv * 4).reshape(1, nv, nu)
    sim = mcrt.Simulator(mcrt.scene_io.load_scene_file(scene), tr, n_samples=S, sweep=(K, step), sweep_pivot_mm=pivot)
    try:
        g = mcrt.cplane_grid(depth, nu, nv, pitch)
        ic.assert_same_bits(cut, sim.volume(frame, g), "shim vs python, float")
        assert np.array_equal(bytes_, sim.bmode_volume(frame, g))
    finally:
        sim.close()
    assert np.count_nonzero(cut) > 1000 and len(np.unique(bytes_)) > 20


def test_cli_sweep_options(mcrt, tmp_path):
    exe = os.path.join(ROOT, "mcray-tracing_amd", "mattausch_hip")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "mcray-tracing_amd"), "mattausch_hip"])
    cfg, scene = _write_scene(mcrt, tmp_path)
    K, step_deg, pivot = 5, 2.0, 10.0
    pgm = tmp_path / "cplane.pgm"
    r = subprocess.run([exe, scene, "2", "5", str(pgm), "--sweep", str(K), "--sweep-step-deg", repr(step_deg), "--sweep-pivot-mm", repr(pivot), "--cplane-mm", "80",
                        "--db", "50"], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = pgm.read_bytes()
    head = b"P5\n500 400\n255\n"
    assert raw.startswith(head) and len(raw) == len(head) + 200000
    tr = mcrt.Transducer(512, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    sim = mcrt.Simulator(mcrt.scene_io.load_scene_file(scene), tr, n_samples=5, sweep=(K, float(f32(step_deg * math.pi / 180.0))), sweep_pivot_mm=pivot)
    try:
        want = sim.bmode_volume(1, mcrt.cplane_grid(80.0, 500, 400, 0.25), dynamic_range_db=50.0)      # the last of the run's two frames
    finally:
        sim.close()
    assert np.array_equal(np.frombuffer(raw, np.uint8, 200000, len(head)).reshape(1, 400, 500), want)
    assert len(np.unique(want)) > 20 and (want == 0).any()                  # the sweep is a strip of the C-plane: black beside it
    for bad in (["--sweep", "3", "--sweep-step-deg", "2", "--cplane-mm", "80", "--compound", "3"], ["--sweep", "3", "--sweep-step-deg", "2", "--cplane-mm", "80", "--elevation", "3"],
                ["--sweep", "3", "--cplane-mm", "80"], ["--sweep", "3", "--sweep-step-deg", "2"], ["--sweep", "0", "--sweep-step-deg", "2", "--cplane-mm", "80"],
                ["--sweep", "3", "--sweep-step-deg", "2", "--cplane-mm", "80", "--sagittal-mm", "0"], ["--sweep", "3", "--sweep-step-deg", "90", "--cplane-mm", "80"],
                ["--cplane-mm", "80"]):
        r = subprocess.run([exe, scene, "1", "5"] + bad, capture_output=True, text=True, timeout=240)
        assert r.returncode == 1 and "--sweep" in r.stdout, (bad, r.stdout)
