"""Ground-truth label maps on the MI355X: mcrt_label_frames (k_label) against the numpy mirror (tests/label_mirror.py, on the CPU oracle's closest
hit) and, independently of the mirror, against the tracer's own first hits; mcrt_label_scan_convert_frames and mcrt_label_volume_frames
(k_label_gather) against the mirror fed with the product's own maps; the argument errors; the Simulator, the C++ shim, the CLI and a
two-rank group.  Every comparison is exact equality of integers."""
import ctypes as C
import json
import math
import os
import subprocess
import numpy as np
import pytest

import image_cases as ic
import label_mirror as lm
import volume_mirror as vm
from test_gpu_focus import Dev

pytestmark = pytest.mark.gpu

f32 = np.float32
INVALID, LIMIT = -1, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL_T, FILL_I, FILL_C = 0xEE, -7, 0xDEADBEEF
SWEEP_E = (1, 3, 64, 65, 130)          # one lane, a ragged wavefront, a full one, one more, three workgroups
SWEEP_R = (1, 2, 465, 2048)            # no row to speak of, the reference's 465 (no multiple of 4), the largest image
RULES = ((lm.TRACED, "traced", None), (lm.GEOMETRIC, "geometric", 1e-3))
_mirror_cache = {}


@pytest.fixture
def dev_of():
    made = []

    def make(ctx):
        made.append(Dev(ctx))
        return made[-1]
    yield make
    for d in made:
        if d.ctx.h:
            d.close()


def scene_of(mcrt, name):
    cfg, meshes = mcrt.synth.sphere_scene(2) if name == "sphere" else mcrt.synth.liver_scene(2)
    return cfg, mcrt.scene_io.build_scene(cfg, meshes)


def context(mcrt, sd, builder="sah", **params):
    c = mcrt.Context(0)
    c.set_bvh_builder(builder)
    if params:
        c.set_params(**params)
    c.upload_scene(sd)
    return c


def done(ctx, dev):
    """a test's own context: its buffers first"""
    dev.close(); dev.bufs = []
    ctx.close()


def label(ctx, dev, R, pos=None, dirs=None, rule="traced", offs=None, e0=0, e1=None, n_frames=None, want=(True, True, True)):
    """one mcrt_label_frames call into pre-filled buffers -> [tissue, interface, crossings] (None where not asked for)"""
    E = ctx.params.n_elements
    e1 = E if e1 is None else e1
    F = n_frames if n_frames is not None else (1 if pos is None else len(pos))
    ne = e1 - e0
    fills = (np.full((F, ne, R), FILL_T, np.uint8), np.full((F, ne, R), FILL_I, np.int32), np.full((F, ne), FILL_C, np.uint32))
    bufs = [dev.upload(a) if w else None for a, w in zip(fills, want)]
    ctx.label_frames(pos, dirs, rule=rule, start_offset=offs, e_begin=e0, e_end=e1, n_frames=n_frames, tissue_dev=bufs[0], interface_dev=bufs[1],
                     crossings_dev=bufs[2])
    ctx.synchronize()
    return [ctx.d2h(b, a.shape, a.dtype) if b else None for b, a in zip(bufs, fills)]


def mirror(orc, key, sd, pos, dirs, R, rule, offs):
    k = (key, R, rule, offs, np.asarray(pos).tobytes(), np.asarray(dirs).tobytes())
    if k not in _mirror_cache:
        _mirror_cache[k] = lm.label_frames(lm.oracle_scene(orc, sd), orc, pos, dirs, R, rule=rule, offs=0.1 if offs is None else offs)
    return _mirror_cache[k]


def same(got, want, what):
    for g, w, n in zip(got, want, ("tissue", "interface", "crossings")):
        if g is None:
            continue
        w = np.asarray(w).reshape(g.shape)
        assert np.array_equal(g, w), "%s: %s differs in %d places, first at %s" % (what, n, int((g != w).sum()), tuple(np.argwhere(g != w)[0]))


# ------------------------------------------------------------------ the label pass
@pytest.mark.parametrize("builder", ["sah", "lbvh"])
@pytest.mark.parametrize("name", ["sphere", "liver"])
def test_scene_and_shape_sweep(mcrt, orc, dev_of, name, builder):
    """both rules at every E x R, every element of every output; the outputs are pre-filled so that an unwritten element shows"""
    cfg, sd = scene_of(mcrt, name)
    ctx = context(mcrt, sd, builder)
    dev = dev_of(ctx)
    try:
        for E in SWEEP_E:
            tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
            for R in SWEEP_R:
                ctx.set_params(n_elements=E, n_rows=R)
                ctx.set_transducer(tr.pos, tr.dir)
                for rule, rname, offs in RULES:
                    want = mirror(orc, name, sd, tr.pos, tr.dir, R, rule, offs)
                    same(label(ctx, dev, R, rule=rname, offs=offs), want, "%s %s E %d R %d %s" % (name, builder, E, R, rname))
                    if (E, R) == (65, 465):                  # each output pointer null in turn: the others are what they were
                        for skip in range(3):
                            ask = tuple(i != skip for i in range(3))
                            same(label(ctx, dev, R, rule=rname, offs=offs, want=ask), want, "%s %s without output %d" % (name, rname, skip))
            dev.close(); dev.bufs = []
    finally:
        done(ctx, dev)


def test_subranges_and_poses(mcrt, orc, dev_of):
    cfg, sd = scene_of(mcrt, "liver")
    E, R = 65, 465
    ctx = context(mcrt, sd, n_elements=E, n_rows=R)
    dev = dev_of(ctx)
    try:
        tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
        ctx.set_transducer(tr.pos, tr.dir)
        full = label(ctx, dev, R)
        same(full, mirror(orc, "liver", sd, tr.pos, tr.dir, R, lm.TRACED, None), "full")
        for e0, e1 in ((0, 1), (3, 64), (64, 65), (10, 65)):
            same(label(ctx, dev, R, e0=e0, e1=e1), [full[0][:, e0:e1], full[1][:, e0:e1], full[2][:, e0:e1]], "scan-lines [%d,%d)" % (e0, e1))
        # a pose table of three frames -- two planes of a sweep and a steered view -- against three set_transducer calls
        sp, sdir = tr.swept(2, 0.05, 10.0)
        vp, vdir = tr.steered([0.1])
        pos = np.concatenate([sp, vp]); dirs = np.concatenate([sdir, vdir])
        for rule, rname, offs in RULES:
            singles = []
            for f in range(3):
                ctx.set_transducer(pos[f], dirs[f])
                singles.append(label(ctx, dev, R, rule=rname, offs=offs))
            want = [np.concatenate([s[i] for s in singles]) for i in range(3)]
            assert not np.array_equal(want[0][0], want[0][2])
            same(label(ctx, dev, R, pos, dirs, rule=rname, offs=offs), want, "host pose table, " + rname)
            same(label(ctx, dev, R, pos, dirs, rule=rname, offs=offs, e0=7, e1=40), [w[:, 7:40] for w in want], "host pose table, scan-lines [7,40)")
            same(label(ctx, dev, R, dev.upload(pos), dev.upload(dirs), rule=rname, offs=offs, n_frames=3), want, "device pose table, " + rname)
    finally:
        done(ctx, dev)


def test_tissue_pointer_of_any_alignment(mcrt, dev_of):
    """the tissue map is written as aligned 32-bit words with single bytes at the two ragged ends: a pointer 1, 2 or 3 bytes off a word gives
    the same map, and not a byte beside it is touched (one beam of one row up to three workgroups)"""
    cfg, sd = scene_of(mcrt, "liver")
    ctx = context(mcrt, sd)
    dev = dev_of(ctx)
    try:
        for E, R in ((1, 1), (1, 2), (3, 1), (3, 465), (65, 2), (130, 465)):
            tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
            ctx.set_params(n_elements=E, n_rows=R)
            ctx.set_transducer(tr.pos, tr.dir)
            want = label(ctx, dev, R, want=(True, False, False))[0]
            for skew in (1, 2, 3):
                buf = dev.upload(np.full(E * R + 8, FILL_T, np.uint8))
                ctx.label_frames(tissue_dev=buf + skew)
                ctx.synchronize()
                got = ctx.d2h(buf, (E * R + 8,), np.uint8)
                assert np.array_equal(got[skew:skew + E * R], want.reshape(-1)), (E, R, skew)
                assert (got[:skew] == FILL_T).all() and (got[skew + E * R:] == FILL_T).all(), (E, R, skew)
    finally:
        done(ctx, dev)


def test_a_probe_turned_away_sees_the_start_material(mcrt, dev_of):
    cfg, sd = scene_of(mcrt, "sphere")
    E, R = 65, 465
    ctx = context(mcrt, sd, n_elements=E, n_rows=R)
    dev = dev_of(ctx)
    try:
        tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
        ctx.set_transducer(tr.pos, -tr.dir)
        for _, rname, offs in RULES:
            t, i, c = label(ctx, dev, R, rule=rname, offs=offs)
            assert (t == sd.start_mat).all() and (i == -1).all() and (c == 0).all()
    finally:
        done(ctx, dev)


def test_crossing_cap(mcrt, orc, dev_of):
    """70 sheets 2 mm apart (dealt in turn to two meshes): 64 boundaries and bit 31, the rows behind the 64th sheet hold the medium reached
    there; 60 sheets: bit 31 clear"""
    R = 465
    pos, dirs = lm.fan(3, 0.05)
    for n in (70, 60):
        xs = [1.0 + 0.2 * i for i in range(n)]
        sd = lm.sheets_scene(mcrt, xs)
        ctx = context(mcrt, sd, n_elements=3, n_rows=R)
        dev = dev_of(ctx)
        try:
            ctx.set_transducer(pos, dirs)
            for rule, rname, offs in RULES:
                got = label(ctx, dev, R, rule=rname, offs=offs)
                same(got, mirror(orc, "sheets%d" % n, sd, pos, dirs, R, rule, offs), "%d sheets, %s" % (n, rname))
                t, i, c = (g[0] for g in got)
                if n == 70:
                    assert (c == (64 | lm.CAPPED)).all()
                    last = int(np.flatnonzero(i[1] >= 0)[-1])                 # the 64th sheet's row on the central beam
                    # (sheet 63 is mesh 1's; behind it TRACED carries that mesh's material, GEOMETRIC has left both meshes 16 times each)
                    assert abs(last - xs[63] * 10 / 0.322) <= 1 and i[1][last] == 1
                    assert (t[1][last:] == (sd.meshes[1][0] if rule == lm.TRACED else sd.start_mat)).all()
                else:
                    assert (c == 60).all()
        finally:
            done(ctx, dev)


def test_thin_layers_and_the_start_offset(mcrt, orc, dev_of):
    """two sheets 0.1 mm apart: with a 1e-3 offset both are met in ONE row -- one interface row, the shallower sheet's, and no tissue row of the
    layer between them; with the tracer's 0.1 the beam restarts behind the second sheet and never meets it"""
    R = 465
    sd = lm.sheets_scene(mcrt, [5.0, 5.01])
    LIVER, FAT, GEL = (sd.material_names.index(n) for n in ("LIVER", "FAT", "GEL"))
    pos, dirs = lm.fan(1, 0.0)
    ctx = context(mcrt, sd, n_elements=1, n_rows=R)
    dev = dev_of(ctx)
    try:
        ctx.set_transducer(pos, dirs)
        for rule, rname, _ in RULES:
            fine = label(ctx, dev, R, rule=rname, offs=1e-3)
            coarse = label(ctx, dev, R, rule=rname, offs=0.1)
            same(fine, mirror(orc, "thin", sd, pos, dirs, R, rule, 1e-3), "offset 1e-3, " + rname)
            same(coarse, mirror(orc, "thin", sd, pos, dirs, R, rule, 0.1), "offset 0.1, " + rname)
            t, i, c = (g[0][0] for g in fine)
            row = int(5.0 * 10 / 0.322)
            assert c == 2 and np.flatnonzero(i >= 0).tolist() == [row] and i[row] == 0
            assert (t[:row] == GEL).all() and (t[row:] == FAT).all() and LIVER not in t
            t, i, c = (g[0][0] for g in coarse)
            assert c == 1 and np.flatnonzero(i >= 0).tolist() == [row] and (t[row:] == LIVER).all()
    finally:
        done(ctx, dev)


def test_geometric_stack_overflow(mcrt, orc, dev_of):
    """17 nested boxes: the 17th does not fit the stack of 16 -- dropped, bit 31 set, the walk goes on"""
    R = 465
    sd = lm.boxes_scene(mcrt, 17)
    pos, dirs = lm.fan(3, 0.02, dz=0.013)
    ctx = context(mcrt, sd, n_elements=3, n_rows=R)
    dev = dev_of(ctx)
    try:
        ctx.set_transducer(pos, dirs)
        got = label(ctx, dev, R, rule="geometric", offs=1e-3)
        same(got, mirror(orc, "boxes17", sd, pos, dirs, R, lm.GEOMETRIC, 1e-3), "17 boxes")
        assert (got[2] == (34 | lm.CAPPED)).all()
        got = label(ctx, dev, R, rule="traced", offs=1e-3)
        assert (got[2] == 34).all()
    finally:
        done(ctx, dev)
    sd = lm.boxes_scene(mcrt, 16)
    ctx = context(mcrt, sd, n_elements=3, n_rows=R)
    dev = dev_of(ctx)
    try:
        ctx.set_transducer(pos, dirs)
        got = label(ctx, dev, R, rule="geometric", offs=1e-3)
        assert (got[2] == 32).all() and (got[0][:, :, -1] == sd.start_mat).all()
    finally:
        done(ctx, dev)


def test_first_interface_is_the_tracers_first_hit(mcrt, dev_of):
    """independent of the mirror: bounce 0 of every sample path is the central beam, so the mesh of mcrt_cast_rays' first hit is the first
    interface the label pass reports, and a path that hits nothing is a scan-line without crossings"""
    cfg, sd = scene_of(mcrt, "liver")
    E, R, S = 64, 465, 2
    ctx = context(mcrt, sd, n_elements=E, n_rows=R, n_samples=S, tex_n=32)
    dev = dev_of(ctx)
    try:
        ctx.upload_texture(mcrt.host_texture(32), 32)
        tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
        ctx.set_transducer(tr.pos, tr.dir)
        _, _, hits = ctx.cast_rays(0)
        t, i, c = (g[0] for g in label(ctx, dev, R))
        assert (hits[:, 0, 0] == hits[:, 1, 0]).all()
        n_hit = 0
        for e in range(E):
            tri = int(hits[e, 0, 0])
            if tri < 0:
                assert c[e] == 0, e
                continue
            n_hit += 1
            assert c[e] >= 1 and int(i[e][np.flatnonzero(i[e] >= 0)[0]]) == int(sd.tri_mesh[tri]), e
        assert n_hit >= E // 2
    finally:
        done(ctx, dev)


# ------------------------------------------------------------------ labels as pictures
@pytest.fixture(scope="module")
def ctx(mcrt):
    c = mcrt.Context(0)
    yield c
    c.close()


def tissue_maps(F, K, E, R, seed):
    return np.random.default_rng(seed).integers(0, 200, (F, K, E, R)).astype(np.uint8)


@pytest.mark.parametrize("gi", range(len(ic.SCAN_GEOMETRIES)))
def test_scan_converted_labels_match_the_mirror(mcrt, ctx, dev_of, gi):
    """every pixel, pre-filled; alternating with the float call leaves its picture as it was (the same maps serve both)"""
    radius, angle, rows, cols = ic.SCAN_GEOMETRIES[gi]
    dev = dev_of(ctx)
    for si, (E, R) in enumerate(ic.SCAN_SHAPES):
        F = 1 + (gi + si) % 3
        t = tissue_maps(F, 1, E, R, gi * 10 + si)[:, 0]
        mr, mc = mcrt.host_scan_maps(E, R, radius, angle, 100, 1500, rows, cols)
        want = np.stack([lm.scan_convert(t[f], mr, mc) for f in range(F)])
        rf = np.stack([ic.scan_image(E, R, seed=f) for f in range(F)])
        p_rf = dev.upload(rf); p_t = dev.upload(t); q = dev.upload(np.full((F, rows, cols), 7, np.uint8)); qf = dev(F * rows * cols * 4)
        ctx.scan_convert_frames(p_rf, F, E, R, qf, radius, angle, rows, cols)
        before = ctx.d2h(qf, (F, rows, cols))
        ctx.label_scan_convert_frames(p_t, F, E, R, q, radius, angle, rows, cols)
        got = ctx.d2h(q, (F, rows, cols), np.uint8)
        assert np.array_equal(got, want), (gi, E, R, int((got != want).sum()))
        assert (got == lm.NONE).any() and (rows * cols == 1 or (got != lm.NONE).any())
        ctx.scan_convert_frames(p_rf, F, E, R, qf, radius, angle, rows, cols)
        ic.assert_same_bits(ctx.d2h(qf, (F, rows, cols)), before, "the float picture after its labels")
        dev.close(); dev.bufs = []


def cuts_and_blocks(mcrt, E, R, K, pivot):
    """the grids of the float tests, and a C-plane and a sagittal cut that reach beyond the sweep (points outside it: MCRT_LABEL_NONE)"""
    gs = [vm.grid_for(mcrt, w, E, R, K, pivot) for w in vm.GRID_SHAPES]
    return gs + [mcrt.cplane_grid(90.0, 61, 35, 1.5), mcrt.sagittal_grid(2.0, 37, 50, 3.0, 25.0)]


@pytest.mark.parametrize("si", range(len(ic.SCAN_SHAPES)))
def test_volume_labels_match_the_mirror(mcrt, ctx, dev_of, si):
    E, R = ic.SCAN_SHAPES[si]
    dev = dev_of(ctx)
    for K, F, pivot in ((1, 2, 0.0), (2, 1, 10.0), (8, 3, -20.0)):
        sweep = (K, vm.STEP, pivot)
        t = tissue_maps(F, K, E, R, 100 + si + K)
        p_t = dev.upload(t)
        p_rf = dev.upload(np.stack([np.stack([ic.scan_image(E, R, seed=k + f) for k in range(K)]) for f in range(F)]))
        for g in cuts_and_blocks(mcrt, E, R, K, pivot):
            shape = (F, g.nw, g.nv, g.nu)
            maps = mcrt.host_volume_maps(E, R, sweep, g)
            want = np.stack([lm.volume(t[f], maps) for f in range(F)])
            q = dev.upload(np.full(shape, 7, np.uint8)); qf = dev(int(np.prod(shape)) * 4)
            ctx.volume_frames(p_rf, F, E, R, sweep, g, qf)
            before = ctx.d2h(qf, shape)
            ctx.label_volume_frames(p_t, F, E, R, sweep, g, q)
            got = ctx.d2h(q, shape, np.uint8)
            assert np.array_equal(got, want), (E, R, K, shape, int((got != want).sum()))
            ctx.volume_frames(p_rf, F, E, R, sweep, g, qf)
            ic.assert_same_bits(ctx.d2h(qf, shape), before, "the float volume after its labels")
        dev.close(); dev.bufs = []
    g = mcrt.cplane_grid(90.0, 61, 35, 1.5)
    maps = mcrt.host_volume_maps(E, R, (8, vm.STEP, -20.0), g)
    assert (lm.volume(tissue_maps(1, 8, E, R, 0)[0], maps) == lm.NONE).any()        # (the cut does reach beyond the sweep)


def test_nan_maps_give_no_data(mcrt, ctx, dev_of):
    """a radius that is not finite passes the float calls' checks and fills the cached maps with NaN (or puts every point outside): every
    label is MCRT_LABEL_NONE, every element is written, and the float picture through the same maps is what it was before"""
    dev = dev_of(ctx)
    E, R, F = 8, 16, 2
    t = tissue_maps(F, 2, E, R, 5)
    p_t = dev.upload(t); p_rf = dev.upload(np.stack([ic.scan_image(2 * E, R, seed=f) for f in range(F)]))
    saw_nan = {"scan": False, "volume": False}
    for radius in (float("nan"), float("inf")):
        for rows, cols in ((12, 20), (11, 21), (40, 64)):            # words, single bytes, more than one wavefront
            mr, mc = mcrt.host_scan_maps(E, R, radius, vm.DEFAULT_ANGLE, 100, 1500, rows, cols)
            saw_nan["scan"] |= bool(np.isnan(mr).all() and np.isnan(mc).all())
            q = dev.upload(np.full((F, rows, cols), 7, np.uint8)); qf = dev(F * rows * cols * 4)
            ctx.scan_convert_frames(p_rf, F, E, R, qf, radius, vm.DEFAULT_ANGLE, rows, cols)
            before = ctx.d2h(qf, (F, rows, cols))
            ctx.label_scan_convert_frames(p_t, F, E, R, q, radius, vm.DEFAULT_ANGLE, rows, cols)
            got = ctx.d2h(q, (F, rows, cols), np.uint8)
            assert (got == lm.NONE).all() and np.array_equal(got, np.stack([lm.scan_convert(t[f, 0], mr, mc) for f in range(F)])), (radius, rows, cols)
            ctx.scan_convert_frames(p_rf, F, E, R, qf, radius, vm.DEFAULT_ANGLE, rows, cols)
            ic.assert_same_bits(ctx.d2h(qf, (F, rows, cols)), before, "the float picture after its labels, radius %r" % radius)
            sweep = (2, vm.STEP, 0.0); g = mcrt.cplane_grid(80.0, cols, rows, 1.0)
            maps = mcrt.host_volume_maps(E, R, sweep, g, radius)
            saw_nan["volume"] |= bool(np.isnan(maps[1]).all())
            ctx.h2d(q, np.full((F, rows, cols), 7, np.uint8))
            ctx.volume_frames(p_rf, F, E, R, sweep, g, qf, radius)
            before = ctx.d2h(qf, (F, rows, cols))
            ctx.label_volume_frames(p_t, F, E, R, sweep, g, q, radius)
            got = ctx.d2h(q, (F, rows, cols), np.uint8)
            assert (got == lm.NONE).all() and np.array_equal(got, np.stack([lm.volume(t[f], maps) for f in range(F)]).reshape(got.shape)), (radius, rows, cols)
            ctx.volume_frames(p_rf, F, E, R, sweep, g, qf, radius)
            ic.assert_same_bits(ctx.d2h(qf, (F, rows, cols)), before, "the float volume after its labels, radius %r" % radius)
    assert saw_nan["scan"] and saw_nan["volume"]


# ------------------------------------------------------------------ errors
def _rc(mcrt, fn, *args):
    rc = fn(*args)
    return rc, mcrt.load_library().mcrt_last_error().decode()


def test_label_frames_errors_leave_the_outputs_untouched(mcrt, dev_of):
    L = mcrt.load_library()
    from mcray_tracing_amd import LabelOpts
    from mcray_tracing_amd._lib import ptr
    cfg, sd = scene_of(mcrt, "sphere")
    E, R = 8, 64
    tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    bare = mcrt.Context(0)
    ctx = context(mcrt, sd, n_elements=E, n_rows=R)
    dev = dev_of(ctx)
    try:
        fills = (np.full((3, E, R), FILL_T, np.uint8), np.full((3, E, R), FILL_I, np.int32), np.full((3, E), FILL_C, np.uint32))
        bufs = [dev.upload(a) for a in fills]
        pos3 = np.stack([tr.pos] * 3); dir3 = np.stack([tr.dir] * 3)

        def call(c, F=1, e0=0, e1=E, pos=None, dirs=None, opts=None, outs=(0, 1, 2)):
            o = [C.c_void_p(bufs[i]) if i in outs else None for i in range(3)]
            return _rc(mcrt, L.mcrt_label_frames, c.h if c is not None else None, F, e0, e1, ptr(pos), ptr(dirs), C.byref(opts) if opts is not None else None, *o)

        assert call(None)[0] == INVALID
        rc, msg = call(bare); assert rc == INVALID and "no scene" in msg
        rc, msg = call(ctx); assert rc == INVALID and "no transducer" in msg
        ctx.set_transducer(tr.pos, tr.dir)
        assert call(ctx)[0] == 0
        ctx.synchronize()
        for b, a in zip(bufs, fills):
            ctx.h2d(b, a)
        for kw in (dict(e0=3, e1=3), dict(e0=5, e1=4), dict(e1=E + 1), dict(pos=pos3, F=3), dict(dirs=dir3, F=3), dict(outs=()), dict(F=2), dict(F=0),
                   dict(opts=LabelOpts(2, -1.0)), dict(opts=LabelOpts(0, float("nan"))), dict(opts=LabelOpts(0, float("inf"))), dict(opts=LabelOpts(1, 0.0))):
            rc, msg = call(ctx, **kw)
            assert rc == INVALID and msg.startswith("mcrt_label_frames"), (kw, rc, msg)
        big = np.zeros((1025, E, 3), f32)
        rc, msg = call(ctx, F=1025, pos=big, dirs=big); assert rc == LIMIT and "1024" in msg
        ctx.synchronize()
        for b, a in zip(bufs, fills):
            assert np.array_equal(ctx.d2h(b, a.shape, a.dtype), a)
        # 255 materials: MCRT_LABEL_NONE would be one of them
        many = mcrt.scene_io.SceneData(sd.tri, sd.tri_mesh, sd.meshes, np.resize(sd.materials, (255, 8)), ["m%d" % i for i in range(255)], sd.start_mat, sd.spacing, cfg)
        ctx.upload_scene(many)
        rc, msg = call(ctx); assert rc == LIMIT and "254" in msg
        ctx.upload_scene(mcrt.scene_io.SceneData(sd.tri, sd.tri_mesh, sd.meshes, np.resize(sd.materials, (254, 8)), ["m%d" % i for i in range(254)], sd.start_mat, sd.spacing, cfg))
        assert call(ctx)[0] == 0
        ctx.synchronize()
    finally:
        done(ctx, dev); bare.close()


def test_gather_errors_leave_the_output_untouched(mcrt, ctx, dev_of):
    L = mcrt.load_library()
    dev = dev_of(ctx)
    E, R, rows, cols = 8, 16, 12, 20
    t = dev.upload(tissue_maps(2, 2, E, R, 1)); fill = np.full((2, rows, cols), 9, np.uint8); q = dev.upload(fill)
    vp = C.c_void_p
    a, ang = 30.0, vm.DEFAULT_ANGLE
    sc = L.mcrt_label_scan_convert_frames
    for args in ((None, 1, E, R, a, ang, vp(q), rows, cols), (vp(t), 1, E, R, a, ang, None, rows, cols), (vp(t), 0, E, R, a, ang, vp(q), rows, cols),
                 (vp(t), 1, 0, R, a, ang, vp(q), rows, cols), (vp(t), 1, E, 0, a, ang, vp(q), rows, cols), (vp(t), 1, E, R, a, ang, vp(q), 0, cols),
                 (vp(t), 1, E, R, a, ang, vp(t), 2, 2)):
        assert _rc(mcrt, sc, ctx.h, *args)[0] == INVALID, args
    assert _rc(mcrt, sc, ctx.h, vp(t), 65536, E, R, a, ang, vp(q), rows, cols)[0] == LIMIT
    assert _rc(mcrt, sc, None, vp(t), 1, E, R, a, ang, vp(q), rows, cols)[0] == INVALID
    sw = mcrt.sweep_struct(2, 0.05, 0.0); g = mcrt.cplane_grid(80.0, cols, rows, 1.0)
    bad_sw = mcrt.sweep_struct(0, 0.05, 0.0); bad_g = mcrt.cplane_grid(80.0, cols, 0, 1.0)
    vol = L.mcrt_label_volume_frames
    for args in ((None, 1, E, R, a, ang, C.byref(sw), C.byref(g), vp(q)), (vp(t), 1, E, R, a, ang, C.byref(sw), C.byref(g), None),
                 (vp(t), 0, E, R, a, ang, C.byref(sw), C.byref(g), vp(q)), (vp(t), 1, E, R, a, 0.0, C.byref(sw), C.byref(g), vp(q)),
                 (vp(t), 1, E, R, a, ang, None, C.byref(g), vp(q)), (vp(t), 1, E, R, a, ang, C.byref(sw), None, vp(q)),
                 (vp(t), 1, E, R, a, ang, C.byref(bad_sw), C.byref(g), vp(q)), (vp(t), 1, E, R, a, ang, C.byref(sw), C.byref(bad_g), vp(q)),
                 (vp(t), 1, E, R, a, ang, C.byref(sw), C.byref(g), vp(t))):
        assert _rc(mcrt, vol, ctx.h, *args)[0] == INVALID, args
    assert _rc(mcrt, vol, ctx.h, vp(t), 1, E, 2049, a, ang, C.byref(sw), C.byref(g), vp(q))[0] == LIMIT
    assert _rc(mcrt, vol, ctx.h, vp(t), 32768, E, R, a, ang, C.byref(sw), C.byref(g), vp(q))[0] == LIMIT
    ctx.synchronize()
    assert np.array_equal(ctx.d2h(q, fill.shape, np.uint8), fill)


# ------------------------------------------------------------------ the layers above
def _write_scene(mcrt, tmp_path):
    cfg, meshes = mcrt.synth.sphere_scene(3)
    cfg["workingDirectory"] = str(tmp_path) + "/"
    for f, (V, F) in meshes.items():
        mcrt.scene_io.save_obj(str(tmp_path / f), V, F)
    (tmp_path / "sphere.scene").write_text(json.dumps(cfg))
    return cfg, str(tmp_path / "sphere.scene")


def _sim(mcrt, sd, tr, **kw):
    return mcrt.Simulator(sd, tr, n_samples=2, texture=mcrt.host_texture(32), tex_n=32, **kw)


def test_simulator_labels(mcrt, orc):
    """labels() is the unsteered probe's own plane under compound= and elevation=, the K planes under sweep=; the picture is the mirror's"""
    cfg, sd = scene_of(mcrt, "liver")
    E = 64
    tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    sim = _sim(mcrt, sd, tr)
    try:
        R = sim.R
        plain = sim.labels()
        geo = sim.labels(rule="geometric", start_offset=1e-3, picture=False)
    finally:
        sim.close()
    want = mirror(orc, "liver", sd, tr.pos, tr.dir, R, lm.TRACED, None)
    same([plain["tissue"], plain["interface"], plain["crossings"]], want, "Simulator.labels")
    same([geo["tissue"], geo["interface"], geo["crossings"]], mirror(orc, "liver", sd, tr.pos, tr.dir, R, lm.GEOMETRIC, 1e-3), "Simulator.labels geometric")
    assert geo["picture"] is None and not np.array_equal(geo["tissue"], plain["tissue"])
    mr, mc = mcrt.host_scan_maps(E, R, 30.0, vm.DEFAULT_ANGLE, 100, 1500, 400, 500)
    assert np.array_equal(plain["picture"], lm.scan_convert(plain["tissue"], mr, mc))
    assert len(np.unique(plain["picture"])) >= 5 and (plain["picture"] == lm.NONE).any()
    for kw in (dict(compound=(-0.1, 0.0, 0.1)), dict(elevation=True), dict(compound=(-0.1, 0.1), elevation=True)):
        sim = _sim(mcrt, sd, tr, **kw)
        try:
            got = sim.labels()
        finally:
            sim.close()
        for k in ("tissue", "interface", "crossings", "picture"):
            assert np.array_equal(got[k], plain[k]), (kw, k)
    K, step, pivot = 3, 0.05, 10.0
    sim = _sim(mcrt, sd, tr, sweep=(K, step), sweep_pivot_mm=pivot)
    try:
        got = sim.labels()
        g = mcrt.cplane_grid(80.0, 96, 40, 0.5)
        cut = sim.label_volume(g)
    finally:
        sim.close()
    pos, dirs = tr.swept(K, step, pivot)
    same([got["tissue"], got["interface"], got["crossings"]], mirror(orc, "liver", sd, pos, dirs, R, lm.TRACED, None), "Simulator.labels, sweep")
    assert got["picture"] is None and got["tissue"].shape == (K, E, R)
    assert np.array_equal(cut, lm.volume(got["tissue"], mcrt.host_volume_maps(E, R, (K, step, pivot), g)))
    assert np.array_equal(got["tissue"][1], plain["tissue"])          # (the middle plane of an odd sweep is the probe's own)


def test_host_shim(mcrt, tmp_path):
    """rf_image::labels / label_picture / label_volume write what Python's Simulator produces -- on one context, on a two-rank group sharing
    the GPU (the pass runs on rank 0's context), and after a swept trace"""
    pkg = os.path.join(ROOT, "mcray-tracing_amd")
    exe = str(tmp_path / "label_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(pkg, "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "label_driver.cpp"), "-L", pkg, "-lmcrt_hip", "-Wl,-rpath," + pkg])
    cfg, scene = _write_scene(mcrt, tmp_path)
    sd = mcrt.scene_io.load_scene_file(scene)
    E, R = 64, 465
    tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    K, step, pivot, depth, nu, nv, pitch = 4, 0.05, 10.0, 160.0, 96, 40, 1.5      # (a cut wide enough to leave the sphere, the box and the sweep)

    def run(devices, rule, offs, sweep):
        out = tmp_path / "labels.bin"
        args = [exe, scene, str(out), devices, str(rule), repr(offs)] + ([str(K), repr(step), repr(pivot), repr(depth), str(nu), str(nv), repr(pitch)] if sweep else [])
        r = subprocess.run(args, capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout + r.stderr
        raw = out.read_bytes()
        P = K if sweep else 1
        n = P * E * R
        npic = nu * nv if sweep else 200000
        assert len(raw) == 5 * n + 4 * P * E + npic
        return (np.frombuffer(raw, np.uint8, n).reshape(P, E, R), np.frombuffer(raw, np.int32, n, n).reshape(P, E, R),
                np.frombuffer(raw, np.uint32, P * E, 5 * n).reshape(P, E), np.frombuffer(raw, np.uint8, npic, 5 * n + 4 * P * E))

    sim = _sim(mcrt, sd, tr)
    try:
        want = {0: sim.labels(), 1: sim.labels(rule="geometric", start_offset=1e-3)}
    finally:
        sim.close()
    for devices, rule, offs in (("0", 0, -1.0), ("0", 1, 1e-3), ("0,0", 0, -1.0)):
        t, i, c, pic = run(devices, rule, offs, False)
        w = want[rule]
        assert np.array_equal(t[0], w["tissue"]) and np.array_equal(i[0], w["interface"]) and np.array_equal(c[0], w["crossings"]), (devices, rule)
        assert np.array_equal(pic.reshape(400, 500), w["picture"]), (devices, rule)
    assert len(np.unique(want[0]["picture"])) >= 3
    sim = _sim(mcrt, sd, tr, sweep=(K, step), sweep_pivot_mm=pivot)
    try:
        w = sim.labels()
        cut = sim.label_volume(mcrt.cplane_grid(depth, nu, nv, pitch))
    finally:
        sim.close()
    t, i, c, pic = run("0", 0, -1.0, True)
    assert np.array_equal(t, w["tissue"]) and np.array_equal(i, w["interface"]) and np.array_equal(c, w["crossings"])
    assert np.array_equal(pic.reshape(1, nv, nu), cut) and len(np.unique(cut)) >= 2


def test_cli_labels(mcrt, tmp_path):
    """--labels writes the API's bytes: the sector's tissue map, and with --sweep the cut's"""
    exe = os.path.join(ROOT, "mcray-tracing_amd", "mattausch_hip")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "mcray-tracing_amd"), "mattausch_hip"])
    cfg, scene = _write_scene(mcrt, tmp_path)
    sd = mcrt.scene_io.load_scene_file(scene)
    tr = mcrt.Transducer(512, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    head = b"P5\n500 400\n255\n"
    pgm = tmp_path / "labels.pgm"
    r = subprocess.run([exe, scene, "1", "1", "--labels", str(pgm), "--label-rule", "geometric", "--label-offset", "0.001"], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = pgm.read_bytes()
    assert raw.startswith(head) and len(raw) == len(head) + 200000
    sim = _sim(mcrt, sd, tr)                      # (labels depend on neither samples nor texture: the small texture is quicker to make)
    try:
        want = sim.labels(rule="geometric", start_offset=float(f32(0.001)))["picture"]
    finally:
        sim.close()
    assert raw[len(head):] == want.tobytes() and len(np.unique(want)) >= 3
    K, step_deg, pivot = 3, 2.0, 10.0
    r = subprocess.run([exe, scene, "1", "1", "--labels", str(pgm), "--sweep", str(K), "--sweep-step-deg", repr(step_deg), "--sweep-pivot-mm", repr(pivot),
                        "--cplane-mm", "160"], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = pgm.read_bytes()
    assert raw.startswith(head) and len(raw) == len(head) + 200000
    sim = _sim(mcrt, sd, tr, sweep=(K, float(f32(step_deg * math.pi / 180.0))), sweep_pivot_mm=pivot)
    try:
        want = sim.label_volume(mcrt.cplane_grid(160.0, 500, 400, 0.25))
    finally:
        sim.close()
    assert raw[len(head):] == want.tobytes() and len(np.unique(want)) >= 2


def test_two_rank_group_labels_from_member_0(mcrt, orc, dev_of):
    """there is no group call: the root has no scene.  Rank 0's context shares the root's GPU and holds the scene and the whole transducer: it
    labels into the root's memory, is synchronised, and the root scan-converts"""
    cfg, sd = scene_of(mcrt, "liver")
    E, R = 64, 465
    tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    grp = mcrt.Group([0, 0])
    try:
        grp.set_params(n_elements=E, n_rows=R, n_samples=2, tex_n=32)
        grp.upload_scene(sd); grp.upload_texture(mcrt.host_texture(32), 32); grp.set_transducer(tr.pos, tr.dir)
        root, member = grp.root, grp.members[0]
        dev = dev_of(root)
        with pytest.raises(mcrt.McrtError) as e:
            root.label_frames(tissue_dev=dev(E * R))
        assert e.value.code == INVALID and "no scene" in str(e.value)
        rf = dev(E * R * 4)
        grp.trace_frames(0, 1, rf)
        t_dev, i_dev, c_dev = dev.upload(np.full((E, R), FILL_T, np.uint8)), dev.upload(np.full((E, R), FILL_I, np.int32)), dev.upload(np.full(E, FILL_C, np.uint32))
        member.label_frames(tissue_dev=t_dev, interface_dev=i_dev, crossings_dev=c_dev)
        member.synchronize()
        pic = dev(200000)
        root.label_scan_convert_frames(t_dev, 1, E, R, pic)
        got = [root.d2h(t_dev, (1, E, R), np.uint8), root.d2h(i_dev, (1, E, R), np.int32), root.d2h(c_dev, (1, E), np.uint32)]
        same(got, mirror(orc, "liver", sd, tr.pos, tr.dir, R, lm.TRACED, None), "group member 0")
        mr, mc = mcrt.host_scan_maps(E, R, 30.0, vm.DEFAULT_ANGLE, 100, 1500, 400, 500)
        assert np.array_equal(root.d2h(pic, (400, 500), np.uint8), lm.scan_convert(got[0][0], mr, mc))
        grp.synchronize()
    finally:
        grp.close()
