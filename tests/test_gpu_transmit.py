"""Acoustic ground truth on the MI355X: mcrt_transmit_frames (k_transmit) against the numpy mirror (tests/transmit_mirror.py, on the CPU
oracle's closest hit) bit for bit -- transmit, reflect and crossings, at the workgroup's and the store's edges --, against the shipped label
product, through the Simulator's gathers, the argument errors, the C++ shim and the CLI.  Every comparison is exact: floats by their bits."""
import ctypes as C
import json
import os
import subprocess
import numpy as np
import pytest

import label_mirror as lm
import transmit_mirror as tm
from test_gpu_focus import Dev

pytestmark = pytest.mark.gpu

f32 = np.float32
INVALID, LIMIT = -1, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64                               # floats behind every output that must stay as they were
FILL_F, FILL_C = f32(-77.25), 0xDEADBEEF
RULES = {"traced": (lm.TRACED, None), "geometric": (lm.GEOMETRIC, 1e-3)}      # rule -> (the mirror's, the start offset: the tracer's 0.1 and a fine one)
MODES = {"total": tm.TOTAL, "boundaries": tm.BOUNDARIES}
COMBOS = [(m, r) for m in MODES for r in RULES]
N_FAN = 130
RULE_OFFSET = object()                   # "the start offset that goes with the rule"
_cache = {}


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


@pytest.fixture(scope="module")
def spheres(mcrt, orc):
    """LIVER around BONE (tests/label_mirror.py) at subdivision 3, and the beams of all the tests: 130 of them over +-0.35 rad, from grazing the
    liver to the middle of the bone, lifted out of the symmetry plane"""
    sd = lm.spheres_scene(mcrt, 3)
    pos, dirs = lm.fan(N_FAN, 0.35, dz=0.01)
    return {"sd": sd, "osc": lm.oracle_scene(orc, sd), "pos": pos, "dirs": dirs}


def context(mcrt, sd, **params):
    c = mcrt.Context(0)
    c.set_bvh_builder("sah")
    if params:
        c.set_params(**params)
    c.upload_scene(sd)
    return c


def done(ctx, dev):
    dev.close(); dev.bufs = []
    ctx.close()


def mirror(orc, key, osc, pos, dirs, R, mode, rule, offs=RULE_OFFSET):
    """the mirror of a (scene, beams, R, mode, rule), computed once"""
    offs = RULES[rule][1] if offs is RULE_OFFSET else offs
    k = (key, R, mode, rule, offs, np.asarray(pos).tobytes(), np.asarray(dirs).tobytes())
    if k not in _cache:
        _cache[k] = tm.transmit_frames(osc, orc, pos, dirs, R, mode=MODES[mode], rule=RULES[rule][0], offs=0.1 if offs is None else offs)
    return _cache[k]


def transmit(ctx, dev, R, pos=None, dirs=None, mode="total", rule="traced", e0=0, e1=None, n_frames=None, want=(True, True, True), skew=0,
             offs=RULE_OFFSET):
    """one mcrt_transmit_frames call into pre-filled buffers with GUARD floats behind (and `skew` floats before) each -> [transmit, reflect,
    crossings] (None where not asked for); the guards are checked here"""
    E = ctx.params.n_elements
    e1 = E if e1 is None else e1
    F = n_frames if n_frames is not None else (1 if pos is None else len(pos))
    ne = e1 - e0
    shapes = ((F, ne, R), (F, ne, R), (F, ne))
    fills = [np.full(skew + int(np.prod(s)) + GUARD, FILL_F if i < 2 else FILL_C, f32 if i < 2 else np.uint32) for i, s in enumerate(shapes)]
    bufs = [dev.upload(a) if w else None for a, w in zip(fills, want)]
    ptrs = [b + 4 * skew if b else None for b in bufs]
    ctx.transmit_frames(pos, dirs, mode=mode, rule=rule, start_offset=RULES[rule][1] if offs is RULE_OFFSET else offs, e_begin=e0, e_end=e1, n_frames=n_frames, transmit_dev=ptrs[0],
                        reflect_dev=ptrs[1], crossings_dev=ptrs[2])
    ctx.synchronize()
    out = []
    for b, a, s in zip(bufs, fills, shapes):
        if not b:
            out.append(None)
            continue
        got = ctx.d2h(b, a.shape, a.dtype)
        n = int(np.prod(s))
        assert np.array_equal(got[:skew].view(np.uint32), a[:skew].view(np.uint32)), "floats before the output were written"
        assert np.array_equal(got[skew + n:].view(np.uint32), a[skew + n:].view(np.uint32)), "guard floats behind the output were written"
        out.append(got[skew:skew + n].reshape(s))
    return out


def same(got, want, what):
    for g, w, n in zip(got, want, ("transmit", "reflect", "crossings")):
        if g is None:
            continue
        if n == "crossings":
            w = np.asarray(w).reshape(g.shape)
            assert np.array_equal(g, w), "%s: crossings differ in %d places, first at %s" % (what, int((g != w).sum()), tuple(np.argwhere(g != w)[0]))
        else:
            tm.same_bits(g, w, what + ": " + n)


# ------------------------------------------------------------------ the pass against the mirror
@pytest.mark.parametrize("E", [1, 63, 64, 65, 130])
def test_beams_per_pass(mcrt, orc, dev_of, spheres, E):
    """the wavefront's and the workgroup's ends: one lane, one short of a wavefront, a full one, one more, three workgroups; both modes x both rules"""
    R = 465
    pos, dirs = spheres["pos"][:E], spheres["dirs"][:E]
    ctx = context(mcrt, spheres["sd"], n_elements=E, n_rows=R)
    dev = dev_of(ctx)
    try:
        for mode, rule in COMBOS:
            full = mirror(orc, "spheres", spheres["osc"], spheres["pos"], spheres["dirs"], R, mode, rule)
            got = transmit(ctx, dev, R, pos[None], dirs[None], mode=mode, rule=rule)
            same(got, [w[None, :E] for w in full], "E %d %s %s" % (E, mode, rule))
            if E == 130 and mode == "total":          # the beams do what the scene says: a shadow, total reflections, beams that miss
                T, Rf, c = got[0][0], got[1][0], got[2][0]
                assert (T[:, 0] == 1.0).all() and (np.diff(T.astype(np.float64), axis=1) <= 0).all()
                assert 0 < T[N_FAN // 2, -1] < 1e-3 * T.max(axis=0)[-1] and (T[:, -1] == 0).any() and (Rf == 1.0).any() and (c >= 4).any()
    finally:
        done(ctx, dev)


@pytest.mark.parametrize("R", [5, 64, 465, 2048])
def test_rows(mcrt, orc, dev_of, spheres, R):
    """ragged 16-byte stores (R = 5, 465: a quad spans two scan-lines), whole ones (64) and the row limit (2048); 65 beams: two workgroups.
    The beams start 1 mm in front of the liver, so that five rows (1.6 mm) hold a boundary and 64 (20.6 mm) the bone's too"""
    E = 65
    pos, dirs = spheres["pos"][::2] + f32([4.4, 0.0, 0.0]), spheres["dirs"][::2]
    ctx = context(mcrt, spheres["sd"], n_elements=E, n_rows=R)
    dev = dev_of(ctx)
    try:
        for mode, rule in COMBOS if R < 2048 else [("total", "traced"), ("boundaries", "geometric")]:
            want = mirror(orc, "spheres", spheres["osc"], pos, dirs, R, mode, rule)
            assert want[2].max() >= (1 if R == 5 else 2) and np.count_nonzero(want[1]) >= 8
            same(transmit(ctx, dev, R, pos[None], dirs[None], mode=mode, rule=rule), [w[None] for w in want], "R %d %s %s" % (R, mode, rule))
    finally:
        done(ctx, dev)


def test_frames_subranges_and_the_contexts_transducer(mcrt, orc, dev_of, spheres):
    """three pose frames in one pass, host and device tables, a scan-line sub-range; one frame from the context's transducer"""
    E, R = 65, 465
    tables = [lm.fan(E, a, dz=z) for a, z in ((0.35, 0.01), (0.2, 0.02), (0.3, -0.015))]
    pos = np.stack([t[0] for t in tables]); dirs = np.stack([t[1] for t in tables])
    ctx = context(mcrt, spheres["sd"], n_elements=E, n_rows=R)
    dev = dev_of(ctx)
    try:
        for mode, rule in COMBOS:
            want = mirror(orc, "spheres", spheres["osc"], pos, dirs, R, mode, rule)
            assert not np.array_equal(want[0][0], want[0][1])
            same(transmit(ctx, dev, R, pos, dirs, mode=mode, rule=rule), want, "host pose table %s %s" % (mode, rule))
            same(transmit(ctx, dev, R, pos, dirs, mode=mode, rule=rule, e0=7, e1=40), [w[:, 7:40] for w in want], "scan-lines [7,40) %s %s" % (mode, rule))
        want = mirror(orc, "spheres", spheres["osc"], pos, dirs, R, "total", "traced")
        same(transmit(ctx, dev, R, dev.upload(pos), dev.upload(dirs), n_frames=3), want, "device pose table")
        same(transmit(ctx, dev, R, pos, dirs, e0=64, e1=65), [w[:, 64:65] for w in want], "the last scan-line")
        ctx.set_transducer(pos[1], dirs[1])
        same(transmit(ctx, dev, R), [w[1:2] for w in want], "the context's transducer")
        same(transmit(ctx, dev, R, e0=3, e1=64), [w[1:2, 3:64] for w in want], "the context's transducer, scan-lines [3,64)")
    finally:
        done(ctx, dev)


def test_outputs_of_any_alignment_and_each_left_out(mcrt, orc, dev_of, spheres):
    """the maps are written as 16-byte stores where the address allows, single floats at the ragged ends: an output 4, 8 or 12 bytes off a
    16-byte boundary is the same map, with nothing written before or behind it; and each output may be left out"""
    ctx = context(mcrt, spheres["sd"])
    dev = dev_of(ctx)
    try:
        for E, R in ((3, 465), (65, 5), (130, 64), (1, 2)):
            pos, dirs = spheres["pos"][N_FAN // 2 - E // 2:][:E], spheres["dirs"][N_FAN // 2 - E // 2:][:E]
            ctx.set_params(n_elements=E, n_rows=R)
            for mode in MODES:
                want = [w[None] for w in mirror(orc, "spheres", spheres["osc"], pos, dirs, R, mode, "traced")]
                for skew in (0, 1, 2, 3):
                    same(transmit(ctx, dev, R, pos[None], dirs[None], mode=mode, skew=skew), want, "E %d R %d %s, %d bytes off" % (E, R, mode, 4 * skew))
            dev.close(); dev.bufs = []
        E, R = 65, 465
        pos, dirs = spheres["pos"][::2], spheres["dirs"][::2]
        ctx.set_params(n_elements=E, n_rows=R)
        want = [w[None] for w in mirror(orc, "spheres", spheres["osc"], pos, dirs, R, "total", "traced")]
        for skip in range(3):
            got = transmit(ctx, dev, R, pos[None], dirs[None], want=tuple(i != skip for i in range(3)))
            assert got[skip] is None
            same(got, want, "without output %d" % skip)
    finally:
        done(ctx, dev)


def test_crossing_cap(mcrt, orc, dev_of):
    """40 nested boxes 0.95 mm apart are 80 boundaries (a start offset of 1e-3 under both rules: the tracer's 0.1 would step over every other
    wall): the walk stops at 64 with bit 31 set, and the rows still equal the mirror's"""
    R = 465
    sd = lm.boxes_scene(mcrt, 40, step=0.095)
    osc = lm.oracle_scene(orc, sd)
    pos, dirs = lm.fan(3, 0.02, dz=0.013)
    ctx = context(mcrt, sd, n_elements=3, n_rows=R)
    dev = dev_of(ctx)
    try:
        for mode, rule in COMBOS:
            got = transmit(ctx, dev, R, pos[None], dirs[None], mode=mode, rule=rule, offs=1e-3)
            same(got, [w[None] for w in mirror(orc, "boxes40", osc, pos, dirs, R, mode, rule, offs=1e-3)], "40 boxes %s %s" % (mode, rule))
            assert ((got[2] & 0x7fffffff) == lm.MAX_CROSSINGS).all() and (got[2] >> 31).all()
            assert np.count_nonzero(got[1][0, 1]) >= 16          # LIVER | FAT | KIDNEY in turn: most boundaries turn something back
    finally:
        done(ctx, dev)


# ------------------------------------------------------------------ against the shipped label product
def _liver(mcrt, E):
    cfg, meshes = mcrt.synth.liver_scene(2)
    sd = mcrt.scene_io.build_scene(cfg, meshes)
    return cfg, sd, mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])


def test_consistent_with_the_label_maps(mcrt, dev_of):
    """exact, and independent of the mirror: crossings equals mcrt_label_frames' on the same poses and options, and every row that turns
    something back holds an interface"""
    E, R = 130, 465
    cfg, sd, tr = _liver(mcrt, E)
    ctx = context(mcrt, sd, n_elements=E, n_rows=R)
    dev = dev_of(ctx)
    try:
        sp, sdir = tr.swept(3, 0.05, 10.0)
        for rule in RULES:
            offs = RULES[rule][1]
            i_dev, c_dev = dev(3 * E * R * 4), dev(3 * E * 4)
            ctx.label_frames(sp, sdir, rule=rule, start_offset=offs, interface_dev=i_dev, crossings_dev=c_dev)
            interface, crossings = ctx.d2h(i_dev, (3, E, R), np.int32), ctx.d2h(c_dev, (3, E), np.uint32)
            for mode in MODES:
                T, Rf, c = transmit(ctx, dev, R, sp, sdir, mode=mode, rule=rule)
                assert np.array_equal(c, crossings), (rule, mode)
                assert ((Rf != 0) <= (interface != -1)).all() and (Rf != 0).any(), (rule, mode)
                assert (T[:, :, 0] == 1.0).all() and (T >= 0).all() and (T <= 1).all() and (Rf >= 0).all() and (Rf <= 1).all()
            assert crossings.max() >= 4
    finally:
        done(ctx, dev)


# ------------------------------------------------------------------ the layers above
def _sim(mcrt, sd, tr, **kw):
    return mcrt.Simulator(sd, tr, n_samples=2, texture=mcrt.host_texture(32), tex_n=32, **kw)


def test_simulator_plumbing(mcrt, dev_of):
    """transmission()'s picture is mcrt_scan_convert_frames of its own stack, transmission_volume() mcrt_volume_frames of the planes' stacks,
    freehand_transmission() mcrt_recon_frames of the poses' stacks: bit for bit"""
    E = 64
    cfg, sd, tr = _liver(mcrt, E)
    sim = _sim(mcrt, sd, tr)
    try:
        R = sim.R
        dev = dev_of(sim.ctx)
        got = sim.transmission()
        bnd = sim.transmission(mode="boundaries", picture=False, out_rows=100, out_cols=120)
        geo = sim.transmission(rule="geometric", start_offset=1e-3, picture=False)
        small = sim.transmission(out_rows=100, out_cols=120)
        labels = sim.labels()
        assert got["transmit"].shape == (E, R) and got["reflect"].shape == (E, R) and got["crossings"].shape == (E,) and got["picture"].shape == (400, 500)
        assert got["transmit"].dtype == f32 and got["picture"].dtype == f32 and got["crossings"].dtype == np.uint32
        assert np.array_equal(got["crossings"], labels["crossings"]) and bnd["picture"] is None and small["picture"].shape == (100, 120)
        # the boundaries alone lose no more than everything does (the same walk; a part in a million for the roundings of the two chains)
        assert (np.diff(bnd["transmit"].astype(np.float64), axis=1) <= 0).all() and (bnd["transmit"] >= got["transmit"] * f32(1 - 1e-6)).all()
        assert np.array_equal(bnd["reflect"] != 0, got["reflect"] != 0) and not np.array_equal(geo["transmit"], got["transmit"])
        stack, pic = dev.upload(got["transmit"]), dev(400 * 500 * 4)
        sim.ctx.scan_convert_frames(stack, 1, E, R, pic)
        tm.same_bits(got["picture"], sim.ctx.d2h(pic, (400, 500)), "transmission()['picture']")
        # 0 outside the sector, and the label picture is its mask -- but for the outline, where the nearest rule of the labels and the
        # interpolation of the floats end a pixel apart: two radial edges of ~400 pixels and two arcs of ~500, a band of two pixels, 2 % of 200000
        outside = labels["picture"] == lm.NONE
        assert got["picture"][0, 0] == 0 and got["picture"][0, -1] == 0 and (got["picture"] > 0).any() and outside[0, 0]
        assert np.count_nonzero((got["picture"] != 0) & outside) < 0.02 * outside.size
        # a freehand sweep of five poses, binned into 2 mm voxels of the WORLD frame about the cloud's middle
        sp, sdir = tr.swept(5, 0.04, 10.0)
        mid = np.round((sp + 4.0 * sdir).reshape(-1, 3).astype(np.float64).mean(0) * 10.0)
        shape = (8, 24, 24)
        grid = mcrt.volume_grid(mid - np.array([24.0, 24.0, 8.0]), (2.0, 0, 0), (0, 2.0, 0), (0, 0, 2.0), 24, 24, 8)
        vol = sim.freehand_transmission(sp, sdir, grid)
        vol2, cnt = sim.freehand_transmission(sp, sdir, grid, counts=True, fill_radius=0)
        n = shape[0] * shape[1] * shape[2]
        st, out, cn = dev(5 * E * R * 4), dev(n * 4), dev(n * 4)
        sim.ctx.transmit_frames(sp, sdir, transmit_dev=st)
        sim.ctx.recon_frames(st, sp, sdir, 5, E, R, grid, out)
        tm.same_bits(vol, sim.ctx.d2h(out, shape), "freehand_transmission()")
        sim.ctx.recon_frames(st, sp, sdir, 5, E, R, grid, out, count_dev=cn, fill_radius=0)
        tm.same_bits(vol2, sim.ctx.d2h(out, shape), "freehand_transmission(fill_radius=0)")
        assert np.array_equal(cnt, sim.ctx.d2h(cn, shape, np.uint32)) and cnt.any() and (vol > 0).any() and vol.shape == shape
        with pytest.raises(RuntimeError):
            sim.transmission_volume(mcrt.cplane_grid(80.0, 96, 40, 0.5))
    finally:
        sim.close()
    K, step, pivot = 3, 0.05, 10.0
    sim = _sim(mcrt, sd, tr, sweep=(K, step), sweep_pivot_mm=pivot)
    try:
        dev = dev_of(sim.ctx)
        got = sim.transmission()
        assert got["picture"] is None and got["transmit"].shape == (K, E, R) and got["crossings"].shape == (K, E)
        g = mcrt.cplane_grid(80.0, 96, 40, 0.5)
        cut = sim.transmission_volume(g)
        stack, out = dev.upload(got["transmit"]), dev(96 * 40 * 4)
        sim.ctx.volume_frames(stack, 1, E, R, (K, step, pivot), g, out)
        tm.same_bits(cut, sim.ctx.d2h(out, (1, 40, 96)), "transmission_volume()")
        assert (cut > 0).any() and (cut == 0).any()
        with pytest.raises(RuntimeError):
            sim.freehand_transmission(*tr.swept(2, 0.04, 10.0), g)
    finally:
        sim.close()
    for kw in (dict(compound=(-0.1, 0.0, 0.1)), dict(elevation=True)):
        sim = _sim(mcrt, sd, tr, **kw)
        try:
            with pytest.raises(RuntimeError):
                sim.freehand_transmission(*tr.swept(2, 0.04, 10.0), mcrt.cplane_grid(80.0, 48, 20, 1.0))
        finally:
            sim.close()


def test_refusals_launch_nothing(mcrt, dev_of, spheres):
    """every refusal returns MCRT_ERR_INVALID / MCRT_ERR_LIMIT, names the call and its field, and leaves the pre-filled outputs as they were"""
    from mcray_tracing_amd import TransmitOpts
    L = mcrt.load_library()
    E, R = 8, 64
    sd = spheres["sd"]
    pos, dirs = spheres["pos"][:E].copy(), spheres["dirs"][:E].copy()
    bare = mcrt.Context(0)
    ctx = context(mcrt, sd, n_elements=E, n_rows=R)
    dev = dev_of(ctx)
    try:
        fills = (np.full((3, E, R), FILL_F, f32), np.full((3, E, R), FILL_F, f32), np.full((3, E), FILL_C, np.uint32))
        bufs = [dev.upload(a) for a in fills]
        pos3, dir3 = np.stack([pos] * 3), np.stack([dirs] * 3)
        vp = C.c_void_p

        def call(c, F=1, e0=0, e1=E, p=None, d=None, opts=None, outs=(0, 1, 2), off=(0, 0, 0)):
            o = [vp(bufs[i] + off[i]) if i in outs else None for i in range(3)]
            rc = L.mcrt_transmit_frames(c.h if c is not None else None, F, e0, e1, p.ctypes.data_as(vp) if p is not None else None,
                                        d.ctypes.data_as(vp) if d is not None else None, C.byref(opts) if opts is not None else None, *o)
            return rc, L.mcrt_last_error().decode()

        assert call(None)[0] == INVALID
        rc, msg = call(bare); assert rc == INVALID and "no scene" in msg
        rc, msg = call(ctx); assert rc == INVALID and "no transducer" in msg
        ctx.set_transducer(pos, dirs)
        assert call(ctx)[0] == 0
        ctx.synchronize()
        for b, a in zip(bufs, fills):
            ctx.h2d(b, a)
        cases = [(dict(e0=3, e1=3), "scan-line range"), (dict(e0=5, e1=4), "scan-line range"), (dict(e1=E + 1), "scan-line range"),
                 (dict(p=pos3, F=3), "pos and dir"), (dict(d=dir3, F=3), "pos and dir"), (dict(outs=()), "no output"), (dict(F=2), "n_frames"), (dict(F=0), "n_frames"),
                 (dict(opts=TransmitOpts(0, 2, -1.0)), "rule"), (dict(opts=TransmitOpts(2, 0, -1.0)), "mode"), (dict(opts=TransmitOpts(0, 0, float("nan"))), "start_offset"),
                 (dict(opts=TransmitOpts(0, 0, float("inf"))), "start_offset"), (dict(opts=TransmitOpts(1, 1, 0.0)), "start_offset"),
                 (dict(off=(2, 0, 0)), "transmit_dev"), (dict(off=(0, 1, 0)), "reflect_dev"), (dict(off=(0, 0, 3)), "crossings_dev")]
        for kw, field in cases:
            rc, msg = call(ctx, **kw)
            assert rc == INVALID and msg.startswith("mcrt_transmit_frames") and field in msg, (kw, rc, msg)
        big = np.zeros((1025, E, 3), f32)
        rc, msg = call(ctx, F=1025, p=big, d=big); assert rc == LIMIT and "n_frames" in msg and "1024" in msg
        ctx.synchronize()
        for b, a in zip(bufs, fills):
            assert np.array_equal(ctx.d2h(b, a.shape, a.dtype).view(np.uint32), a.view(np.uint32))
        # the limit of 254 materials is the tissue byte's, not this call's
        many = mcrt.scene_io.SceneData(sd.tri, sd.tri_mesh, sd.meshes, np.resize(sd.materials, (300, 8)), ["m%d" % i for i in range(300)], sd.start_mat, sd.spacing, sd.config)
        ctx.upload_scene(many)
        assert call(ctx)[0] == 0
        rc = L.mcrt_label_frames(ctx.h, 1, 0, E, None, None, None, vp(bufs[0]), None, None); assert rc == LIMIT
        ctx.synchronize()
    finally:
        done(ctx, dev); bare.close()


def _write_scene(mcrt, tmp_path):
    cfg, meshes = mcrt.synth.sphere_scene(3)
    cfg["workingDirectory"] = str(tmp_path) + "/"
    for f, (V, F) in meshes.items():
        mcrt.scene_io.save_obj(str(tmp_path / f), V, F)
    (tmp_path / "sphere.scene").write_text(json.dumps(cfg))
    return cfg, str(tmp_path / "sphere.scene")


def test_host_shim(mcrt, tmp_path):
    """rf_image::transmission / transmission_picture against the C ABI called beside them (tests/host/transmit_driver.cpp checks that itself),
    and against Python's Simulator -- on one context and on a two-rank group sharing the GPU"""
    pkg = os.path.join(ROOT, "mcray-tracing_amd")
    exe = str(tmp_path / "transmit_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(pkg, "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "transmit_driver.cpp"), "-L", pkg, "-lmcrt_hip", "-Wl,-rpath," + pkg])
    cfg, scene = _write_scene(mcrt, tmp_path)
    sd = mcrt.scene_io.load_scene_file(scene)
    E, R = 64, 465
    tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    sim = _sim(mcrt, sd, tr)
    try:
        want = {0: sim.transmission(), 1: sim.transmission(mode="boundaries", rule="geometric", start_offset=1e-3)}
    finally:
        sim.close()
    for devices, mode, rule, offs in (("0", 0, 0, -1.0), ("0", 1, 1, 1e-3), ("0,0", 0, 0, -1.0)):
        out = tmp_path / "transmit.bin"
        r = subprocess.run([exe, scene, str(out), devices, str(mode), str(rule), repr(offs)], capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout + r.stderr
        raw = out.read_bytes()
        n = E * R
        assert len(raw) == 4 * (2 * n + E + 200000)
        w = want[mode]
        tm.same_bits(np.frombuffer(raw, f32, n).reshape(E, R), w["transmit"], "shim transmit " + devices)
        tm.same_bits(np.frombuffer(raw, f32, n, 4 * n).reshape(E, R), w["reflect"], "shim reflect " + devices)
        assert np.array_equal(np.frombuffer(raw, np.uint32, E, 8 * n), w["crossings"])
        tm.same_bits(np.frombuffer(raw, f32, 200000, 8 * n + 4 * E).reshape(400, 500), w["picture"], "shim picture " + devices)
    assert (want[0]["picture"] > 0).any() and want[0]["transmit"].min() < 1e-3


def test_cli_transmission(mcrt, tmp_path):
    """--transmission writes the API's picture as grey made on the host: linear, and in decibels over a range"""
    pkg = os.path.join(ROOT, "mcray-tracing_amd")
    exe = os.path.join(pkg, "mattausch_hip")
    sources = [os.path.join(pkg, "host", "mattausch_main.cpp"), os.path.join(pkg, "host", "mcrt_host.hpp"), os.path.join(pkg, "libmcrt_hip.so")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in sources):      # (the program the build made, unless it is stale)
        subprocess.check_call(["make", "-C", pkg, "mattausch_hip"])
    cfg, scene = _write_scene(mcrt, tmp_path)
    sd = mcrt.scene_io.load_scene_file(scene)
    tr = mcrt.Transducer(512, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    sim = _sim(mcrt, sd, tr)
    try:
        total = sim.transmission()["picture"]
        bnd = sim.transmission(mode="boundaries", rule="geometric", start_offset=float(f32(0.001)))["picture"]
    finally:
        sim.close()
    head = b"P5\n500 400\n255\n"
    lin, log = tmp_path / "lin.pgm", tmp_path / "log.pgm"
    runs = [subprocess.Popen([exe, scene, "1", "1", "--transmission", str(lin)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True),
            subprocess.Popen([exe, scene, "1", "1", "--transmission", str(log), "--transmission-mode", "boundaries", "--transmission-db", "40", "--label-rule", "geometric",
                              "--label-offset", "0.001"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)]      # (side by side: most of a run is the program's start)
    for r in runs:
        text, _ = r.communicate(timeout=240)
        assert r.returncode == 0, text
    raw = lin.read_bytes()
    want = (np.minimum(np.maximum(total, f32(0)), f32(1)) * f32(255) + f32(0.5)).astype(np.uint8)
    assert raw.startswith(head) and raw[len(head):] == want.tobytes() and len(np.unique(want)) >= 10
    got = np.frombuffer(log.read_bytes()[len(head):], np.uint8).reshape(400, 500)
    with np.errstate(divide="ignore"):
        db = np.where(bnd > 0, np.clip((10.0 * np.log10(np.maximum(bnd, f32(1e-30)).astype(np.float64)) + 40.0) / 40.0, 0.0, 1.0), 0.0)
    want = (db * 255.0 + 0.5).astype(np.uint8)
    assert (np.abs(got.astype(int) - want.astype(int)) <= 1).all() and (got == 0).any() and (got == 255).any()      # (log10f against log10: a grey level at a rounding edge)
