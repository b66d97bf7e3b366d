"""Slice thickness on the MI355X: mcrt_elevation_frames (k_elevation) against the numpy mirror (tests/elevation_mirror.py) bit for bit
on random plane stacks, NaN / infinity under a zero weight, passes against single calls, table uploads between back-to-back calls and
beside the focal zones' table, argument errors, a target BESIDE the image plane end to end against the CPU oracle, the Simulator, a
two-rank group, the C++ shim and the CLI."""
import ctypes as C
import json
import os
import subprocess
import numpy as np
import pytest

import elevation_mirror as em
import focus_mirror as fm
import image_cases as ic
from test_gpu_focus import Dev, table

pytestmark = pytest.mark.gpu

f32 = np.float32
INVALID, LIMIT = -1, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the elevation PSF of the end-to-end tests: planes 1.5 mm apart (K = 7: z = -4.5 .. +4.5 mm) under var_z = 9 mm^2, a slice of
# sigma = 3 mm ("several millimetres thick").  With the reference's var_z = 0.1 mm^2 the outermost plane would weigh exp(-101): nothing.
PITCH_UM, VAR_Z = 1500, 9.0


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


def stack(F, K, E, R, seed=0):
    """random plane stacks [F][K][E][R] with -0.0, NaN and inf taps (ic.conv_image per plane)"""
    return np.stack([np.stack([ic.conv_image(E, R, seed=seed + 100 * f + k) for k in range(K)]) for f in range(F)])


SHAPES = sorted(set(ic.conv_shapes(7, 13) + ic.SCAN_SHAPES + [(37, 1001), (130, 2047), (128, 465), (3, 2048)]))


@pytest.mark.parametrize("K", [1, 2, 7, 32])
def test_random_stacks_match_the_mirror(ctx, dev, K):
    """every pixel compared; (E, R) with E*R % 4 == 0 take the float4 lanes, the others (an odd E*R among them) the scalar ones"""
    odd = 0
    for E, R in SHAPES:
        odd += (E * R) % 2
        for F in (1, 3):
            st = stack(F, K, E, R)
            w = table(R, K)
            p, q = dev.upload(st), dev(F * E * R * 4)
            ctx.elevation_frames(p, F, K, E, R, w, q)
            ic.assert_same_bits(ctx.d2h(q, (F, E, R)), em.fold(st, w), "fold %dx%dx%dx%d" % (F, K, E, R))
    assert odd > 0


@pytest.mark.parametrize("in_off,out_off", [(4, 0), (0, 4), (4, 4), (8, 12)])
def test_sub_buffers_take_the_scalar_path(ctx, dev, in_off, out_off):
    """E*R % 4 == 0 but a pointer that is not 16-byte aligned: the same sums through the scalar lanes, nothing written beside the image"""
    F, K, E, R = 2, 7, 128, 465
    st = stack(F, K, E, R, seed=3)
    w = table(R, K, seed=3)
    p = dev(st.nbytes + 64); q = dev(F * E * R * 4 + 64)
    guard = np.full(F * E * R + 16, -7.25, f32)
    ctx.h2d(p + in_off, st); ctx.h2d(q, guard)
    ctx.elevation_frames(p + in_off, F, K, E, R, w, q + out_off)
    got = ctx.d2h(q, (F * E * R + 16,))
    o = out_off // 4
    ic.assert_same_bits(got[o:o + F * E * R].reshape(F, E, R), em.fold(st, w), "offset %d/%d" % (in_off, out_off))
    assert (got[:o] == f32(-7.25)).all() and (got[o + F * E * R:] == f32(-7.25)).all()


def test_one_plane_with_weight_one_copies_the_image(ctx, dev):
    E, R = 128, 465
    st = stack(1, 1, E, R, seed=9)
    assert (np.signbit(st) & (st == 0)).any()
    p, q = dev.upload(st), dev(E * R * 4)
    ctx.elevation_frames(p, 1, 1, E, R, np.ones((R, 1), f32), q)
    got = ctx.d2h(q, (E, R))
    want = st[0, 0].copy()
    want[want == 0] = 0.0                                    # a -0.0 becomes +0.0
    ic.assert_same_bits(got, want, "copy")


def test_a_nan_under_a_zero_weight_reaches_its_own_pixel_only(ctx, dev):
    F, K, E, R = 2, 7, 40, 120
    rng = np.random.default_rng(5)
    st = rng.standard_normal((F, K, E, R)).astype(f32)
    st[1, 3, 20, 60] = np.nan
    st[0, 5, 7, 11] = np.inf
    st[1, 0, 39, 119] = -np.inf
    w = table(R, K, seed=5)
    w[:, 3] = 0.0; w[11, 5] = 0.0; w[119, 0] = 0.0          # 0 * NaN and 0 * inf are NaN
    p, q = dev.upload(st), dev(F * E * R * 4)
    ctx.elevation_frames(p, F, K, E, R, w, q)
    got = ctx.d2h(q, (F, E, R))
    ic.assert_same_bits(got, em.fold(st, w), "nan")
    assert sorted(map(tuple, np.argwhere(np.isnan(got)))) == [(0, 7, 11), (1, 20, 60), (1, 39, 119)]


@pytest.mark.parametrize("E,R", [(128, 465), (3, 2048), (129, 465)])
def test_a_pass_equals_single_calls(ctx, dev, E, R):
    F, K = 4, 7
    st = stack(F, K, E, R, seed=2)
    w = table(R, K, seed=2)
    p, q, one = dev.upload(st), dev(F * E * R * 4), dev(E * R * 4)
    ctx.elevation_frames(p, F, K, E, R, w, q)
    got = ctx.d2h(q, (F, E, R))
    for f in range(F):
        ctx.elevation_frames(p + f * K * E * R * 4, 1, K, E, R, w, one)
        assert np.array_equal(got[f].view(np.uint32), ctx.d2h(one, (E, R)).view(np.uint32)), f
    ic.assert_same_bits(got, em.fold(st, w), "pass")


def test_back_to_back_calls_each_get_their_own_table(ctx, dev):
    """no synchronisation between the calls, and the caller's array rewritten as soon as each call returns"""
    E, R, K = 96, 465, 7
    tabs = [table(R, K, seed=s) for s in (11, 12, 11, 13)] + [table(2048, 5, seed=14)]
    shapes = [(K, E, R)] * 4 + [(5, 8, 2048)]
    sts = [stack(1, k, e, r, seed=20 + i) for i, (k, e, r) in enumerate(shapes)]
    ps = [dev.upload(s) for s in sts]
    qs = [dev(e * r * 4) for _, e, r in shapes]
    ctx.synchronize()
    buf = np.empty((R, K), f32)
    for p, q, t, (k, e, r) in zip(ps, qs, tabs, shapes):
        if t.shape == buf.shape:
            buf[:] = t
            ctx.elevation_frames(p, 1, k, e, r, buf, q)
            buf[:] = np.nan                                  # the call has returned: the table is the caller's again
        else:
            ctx.elevation_frames(p, 1, k, e, r, t, q)
    ctx.synchronize()
    for i, (q, t, s, (k, e, r)) in enumerate(zip(qs, tabs, sts, shapes)):
        ic.assert_same_bits(ctx.d2h(q, (1, e, r)), em.fold(s, t), "call %d" % i)


def test_the_elevation_and_the_focal_tables_live_side_by_side(ctx, dev):
    """a frame uses both tables in turn: alternating calls, each table changed half way, keep both right"""
    E, R, K, n_lat = 64, 465, 7, 13
    ax, _ = ic.conv_taps(7, n_lat, seed=6)
    st = stack(1, K, E, R, seed=6)
    p = dev.upload(st)
    qs = [dev(E * R * 4) for _ in range(4)]
    ws = [table(R, K, seed=31), table(R, K, seed=31), table(R, K, seed=32), table(R, K, seed=32)]
    lats = [table(R, n_lat, seed=41), table(R, n_lat, seed=42), table(R, n_lat, seed=42), table(R, n_lat, seed=41)]
    for q, w, lat in zip(qs, ws, lats):
        ctx.elevation_frames(p, 1, K, E, R, w, q)
        ctx.convolve_frames_depth(q, 1, E, R, ax, lat)
    ctx.synchronize()
    for i, (q, w, lat) in enumerate(zip(qs, ws, lats)):
        ic.assert_same_bits(ctx.d2h(q, (E, R)), fm.convolve_depth(em.fold(st, w)[0], ax, lat), "frame %d" % i)


def test_errors_leave_the_image_untouched(mcrt, ctx, dev):
    K, E, R = 3, 40, 60
    st = stack(1, K, E, R)
    p = dev.upload(st)
    img = ic.conv_image(E, R, seed=77)
    q = dev.upload(img)
    big = dev.upload(stack(1, 1, 3, 2049))
    w = table(R, K)
    L = ctx.L
    wp, pv, qv = w.ctypes.data_as(C.c_void_p), C.c_void_p(p), C.c_void_p(q)
    assert L.mcrt_elevation_frames(ctx.h, None, 1, K, E, R, wp, qv) == INVALID
    assert L.mcrt_elevation_frames(ctx.h, pv, 1, K, E, R, None, qv) == INVALID
    assert L.mcrt_elevation_frames(ctx.h, pv, 1, K, E, R, wp, None) == INVALID
    assert L.mcrt_elevation_frames(None, pv, 1, K, E, R, wp, qv) == INVALID
    for sizes in ((0, K, E, R), (1, 0, E, R), (1, K, 0, R), (1, K, E, 0)):
        assert L.mcrt_elevation_frames(ctx.h, pv, *sizes, wp, qv) == INVALID, sizes
    w33 = table(R, 33)
    assert L.mcrt_elevation_frames(ctx.h, pv, 1, 33, E, R, w33.ctypes.data_as(C.c_void_p), qv) == LIMIT
    w2049 = table(2049, 1)
    assert L.mcrt_elevation_frames(ctx.h, C.c_void_p(big), 1, 1, 3, 2049, w2049.ctypes.data_as(C.c_void_p), qv) == LIMIT
    # overlap: the output inside the stack, the stack's end inside the output, the same pointer
    for out in (p, p + (K - 1) * E * R * 4, p + K * E * R * 4 - 4, p - E * R * 4 + 4):
        assert L.mcrt_elevation_frames(ctx.h, pv, 1, K, E, R, wp, C.c_void_p(out)) == INVALID and b"overlap" in L.mcrt_last_error()
    with pytest.raises(ValueError):
        ctx.elevation_frames(p, 1, K, E, R, table(R + 1, K), q)
    with pytest.raises(ValueError):
        ctx.elevation_frames(p, 1, K, E, R, table(R, K + 1), q)
    ctx.synchronize()
    assert np.array_equal(ctx.d2h(q, (E, R)).view(np.uint32), img.view(np.uint32))
    assert np.array_equal(ctx.d2h(p, (1, K, E, R)).view(np.uint32), st.view(np.uint32))
    ctx.elevation_frames(p, 1, K, E, R, w, q)                # adjacent buffers are fine; the context still works
    ic.assert_same_bits(ctx.d2h(q, (1, E, R)), em.fold(st, w), "after the errors")


# ------------------------------------------------------------------ end to end: a target beside the image plane
def _beside_scenes(mcrt):
    """the sphere scene with its sphere moved BESIDE the image plane (centre z = 2.3 cm, radius 2: it reaches down to z = 0.3 cm), and the
    same scene without the sphere"""
    cfg, meshes = mcrt.synth.sphere_scene(3)
    meshes["SPHERE.obj"] = mcrt.synth.icosphere(3, 2.0, center=(0.0, 0.0, 2.3))
    with_sphere = mcrt.scene_io.build_scene(cfg, meshes)
    cfg2 = dict(cfg, meshes=[m for m in cfg["meshes"] if m["file"] != "SPHERE.obj"])
    without = mcrt.scene_io.build_scene(cfg2, {"BOX.obj": meshes["BOX.obj"]})
    return cfg, with_sphere, without


def _oracle(orc, sd):
    return orc.OracleScene(sd.tri, sd.tri_mesh, sd.meshes, sd.materials, sd.start_mat, sd.spacing)


def _setup(obj, sd, tr, S, tex):
    obj.set_params(n_elements=tr.n_elements, n_samples=S, frequency=tr.frequency)
    obj.upload_scene(sd)
    obj.upload_texture(tex, 256)
    obj.set_transducer(tr.pos, tr.dir)


def test_a_target_beside_the_image_plane(mcrt, orc, tex256):
    cfg, sd_a, sd_b = _beside_scenes(mcrt)
    E, S, K = 32, 16, 7
    tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    pos, dirs, z = tr.planes(K, PITCH_UM)
    assert z.tolist() == [-4.5, -3.0, -1.5, 0.0, 1.5, 3.0, 4.5]
    p = orc.default_params(n_elements=E, n_samples=S)
    R = p.n_rows
    sphere_tri = np.flatnonzero(sd_a.tri_mesh == 1)
    o_a = [_oracle(orc, sd_a).trace_frame(p, pos[k], dirs[k], tex256, frame_id=k, use_bvh=False) for k in range(K)]
    o_b = [_oracle(orc, sd_b).trace_frame(p, pos[k], dirs[k], tex256, frame_id=k, use_bvh=False) for k in range(K)]
    # the facts of the input, from the CPU oracle: only the outermost plane meets the sphere
    for k in range(K):
        n_hits = int(np.isin(o_a[k]["hits"], sphere_tri).sum())
        diff = o_a[k]["rf"].view(np.uint32) != o_b[k]["rf"].view(np.uint32)           # [R][E]
        assert not np.isnan(o_a[k]["rf"]).any() and not np.isnan(o_b[k]["rf"]).any()
        if k < 6:
            assert n_hits == 0 and not diff.any(), k
        else:
            rows, cols = np.nonzero(diff)
            assert n_hits == 64 and diff.sum() == 467 and (rows.min(), rows.max()) == (302, 464) and (cols.min(), cols.max()) == (14, 17)
    plane6 = (o_a[6]["rf"].view(np.uint32) != o_b[6]["rf"].view(np.uint32)).T             # [E][R]
    psf = mcrt.Psf(freq=tr.frequency, var_z=VAR_Z, elevation_pitch_um=PITCH_UM)
    folds = []
    for sd, o in ((sd_a, o_a), (sd_b, o_b)):
        c = mcrt.Context(0)
        try:
            _setup(c, sd, tr, S, tex256)
            w = psf.elevation_rows(R, mcrt.row_pitch_mm(tr.frequency))
            st_dev, rf_dev = c.alloc(K * E * R * 4), c.alloc(E * R * 4)
            c.trace_frames_poses(0, pos, dirs, st_dev)
            c.elevation_frames(st_dev, 1, K, E, R, w, rf_dev)
            c.synchronize()
            st = c.d2h(st_dev, (1, K, E, R))
            for k in range(K):
                ic.assert_same_bits(st[0, k], o[k]["rf"].T, "plane %d vs the oracle" % k)
            fold = c.d2h(rf_dev, (E, R))
            ic.assert_same_bits(fold, em.fold(st, w)[0], "fold vs the mirror")
            folds.append((st[0, 3].copy(), fold))
            c.free(st_dev); c.free(rf_dev)
        finally:
            c.close()
    (centre_a, fold_a), (centre_b, fold_b) = folds
    assert np.array_equal(centre_a.view(np.uint32), centre_b.view(np.uint32))            # the thin sheet is blind to the sphere ...
    seen = fold_a.view(np.uint32) != fold_b.view(np.uint32)                              # ... the slice is not
    assert seen.any() and not (seen & ~plane6).any()


def test_simulator(mcrt, orc, tex256):
    cfg, sd, _ = _beside_scenes(mcrt)
    E, S, K = 16, 16, 3
    tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    p = orc.default_params(n_elements=E, n_samples=S)
    osc = _oracle(orc, sd)
    plain = mcrt.Simulator(sd, tr, n_samples=S, texture=tex256)
    try:
        assert not plain.elevation
        o = osc.trace_frame(p, tr.pos, tr.dir, tex256, frame_id=2, use_bvh=False)
        ic.assert_same_bits(plain.frame(2, convolve=False), o["rf"], "without elevation: the thin sheet")
        ic.assert_same_bits(plain.frame(2), orc.convolve(o["rf"], plain.psf.axial_kernel, plain.psf.lateral_kernel), "without elevation, convolved")
    finally:
        plain.close()
    psf = mcrt.Psf(freq=tr.frequency, var_z=VAR_Z, elevation_size=K, elevation_pitch_um=PITCH_UM, elevation_focus_mm=(60.0,))
    sim = mcrt.Simulator(sd, tr, n_samples=S, texture=tex256, psf=psf, elevation=True)
    try:
        pos, dirs, z = tr.planes(K, PITCH_UM)
        assert sim.K == K and np.array_equal(sim.plane_z_mm, z) and z.tolist() == [-1.5, 0.0, 1.5]
        w = psf.elevation_rows(sim.R, sim.row_mm)
        alone = {}
        for f in (0, 2):
            planes = np.stack([osc.trace_frame(p, pos[k], dirs[k], tex256, frame_id=f * K + k, use_bvh=False)["rf"].T for k in range(K)])
            want = em.fold(planes[None], w)[0]
            alone[f] = sim.frame(f, convolve=False)
            ic.assert_same_bits(alone[f].T, want, "frame %d vs the mirror of the oracle's planes" % f)
            ic.assert_same_bits(sim.frame(f), orc.convolve(want.T, psf.axial_kernel, psf.lateral_kernel), "frame %d convolved" % f)
        # frame f traced alone is frame f of a hand-made pass of 3 frames
        F = 3
        st_dev, rf_dev = sim.ctx.alloc(F * K * E * sim.R * 4), sim.ctx.alloc(F * E * sim.R * 4)
        sim.ctx.trace_frames_poses(0, np.tile(pos, (F, 1, 1)), np.tile(dirs, (F, 1, 1)), st_dev)
        sim.ctx.elevation_frames(st_dev, F, K, E, sim.R, w, rf_dev)
        got = sim.ctx.d2h(rf_dev, (F, E, sim.R))
        for f in (0, 2):
            assert np.array_equal(got[f].T.view(np.uint32), alone[f].view(np.uint32)), f
        assert not np.array_equal(got[0], got[2])
        sim.ctx.free(st_dev); sim.ctx.free(rf_dev)
        img = sim.bmode(0, dynamic_range_db=50.0)
        assert img.shape == (400, 500) and img.max() > 200
    finally:
        sim.close()


def test_a_two_rank_group_equals_one_context(mcrt, sphere, tex256):
    cfg, sd = sphere
    E, S, K, F = 16, 32, 3, 2
    tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    pos, dirs, _ = tr.planes(K, PITCH_UM)
    pos, dirs = np.tile(pos, (F, 1, 1)), np.tile(dirs, (F, 1, 1))
    one = mcrt.Context(0); _setup(one, sd, tr, S, tex256)
    grp = mcrt.Group([0, 0]); _setup(grp, sd, tr, S, tex256)
    try:
        R = one.params.n_rows
        w = mcrt.host_psf_elevation(VAR_Z, PITCH_UM, R, mcrt.row_pitch_mm(tr.frequency), (), 20.0, K, True)
        out = []
        for tracer, c in ((one, one), (grp, grp.root)):
            st_dev, rf_dev = c.alloc(F * K * E * R * 4), c.alloc(F * E * R * 4)
            tracer.trace_frames_poses(5 * K, pos, dirs, st_dev)
            c.elevation_frames(st_dev, F, K, E, R, w, rf_dev)
            tracer.synchronize()
            out.append((c.d2h(st_dev, (F, K, E, R)), c.d2h(rf_dev, (F, E, R))))
            c.free(st_dev); c.free(rf_dev)
        assert np.array_equal(out[0][0].view(np.uint32), out[1][0].view(np.uint32))
        assert np.array_equal(out[0][1].view(np.uint32), out[1][1].view(np.uint32)) and np.abs(np.nan_to_num(out[0][1])).sum() > 0
        ic.assert_same_bits(out[1][1], em.fold(out[1][0], w), "the group's fold vs the mirror")
    finally:
        grp.close(); one.close()


# ------------------------------------------------------------------ the C++ shim and the CLI
def _write_scene(mcrt, tmp_path):
    cfg, meshes = mcrt.synth.sphere_scene(3)
    meshes["SPHERE.obj"] = mcrt.synth.icosphere(3, 2.0, center=(0.0, 0.0, 2.3))
    cfg["workingDirectory"] = str(tmp_path) + "/"
    for f, (V, F) in meshes.items():
        mcrt.scene_io.save_obj(str(tmp_path / f), V, F)
    (tmp_path / "beside.scene").write_text(json.dumps(cfg))
    return cfg, str(tmp_path / "beside.scene")


def _build_driver(tmp_path):
    pkg = os.path.join(ROOT, "mcray-tracing_amd")
    exe = str(tmp_path / "elevation_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(pkg, "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "elevation_driver.cpp"), "-L", pkg, "-lmcrt_hip", "-Wl,-rpath," + pkg])
    return exe


@pytest.mark.parametrize("n_planes,devices", [(0, None), (3, "0,0")])
def test_host_shim(mcrt, tmp_path, n_planes, devices):
    """rf_image::trace(frame) and rf_image::trace(frame, transducer, psf) write the images Python's Simulator produces, bit for bit --
    on one context and on a two-rank group"""
    exe = _build_driver(tmp_path)
    cfg, scene = _write_scene(mcrt, tmp_path)
    out = tmp_path / "elev.bin"
    E, R, S, frame, K = 64, 465, 8, 3, n_planes or 7
    r = subprocess.run([exe, scene, str(out), str(frame), str(S), repr(VAR_Z), str(PITCH_UM), str(n_planes)] + (["--devices", devices] if devices else []),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    both = np.fromfile(str(out), f32).reshape(2, R, E)
    sd = mcrt.scene_io.load_scene_file(scene)
    tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    psf = mcrt.Psf(freq=tr.frequency, var_z=VAR_Z, elevation_size=K, elevation_pitch_um=PITCH_UM)
    for elevation, img in ((False, both[0]), (True, both[1])):
        sim = mcrt.Simulator(sd, tr, n_samples=S, psf=psf, elevation=elevation)
        try:
            ic.assert_same_bits(img, sim.frame(frame, convolve=False), "shim vs python, elevation=%s" % elevation)
        finally:
            sim.close()
    assert np.count_nonzero(both[0]) > 1000 and not np.array_equal(both[0], both[1])


def test_cli_elevation_options(mcrt, tmp_path):
    exe = os.path.join(ROOT, "mcray-tracing_amd", "mattausch_hip")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "mcray-tracing_amd"), "mattausch_hip"])
    _, scene = _write_scene(mcrt, tmp_path)

    def run(name, *opts):
        r = subprocess.run([exe, scene, "2", "5", str(tmp_path / (name + ".pgm")), str(tmp_path / (name + ".bin"))] + list(opts),
                           capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout + r.stderr
        return (tmp_path / (name + ".pgm")).read_bytes(), np.fromfile(str(tmp_path / (name + ".bin")), f32)

    def same(a, b):
        return a[0] == b[0] and a[1].shape == b[1].shape and np.array_equal(a[1], b[1], equal_nan=True)

    plain = run("plain")
    assert same(run("one", "--elevation", "1"), plain)                     # one plane at z = 0, weight 1, frame id f
    assert same(run("one_wide", "--elevation", "1", "--elevation-pitch-um", "900", "--var-z", "4"), plain)
    unused = run("unused", "--elevation-pitch-um", "900", "--var-z", "4")
    assert unused[0] == plain[0] and unused[1].tobytes() == plain[1].tobytes()     # without --elevation: byte for byte
    seven = run("seven", "--elevation", "7", "--elevation-pitch-um", str(PITCH_UM), "--var-z", str(VAR_Z))
    assert len(seven[0]) == len(plain[0]) and seven[0] != plain[0] and not np.array_equal(seven[1], plain[1], equal_nan=True)
    assert run("seven_default", "--elevation", "7")[0] != plain[0]
    assert run("seven_db", "--elevation", "7", "--db", "60")[0] != run("db", "--db", "60")[0]
    for bad in ("4", "33", "0", "-3"):
        r = subprocess.run([exe, scene, "1", "5", "--elevation", bad], capture_output=True, text=True, timeout=240)
        assert r.returncode == 1 and "--elevation" in r.stdout, (bad, r.stdout)
