"""Ground-truth label maps without a GPU: the ABI (symbols, version, mcrt_label_opts and its defaults), the two medium rules on a scene with a
closed-form answer -- two concentric spheres, through the numpy mirror (tests/label_mirror.py) on the CPU oracle's closest hit --, the
nearest-neighbour rule of the gathers, and the CLI's option errors.  The kernels are tests/test_gpu_label.py's."""
import ctypes as C
import math
import os
import re
import subprocess
import numpy as np

import label_mirror as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NEW = ("mcrt_default_label_opts", "mcrt_label_frames", "mcrt_label_scan_convert_frames", "mcrt_label_volume_frames")


def test_symbols_exported_and_declared(mcrt):
    L = mcrt.load_library()
    hdr = open(os.path.join(ROOT, "include", "mcrt.h")).read()
    lib_mod = __import__("mcray_tracing_amd._lib", fromlist=["SYMBOLS"])
    for n in NEW:
        assert hasattr(L, n) and n in lib_mod.SYMBOLS and re.search(r"\bint " + n + r"\(", hdr), n
        assert getattr(L, n).argtypes is not None, n
    assert len(L.mcrt_label_frames.argtypes) == 10 and len(L.mcrt_label_scan_convert_frames.argtypes) == 10 and len(L.mcrt_label_volume_frames.argtypes) == 10


def test_version_is_still_109_and_the_addition_is_recorded(mcrt):
    assert mcrt.load_library().mcrt_version() == 109
    hdr = open(os.path.join(ROOT, "include", "mcrt.h")).read()
    block = hdr[hdr.index("#define MCRT_VERSION 109"):hdr.index("typedef enum {")]
    assert "mcrt_label_frames" in block and "additive" in block[block.index("mcrt_label_frames"):]


def test_label_opts_layout_and_defaults(mcrt):
    from mcray_tracing_amd import LabelOpts
    assert C.sizeof(LabelOpts) == 8 and LabelOpts.rule.offset == 0 and LabelOpts.start_offset.offset == 4
    o = LabelOpts(7, 3.0)
    assert mcrt.load_library().mcrt_default_label_opts(C.byref(o)) == 0
    assert o.rule == 0 and o.start_offset == -1.0
    assert mcrt.load_library().mcrt_default_label_opts(None) == -1
    o = mcrt.label_opts_struct("geometric", 1e-3)
    assert o.rule == 1 and o.start_offset == f32(1e-3)
    assert mcrt.label_opts_struct().start_offset == -1.0
    hdr = open(os.path.join(ROOT, "include", "mcrt.h")).read()
    assert re.search(r"MCRT_LABEL_TRACED = 0, MCRT_LABEL_GEOMETRIC = 1", hdr) and re.search(r"#define MCRT_LABEL_NONE 255u", hdr)
    assert re.search(r"#define MCRT_LABEL_MAX_CROSSINGS 64u", hdr)
    assert (mcrt.LABEL_NONE, mcrt.LABEL_MAX_CROSSINGS, mcrt.LABEL_CAPPED) == (lm.NONE, lm.MAX_CROSSINGS, lm.CAPPED) == (255, 64, 1 << 31)


def _chord(u, centre, r):
    """path lengths [cm] at which the beam from the origin along the unit vector u enters and leaves the sphere"""
    b = float(np.dot(u, centre)); disc = b * b - float(np.dot(centre, centre)) + r * r
    assert disc > 0
    return b - math.sqrt(disc), b + math.sqrt(disc)


def test_concentric_spheres_have_the_closed_form_rows(mcrt, orc):
    """GEOMETRIC: GEL | LIVER | BONE | LIVER | GEL with the boundaries at the spheres' radii, to +-1 row (the faceted spheres are within
    0.03 mm of the true ones, a row is 0.322 mm).  TRACED keeps BONE behind the inner sphere (quirk 1: leaving a non-vascular mesh keeps
    its mat_inside) and LIVER behind the outer one: it does not return to the outer tissue."""
    sd = lm.spheres_scene(mcrt, 4)
    osc = lm.oracle_scene(orc, sd)
    names = sd.material_names
    GEL, LIVER, BONE = names.index("GEL"), names.index("LIVER"), names.index("BONE")
    R = 465
    pos, dirs = lm.fan(5, 0.15)
    row_mm = 322.0 / 1000.0
    geo = lm.label_frames(osc, orc, pos, dirs, R, rule=lm.GEOMETRIC, offs=1e-3)
    tra = lm.label_frames(osc, orc, pos, dirs, R, rule=lm.TRACED, offs=0.1)
    centre = np.asarray(lm.SPHERES_CENTRE)
    for e in range(5):
        u = dirs[e].astype(np.float64)
        o0, o1 = _chord(u, centre, lm.SPHERES_OUTER); i0, i1 = _chord(u, centre, lm.SPHERES_INNER)
        want_rows = [d * 10.0 / row_mm for d in (o0, i0, i1, o1)]
        t = geo[0][e].astype(int)
        change = np.flatnonzero(np.diff(t)) + 1
        assert len(change) == 4 and all(abs(c - w) <= 1.0 for c, w in zip(change, want_rows)), (e, change, want_rows)
        assert [t[0]] + [t[c] for c in change] == [GEL, LIVER, BONE, LIVER, GEL], e
        assert int(geo[2][e]) == 4 and int(tra[2][e]) == 4
        assert np.array_equal(np.flatnonzero(geo[1][e] >= 0), change) and [int(geo[1][e][c]) for c in change] == [0, 1, 1, 0]
        # the tracer's media: the same boundaries, BONE up to the outer sphere's far wall, LIVER behind it
        tt = tra[0][e].astype(int)
        tchange = np.flatnonzero(np.diff(tt)) + 1
        assert [tt[0]] + [tt[c] for c in tchange] == [GEL, LIVER, BONE, LIVER], e
        assert np.array_equal(np.flatnonzero(tra[1][e] >= 0), np.flatnonzero(geo[1][e] >= 0))
        assert tt[-1] == LIVER and t[-1] == GEL and (tt[change[2]:change[3]] == BONE).all()


def test_reference_scenes_terminate_and_show_both_vascular_branches(mcrt, orc):
    """sphere_scene: from the sphere's row on the whole line is BONE (quirk 1); liver_scene: several tissues, vascular meshes among the interfaces"""
    cfg, meshes = mcrt.synth.sphere_scene(2)
    sd = mcrt.scene_io.build_scene(cfg, meshes)
    tr = mcrt.Transducer(16, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    t, i, c = lm.label_frames(lm.oracle_scene(orc, sd), orc, tr.pos, tr.dir, 465)
    BONE = sd.material_names.index("BONE")
    assert 1 <= c.min() and c.max() <= 3
    for e in np.flatnonzero((i == 1).any(axis=1)):
        assert (t[e, np.flatnonzero(i[e] == 1)[0]:] == BONE).all()
    cfg, meshes = mcrt.synth.liver_scene(2)
    sd = mcrt.scene_io.build_scene(cfg, meshes)
    tr = mcrt.Transducer(16, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    t, i, c = lm.label_frames(lm.oracle_scene(orc, sd), orc, tr.pos, tr.dir, 465)
    assert 2 <= c.min() and c.max() <= 7 and len(np.unique(t)) >= 5
    vascular = {m for m, rec in enumerate(sd.meshes) if rec[2]}
    assert vascular & set(np.unique(i).tolist()) and (set(np.unique(i).tolist()) - {-1} - vascular)


def test_nearest_rule_of_the_gathers():
    m = np.array([-0.6, -0.5, -0.4, 0.0, 0.49999997, 0.5, 1.5, 2.4999998, 2.5, 3.0, np.nan, np.inf, -np.inf, 1e30, -1e30], f32)
    idx, inside = lm.nearest(m, 3)
    assert inside.tolist() == [False, True, True, True, True, True, True, True, False, False, False, False, False, False, False]
    assert idx[inside].tolist() == [0, 0, 0, 0, 1, 2, 2]
    tissue = np.arange(6, dtype=np.uint8).reshape(2, 3)
    got = lm.scan_convert(tissue, np.array([0.0, 2.6, np.nan, 1.0], f32), np.array([0.0, 1.0, 0.0, 1.4], f32))
    assert got.tolist() == [0, 255, 255, 4]


def test_cli_label_option_errors(mcrt):
    """bad values exit 1 with a message, before the scene file is opened, as the other options do"""
    exe = os.path.join(ROOT, "mcray-tracing_amd", "mattausch_hip")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "mcray-tracing_amd"), "mattausch_hip"], stdout=subprocess.DEVNULL)
    cases = [(["--label-rule", "traced"], "--label-rule needs --labels"), (["--label-offset", "0.01"], "--label-offset needs --labels"),
             (["--labels", "x.pgm", "--label-rule", "anatomy"], "--label-rule takes traced or geometric"),
             (["--labels", "x.pgm", "--label-offset", "0"], "--label-offset takes a finite offset > 0"),
             (["--labels", "x.pgm", "--label-offset", "nan"], "--label-offset takes a finite offset > 0"),
             (["--labels", "x.pgm", "--label-offset", "-1"], "--label-offset takes a finite offset > 0")]
    for args, msg in cases:
        r = subprocess.run([exe, "/nonexistent/scene.json", "1", "1"] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and msg in r.stdout, (args, r.stdout, r.stderr)
