"""Acoustic ground truth without a GPU: the ABI (symbols, mcrt_transmit_opts and its defaults), mcrt_transmit_boundary -- host code -- against
the numpy mirror's boundary arithmetic bit for bit, the properties of the contract on a scene whose answer is known (two concentric
spheres, LIVER around BONE, through tests/transmit_mirror.py on the CPU oracle's closest hit), a sheet at normal incidence against the
closed form, and the CLI's option errors.  The kernel is tests/test_gpu_transmit.py's."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest

import label_mirror as lm
import transmit_mirror as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NEW = ("mcrt_default_transmit_opts", "mcrt_transmit_boundary", "mcrt_transmit_frames")
R = 465


def test_symbols_exported_and_declared(mcrt):
    L = mcrt.load_library()
    hdr = open(os.path.join(ROOT, "include", "mcrt.h")).read()
    lib_mod = __import__("mcray_tracing_amd._lib", fromlist=["SYMBOLS"])
    for n in NEW:
        assert hasattr(L, n) and n in lib_mod.SYMBOLS and re.search(r"\bint " + n + r"\(", hdr), n
        assert getattr(L, n).argtypes is not None, n
    assert len(L.mcrt_transmit_frames.argtypes) == 10 and len(L.mcrt_transmit_boundary.argtypes) == 6
    assert L.mcrt_version() == 109
    block = hdr[hdr.index("#define MCRT_VERSION 109"):hdr.index("typedef enum {")]
    assert "mcrt_transmit_frames" in block and "additive" in block[block.index("mcrt_transmit_frames"):]


def test_transmit_opts_layout_and_defaults(mcrt):
    from mcray_tracing_amd import TransmitOpts
    assert C.sizeof(TransmitOpts) == 12
    assert (TransmitOpts.mode.offset, TransmitOpts.rule.offset, TransmitOpts.start_offset.offset) == (0, 4, 8)
    o = TransmitOpts(9, 7, 3.0)
    assert mcrt.load_library().mcrt_default_transmit_opts(C.byref(o)) == 0
    assert (o.mode, o.rule, o.start_offset) == (0, 0, -1.0)
    assert mcrt.load_library().mcrt_default_transmit_opts(None) == -1 and b"null options" in mcrt.load_library().mcrt_last_error()
    o = mcrt.transmit_opts_struct("boundaries", "geometric", 1e-3)
    assert (o.mode, o.rule, o.start_offset) == (1, 1, f32(1e-3))
    hdr = open(os.path.join(ROOT, "include", "mcrt.h")).read()
    assert re.search(r"MCRT_TRANSMIT_TOTAL = 0,", hdr) and re.search(r"MCRT_TRANSMIT_BOUNDARIES = 1 \}", hdr)
    assert (mcrt.TRANSMIT_MODES["total"], mcrt.TRANSMIT_MODES["boundaries"]) == (tm.TOTAL, tm.BOUNDARIES)


def _bits(x):
    return np.asarray(x, f32).view(np.uint32)


def test_boundary_rule_equals_the_mirror_bit_for_bit(mcrt):
    """a few thousand random crossings, with total internal reflection, equal impedances (nothing turned back) and inc == 0 among them"""
    L = mcrt.load_library()
    rng = np.random.default_rng(5)
    n = 3000
    z1 = rng.uniform(4e-4, 8.0, n).astype(f32); z2 = rng.uniform(4e-4, 8.0, n).astype(f32)
    inc = rng.uniform(0.0, 1.0, n).astype(f32); ia = rng.uniform(0.0, 1.0, n).astype(f32)
    z2[:200] = z1[:200]                                   # Z1 == Z2: nothing is turned back ...
    inc[:100] = 1.0; inc[100:200] = rng.uniform(0.1, 1.0, 100).astype(f32)
    inc[200:300] = 0.0; inc[300:320] = -0.0               # a grazing beam
    z1[320:700] = f32(7.8); z2[320:700] = rng.uniform(1.3, 2.0, 380).astype(f32)      # out of bone: total internal reflection below the critical angle
    ia[700:720] = 0.0
    inc[720:740] = 1.0
    z1[740] = 0.0; z2[741] = 0.0; z1[742] = z2[742] = 0.0; ia[743] = np.inf; inc[744] = np.nan      # the non-finite corners: the same bits too
    tir = same_z = 0
    for k in range(n):
        want = tm.boundary(z1[k], z2[k], inc[k], ia[k])
        a, b = C.c_float(), C.c_float()
        assert L.mcrt_transmit_boundary(z1[k], z2[k], inc[k], ia[k], C.byref(a), C.byref(b)) == 0
        got = (f32(a.value), f32(b.value))
        assert (_bits(got[0]), _bits(got[1])) == (_bits(want[0]), _bits(want[1])), (k, z1[k], z2[k], inc[k], ia[k], got, want)
        assert mcrt.transmit_boundary(z1[k], z2[k], inc[k], ia[k]) == got or k >= 740
        if k < 100:                                       # ... exactly at normal incidence (refa == 1 == inc: num == 0)
            assert got[0] == 0.0 and got[1] == ia[k]
            same_z += 1
        elif k < 200:
            # ... and to rounding at an oblique one: refa^2 = 1 - (1 - inc^2) is inc^2 to within 1.5 * 2^-24 absolute, so |inc - refa| <= 2^-24 / inc and
            # |qq| <= 2^-25 / inc^2 <= 3e-6 for inc >= 0.1: i_refl <= 1e-11 Ia
            assert 0.0 <= got[0] <= 1e-11 * ia[k] and got[1] == f32(ia[k] - got[0])
            same_z += 1
        if 320 <= k < 700 and got[1] == 0.0 and got[0] == ia[k] and ia[k] > 0:
            tir += 1
    assert same_z == 200 and tir >= 100
    assert L.mcrt_transmit_boundary(1.0, 2.0, 1.0, 1.0, None, C.byref(C.c_float())) == -1 and b"i_refl" in L.mcrt_last_error()
    assert L.mcrt_transmit_boundary(1.0, 2.0, 1.0, 1.0, C.byref(C.c_float()), None) == -1 and b"i_refr" in L.mcrt_last_error()


def test_boundary_rule_runs_clean_under_asan_ubsan(tmp_path):
    """the host code as a stand-alone program (tests/host/transmit_sanitize_driver.cpp + csrc/mcrt_host.cpp, no GPU, nothing loaded into
    Python): the sanitized build gives the mirror's bits, the non-finite corners included"""
    pkg = os.path.join(ROOT, "mcray-tracing_amd")
    exe = str(tmp_path / "transmit_sanitize_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
                           "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "host", "transmit_sanitize_driver.cpp"),
                           os.path.join(pkg, "csrc", "mcrt_host.cpp")])
    rng = np.random.default_rng(11)
    n = 400
    q = np.stack([rng.uniform(4e-4, 8.0, n), rng.uniform(4e-4, 8.0, n), rng.uniform(0.0, 1.0, n), rng.uniform(0.0, 1.0, n)], 1).astype(f32)
    q[:8] = [[0, 1, 1, 1], [1, 0, 1, 1], [0, 0, 0, 0], [1, 2, np.nan, 1], [1, 2, 1, np.inf], [np.inf, np.inf, 1, 1], [7.8, 1.5, 0.2, 1], [3e38, 1e-38, 1, 3e38]]
    cases = tmp_path / "cases.txt"
    cases.write_text("".join("%08x %08x %08x %08x\n" % tuple(int(w) for w in row.view(np.uint32)) for row in q))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, str(cases)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("DONE"), r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.split()[:-1]
    assert len(lines) == 2 * n
    for k in range(n):
        want = tm.boundary(*q[k])
        assert (int(lines[2 * k], 16), int(lines[2 * k + 1], 16)) == (int(_bits(want[0])), int(_bits(want[1]))), (k, q[k], want)


@pytest.fixture(scope="module")
def spheres(mcrt, orc):
    """LIVER (radius 3 cm) around BONE (1.5 cm), nine beams over +-0.35 rad: 0 and 8 graze the liver, 1 and 7 cross only the liver shell,
    2, 3, 5, 6 leave the bone obliquely, 4 runs through its middle"""
    sd = lm.spheres_scene(mcrt, 3)
    osc = lm.oracle_scene(orc, sd)
    pos, dirs = lm.fan(9, 0.35, dz=0.01)
    out = {"sd": sd, "osc": osc, "pos": pos, "dirs": dirs}
    for mode in (tm.TOTAL, tm.BOUNDARIES):
        detail = [[] for _ in range(9)]
        rows = [tm.walk(osc, orc, pos[e], dirs[e], R, mode=mode, detail=detail[e]) for e in range(9)]
        out[mode] = (np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), np.array([r[2] for r in rows], np.uint32), detail)
    return out


def test_spheres_row_zero_and_monotony(spheres):
    for mode in (tm.TOTAL, tm.BOUNDARIES):
        T, Rf, c, _ = spheres[mode]
        assert (_bits(T[:, 0]) == _bits(f32(1.0))).all()
        assert (np.diff(T.astype(np.float64), axis=1) <= 0).all() and (T >= 0).all() and np.isfinite(T).all()
        assert (Rf >= 0).all() and (Rf <= 1).all()
    assert spheres[tm.TOTAL][2].tolist() == [2, 2, 4, 4, 4, 4, 4, 2, 2]


def test_spheres_shadow_behind_the_bone(spheres):
    """the beam through the bone core ends below 1e-3 of the beam that only crosses the liver shell: the shadow"""
    T = spheres[tm.TOTAL][0]
    assert 0 < T[4, -1] < 1e-3 * T[1, -1] and T[1, -1] == T[7, -1]
    assert 1e-6 < T[4, -1] < 3e-6 and 0.03 < T[1, -1] < 0.05


def test_spheres_total_internal_reflection_and_grazing(spheres):
    """beams that leave the bone obliquely end at exactly 0; a grazing first contact turns everything back: reflect == 1.0 in its row, zeros behind"""
    T, Rf, c, detail = spheres[tm.TOTAL]
    for e in (2, 3, 5, 6):
        # (TRACED keeps BONE behind the inner sphere: the total internal reflection is at the outer sphere's far wall, BONE -> LIVER)
        tir = [j for j, (b, ia, i_refl, behind) in enumerate(detail[e]) if i_refl == ia > 0 and behind == 0.0]
        assert T[e, -1] == 0.0 and len(tir) == 1 and int(c[e]) == 4, e      # i_refl == Ia: nothing goes on
        assert (T[e, detail[e][tir[0]][0]:] == 0.0).all() and T[e, detail[e][tir[0]][0] - 1] > 0
    for e in (0, 8):
        row = detail[e][0][0]
        assert Rf[e, row] == 1.0 and np.count_nonzero(Rf[e]) == 1 and (T[e, :row] == 1.0).all() and (T[e, row:] == 0.0).all(), e
        assert int(c[e]) == 2


def test_spheres_boundaries_mode_is_the_running_product(spheres):
    T, Rf, c, detail = spheres[tm.BOUNDARIES]
    for e in range(9):
        I, b_prev = f32(1.0), 0
        for b, ia, i_refl, behind in detail[e]:
            assert ia == I and (T[e, b_prev:b] == I).all(), e          # nothing is lost between boundaries
            i_refr = f32(ia - i_refl) if i_refl != ia else f32(0.0)
            I = i_refr if i_refr > 0 else f32(0.0)
            assert behind == I
            b_prev = b
        assert (T[e, b_prev:] == I).all()
        assert len(np.unique(T[e])) <= len(detail[e]) + 1


def test_a_beam_that_misses_is_the_start_medium_alone(mcrt, orc, spheres):
    osc = spheres["osc"]
    pos, dirs = lm.fan(1, 0.0)
    T, Rf, c = tm.walk(osc, orc, pos[0], -dirs[0], R)
    assert c == 0 and not Rf.any()
    const = orc.constants(4.5, 1500, 15.0)
    att = f32(osc.mat[int(osc.c.start_mat), tm.M_ATT])
    want = [tm.attenuated(orc.lib().orc_expf, f32(1.0), att, (r * const.row_dt_us * 1500.0) / 1000.0, f32(4.5)) for r in range(R)]
    tm.same_bits(T, np.array(want, f32), "a miss")
    Tb, _, _ = tm.walk(osc, orc, pos[0], -dirs[0], R, mode=tm.BOUNDARIES)
    assert (Tb == 1.0).all()


def test_crossings_are_the_label_walks(orc, spheres):
    osc, pos, dirs = spheres["osc"], spheres["pos"], spheres["dirs"]
    for rule, offs in ((lm.TRACED, 0.1), (lm.GEOMETRIC, 1e-3)):
        want = lm.label_frames(osc, orc, pos, dirs, R, rule=rule, offs=offs)
        got = tm.transmit_frames(osc, orc, pos, dirs, R, rule=rule, offs=offs)
        assert np.array_equal(got[2], want[2]), rule
        assert ((got[1] != 0) <= (want[1] >= 0)).all()          # a row that turns something back holds an interface


def _ulps(a, b):
    a, b = f32(a), f32(b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


def test_one_sheet_at_normal_incidence_is_the_closed_form(mcrt, orc):
    """reflect in the sheet's row = ((Z1 - Z2) / (Z1 + Z2))^2 Ia, within 4 ulp of the closed form evaluated in double: inc, rr, refa and the
    quotient each round once in float (four operations), the closed form none"""
    for mat in ("LIVER", "BONE", "FAT"):
        sd = lm.sheets_scene(mcrt, [5.0], materials=(mat,))
        osc = lm.oracle_scene(orc, sd)
        pos, dirs = lm.fan(1, 0.0)
        detail = []
        T, Rf, c = tm.walk(osc, orc, pos[0], dirs[0], R, detail=detail)
        assert c == 1 and len(detail) == 1
        row, ia, i_refl, behind = detail[0]
        assert abs(row - 5.0 * 10 / 0.322) <= 1 and np.count_nonzero(Rf) == 1 and Rf[row] == i_refl
        z1 = float(osc.mat[int(osc.c.start_mat), tm.M_IMP]); z2 = float(osc.mat[sd.material_names.index(mat), tm.M_IMP])
        closed = ((z1 - z2) / (z1 + z2)) ** 2 * float(ia)
        assert _ulps(i_refl, f32(closed)) <= 4, (mat, i_refl, closed)
        assert behind == f32(ia - i_refl) and T[row] == behind
        # the host's rule on the same numbers
        assert mcrt.transmit_boundary(z1, z2, 1.0, ia)[0] == i_refl


def test_cli_transmission_option_errors(mcrt):
    """bad values exit 1 with a message, before the scene file is opened, as the other options do"""
    exe = os.path.join(ROOT, "mcray-tracing_amd", "mattausch_hip")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "mcray-tracing_amd"), "mattausch_hip"], stdout=subprocess.DEVNULL)
    cases = [(["--transmission-mode", "total"], "--transmission-mode needs --transmission"), (["--transmission-db", "40"], "--transmission-db needs --transmission"),
             (["--transmission", "x.pgm", "--transmission-mode", "all"], "--transmission-mode takes total or boundaries"),
             (["--transmission", "x.pgm", "--transmission-db", "0"], "--transmission-db takes a finite range > 0"),
             (["--transmission", "x.pgm", "--transmission-db", "nan"], "--transmission-db takes a finite range > 0"),
             (["--transmission", "x.pgm", "--label-rule", "anatomy"], "--label-rule takes traced or geometric")]
    for args, msg in cases:
        r = subprocess.run([exe, "/nonexistent/scene.json", "1", "1"] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and msg in r.stdout, (args, r.stdout, r.stderr)
