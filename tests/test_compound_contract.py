"""Spatial compounding without a GPU (include/mcrt.h): the steered element table, the steered scan-conversion maps against the forward
geometry they invert, the struct layout, and the tie of tests/compound_mirror.py to the oracle's scan conversion."""
import ctypes as C
import math
import numpy as np
import pytest

import compound_mirror as cm
import image_cases as ic

E, R = 128, 465
STEERS = (0.1, -0.1, 0.3, -0.3, 0.5)
GEOMETRIES = ic.SCAN_GEOMETRIES


def rotate(v, axis, ang):
    """Rodrigues' rotation of the rows of v about the unit vector axis, in double"""
    v = np.asarray(v, np.float64); k = np.asarray(axis, np.float64)
    return v * math.cos(ang) + np.cross(k, v) * math.sin(ang) + np.outer(v @ k, k) * (1 - math.cos(ang))


# ------------------------------------------------------------------ mcrt_transducer_steered
@pytest.mark.parametrize("angles", [(0, 0, 0), (20, -35, 50)])
def test_steered_table(mcrt, angles):
    tr = mcrt.Transducer(n_elements=64, position=(1.0, -2.0, 0.5), angles_deg=angles)
    args = (tr.n_elements, tr.radius_cm, tr.separation_mm, tr.position, tr.angles)
    p0, d0 = mcrt.host_transducer(*args)
    ps, ds = mcrt.host_transducer_steered(*args, 0.0)
    assert p0.tobytes() == ps.tobytes() and d0.tobytes() == ds.tobytes()          # steer 0: mcrt_transducer_elements bit for bit
    axis = mcrt.host_elevation_axis(angles).astype(np.float64)
    for s in (0.25, -0.4, 1.2):
        ps, ds = mcrt.host_transducer_steered(*args, s)
        assert ps.tobytes() == p0.tobytes()                                       # the beams pivot on their elements
        # local frame (sin a, cos a, 0), elevation z: a larger angle is a rotation by -s about z, whatever the probe's pose
        want = rotate(d0, axis, -float(np.float32(s)))
        assert np.abs(ds - want).max() <= 2e-6, (s, np.abs(ds - want).max())
        assert np.abs(np.linalg.norm(ds.astype(np.float64), axis=1) - 1).max() < 1e-6
    # a positive steer tilts towards higher element numbers: the direction gains a component along the arc's tangent e(last) - e(first)
    _, ds = mcrt.host_transducer_steered(*args, 0.3)
    along = (p0[-1] - p0[0]).astype(np.float64)
    assert np.all((ds - d0).astype(np.float64) @ along > 0)
    pos, dirs = tr.steered((-0.15, 0.0, 0.15))
    assert pos.shape == dirs.shape == (3, 64, 3) and dirs[1].tobytes() == d0.tobytes() and pos[2].tobytes() == p0.tobytes()


def test_steered_table_errors(mcrt):
    L = mcrt.load_library()
    pos = np.full((4, 3), 7.0, np.float32); d = np.full((4, 3), 7.0, np.float32)
    p = np.zeros(3, np.float32); a = np.zeros(3, np.float32)
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)
    bad = [(0, ptr(p), ptr(a), 0.1, ptr(pos), ptr(d)), (4, None, ptr(a), 0.1, ptr(pos), ptr(d)), (4, ptr(p), None, 0.1, ptr(pos), ptr(d)),
           (4, ptr(p), ptr(a), 0.1, None, ptr(d)), (4, ptr(p), ptr(a), 0.1, ptr(pos), None)]
    bad += [(4, ptr(p), ptr(a), s, ptr(pos), ptr(d)) for s in (math.nan, math.inf, -math.inf, math.pi / 2, -math.pi / 2, 2.0, -1.6)]
    for n, pp, aa, s, po, do in bad:
        assert L.mcrt_transducer_steered(n, 3.0, 0.5, pp, aa, s, po, do) == -1, (n, s)
        assert b"mcrt_transducer_steered" in L.mcrt_last_error()
        assert np.all(pos == 7.0) and np.all(d == 7.0)
    assert L.mcrt_transducer_steered(4, 3.0, 0.5, ptr(p), ptr(a), 1.5, ptr(pos), ptr(d)) == 0


# ------------------------------------------------------------------ mcrt_compound_maps
def grid_mm(radius_mm, total_angle, rows, cols, max_travel_us=100, sos=1500):
    """the pixel positions (x, y) [mm from the arc's centre] in double, from mcrt_scan_maps' float statements, and depth_mm"""
    f32 = np.float32
    radius_f = f32(radius_mm); ta_f = f32(total_angle)
    depth = f32(f32(max_travel_us * sos) * f32(0.001))
    ratio = f32((float(f32(depth + radius_f)) - float(radius_f) * math.cos(float(ta_f) / 2.0)) / rows)
    shift_y = radius_mm * float(np.cos(f32(ta_f / f32(2.0))))
    fi = (np.arange(rows, dtype=f32) + f32(f32(shift_y) / ratio)).astype(f32)
    fj = (np.arange(cols, dtype=f32) - f32(f32(cols) / f32(2.0))).astype(f32)
    x = np.broadcast_to(fj.astype(np.float64)[None, :] * float(ratio), (rows, cols))
    y = np.broadcast_to(fi.astype(np.float64)[:, None] * float(ratio), (rows, cols))
    return x, y, float(depth)


@pytest.mark.parametrize("geom", ic.SCAN_GEOMETRIES)
def test_steer_zero_is_scan_maps(mcrt, geom):
    radius, angle, rows, cols = geom
    for e, r in ic.SCAN_SHAPES + [(E, R)]:
        a = mcrt.host_scan_maps(e, r, radius, angle, out_rows=rows, out_cols=cols)
        for z in (0.0, -0.0):
            b = mcrt.host_compound_maps(e, r, z, radius, angle, out_rows=rows, out_cols=cols)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("geom", GEOMETRIES)
@pytest.mark.parametrize("steer", STEERS)
def test_maps_invert_the_forward_geometry(mcrt, geom, steer):
    """every pixel with finite maps, pushed back through P = radius u(phi) + t u(phi + steer) in double, lands within 2e-4 mm of itself
    (ten times what the issue's numpy evaluation measured; float rounding of a row coordinate below 2048 is 4e-5 mm); NaN exactly
    where rho < |q|"""
    radius, angle, rows, cols = geom
    mr, mc = mcrt.host_compound_maps(E, R, steer, radius, angle, out_rows=rows, out_cols=cols)
    x, y, depth = grid_mm(radius, angle, rows, cols)
    s = float(np.float32(steer))
    rho = np.sqrt(x * x + y * y)
    no_beam = rho < abs(radius * math.sin(s))
    assert np.array_equal(np.isnan(mr), no_beam) and np.array_equal(np.isnan(mc), no_beam)
    ok = ~no_beam
    t = mr.astype(np.float64) / R * depth
    phi = mc.astype(np.float64) / float(np.float32(E)) * angle - angle / 2
    px = radius * np.sin(phi) + t * np.sin(phi + s)
    py = radius * np.cos(phi) + t * np.cos(phi + s)
    err = np.hypot(px - x, py - y)[ok]
    print("geometry %s steer %+.2f: worst round trip %.3g mm, %d pixels without a beam" % (geom, steer, err.max(), int(no_beam.sum())))
    assert err.max() <= 2e-4, err.max()
    if geom == ic.SCAN_GEOMETRIES[0]:
        assert not no_beam.any()                        # the default geometry has a beam through every pixel for |steer| <= 0.5
    if geom == ic.SCAN_GEOMETRIES[3] and steer == 0.5:
        assert no_beam.any()


@pytest.mark.parametrize("geom", GEOMETRIES)
def test_maps_are_symmetric(mcrt, geom):
    """the maps of -steer are the left-right mirror of those of +steer: pixel column j <-> cols - j (fj -> -fj), scan-line coordinate
    c <-> E - c, to 1e-3 of a coordinate"""
    radius, angle, rows, cols = geom
    for steer in (0.1, 0.3, 0.5):
        pr, pc = mcrt.host_compound_maps(E, R, steer, radius, angle, out_rows=rows, out_cols=cols)
        nr, nc = mcrt.host_compound_maps(E, R, -steer, radius, angle, out_rows=rows, out_cols=cols)
        if cols == 1:                                   # one column: fj = -0.5 has no mirror pixel in the picture (that would be fj = +0.5); compare its
            x, y, depth = grid_mm(radius, angle, rows, cols)          # maps with the mirrored pixel's own inverse, evaluated here in double
            rho = np.hypot(x, y); q = radius * math.sin(-float(np.float32(steer)))
            phi = np.arctan2(-x, y) + float(np.float32(steer)) + np.arcsin(q / rho)
            t = np.sqrt(rho * rho - q * q) - radius * math.cos(float(np.float32(steer)))
            assert np.abs(pr - t / depth * R).max() <= 1e-3 and np.abs(pc - (np.float32(E) - (phi + angle / 2) / angle * E)).max() <= 1e-3
            assert np.abs(nr - pr).max() > 0 or np.abs(nc - pc).max() > 0
            continue
        a_r, a_c = pr[:, 1:], pc[:, 1:]                 # column j = 1 .. cols-1  <->  cols - j = cols-1 .. 1
        b_r, b_c = nr[:, 1:][:, ::-1], nc[:, 1:][:, ::-1]
        assert np.array_equal(np.isnan(a_r), np.isnan(b_r))
        # a pixel straight behind the arc's centre (x = 0, y < 0; only where total_angle > pi puts rows there) is its own mirror image and
        # lies on atan2's cut: alpha = +pi for either sign of the steer, so its two scan-line coordinates differ by a whole turn.  It is
        # more than half a turn outside the sector; every other pixel is compared
        x, y, _ = grid_mm(radius, angle, rows, cols)
        ok = ~np.isnan(a_r) & ~((x == 0) & (y < 0))[:, 1:]
        assert np.abs(a_r[ok] - b_r[ok]).max() <= 1e-3 and np.abs(a_c[ok] - (np.float32(E) - b_c[ok])).max() <= 1e-3


def test_map_errors(mcrt):
    L = mcrt.load_library()
    mr = np.full((4, 5), 7.0, np.float32); mc = np.full((4, 5), 7.0, np.float32)
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)
    good = dict(E=8, R=16, radius=30.0, angle=1.0, rows=4, cols=5, steer=0.1, mr=ptr(mr), mc=ptr(mc))
    for k, v in [("E", 0), ("R", 0), ("rows", 0), ("cols", 0), ("angle", 0.0), ("angle", -1.0), ("angle", math.nan), ("mr", None), ("mc", None),
                 ("steer", math.nan), ("steer", math.inf), ("steer", math.pi / 2), ("steer", -1.6)]:
        a = dict(good); a[k] = v
        assert L.mcrt_compound_maps(a["E"], a["R"], a["radius"], a["angle"], 100, 1500, a["rows"], a["cols"], a["steer"], a["mr"], a["mc"]) == -1, (k, v)
        assert np.all(mr == 7.0) and np.all(mc == 7.0)


# ------------------------------------------------------------------ the struct, the mirror
def test_struct_layout(mcrt):
    cp = mcrt.Compound
    assert C.sizeof(cp) == 68 and cp.n_views.offset == 0 and cp.steer_rad.offset == 4 and cp.steer_rad.size == 64
    s = mcrt.compound_struct((0.5, -0.25))
    assert s.n_views == 2 and s.steer_rad[0] == 0.5 and s.steer_rad[1] == -0.25 and s.steer_rad[2] == 0.0
    assert mcrt.load_library().mcrt_version() == 109


@pytest.mark.parametrize("geom", ic.SCAN_GEOMETRIES)
def test_the_mirror_is_the_oracle_for_one_unsteered_view(mcrt, orc, geom):
    """the mirror's single-view conversion with the unsteered maps equals orc.scan_convert bit for bit; the compound of that one view equals
    it up to -0.0 (0.0f + -0.0f is +0.0f)"""
    radius, angle, rows, cols = geom
    for e, r in [(3, 2), (128, 465), (1, 2048)]:
        img = ic.scan_image(e, r)
        want = orc.scan_convert(np.ascontiguousarray(img.T), radius_mm=radius, total_angle=angle, out_rows=rows, out_cols=cols)
        mr, mc = mcrt.host_compound_maps(e, r, 0.0, radius, angle, out_rows=rows, out_cols=cols)
        ic.assert_same_bits(cm.convert(img, mr, mc), want, "convert %s %s" % (geom, (e, r)))
        got, cnt = cm.compound(img[None], [(mr, mc)])
        ic.assert_same_bits(got, want + np.float32(0.0), "compound %s %s" % (geom, (e, r)))
        # an uncovered pixel has no tap inside: the plain conversion is 0 there as well
        assert np.all(want[cnt == 0] == 0)
