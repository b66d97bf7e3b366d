"""numpy mirror of volume imaging (include/mcrt.h: mcrt_volume_frames, mcrt_bmode_volume_frames), in np.float32: compound_mirror's point and
blend of the scan conversion on the two planes around map_plane, their blend along the sweep, and the 8-bit display built on bmode_mirror's
steps 1-3 and 6.  The maps are an INPUT -- the product's own (mcrt_volume_maps) -- so that libm differences between numpy and the C library
cannot enter the kernel comparisons; tests/test_volume_contract.py checks the maps themselves against the forward geometry.
Also here: the double-precision model of the maps and of the forward geometry, and the grids both test files use."""
import math
import numpy as np

import bmode_mirror as bm
import compound_mirror as cm

f32 = np.float32
DEFAULT_ANGLE = 1.0471975511965976


# ------------------------------------------------------------------ the gather
def plane_taps(stack, z, inside, pt):
    """stack [K][E][R], z the plane per point (int64, any value where not inside) -> v[dy][dx]: the tap inside plane z, 0 elsewhere"""
    ax, ay, x0, y0, mapped = pt
    K, E, R = stack.shape
    zc = np.clip(z, 0, K - 1)
    v = [[None, None], [None, None]]
    for dy in (0, 1):
        for dx in (0, 1):
            xx = x0 + dx; yy = y0 + dy
            ok = inside & mapped & (xx >= 0) & (yy >= 0) & (xx < E) & (yy < R)
            t = stack[zc, np.clip(xx, 0, E - 1), np.clip(yy, 0, R - 1)]
            v[dy][dx] = np.where(ok, t, f32(0)).astype(f32)
    return v


def volume(stack, maps):
    """stack [K][E][R], maps (map_plane, map_row, map_col) of any shape -> float32 of that shape"""
    stack = np.asarray(stack, f32)
    K = stack.shape[0]
    mz, mr, mc = (np.asarray(m, f32) for m in maps)
    pt = cm.remap_point(mc, mr)
    mapped = pt[4] & ~np.isnan(mz)
    with np.errstate(invalid="ignore"):
        fz = np.floor(mz)
        az = (mz - fz).astype(f32)
        zf = np.where(mapped, np.clip(fz, -4, K + 4), -4).astype(np.int64)
    v = []
    for d in (0, 1):
        inside = mapped & (zf + d >= 0) & (zf + d < K)
        v.append(cm.blend(pt, plane_taps(stack, zf + d, inside, pt)))
    with np.errstate(invalid="ignore", over="ignore"):
        return ((v[0] * (f32(1.0) - az)).astype(f32) + (v[1] * az).astype(f32)).astype(f32)


def volume_frames(frames, maps):
    """frames [F][K][E][R] -> float32 [F] + the maps' shape"""
    return np.stack([volume(fr, maps) for fr in np.asarray(frames, f32)])


def bmode_volume(frames, maps, mode="db", dynamic_range_db=60.0, gain_db=0.0, ref=None, tgc_db=None):
    """frames [F][K][E][R] -> (bytes [F] + the maps' shape, refs [F] float32): bmode_mirror's steps 1-3 over the K planes of a frame together
    (one reference: the largest amplitude of the whole sweep), the gather of the grey levels, the quantisation"""
    frames = np.asarray(frames, f32)
    F, K, E, R = frames.shape
    k = bm.tgc_factors(tgc_db, R)
    out = np.zeros((F,) + np.asarray(maps[0]).shape, np.uint8)
    refs = np.zeros(F, f32)
    for f in range(F):
        a = bm.amplitude(frames[f].reshape(K * E, R), k)
        r = f32(ref) if ref is not None and ref > 0 else a.max()
        refs[f] = r
        g = bm.grey(a, r, mode, gain_db, dynamic_range_db).reshape(K, E, R)
        out[f] = bm.quantise(volume(g, maps))
    return out, refs


# ------------------------------------------------------------------ the geometry, in double
def depth_mm(max_travel_us=100, speed_of_sound=1500):
    """mcrt_scan_maps' depth_mm_f as a double"""
    return float(f32(max_travel_us * speed_of_sound) * f32(0.001))


def grid_points(g):
    """the points of an mcrt_volume_grid, double [nw][nv][nu][3]: ((origin + i*du) + j*dv) + l*dw in that order"""
    o, du, dv, dw = (np.array(list(v), np.float64) for v in (g.origin_mm, g.du_mm, g.dv_mm, g.dw_mm))
    i = np.arange(g.nu, dtype=np.float64)[None, None, :, None]; j = np.arange(g.nv, dtype=np.float64)[None, :, None, None]
    l = np.arange(g.nw, dtype=np.float64)[:, None, None, None]
    return ((o + i * du) + j * dv) + l * dw


def maps_model(P, E, R, K, step_rad, pivot_mm, radius_mm, total_angle, depth):
    """include/mcrt.h's formulas of mcrt_volume_maps in numpy double, rounded once: (map_plane, map_row, map_col)"""
    step = float(f32(step_rad)); pivot = float(f32(pivot_mm))
    X, Y, Z = P[..., 0], P[..., 1], P[..., 2]
    h = np.sqrt((Y - pivot) ** 2 + Z ** 2); theta = np.arctan2(Z, Y - pivot)
    y = pivot + h
    rho = np.sqrt(X ** 2 + y ** 2); alpha = np.arctan2(X, y)
    return ((theta / step + (K - 1) / 2.0).astype(f32), ((rho - radius_mm) / depth * R).astype(f32),
            ((alpha + total_angle / 2) / total_angle * float(f32(E))).astype(f32))


def forward(phi, theta, t, radius_mm, pivot_mm):
    """the forward geometry: the point at path length t on the beam at arc angle phi in the plane tilted by theta"""
    a = radius_mm + t
    return np.stack([a * np.sin(phi), pivot_mm + (a * np.cos(phi) - pivot_mm) * np.cos(theta), (a * np.cos(phi) - pivot_mm) * np.sin(theta)], axis=-1)


def maps_to_points(maps, E, R, K, step_rad, pivot_mm, radius_mm, total_angle, depth):
    """the float maps pushed back through the forward geometry"""
    mz, mr, mc = (np.asarray(m, np.float64) for m in maps)
    step = float(f32(step_rad)); pivot = float(f32(pivot_mm))
    phi = mc / float(f32(E)) * total_angle - total_angle / 2
    return forward(phi, (mz - (K - 1) / 2.0) * step, mr * depth / R, radius_mm, pivot)


# ------------------------------------------------------------------ the grids of the tests
STEP = 0.05          # rad between the planes of the test sweeps
Q = 2.0 ** -10       # every grid entry is a multiple of 2^-10 mm: i * du and the sums are exact doubles, a cut's points ARE its layer's


def _q(v):
    return [math.floor(x / Q + 0.5) * Q for x in v]


def box(E, R, K, pivot_mm, radius_mm=30.0, total_angle=DEFAULT_ANGLE, depth=150.0):
    """centre and half-extents (x, y, z) of an axis-aligned box inside the swept region of a stack [K][E][R]: around the middle scan-line,
    the middle of the rows that have a next row, tilt 0"""
    dphi = total_angle * max(E - 1, 0.5) / E                         # the columns that have a next column (E = 1: half the sector)
    phi_c = ((E - 1) / 2.0) / E * total_angle - total_angle / 2 if E > 1 else 0.0
    tspan = depth * max(R - 1, 0.5) / R
    a_mid = radius_mm + 0.5 * tspan; hy = 0.15 * tspan; a_lo = a_mid - hy
    zspan = max(K - 1, 1) * STEP
    hx = 0.45 * a_lo * math.sin(min(dphi / 2, 1.2))
    hz = 0.45 * (a_lo * math.cos(min(dphi / 2, 1.2)) - pivot_mm) * math.tan(zspan / 2)
    return (a_mid * math.sin(phi_c), a_mid * math.cos(phi_c), 0.0), (hx, hy, max(hz, 4 * Q))


GRID_SHAPES = [(33, 35, 5), (1, 1, 1), (257, 3, 2), "oblique"]


def grid_for(mcrt, which, E, R, K, pivot_mm, radius_mm=30.0, total_angle=DEFAULT_ANGLE):
    """the grids of tests/test_gpu_volume.py inside box(): 33 x 35 x 5 (no multiple of 4 or 256 points), 1 x 1 x 1, 257 x 3 x 2, and an
    oblique cut 64 x 48 x 1 whose two axes mix all three directions"""
    c, (hx, hy, hz) = box(E, R, K, pivot_mm, radius_mm, total_angle)
    if which == "oblique":
        nu, nv = 64, 48
        du = _q([1.2 * hx / nu, 0.5 * hy / nu, 0.6 * hz / nu]); dv = _q([-0.5 * hx / nv, 1.2 * hy / nv, 0.8 * hz / nv])
        o = _q([c[k] - (nu - 1) / 2.0 * du[k] - (nv - 1) / 2.0 * dv[k] for k in range(3)])
        return mcrt.volume_grid(o, du, dv, (0, 0, 0), nu, nv, 1)
    nu, nv, nw = which
    st = _q([2 * hx / max(nu - 1, 1), 2 * hy / max(nv - 1, 1), 2 * hz / max(nw - 1, 1)])
    o = _q([c[0] - (nu - 1) / 2.0 * st[0], c[1] - (nv - 1) / 2.0 * st[1], c[2] - (nw - 1) / 2.0 * st[2]])
    return mcrt.volume_grid(o, (st[0], 0, 0), (0, st[1], 0), (0, 0, st[2]), nu, nv, nw)



def layer_cut(mcrt, g, l):
    """the cut whose points are layer l of volume g (exact: every entry is a multiple of Q)"""
    o = [g.origin_mm[k] + l * g.dw_mm[k] for k in range(3)]
    return mcrt.volume_grid(o, list(g.du_mm), list(g.dv_mm), (0, 0, 0), g.nu, g.nv, 1)


def taps_inside(maps, E, R, K):
    """per point, from the maps alone: every tap that CAN lie inside does -- on an axis with at least two samples both taps, on an axis
    with one sample that one (floor == 0 or -1)"""
    ok = np.ones(np.asarray(maps[0]).shape, bool)
    for m, n in zip(maps, (K, R, E)):
        f = np.floor(np.asarray(m, np.float64))
        ok &= ((f >= 0) & (f + 1 < n)) if n > 1 else ((f == 0) | (f == -1))
    return ok
