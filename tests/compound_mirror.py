"""numpy mirror of spatial compounding (include/mcrt.h: mcrt_compound_frames, mcrt_bmode_compound_frames), in np.float32: the point, taps
and blend of the scan conversion, the coverage rule, the mean over the covering views, and the 8-bit display built on bmode_mirror's steps
1-3 and 5-6.  The maps are an INPUT -- the product's own (mcrt_compound_maps) -- so that libm differences between numpy and the C library
cannot enter the kernel comparisons; tests/test_compound_contract.py checks the maps themselves against the forward geometry."""
import numpy as np

import bmode_mirror as bm

f32 = np.float32


def remap_point(mc, mr):
    """per pixel: (fractions ax, ay as float32, x0, y0 as int64, mapped) from the column map mc and the row map mr"""
    mc = np.asarray(mc, f32); mr = np.asarray(mr, f32)
    mapped = ~(np.isnan(mc) | np.isnan(mr))
    with np.errstate(invalid="ignore"):
        fx = np.floor(mc); fy = np.floor(mr)
        ax = (mc - fx).astype(f32); ay = (mr - fy).astype(f32)
        big = f32(2.0 ** 62)
        x0 = np.where(mapped, np.clip(fx, -big, big), -4).astype(np.int64)
        y0 = np.where(mapped, np.clip(fy, -big, big), -4).astype(np.int64)
    return ax, ay, x0, y0, mapped


def covered(pt, E, R):
    """the coverage rule: both maps not NaN and at least one of the four taps inside the E x R view"""
    ax, ay, x0, y0, mapped = pt
    return mapped & (x0 >= -1) & (x0 < E) & (y0 >= -1) & (y0 < R)


def taps(pt, view):
    """view [E][R] -> v[dy][dx] per pixel: the tap at (x0 + dx, y0 + dy) inside the view, 0 elsewhere"""
    ax, ay, x0, y0, mapped = pt
    E, R = view.shape
    v = [[None, None], [None, None]]
    for dy in (0, 1):
        for dx in (0, 1):
            xx = x0 + dx; yy = y0 + dy
            inside = mapped & (xx >= 0) & (yy >= 0) & (xx < E) & (yy < R)
            t = view[np.clip(xx, 0, E - 1), np.clip(yy, 0, R - 1)]
            v[dy][dx] = np.where(inside, t, f32(0)).astype(f32)
    return v


def blend(pt, v):
    """top = v00 (1 - ax) + v01 ax; bot likewise; top (1 - ay) + bot ay: one float32 rounding per operation"""
    ax, ay = pt[0], pt[1]
    one = f32(1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        top = (v[0][0] * (one - ax)).astype(f32) + (v[0][1] * ax).astype(f32)
        bot = (v[1][0] * (one - ax)).astype(f32) + (v[1][1] * ax).astype(f32)
        return ((top * (one - ay)).astype(f32) + (bot * ay).astype(f32)).astype(f32)


def convert(view, mr, mc):
    """one view [E][R] through one map pair: the scan conversion alone (no coverage rule, no mean)"""
    pt = remap_point(mc, mr)
    return blend(pt, taps(pt, np.asarray(view, f32)))


def compound(stack, maps):
    """stack [N][E][R], maps a list of N (map_row, map_col) -> (picture float32 [rows][cols], looks per pixel)"""
    stack = np.asarray(stack, f32)
    N, E, R = stack.shape
    assert len(maps) == N
    shape = np.asarray(maps[0][0]).shape
    total = np.zeros(shape, f32); cnt = np.zeros(shape, np.int32)
    for n in range(N):
        mr, mc = maps[n]
        pt = remap_point(mc, mr)
        cov = covered(pt, E, R)
        s = blend(pt, taps(pt, stack[n]))
        with np.errstate(invalid="ignore", over="ignore"):
            total = np.where(cov, (total + s).astype(f32), total)
        cnt += cov
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        out = np.where(cnt > 0, (total / np.maximum(cnt, 1).astype(f32)).astype(f32), f32(0)).astype(f32)
    return out, cnt


def compound_frames(frames, maps):
    """frames [F][N][E][R] -> float32 [F][rows][cols]"""
    return np.stack([compound(fr, maps)[0] for fr in np.asarray(frames, f32)])


def combine(singles, covs):
    """the N single-view compounds (each: the view's conversion where it covers, 0 elsewhere) and their coverage masks -> the N-view compound"""
    total = np.zeros(singles[0].shape, f32); cnt = np.zeros(singles[0].shape, np.int32)
    for s, cov in zip(singles, covs):
        with np.errstate(invalid="ignore", over="ignore"):
            total = np.where(cov, (total + s).astype(f32), total)
        cnt += cov
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return np.where(cnt > 0, (total / np.maximum(cnt, 1).astype(f32)).astype(f32), f32(0)).astype(f32)


def bmode_compound(frames, maps, mode="db", dynamic_range_db=60.0, gain_db=0.0, ref=None, tgc_db=None, persistence=0.0, state=None, reset_state=True):
    """frames [F][N][E][R] -> (bytes [F][rows][cols], refs [F] float32, state after the last frame): bmode_mirror's steps 1-3 over the N
    views of a frame together (one reference: the largest amplitude of all its views), the compound of the grey levels, steps 5-6"""
    frames = np.asarray(frames, f32)
    F, N, E, R = frames.shape
    k = bm.tgc_factors(tgc_db, R)
    alpha = f32(persistence)
    shape = np.asarray(maps[0][0]).shape
    out = np.zeros((F,) + shape, np.uint8)
    refs = np.zeros(F, f32)
    y = None if (state is None or reset_state) else np.asarray(state, f32)
    for f in range(F):
        a = bm.amplitude(frames[f].reshape(N * E, R), k)
        r = f32(ref) if ref is not None and ref > 0 else a.max()
        refs[f] = r
        g = bm.grey(a, r, mode, gain_db, dynamic_range_db).reshape(N, E, R)
        s, _ = compound(g, maps)
        if alpha == 0:
            y = s
        else:
            prev = s if y is None else y
            y = (np.float64(alpha) * prev.astype(np.float64) + ((f32(1.0) - alpha) * s).astype(np.float64)).astype(f32)
        out[f] = bm.quantise(y)
    return out, refs, y
