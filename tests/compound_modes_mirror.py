"""numpy mirror of the compounding modes (include/mcrt.h: mcrt_compound_frames_opts, mcrt_bmode_compound_frames_opts, mcrt_compound_weights),
in np.float32, built on compound_mirror's point, coverage rule, taps and blend: a view's weight (its view weight times the lateral edge ramp
of its column map), the weighted mean, the maximum and the median over the contributing views, and the 8-bit display on bmode_mirror's steps
1-3 and 5-6.  The maps are an INPUT -- the product's own (mcrt_compound_maps)."""
import numpy as np

import bmode_mirror as bm
import compound_mirror as cm

f32 = np.float32
MODES = ("mean", "max", "median")


def ramp(mc, E, feather_lines):
    """a = feather > 0 ? fmin(fmax(fmin(mx, (float)(E - 1) - mx) / feather, 0), 1) : 1 -- fmin / fmax drop a NaN operand, as fminf / fmaxf do"""
    mc = np.asarray(mc, f32)
    if not feather_lines > 0:
        return np.ones(mc.shape, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        edge = np.fmin(mc, (f32(E - 1) - mc).astype(f32))
        return np.fmin(np.fmax((edge / f32(feather_lines)).astype(f32), f32(0)), f32(1)).astype(f32)


def view_weights(mr, mc, E, R, view_weight=1.0, feather_lines=0.0):
    """(w, contributes) of one view: w = view_weight * a, contributes = covered && w > 0"""
    w = (f32(view_weight) * ramp(mc, E, feather_lines)).astype(f32)
    con = cm.covered(cm.remap_point(mc, mr), E, R) & (w > 0)
    return w, con


def weight_map(mr, mc, E, R, view_weight=1.0, feather_lines=0.0):
    """what mcrt_compound_weights writes: contributes ? w : 0"""
    w, con = view_weights(mr, mc, E, R, view_weight, feather_lines)
    return np.where(con, w, f32(0)).astype(f32)


def compound(stack, maps, mode="mean", weights=None, feather_lines=0.0):
    """stack [N][E][R], maps a list of N (map_row, map_col) -> (picture float32 [rows][cols], contributing views per pixel)"""
    assert mode in MODES
    stack = np.asarray(stack, f32)
    N, E, R = stack.shape
    assert len(maps) == N
    weights = [1.0] * N if weights is None else list(weights)
    shape = np.asarray(maps[0][0]).shape
    s_all, con_all, w_all = [], [], []
    for n in range(N):
        mr, mc = maps[n]
        pt = cm.remap_point(mc, mr)
        w, con = view_weights(mr, mc, E, R, weights[n], feather_lines)
        s_all.append(cm.blend(pt, cm.taps(pt, stack[n]))); con_all.append(con); w_all.append(w)
    cnt = np.sum(con_all, axis=0).astype(np.int32)
    zero = np.zeros(shape, f32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if mode == "mean":
            total = zero.copy(); wsum = zero.copy()
            for s, con, w in zip(s_all, con_all, w_all):
                total = np.where(con, (total + (w * s).astype(f32)).astype(f32), total)
                wsum = np.where(con, (wsum + w).astype(f32), wsum)
            out = np.where(wsum > 0, (total / np.where(wsum > 0, wsum, f32(1))).astype(f32), f32(0))
            return out.astype(f32), cnt
        bad = np.zeros(shape, bool)
        for s, con in zip(s_all, con_all):
            bad |= con & np.isnan(s)
        if mode == "max":
            m = zero.copy(); have = np.zeros(shape, bool)
            for s, con in zip(s_all, con_all):
                m = np.where(con & ~have, s, np.where(con & (s > m), s, m)); have |= con
            out = (m + f32(0)).astype(f32)
        else:
            v = np.sort(np.stack([np.where(con & ~np.isnan(s), s, f32(np.inf)) for s, con in zip(s_all, con_all)]).astype(f32), axis=0)
            c = np.maximum(cnt, 1)
            lo = np.take_along_axis(v, ((c - 1) // 2)[None], 0)[0]; hi = np.take_along_axis(v, np.minimum(c // 2, N - 1)[None], 0)[0]
            out = (np.where(c % 2 == 1, lo, ((lo + hi).astype(f32) * f32(0.5)).astype(f32)) + f32(0)).astype(f32)
        out = np.where(bad, f32(np.nan), out)
        return np.where(cnt > 0, out, f32(0)).astype(f32), cnt


def compound_frames(frames, maps, mode="mean", weights=None, feather_lines=0.0):
    """frames [F][N][E][R] -> float32 [F][rows][cols]"""
    return np.stack([compound(fr, maps, mode, weights, feather_lines)[0] for fr in np.asarray(frames, f32)])


def bmode_compound(frames, maps, compound_mode="mean", weights=None, feather_lines=0.0, mode="db", dynamic_range_db=60.0, gain_db=0.0, ref=None,
                   tgc_db=None, persistence=0.0, state=None, reset_state=True):
    """compound_mirror.bmode_compound with the compounding rule above in place of the plain mean (step 4)"""
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
        s, _ = compound(g, maps, compound_mode, weights, feather_lines)
        if alpha == 0:
            y = s
        else:
            prev = s if y is None else y
            y = (np.float64(alpha) * prev.astype(np.float64) + ((f32(1.0) - alpha) * s).astype(np.float64)).astype(f32)
        out[f] = bm.quantise(y)
    return out, refs, y
