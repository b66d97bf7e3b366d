"""numpy mirror of mcrt_bmode_frames (include/mcrt.h, steps 1-6): what tests/test_bmode_contract.py and tests/test_gpu_bmode.py compare
the GPU's 8-bit B-mode frames with.  Step 4 (scan conversion) is the oracle's orc.scan_convert applied to the grey levels, unchanged."""
import numpy as np

f32 = np.float32


def tgc_factors(tgc_db, n_rows):
    """k[r] = (float)pow(10.0, tgc_db[r] / 20.0), in double; 1 without a curve"""
    if tgc_db is None:
        return np.ones(n_rows, f32)
    t = np.asarray(tgc_db, f32).astype(np.float64)
    with np.errstate(over="ignore"):
        return (10.0 ** (t / 20.0)).astype(f32)


def amplitude(frame, k):
    """frame [E][R] -> a = |v| * k[r], non-finite a -> 0 (float32)"""
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.abs(np.asarray(frame, f32)) * k[None, :]
    a[~np.isfinite(a)] = 0
    return a.astype(f32)


def grey(a, ref, mode="db", gain_db=0.0, dynamic_range_db=60.0):
    """step 3, per tap in float32; a frame with ref == 0 is black"""
    ref = f32(ref)
    if not ref > 0:
        return np.zeros_like(a)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if mode == "db":
            dr = f32(dynamic_range_db)
            g = (f32(20.0) * np.log10(a / ref) + f32(gain_db) + dr) / dr
            g = np.where(a > 0, g, f32(0)).astype(f32)
        else:
            g = (np.log10(a + f32(1.0)) / np.log10(ref + f32(1.0))).astype(f32)
    return np.fmin(np.fmax(g, f32(0)), f32(1)).astype(f32)


def quantise(y):
    return (y.astype(f32) * f32(255.0) + f32(0.5)).astype(np.uint8)


def bmode(orc, frames, mode="db", dynamic_range_db=60.0, gain_db=0.0, ref=None, tgc_db=None, persistence=0.0, state=None, reset_state=True,
          radius_mm=30.0, total_angle=1.0471975511965976, out_rows=400, out_cols=500):
    """frames [F][E][R] (the device layout) -> (bytes [F][out_rows][out_cols], refs [F] float32, state after the last frame)"""
    frames = np.asarray(frames, f32)
    F, E, R = frames.shape
    k = tgc_factors(tgc_db, R)
    alpha = f32(persistence)
    out = np.zeros((F, out_rows, out_cols), np.uint8)
    refs = np.zeros(F, f32)
    y = None if (state is None or reset_state) else np.asarray(state, f32)
    for f in range(F):
        a = amplitude(frames[f], k)
        r = f32(ref) if ref is not None and ref > 0 else a.max()
        refs[f] = r
        g = grey(a, r, mode, gain_db, dynamic_range_db)
        s = orc.scan_convert(np.ascontiguousarray(g.T), radius_mm=radius_mm, total_angle=total_angle, out_rows=out_rows, out_cols=out_cols)
        if alpha == 0:
            y = s
        else:
            prev = s if y is None else y
            # fmaf(alpha, prev, (1 - alpha) * s): the product of two floats is exact in double
            y = (np.float64(alpha) * prev.astype(np.float64) + ((f32(1.0) - alpha) * s).astype(np.float64)).astype(f32)
        out[f] = quantise(y)
    return out, refs, y


def assert_close(got, want, exact=0.999):
    """within one grey level everywhere and exact on at least `exact` of the pixels (the device log10f may differ in the last place)"""
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    assert d.max() <= 1, "grey levels differ by %d" % d.max()
    assert (d == 0).mean() >= exact, "only %.4f of the pixels exact" % (d == 0).mean()


def tap_boxes(maps, E, R):
    """per output pixel, the RF rows / scan-lines its bilinear taps reach: (row0, col0, all four taps inside, no tap inside)"""
    mr, mc = maps
    with np.errstate(invalid="ignore"):
        y0 = np.floor(mr); x0 = np.floor(mc)
        ok = np.isfinite(mr) & np.isfinite(mc)
        y0 = np.where(ok, y0, -10).astype(np.int64); x0 = np.where(ok, x0, -10).astype(np.int64)
    iny = [(y0 + d >= 0) & (y0 + d < R) for d in (0, 1)]
    inx = [(x0 + d >= 0) & (x0 + d < E) for d in (0, 1)]
    all_in = iny[0] & iny[1] & inx[0] & inx[1]
    none_in = ~((iny[0] | iny[1]) & (inx[0] | inx[1]))
    return y0, x0, all_in, none_in
