"""A numpy mirror of the automatic-gain stage (include/mcrt.h: mcrt_autogain_curve, mcrt_autogain_frames), written from the header's nine
steps: integers decide, and the few float operations are np.float32 operations, one rounding each.  The tests hold the library to it bit
for bit."""
import numpy as np

f32 = np.float32
u32 = np.uint32
BINS = 2048
DEFAULTS = dict(band_rows=16, min_permille=250, floor=0.0, floor_scale=3.0, max_gain=1000.0, apply=1)


def options(opts=None):
    o = dict(DEFAULTS)
    o.update(opts or {})
    assert set(o) == set(DEFAULTS), sorted(set(o) - set(DEFAULTS))
    return o


def bins_of(x):
    """step 1: bin(a) = bits(a) >> 20 with a = |v| where v is finite, else 0"""
    bits = np.ascontiguousarray(x, f32).view(u32) & u32(0x7FFFFFFF)
    return np.where(bits >= u32(0x7F800000), u32(0), bits >> u32(20)).astype(np.int64)


def n_bands(R, band_rows):
    return (R + band_rows - 1) // band_rows


def histograms(frame, band_rows):
    """step 2 for one frame [N][E][R] (or [E][R]) -> uint32 [n_bands][2048]"""
    b = bins_of(frame).reshape(-1, frame.shape[-1])
    R = b.shape[1]
    h = np.zeros((n_bands(R, band_rows), BINS), u32)
    for i in range(h.shape[0]):
        h[i] = np.bincount(b[:, i * band_rows:min((i + 1) * band_rows, R)].ravel(), minlength=BINS).astype(u32)
    return h


def centre(b):
    """the float whose bits are (bin << 20) | (1 << 19)"""
    return np.array([(int(b) << 20) | (1 << 19)], u32).view(f32)[0]


def threshold_bin(floor_f, floor_scale):
    with np.errstate(all="ignore"):
        thr = f32(f32(floor_f) * f32(floor_scale))
    return int(np.array([thr], f32).view(u32)[0] >> 20) if np.isfinite(thr) and thr > 0 else 0


def curve(hist, n_lines, R, floor_f=0.0, opts=None):
    """steps 3 to 8 for one frame -> (k float32 [R], band_bin int32 [n_bands] with -1 for an invalid band, pen)"""
    o = options(opts)
    B = int(o["band_rows"])
    nB = n_bands(R, B)
    hist = np.asarray(hist).astype(np.int64)
    assert hist.shape == (nB, BINS)
    thr_bin = threshold_bin(floor_f, o["floor_scale"])
    m = np.full(nB, -1, np.int32)
    for b in range(nB):
        tissue = hist[b].copy()
        tissue[:thr_bin + 1] = 0
        n_t = int(tissue.sum())
        n_s = int(n_lines) * (min((b + 1) * B, R) - b * B)
        if n_t > 0 and n_t * 1000 >= int(o["min_permille"]) * n_s:
            m[b] = int(np.argmax(2 * np.cumsum(tissue) >= n_t))
    valid = np.flatnonzero(m >= 0)
    kb = np.ones(nB, f32)
    pen = 0
    if valid.size:
        target = centre(sorted(int(v) for v in m[valid])[(valid.size - 1) // 2])
        max_gain = f32(o["max_gain"])
        inv_max = f32(f32(1.0) / max_gain)
        with np.errstate(all="ignore"):
            for b in range(nB):
                shallower = valid[valid <= b]
                src = int(shallower[-1]) if shallower.size else int(valid[0])
                kb[b] = np.minimum(np.maximum(f32(target / centre(m[src])), inv_max), max_gain)
        pen = min(R, (int(valid[-1]) + 1) * B)
    k = np.empty(R, f32)
    for r in range(R):
        n = 2 * r - (B - 1)
        if n <= 0:
            k[r] = kb[0]
            continue
        b = n // (2 * B)
        if b >= nB - 1:
            k[r] = kb[nB - 1]
            continue
        t = f32(f32(n - 2 * B * b) / f32(2 * B))
        k[r] = f32(kb[b] + f32(f32(kb[b + 1] - kb[b]) * t))
    return k, m, pen


def autogain(stack, opts=None, floor=None):
    """the rule over stack [F][N][E][R] -> (out, gain [F][R], band_bin [F][n_bands], pen [F]).  floor: one floor per frame (floor_dev),
    or None: the options' floor"""
    o = options(opts)
    x = np.ascontiguousarray(stack, f32)
    F, N, E, R = x.shape
    nB = n_bands(R, int(o["band_rows"]))
    gain = np.empty((F, R), f32); band = np.empty((F, nB), np.int32); pen = np.empty(F, u32)
    out = x.copy()
    for f in range(F):
        floor_f = o["floor"] if floor is None else floor[f]
        gain[f], band[f], pen[f] = curve(histograms(x[f], int(o["band_rows"])), N * E, R, floor_f, o)
        if o["apply"]:
            with np.errstate(all="ignore"):
                out[f] = x[f] * gain[f]
    return out, gain, band, pen
