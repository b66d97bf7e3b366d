"""numpy mirror of colour Doppler, a reading of the text of include/mcrt.h alone (mcrt_flow_nyquist, mcrt_flow_phasors, mcrt_flow_draws,
mcrt_colour_map, mcrt_flow_split_frames, mcrt_flow_frames, mcrt_colour_frames): float32 arrays, one rounding per operation (numpy rounds
every float32 operation once; / and sqrt are correctly rounded), the host formulas in double."""
import math
import numpy as np

f32 = np.float32
PI = 3.141592653589793
WALL_NONE, WALL_MEAN, WALL_LINEAR = 0, 1, 2
LABEL_NONE = 255
INV_STD = f32(1.0 / math.sqrt(1431655765.0))
ATAN_C = [f32(c) for c in (0.99997726, -0.33262347, 0.19354346, -0.11643287, 0.05265332, -0.01172120)]
QUIET = dict(invalid="ignore", over="ignore", under="ignore", divide="ignore")


def nyquist(prf_hz, freq_mhz, speed_of_sound=1500.0):
    return (float(speed_of_sound) * 1000.0 * float(f32(prf_hz))) / (4.0 * (float(freq_mhz) * 1.0e6))


def phasors(v_nyq, vel, dirs):
    """(phasor float32 [L][E][2], truth float32 [L][E]) of vel [L][3] and dirs [E][3], in double through libm"""
    vel = np.asarray(vel, f32).reshape(-1, 3); dirs = np.asarray(dirs, f32).reshape(-1, 3)
    ph = np.zeros((len(vel), len(dirs), 2), f32); tr = np.zeros((len(vel), len(dirs)), f32)
    for l, v in enumerate(vel.astype(np.float64)):
        for e, d in enumerate(dirs.astype(np.float64)):
            if not v.any():
                ph[l, e] = (1.0, 0.0)
                continue
            v_t = 0.0 - ((v[0] * d[0] + v[1] * d[1]) + v[2] * d[2])
            phi = PI * v_t / v_nyq
            tr[l, e] = f32(v_t); ph[l, e] = (f32(math.cos(phi)), f32(math.sin(phi)))
    return ph, tr


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 over uint64 arrays that hold 32-bit words (broadcast against each other)"""
    M0, M1, W0, W1, MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0 = int(k0) & MASK; k1 = int(k1) & MASK
    for _ in range(10):
        p0 = c0 * np.uint64(M0); p1 = c2 * np.uint64(M1)
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0); n2 = (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)
        c0, c1, c2, c3 = n0, p1 & np.uint64(MASK), n2, p0 & np.uint64(MASK)
        k0 = (k0 + W0) & MASK; k1 = (k1 + W1) & MASK
    return c0, c1, c2, c3


def draws(seed, image_id, E, R, N):
    """int32 [N][E][R][2]: one block per (e, r, n), counter (e, r, 0x464C4F57, n), key (seed, image_id)"""
    n, e, r = np.meshgrid(np.arange(N, dtype=np.uint64), np.arange(E, dtype=np.uint64), np.arange(R, dtype=np.uint64), indexing="ij")
    o = philox4x32_10(e, r, np.uint64(0x464C4F57), n, seed, image_id)
    lo = lambda w: (w & np.uint64(0xffff)).astype(np.int64); hi = lambda w: (w >> np.uint64(16)).astype(np.int64)
    d = np.empty((N, E, R, 2), np.int32)
    d[..., 0] = (lo(o[0]) + hi(o[0]) + lo(o[1]) + hi(o[1])) - 131070
    d[..., 1] = (lo(o[2]) + hi(o[2]) + lo(o[3]) + hi(o[3])) - 131070
    return d


def colour_map(kind=0):
    assert kind == 0
    lut = np.zeros((256, 3), np.uint8)
    for i in range(129, 256):
        k = i - 128
        lut[i] = (128 + k, 0 if k <= 64 else (k - 64) * 4, 0)
    for i in range(1, 128):
        k = 128 - i
        lut[i] = (0, 0 if k <= 64 else (k - 64) * 4, 128 + k)
    lut[0] = lut[1]
    return lut


def split(rf, tissue, moving):
    """out [F][2][E][R]: image 0 what stands still, image 1 what moves; the sample's own bits or +0.0f"""
    rf = np.asarray(rf, f32); tissue = np.asarray(tissue, np.uint8)
    table = np.zeros(256, bool); table[:len(moving)] = np.asarray(moving) != 0
    mv = table[tissue]
    zero = np.zeros_like(rf)
    return np.stack([np.where(mv, zero, rf), np.where(mv, rf, zero)], axis=1)


def atan2f(y, x):
    y = np.asarray(y, f32); x = np.asarray(x, f32)
    with np.errstate(**QUIET):
        ax = np.abs(x); ay = np.abs(y)
        steep = ay > ax
        hi = np.where(steep, ay, ax); lo = np.where(steep, ax, ay)
        zero = hi == 0
        t = (lo / np.where(zero, f32(1), hi)).astype(f32)
        s = (t * t).astype(f32)
        p = np.full(t.shape, ATAN_C[5], f32)
        for j in (4, 3, 2, 1, 0):
            p = ((p * s).astype(f32) + ATAN_C[j]).astype(f32)
        a = (t * p).astype(f32)
        a = np.where(steep, (f32(1.5707964) - a).astype(f32), a)
        a = np.where(x < 0, (f32(3.1415927) - a).astype(f32), a)
        a = np.where(y < 0, -a, a)
        return np.where(zero, f32(0.0), a).astype(f32)


def ensemble(iq_static, iq_moving, tissue, phasor, N, sigma=0.0, seed=0x464C4F57, first_image_id=0):
    """z float32 [N][F][E][R][2].  iq_* [F][E][R][2] (iq_static may be None), tissue [F][E][R], phasor [L][E][2]; sigma: a number or [F]"""
    m = np.array(iq_moving, f32)
    F, E, R, _ = m.shape
    L = phasor.shape[0]
    lab = np.asarray(tissue).astype(np.int64)
    known = lab < L
    p = np.asarray(phasor, f32)[np.where(known, lab, 0), np.arange(E)[None, :, None]]           # [F][E][R][2]
    c = np.where(known, p[..., 0], f32(1.0)); s = np.where(known, p[..., 1], f32(0.0))
    k = (np.broadcast_to(np.asarray(sigma, f32), (F,)) * INV_STD).astype(f32)
    d = {f: draws(seed, first_image_id + f, E, R, N).astype(f32) for f in range(F) if k[f] != 0}     # no draw where k == 0
    z = np.empty((N, F, E, R, 2), f32)
    with np.errstate(**QUIET):
        for n in range(N):
            x = m.copy() if iq_static is None else (np.asarray(iq_static, f32) + m).astype(f32)
            for f in d:
                x[f] = (x[f] + (k[f] * d[f][n]).astype(f32)).astype(f32)
            z[n] = x
            a, b = m[..., 0], m[..., 1]
            m = np.stack([((a * c).astype(f32) - (b * s).astype(f32)).astype(f32), ((a * s).astype(f32) + (b * c).astype(f32)).astype(f32)], axis=-1)
    return z


def wall_filter(z, wall):
    """over axis 0, per component"""
    N = z.shape[0]
    w = np.array(z, f32)
    with np.errstate(**QUIET):
        if wall >= WALL_MEAN:
            t = [w[n] for n in range(N)]                          # the pairwise sum: neighbours in pairs, an odd last term carried up
            while len(t) > 1:
                t = [(t[i] + t[i + 1]).astype(f32) for i in range(0, len(t) - 1, 2)] + ([t[-1]] if len(t) & 1 else [])
            mean = (t[0] / f32(N)).astype(f32)
            w = (w - mean).astype(f32)
        if wall == WALL_LINEAR:
            t = [f32(2 * n - (N - 1)) for n in range(N)]
            num = np.zeros(z.shape[1:], f32); den = f32(0.0)
            for n in range(N):
                num = (num + (t[n] * w[n]).astype(f32)).astype(f32); den = f32(den + f32(t[n] * t[n]))
            slope = (num / den).astype(f32)
            for n in range(N):
                w[n] = (w[n] - (t[n] * slope).astype(f32)).astype(f32)
    return w


def autocorrelation(w):
    """(r0, re, im) float32 [...] of w [N][...][2]"""
    N = w.shape[0]
    r0 = np.zeros(w.shape[1:-1], f32); re = r0.copy(); im = r0.copy()
    with np.errstate(**QUIET):
        for n in range(N):
            r0 = (r0 + ((w[n, ..., 0] * w[n, ..., 0]).astype(f32) + (w[n, ..., 1] * w[n, ..., 1]).astype(f32)).astype(f32)).astype(f32)
        for n in range(N - 1):
            a, b, c, d = w[n + 1, ..., 0], w[n + 1, ..., 1], w[n, ..., 0], w[n, ..., 1]
            re = (re + ((a * c).astype(f32) + (b * d).astype(f32)).astype(f32)).astype(f32)
            im = (im + ((b * c).astype(f32) - (a * d).astype(f32)).astype(f32)).astype(f32)
    return r0, re, im


def average(x, a, b):
    """x [F][E][R]: the sum along the rows (dr = -a..a ascending, inside [0, R)), then across the lines (de = -b..b ascending, inside
    [0, E)), divided by the number of samples inside the clipped window"""
    x = np.asarray(x, f32)
    F, E, R = x.shape
    with np.errstate(**QUIET):
        s = np.zeros_like(x)
        for dr in range(-a, a + 1):
            lo, hi = max(0, -dr), min(R, R - dr)
            if lo < hi:
                s[:, :, lo:hi] = (s[:, :, lo:hi] + x[:, :, lo + dr:hi + dr]).astype(f32)
        S = np.zeros_like(x)
        for de in range(-b, b + 1):
            lo, hi = max(0, -de), min(E, E - de)
            if lo < hi:
                S[:, lo:hi] = (S[:, lo:hi] + s[:, lo + de:hi + de]).astype(f32)
        rows = np.minimum(np.arange(R) + a, R - 1) - np.maximum(np.arange(R) - a, 0) + 1
        lines = np.minimum(np.arange(E) + b, E - 1) - np.maximum(np.arange(E) - b, 0) + 1
        cnt = (lines[:, None] * rows[None, :]).astype(f32)
        return (S / cnt).astype(f32)


def flow(iq_static, iq_moving, tissue, phasor, truth, v_nyq, N=8, wall=WALL_MEAN, avg_rows=2, avg_lines=1, sigma=0.0, seed=0x464C4F57, first_image_id=0):
    """dict(corr [F][3][E][R], vel, var, truth [F][E][R]) of mcrt_flow_frames"""
    z = ensemble(iq_static, iq_moving, tissue, phasor, N, sigma, seed, first_image_id)
    r0, re, im = (average(x, avg_rows, avg_lines) for x in autocorrelation(wall_filter(z, wall)))
    with np.errstate(**QUIET):
        vel = (atan2f(im, re) * f32(v_nyq / PI)).astype(f32)
        v = (f32(1.0) - (np.sqrt(((re * re).astype(f32) + (im * im).astype(f32)).astype(f32)).astype(f32) / r0).astype(f32)).astype(f32)
        v = np.where(v < 0, f32(0.0), v); v = np.where(v > 1, f32(1.0), v)
        var = np.where(r0 > 0, v, f32(0.0)).astype(f32)
    lab = np.asarray(tissue).astype(np.int64)
    known = lab < phasor.shape[0]
    E = lab.shape[1]
    tr = np.where(known, np.asarray(truth, f32)[np.where(known, lab, 0), np.arange(E)[None, :, None]], f32(0.0)).astype(f32)
    return dict(corr=np.stack([r0, re, im], axis=1), vel=vel, var=var, truth=tr)


def colour(corr_img, grey, lut, v_nyq, power_thr=0.0, vel_thr_mm_s=0.0, grey_max=255):
    """(rgb uint8 [F][H][W][3], vel_img float32 [F][H][W]) of mcrt_colour_frames; corr_img [F][3][H][W], grey uint8 [F][H][W]"""
    x = np.asarray(corr_img, f32); g = np.asarray(grey, np.uint8)
    r0, re, im = x[:, 0], x[:, 1], x[:, 2]
    with np.errstate(**QUIET):
        ang = atan2f(im, re)
        v = (ang * f32(v_nyq / PI)).astype(f32)
        show = (r0 > f32(power_thr)) & (np.abs(v) >= f32(vel_thr_mm_s)) & (g <= grey_max)
        k = np.rint((np.where(show, ang, f32(0.0)) * f32(127.0 / PI)).astype(f32)).astype(np.int64)
    idx = np.clip(128 + k, 1, 255)
    rgb = np.where(show[..., None], np.asarray(lut, np.uint8)[idx], g[..., None].repeat(3, axis=-1))
    return rgb.astype(np.uint8), np.where(show, v, f32(0.0)).astype(f32)
