"""numpy mirror of strain elastography, a reading of the text of include/mcrt.h alone (mcrt_strain_table, mcrt_strain_draws, mcrt_strain_map,
mcrt_strain_compress_frames, mcrt_strain_frames, mcrt_elastogram_frames): float32 arrays, one rounding per operation (numpy rounds every
float32 operation once; / and sqrt are correctly rounded), integers where the header has integers, the host formulas in double.  The
tracker loops over window taps and lags and is vectorised over samples."""
import math
import numpy as np

from flow_mirror import philox4x32_10, atan2f, INV_STD, QUIET

f32 = np.float32
LABEL_NONE = 255
COUNTER = 0x5354524E


def strain_table(modulus, applied=0.01, ref_modulus=1.0):
    """int32 [n_labels]: llrint(applied * ref_modulus / modulus * 2^24) in double, 0 for a modulus of exactly 0"""
    out = []
    for m in np.asarray(modulus, np.float64).reshape(-1):
        q = 0 if m == 0.0 else int(np.rint(float(applied) * float(ref_modulus) / m * 16777216.0))
        assert abs(q) <= 1 << 19
        out.append(q)
    return np.array(out, np.int32)


def draws(seed, image_id, E, R):
    """int32 [E][R][2]: one block per (e, r), counter (e, r, 0x5354524E, 0), key (seed, image_id)"""
    e, r = np.meshgrid(np.arange(E, dtype=np.uint64), np.arange(R, dtype=np.uint64), indexing="ij")
    o = philox4x32_10(e, r, np.uint64(COUNTER), np.uint64(0), seed, image_id)
    lo = lambda w: (w & np.uint64(0xffff)).astype(np.int64); hi = lambda w: (w >> np.uint64(16)).astype(np.int64)
    d = np.empty((E, R, 2), np.int32)
    d[..., 0] = (lo(o[0]) + hi(o[0]) + lo(o[1]) + hi(o[1])) - 131070
    d[..., 1] = (lo(o[2]) + hi(o[2]) + lo(o[3]) + hi(o[3])) - 131070
    return d


def strain_map(kind=0):
    assert kind == 0
    lut = np.zeros((256, 3), np.uint8)
    for i in range(256):
        if i <= 128:
            u = min(255, 2 * i)
            lut[i] = (0, u, 255 - u)
        else:
            u = 2 * (i - 128)
            lut[i] = (u, 255 - u, 0)
    return lut


def rotor():
    a = 6.283185307179586 * np.arange(4096) / 4096.0
    return np.stack([np.cos(a).astype(f32), np.sin(a).astype(f32)], axis=-1)


def _turn(z, theta, lut):
    """z [...][2] turned by theta (int64 holding a uint32) through the rotor table: four products, one subtraction, one addition"""
    cs = lut[((theta + 0x80000) >> 20) & 4095]
    c, s = cs[..., 0], cs[..., 1]
    re = ((z[..., 0] * c).astype(f32) - (z[..., 1] * s).astype(f32)).astype(f32)
    im = ((z[..., 0] * s).astype(f32) + (z[..., 1] * c).astype(f32)).astype(f32)
    return re, im


def compress(iq, tissue, eps_q24, cycles_per_row, sigma=0.0, seed=COUNTER, first_image_id=0):
    """dict(post [F][E][R][2], truth_disp, truth_strain [F][E][R]) of mcrt_strain_compress_frames; sigma: a number or [F]"""
    pre = np.asarray(iq, f32)
    F, E, R, _ = pre.shape
    table = np.zeros(256, np.int64); table[:len(eps_q24)] = np.asarray(eps_q24, np.int64)
    eps = table[np.asarray(tissue).astype(np.int64)]                                     # [F][E][R]
    U = np.cumsum(eps, axis=-1) - eps                                                    # U[q] = sum of eps below q
    q = np.arange(R, dtype=np.int64)
    s = (q << 24) + U
    s0 = s >> 24; fr = s & 0xFFFFFF
    carrier = int(np.rint(float(cycles_per_row) * 4294967296.0))
    th0 = ((carrier * fr) >> 24) & 0xFFFFFFFF
    th1 = ((carrier * (fr - (1 << 24))) >> 24) & 0xFFFFFFFF

    def tap(at):
        ok = (at >= 0) & (at < R)
        v = np.take_along_axis(pre, np.clip(at, 0, R - 1)[..., None].repeat(2, axis=-1), axis=2)
        return np.where(ok[..., None], v, f32(0.0)).astype(f32)

    lut = rotor()
    with np.errstate(**QUIET):
        w1 = (fr.astype(f32) * f32(2.0 ** -24)).astype(f32); w0 = (f32(1.0) - w1).astype(f32)
        ar, ai = _turn(tap(s0), th0, lut); br, bi = _turn(tap(s0 + 1), th1, lut)
        post = np.stack([((w0 * ar).astype(f32) + (w1 * br).astype(f32)).astype(f32), ((w0 * ai).astype(f32) + (w1 * bi).astype(f32)).astype(f32)], axis=-1)
        k = (np.broadcast_to(np.asarray(sigma, f32), (F,)) * INV_STD).astype(f32)
        for f in range(F):
            if k[f] != 0:                                                                # no draw where k == 0
                d = draws(seed, first_image_id + f, E, R).astype(f32)
                post[f] = (post[f] + (k[f] * d).astype(f32)).astype(f32)
    return dict(post=post, truth_disp=(U.astype(np.int32).astype(f32) * f32(2.0 ** -24)).astype(f32),
                truth_strain=(eps.astype(np.int32).astype(f32) * f32(2.0 ** -24)).astype(f32))


def _shifted(x, d, fill=0.0):
    """y[..., r] = x[..., r + d] where r + d is inside, `fill` elsewhere (along axis 2 of [F][E][R] or [F][E][R][2])"""
    R = x.shape[2]
    y = np.full_like(x, fill)
    lo, hi = max(0, -d), min(R, R - d)
    if lo < hi:
        y[:, :, lo:hi] = x[:, :, lo + d:hi + d]
    return y


def _inside(R, d):
    r = np.arange(R)
    return (r + d >= 0) & (r + d < R)


def track(pre, post, cycles_per_row, window_rows=16, search_rows=8, lsq_rows=12):
    """dict(disp, rho, strain [F][E][R]) of mcrt_strain_frames"""
    pre = np.asarray(pre, f32); post = np.asarray(post, f32)
    F, E, R, _ = pre.shape
    a, L, g = int(window_rows), int(search_rows), int(lsq_rows)
    with np.errstate(**QUIET):
        def energy(x):
            s = np.zeros((F, E, R), f32)
            for i in range(-a, a + 1):
                v = _shifted(x, i)
                t = ((v[..., 0] * v[..., 0]).astype(f32) + (v[..., 1] * v[..., 1]).astype(f32)).astype(f32)
                s = np.where(_inside(R, i), (s + t).astype(f32), s)
            return s
        e1 = energy(pre); P = energy(post)

        def corr(k):
            re = np.zeros((F, E, R), f32); im = np.zeros((F, E, R), f32)
            for i in range(-a, a + 1):
                u = _shifted(pre, i); v = _shifted(post, i + k)
                ok = _inside(R, i) & _inside(R, i + k)
                tr = ((v[..., 0] * u[..., 0]).astype(f32) + (v[..., 1] * u[..., 1]).astype(f32)).astype(f32)
                ti = ((v[..., 1] * u[..., 0]).astype(f32) - (v[..., 0] * u[..., 1]).astype(f32)).astype(f32)
                re = np.where(ok, (re + tr).astype(f32), re); im = np.where(ok, (im + ti).astype(f32), im)
            rho2 = ((((re * re).astype(f32) + (im * im).astype(f32)).astype(f32)) / (e1 * _shifted(P, k)).astype(f32)).astype(f32)
            return re, im, rho2

        bre, bim, brho = corr(0)
        bk = np.zeros((F, E, R), np.int32)
        for m in range(1, L + 1):
            for k in (-m, m):
                re, im, rho2 = corr(k)
                win = _inside(R, k) & (rho2 > brho)                                      # (a NaN compares false on either side)
                bre = np.where(win, re, bre); bim = np.where(win, im, bim); brho = np.where(win, rho2, brho); bk = np.where(win, np.int32(k), bk)
        scale = f32(1.0 / (6.283185307179586 * float(cycles_per_row)))
        disp = ((atan2f(bim, bre) * scale).astype(f32) - bk.astype(f32)).astype(f32)
        rho = np.sqrt(brho).astype(f32)
        r = np.arange(R)
        j_lo = np.maximum(0, r - g); j_hi = np.minimum(R - 1, r + g)
        num = np.zeros((F, E, R), f32); den = np.zeros(R, f32)
        for o in range(-g, g + 1):                                                       # j = r + o ascends with o
            j = r + o
            ok = (j >= j_lo) & (j <= j_hi)
            t = (2 * j - (j_lo + j_hi)).astype(f32)
            num = np.where(ok, (num + (t * _shifted(disp, o)).astype(f32)).astype(f32), num)
            den = np.where(ok, (den + (t * t).astype(f32)).astype(f32), den)
        strain = np.where(j_lo == j_hi, f32(0.0), ((f32(2.0) * num).astype(f32) / np.where(j_lo == j_hi, f32(1.0), den)).astype(f32)).astype(f32)
    return dict(disp=disp, rho=rho, strain=strain)


def elastogram(strain_img, rho_img, grey, lut, ref_strain=0.01, rho_min=0.7, grey_min=0, alpha=160):
    """rgb uint8 [F][H][W][3] of mcrt_elastogram_frames"""
    s = np.asarray(strain_img, f32); rho = np.asarray(rho_img, f32); g = np.asarray(grey, np.uint8).astype(np.int64)
    with np.errstate(**QUIET):
        x = (s / f32(ref_strain)).astype(f32)
        t = np.rint((x * f32(128.0)).astype(f32))
        show = (x == x) & (rho >= f32(rho_min)) & (g >= grey_min)
        idx = np.where(t < 0, 0, np.where(t > 255, 255, np.where(show, t, 0))).astype(np.int64)
    col = np.asarray(lut, np.uint8).astype(np.int64)[idx]
    mixed = (g[..., None] * (256 - alpha) + col * alpha + 128) >> 8
    return np.where(show[..., None], mixed, g[..., None]).astype(np.uint8)
