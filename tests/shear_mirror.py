"""numpy mirror of shear-wave elastography, a reading of the text of include/mcrt.h alone (mcrt_shear_table, mcrt_shear_pitch,
mcrt_shear_shape, mcrt_shear_decay, mcrt_shear_draws, mcrt_shear_map, mcrt_shear_wave_frames, mcrt_shear_speed_frames): float32 arrays,
one rounding per operation (numpy rounds every float32 operation once; / is correctly rounded), integers where the header has integers,
the host formulas in double.  The tracker loops over pulses and window taps and is vectorised over samples."""
import numpy as np

from flow_mirror import philox4x32_10, atan2f, INV_STD, QUIET
from strain_mirror import rotor, _turn, _shifted, _inside, strain_map

f32 = np.float32
LABEL_NONE = 255
COUNTER = 0x53484552
NEVER = 1 << 40
SHAPE_SHIFT = 10
DEFAULTS = dict(n_pulses=64, window_rows=8, prf_hz=10000.0, sigma=0.0, seed=COUNTER, push_line=0, push_row0=0, push_rows=0, peak_q24=1677722,
                speed_lines=4, avg_rows=2, density=1.0)


def shear_table(speed_m_s, prf_hz=10000.0):
    """(slow_q16 int64 [n_labels], speed_f float32 [n_labels])"""
    c = np.asarray(speed_m_s, np.float64).reshape(-1)
    slow = []
    for v in c:
        q = 0 if v == 0.0 else int(np.rint(65536.0 * 65536.0 * float(prf_hz) / (v * 1e6)))
        assert v == 0.0 or 1 <= q <= 1 << 38
        slow.append(q)
    return np.array(slow, np.int64), c.astype(f32)


def pitch_um(E, R, radius_mm, total_angle, max_travel_us=100, speed_of_sound=1500):
    """the arc between neighbouring scan-lines at the depth of every row [um], in double: E lines share the total angle"""
    depth_mm = float(max_travel_us * speed_of_sound) * 0.001
    return 1000.0 * (float(radius_mm) + np.arange(R, dtype=np.float64) * depth_mm / float(R)) * float(total_angle) / float(E)


def shear_pitch(E, R, radius_mm, total_angle, max_travel_us=100, speed_of_sound=1500):
    """(pitch_q8 uint32 [R], pitch_mm float32 [R])"""
    um = pitch_um(E, R, radius_mm, total_angle, max_travel_us, speed_of_sound)
    return np.rint(256.0 * um).astype(np.uint32), (um * 0.001).astype(f32)


def shear_shape(width_pulses=12):
    n = 64 * int(width_pulses)
    i = np.arange(n, dtype=np.float64)
    return np.rint(65536.0 * (0.5 - 0.5 * np.cos(6.283185307179586 * (i + 0.5) / float(n)))).astype(np.uint32)


def shear_decay(n, d0_lines=8.0):
    d = np.arange(int(n), dtype=np.float64)
    return np.rint(65536.0 / np.sqrt(1.0 + d / float(d0_lines))).astype(np.uint32)


def draws(seed, image_id, E, R, pulse):
    """int32 [E][R][2]: one block per (e, r), counter (e, r, 0x53484552, pulse), key (seed, image_id)"""
    e, r = np.meshgrid(np.arange(E, dtype=np.uint64), np.arange(R, dtype=np.uint64), indexing="ij")
    o = philox4x32_10(e, r, np.uint64(COUNTER), np.uint64(pulse), seed, image_id)
    lo = lambda w: (w & np.uint64(0xffff)).astype(np.int64); hi = lambda w: (w >> np.uint64(16)).astype(np.int64)
    d = np.empty((E, R, 2), np.int32)
    d[..., 0] = (lo(o[0]) + hi(o[0]) + lo(o[1]) + hi(o[1])) - 131070
    d[..., 1] = (lo(o[2]) + hi(o[2]) + lo(o[3]) + hi(o[3])) - 131070
    return d


def shear_map(kind=0):
    """the bytes of the strain map: the index is the modulus over the reference, so blue is soft"""
    return strain_map(kind)


def arrival(tissue, slow_q16, pitch_q8, push_line):
    """int64 [F][E][R] ticks: saturating sums of the crossing costs outwards from the pushed line"""
    tissue = np.asarray(tissue).astype(np.int64)
    F, E, R = tissue.shape
    assert E < 1 << 20
    table = np.zeros(256, np.int64); table[:len(slow_q16)] = np.asarray(slow_q16, np.int64)
    slow = table[tissue]
    pitch = np.asarray(pitch_q8, np.int64).reshape(1, 1, R)
    cost = np.where(slow != 0, (slow * pitch) >> 24, NEVER)
    A = np.zeros((F, E, R), np.int64)
    p = int(push_line)
    if p + 1 < E:
        A[:, p + 1:] = np.cumsum(cost[:, p:E - 1], axis=1)                                # the crossing e-1 -> e costs what line e-1 costs
    if p > 0:
        A[:, :p] = np.cumsum(cost[:, p:0:-1], axis=1)[:, ::-1]                           # the crossing e+1 -> e costs what line e+1 costs
    return np.minimum(A, NEVER)


def displacement(A, n, shape_q16, amp_q16, peak_q24, push_line, row0, row1):
    """int64 [F][E][R]: the particle displacement of pulse n in Q24 rows"""
    F, E, R = A.shape
    shape = np.asarray(shape_q16, np.int64); amp = np.asarray(amp_q16, np.int64)
    dist = np.abs(np.arange(E) - int(push_line))
    pa = (int(peak_q24) * np.where(dist < len(amp), amp[np.minimum(dist, len(amp) - 1)], 0)) >> 16        # [E]
    t = (int(n) << 16) - A
    idx = t >> SHAPE_SHIFT
    r = np.arange(R)
    ok = ((r >= row0) & (r < row1))[None, None, :] & (A < NEVER) & (t >= 0) & (idx < len(shape))
    return np.where(ok, (pa[None, :, None] * shape[np.clip(idx, 0, len(shape) - 1)]) >> 16, 0)


def warp(pre, u, cycles_per_row, lut):
    """mcrt_strain_compress_frames' post of U = u (int64 [F][E][R]), without the noise"""
    F, E, R, _ = pre.shape
    q = np.arange(R, dtype=np.int64)
    s = (q << 24) + u
    s0 = s >> 24; fr = s & 0xFFFFFF
    carrier = int(np.rint(float(cycles_per_row) * 4294967296.0))
    th0 = ((carrier * fr) >> 24) & 0xFFFFFFFF
    th1 = ((carrier * (fr - (1 << 24))) >> 24) & 0xFFFFFFFF

    def tap(at):
        ok = (at >= 0) & (at < R)
        v = np.take_along_axis(pre, np.clip(at, 0, R - 1)[..., None].repeat(2, axis=-1), axis=2)
        return np.where(ok[..., None], v, f32(0.0)).astype(f32)

    w1 = (fr.astype(f32) * f32(2.0 ** -24)).astype(f32); w0 = (f32(1.0) - w1).astype(f32)
    ar, ai = _turn(tap(s0), th0, lut); br, bi = _turn(tap(s0 + 1), th1, lut)
    return np.stack([((w0 * ar).astype(f32) + (w1 * br).astype(f32)).astype(f32), ((w0 * ai).astype(f32) + (w1 * bi).astype(f32)).astype(f32)], axis=-1)


def wave(iq, tissue, slow_q16, speed_f, pitch_q8, shape_q16, amp_q16, cycles_per_row, sigma=None, first_image_id=0, movie=True, **opts):
    """dict(peak_time, peak_disp, truth_arrival, truth_speed [F][E][R], disp [F][T][E][R] if movie) of mcrt_shear_wave_frames; sigma: a
    number or [F] (None: the options'); opts: the fields of mcrt_shear_opts over the defaults"""
    o = dict(DEFAULTS, **opts)
    pre = np.asarray(iq, f32)
    F, E, R, _ = pre.shape
    T, a, p = int(o["n_pulses"]), int(o["window_rows"]), int(o["push_line"])
    row0 = int(o["push_row0"]); row1 = row0 + int(o["push_rows"]) if o["push_rows"] else R
    A = arrival(tissue, slow_q16, pitch_q8, p)
    lut = rotor()
    sig = o["sigma"] if sigma is None else sigma
    with np.errstate(**QUIET):
        k = (np.broadcast_to(np.asarray(sig, f32), (F,)) * INV_STD).astype(f32)
        scale = f32(1.0 / (6.283185307179586 * float(cycles_per_row)))
        disp = np.zeros((F, T, E, R), f32) if movie else None
        best = um = up = prev = None
        bn = np.zeros((F, E, R), np.int64); pending = np.zeros((F, E, R), bool)
        for n in range(T):
            z = warp(pre, displacement(A, n, shape_q16, amp_q16, o["peak_q24"], p, row0, row1), cycles_per_row, lut)
            for f in range(F):
                if k[f] != 0:                                                            # no draw where k == 0
                    z[f] = (z[f] + (k[f] * draws(o["seed"], first_image_id + f, E, R, n).astype(f32)).astype(f32)).astype(f32)
            re = np.zeros((F, E, R), f32); im = np.zeros((F, E, R), f32)
            for i in range(-a, a + 1):
                u = _shifted(pre, i); v = _shifted(z, i)
                ok = _inside(R, i)
                tr = ((v[..., 0] * u[..., 0]).astype(f32) + (v[..., 1] * u[..., 1]).astype(f32)).astype(f32)
                ti = ((v[..., 1] * u[..., 0]).astype(f32) - (v[..., 0] * u[..., 1]).astype(f32)).astype(f32)
                re = np.where(ok, (re + tr).astype(f32), re); im = np.where(ok, (im + ti).astype(f32), im)
            d = (atan2f(im, re) * scale).astype(f32)
            if movie:
                disp[:, n] = d
            if n == 0:
                best = d.copy(); um = np.zeros_like(d); up = np.zeros_like(d); pending[:] = True
            else:
                up = np.where(pending, d, up); pending[:] = False
                win = d > best                                                           # (a NaN compares false on either side)
                best = np.where(win, d, best); bn = np.where(win, n, bn); um = np.where(win, prev, um); pending = win
            prev = d
        den = ((um - (f32(2.0) * best).astype(f32)).astype(f32) + up).astype(f32)
        num = (f32(0.5) * (um - up).astype(f32)).astype(f32)
        bad = (bn == 0) | (bn == T - 1) | (den == 0)
        peak_time = np.where(bad, f32(np.nan), (bn.astype(f32) + (num / np.where(bad, f32(1.0), den)).astype(f32)).astype(f32)).astype(f32)
        truth_arrival = np.where(A >= NEVER, f32(np.inf), (A.astype(f32) * f32(2.0 ** -16)).astype(f32)).astype(f32)
    table = np.zeros(256, f32); table[:len(speed_f)] = np.asarray(speed_f, f32)
    out = dict(peak_time=peak_time, peak_disp=best, truth_arrival=truth_arrival, truth_speed=table[np.asarray(tissue).astype(np.int64)], arrival=A)
    if movie:
        out["disp"] = disp
    return out


def speed(peak_time, pitch_mm, **opts):
    """dict(speed, modulus, quality [F][E][R]) of mcrt_shear_speed_frames"""
    o = dict(DEFAULTS, **opts)
    pt = np.asarray(peak_time, f32)
    F, E, R = pt.shape
    b, v, p = int(o["speed_lines"]), int(o["avg_rows"]), int(o["push_line"])
    kf = f32(float(f32(o["prf_hz"])) * 0.001); d3 = (f32(3.0) * f32(o["density"])).astype(f32)
    with np.errstate(**QUIET):
        # the row means of every line: the sum ascends over the rows inside the line, NaN rows skipped
        s = np.zeros((F, E, R), f32); c = np.zeros((F, E, R), np.int64)
        for i in range(-v, v + 1):
            x = _shifted(pt, i, fill=np.nan)
            ok = _inside(R, i) & ~np.isnan(x)
            s = np.where(ok, (s + np.where(ok, x, f32(0.0))).astype(f32), s); c = c + ok
        y = (s / c.astype(f32)).astype(f32)                                              # [F][E][R]; no row: 0 / 0, a NaN

        def line(j):                                                                     # y of line e + j, zeros where it is outside (masked below)
            out = np.zeros_like(y)
            lo, hi = max(0, -j), min(E, E - j)
            if lo < hi:
                out[:, lo:hi] = y[:, lo + j:hi + j]
            return out

        e = np.arange(E)
        window = ((e - b >= 0) & (e + b < E) & ~((e - b <= p) & (p <= e + b)))[None, :, None]
        total = np.zeros((F, E, R), f32); bad = np.zeros((F, E, R), bool)
        for j in range(-b, b + 1):
            yj = line(j)
            bad |= np.isnan(yj); total = (total + yj).astype(f32)
        mean = (total / f32(2 * b + 1)).astype(f32)
        num = np.zeros((F, E, R), f32); den = f32(0.0); syy = np.zeros((F, E, R), f32)
        for j in range(-b, b + 1):
            yj = line(j); t = f32(2 * j); dy = (yj - mean).astype(f32)
            num = (num + (t * yj).astype(f32)).astype(f32); den = f32(den + f32(t * t)); syy = (syy + (dy * dy).astype(f32)).astype(f32)
        slope = ((f32(2.0) * num).astype(f32) / den).astype(f32)
        slope = np.where((e < p)[None, :, None], -slope, slope)
        valid = window & ~bad & (slope > 0)
        safe = np.where(valid, slope, f32(1.0))
        sp = ((np.asarray(pitch_mm, f32).reshape(1, 1, R) * kf).astype(f32) / safe).astype(f32)
        mod = (d3 * (sp * sp).astype(f32)).astype(f32)
        r2 = ((num * num).astype(f32) / (den * syy).astype(f32)).astype(f32)
        q = np.where(r2 > 1, f32(1.0), np.where(r2 >= 0, r2, f32(0.0))).astype(f32)
    nan = f32(np.nan)
    return dict(speed=np.where(valid, sp, nan).astype(f32), modulus=np.where(valid, mod, nan).astype(f32), quality=np.where(valid, q, f32(0.0)).astype(f32))
