"""numpy mirror of spectral Doppler, a reading of the text of include/mcrt.h alone (mcrt_spectral_rotor, mcrt_spectral_phase,
mcrt_spectral_profile, mcrt_spectral_rates, mcrt_spectral_window, mcrt_spectral_twiddles, mcrt_spectral_draws, mcrt_pulse_waveform,
mcrt_spectral_series_frames, mcrt_spectral_frames, mcrt_sonogram_frames): float32 arrays, one rounding per operation (numpy rounds every
float32 operation once; / and sqrt are correctly rounded), phases as Python ints, the host formulas in double through math."""
import math
import numpy as np

from flow_mirror import philox4x32_10, INV_STD, QUIET

f32 = np.float32
TWO_PI = 6.283185307179586
WALL_NONE, WALL_MEAN = 0, 1
FFT_SIZES = (32, 64, 128, 256, 512)
DEFAULT_SEED = 0x53504543


def rotor():
    return np.array([(f32(math.cos(TWO_PI * i / 4096.0)), f32(math.sin(TWO_PI * i / 4096.0))) for i in range(4096)], f32)


def llrint(x):
    """round half to even, as llrint does in the default rounding mode"""
    return int(round(x))


def phase(v_nyq, speed):
    """Python ints [T]"""
    out, p = [], 0
    for s in np.asarray(speed, f32):
        out.append(p)
        p += llrint(float(s) / v_nyq * 2147483648.0)
    return out


def profile(tissue_line, row0, G, moving, exponent):
    t = [int(v) for v in np.asarray(tissue_line, np.uint8)]
    frac = np.zeros(G, f32)
    for i in range(G):
        r = row0 + i
        l = t[r]
        if l >= len(moving) or not moving[l]:
            continue
        a = b = r
        while a > 0 and t[a - 1] == l:
            a -= 1
        while b + 1 < len(t) and t[b + 1] == l:
            b += 1
        x = (r - (a + b) / 2.0) / ((b - a + 1) / 2.0)
        frac[i] = f32(1.0) if exponent == 0 else f32(1.0 - math.pow(math.fabs(x), exponent))
    return frac


def rates(frac, axial):
    return np.array([llrint(65536.0 * float(f) * axial) for f in np.asarray(frac, f32)], np.int32)


def window(kind, N):
    if kind == 0:
        return np.ones(N, f32)
    return np.array([f32(0.5 - 0.5 * math.cos(TWO_PI * n / N)) for n in range(N)], f32)


def twiddles(N):
    return np.array([(f32(math.cos(TWO_PI * k / N)), f32(0.0 - math.sin(TWO_PI * k / N))) for k in range(N // 2)], f32)


def draws(seed, image_id, line, row0, T):
    """int32 [T][2]: one block per pulse, counter (line, row0, 0x53504543, t), key (seed, image_id)"""
    t = np.arange(T, dtype=np.uint64)
    o = philox4x32_10(np.uint64(line), np.uint64(row0), np.uint64(0x53504543), t, seed, image_id)
    lo = lambda w: (w & np.uint64(0xffff)).astype(np.int64); hi = lambda w: (w >> np.uint64(16)).astype(np.int64)
    d = np.empty((T, 2), np.int32)
    d[:, 0] = (lo(o[0]) + hi(o[0]) + lo(o[1]) + hi(o[1])) - 131070
    d[:, 1] = (lo(o[2]) + hi(o[2]) + lo(o[3]) + hi(o[3])) - 131070
    return d


def pulse_waveform(prf_hz, beats_per_min, v_peak, v_min, T):
    out = np.zeros(T, f32)
    for t in range(T):
        u = t * beats_per_min / (60.0 * prf_hz)
        x = u - math.floor(u)
        s = math.sin(3.141592653589793 * x / 0.3)
        out[t] = f32(v_min + (v_peak - v_min) * (s * s if x < 0.3 else 0.0))
    return out


def rotor_index(ph, rate):
    """idx [T] of Python-int phases and one rate: theta = (uint32)((phase * rate) >> 16), idx = ((theta + 0x80000) >> 20) & 4095"""
    return np.array([((((p * int(rate)) >> 16) & 0xFFFFFFFF) + 0x80000 >> 20) & 4095 for p in ph], np.int64)


def series(iq_static, iq_moving, gates, weight, rate, ph, sigma=0.0, seed=DEFAULT_SEED, first_image_id=0, lut=None):
    """z float32 [n_gates][T][2].  iq_* [F][E][R][2] (iq_static may be None), gates [n_gates][3], weight [G], rate [n_gates][G], ph: Python
    ints [T]; sigma: a number or [F]"""
    lut = rotor() if lut is None else lut
    m = np.asarray(iq_moving, f32)
    w = np.asarray(weight, f32); G, T = len(w), len(ph)
    rate = np.asarray(rate, np.int32).reshape(len(gates), G)
    sig = np.broadcast_to(np.asarray(sigma, f32), (m.shape[0],))
    wnorm = f32(math.sqrt(sum(float(v) * float(v) for v in w)))
    out = np.empty((len(gates), T, 2), f32)
    with np.errstate(**QUIET):
        for j, (image, line, row0) in enumerate(np.asarray(gates).reshape(-1, 3).tolist()):
            zs = np.zeros(2, f32); acc = np.zeros((T, 2), f32)
            for i in range(G):
                if iq_static is not None:
                    zs = (zs + (w[i] * np.asarray(iq_static, f32)[image, line, row0 + i]).astype(f32)).astype(f32)
                A = (w[i] * m[image, line, row0 + i]).astype(f32)
                cs = lut[rotor_index(ph, rate[j, i])]
                c, s = cs[:, 0], cs[:, 1]
                acc[:, 0] = (acc[:, 0] + ((A[0] * c).astype(f32) - (A[1] * s).astype(f32)).astype(f32)).astype(f32)
                acc[:, 1] = (acc[:, 1] + ((A[0] * s).astype(f32) + (A[1] * c).astype(f32)).astype(f32)).astype(f32)
            z = (zs[None, :] + acc).astype(f32)
            k = f32(f32(sig[image] * wnorm) * INV_STD)
            if k != 0:
                d = draws(seed, first_image_id + image, line, row0, T).astype(f32)
                z = (z + (k * d).astype(f32)).astype(f32)
            out[j] = z
    return out


def pair_sum(x, axis):
    """the plain tree over a power-of-two axis: neighbours in pairs, level by level"""
    x = np.moveaxis(np.asarray(x, f32), axis, -1)
    while x.shape[-1] > 1:
        x = (x[..., 0::2] + x[..., 1::2]).astype(f32)
    return x[..., 0]


def bit_reverse(N):
    bits = N.bit_length() - 1
    return np.array([int(format(n, "0%db" % bits)[::-1], 2) for n in range(N)])


def fft(y, tw):
    """radix 2, decimation in time, over the last but one axis of y [...][N][2], as the contract orders it"""
    y = np.array(y, f32)
    N = y.shape[-2]
    out = np.empty_like(y)
    out[..., bit_reverse(N), :] = y
    y = out
    s = 1
    with np.errstate(**QUIET):
        while (1 << s) <= N:
            half = 1 << (s - 1)
            w = np.asarray(tw, f32)[np.arange(half) * (N >> s)]
            blk = y.reshape(y.shape[:-2] + (N // (2 * half), 2, half, 2))
            u = blk[..., 0, :, :].copy(); v = blk[..., 1, :, :].copy()
            tr = ((v[..., 0] * w[:, 0]).astype(f32) - (v[..., 1] * w[:, 1]).astype(f32)).astype(f32)
            ti = ((v[..., 0] * w[:, 1]).astype(f32) + (v[..., 1] * w[:, 0]).astype(f32)).astype(f32)
            t = np.stack([tr, ti], axis=-1)
            blk[..., 0, :, :] = (u + t).astype(f32); blk[..., 1, :, :] = (u - t).astype(f32)
            s += 1
    return y


def n_cols(T, N, hop):
    return (T - N) // hop + 1


def spectrum(z, h, v_nyq, N=128, hop=32, wall=WALL_MEAN, wall_bins=2, tw=None):
    """(power float32 [n_gates][n_cols][N] in velocity order, mean float32 [n_gates][n_cols]) of z [n_gates][T][2]"""
    z = np.asarray(z, f32)
    tw = twiddles(N) if tw is None else tw
    C_ = n_cols(z.shape[1], N, hop)
    idx = (np.arange(C_) * hop)[:, None] + np.arange(N)[None, :]
    x = z[:, idx, :]                                                   # [n_gates][n_cols][N][2]
    with np.errstate(**QUIET):
        if wall == WALL_MEAN:
            mean = (pair_sum(x, 2) / f32(N)).astype(f32)
            x = (x - mean[:, :, None, :]).astype(f32)
        y = (x * np.asarray(h, f32)[None, None, :, None]).astype(f32)
        X = fft(y, tw)
        P = ((X[..., 0] * X[..., 0]).astype(f32) + (X[..., 1] * X[..., 1]).astype(f32)).astype(f32)
        out = P[..., (np.arange(N) + N // 2) % N]
        d = np.arange(N) - N // 2
        out = np.where(np.abs(d) < wall_bins, f32(0.0), out).astype(f32)
        num = pair_sum((out * d.astype(f32)).astype(f32), -1); den = pair_sum(out, -1)
        scale = f32(2.0 * v_nyq / N)
        mean_v = np.where(den > 0, ((num / np.where(den > 0, den, f32(1))).astype(f32) * scale).astype(f32), f32(0.0)).astype(f32)
    return out, mean_v


def sonogram(power, dynamic_range_db=40.0, gain_db=0.0, ref=0.0):
    """(bytes uint8 [n_gates][N][n_cols], peak float32 [n_gates]) of power [n_gates][n_cols][N]; log10 in float32 through numpy (the device's may
    differ by one level)"""
    p = np.asarray(power, f32)
    with np.errstate(**QUIET):
        p = np.where(np.isfinite(p) & (p > 0), p, f32(0.0)).astype(f32)
        peak = p.reshape(p.shape[0], -1).max(axis=1).astype(f32)
        r = np.full(p.shape[0], f32(ref), f32) if ref > 0 else peak
        q = (p / r[:, None, None]).astype(f32)
        dr, gain = f32(dynamic_range_db), f32(gain_db)
        v = ((((f32(10.0) * np.log10(np.where(p > 0, q, f32(1))).astype(f32)).astype(f32) + gain).astype(f32) + dr).astype(f32) / dr).astype(f32)
        v = np.where(p > 0, np.clip(v, f32(0.0), f32(1.0)), f32(0.0)).astype(f32)
        b = ((v * f32(255.0)).astype(f32) + f32(0.5)).astype(f32).astype(np.uint8)
    return np.ascontiguousarray(b.transpose(0, 2, 1)[:, ::-1, :]), peak
