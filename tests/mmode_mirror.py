"""numpy mirror of M-mode, a reading of the text of include/mcrt.h alone (mcrt_mmode_table, mcrt_mmode_waveform, mcrt_mmode_bulk,
mcrt_mmode_draws, mcrt_mmode_rows, mcrt_mmode_lines_frames, mcrt_mmode_picture_frames): float32 arrays, one rounding per operation (numpy
rounds every float32 operation once; / and sqrt are correctly rounded), integers where the header has integers, the host formulas in
double.  The line reading (the rotor, the turn) and the Philox blocks are strain_mirror's, not derived again."""
import math
import numpy as np

from strain_mirror import rotor, _turn, philox4x32_10, INV_STD, QUIET

f32 = np.float32
LABEL_NONE = 255
COUNTER = 0x4D4D4F44
SATURATION = 127 << 24
DEFAULTS = dict(n_pulses=1024, sigma=0.0, seed=COUNTER)
DISPLAY_DEFAULTS = dict(hop=4, height=400, row_lo=0, row_hi=0, dynamic_range_db=60.0, gain_db=0.0, ref=0.0)


def mmode_table(dilation):
    """int32 [n_labels]: llrint(dilation * 2^24) in double"""
    out = [int(np.rint(float(d) * 16777216.0)) for d in np.asarray(dilation, np.float64).reshape(-1)]
    assert all(abs(q) <= 1 << 22 for q in out)
    return np.array(out, np.int32)


def waveform(prf_hz, beats_per_min, T):
    """int32 [T]: spectral_mirror.pulse_waveform's x and s, llrint(65536 * (x < 0.3 ? s * s : 0))"""
    out = np.zeros(T, np.int32)
    for t in range(T):
        u = t * beats_per_min / (60.0 * prf_hz)
        x = u - math.floor(u)
        s = math.sin(3.141592653589793 * x / 0.3)
        out[t] = int(np.rint(65536.0 * (s * s if x < 0.3 else 0.0)))
    return out


def bulk(prf_hz, cycles_per_min, amplitude_rows, T):
    """int32 [T]: llrint(amplitude_rows * 2^24 * sin(2 pi t cycles_per_min / (60 prf_hz)))"""
    out = np.zeros(T, np.int32)
    for t in range(T):
        out[t] = int(np.rint(amplitude_rows * 16777216.0 * math.sin(6.283185307179586 * t * cycles_per_min / (60.0 * prf_hz))))
    return out


def draws(seed, image_id, line, R, T):
    """int32 [T][R][2]: one block per (row, pulse), counter (line, r, 0x4D4D4F44, t), key (seed, image_id)"""
    t, r = np.meshgrid(np.arange(T, dtype=np.uint64), np.arange(R, dtype=np.uint64), indexing="ij")
    o = philox4x32_10(np.full_like(t, line), r, np.uint64(COUNTER), t, seed, image_id)
    lo = lambda w: (w & np.uint64(0xffff)).astype(np.int64); hi = lambda w: (w >> np.uint64(16)).astype(np.int64)
    d = np.empty((T, R, 2), np.int32)
    d[..., 0] = (lo(o[0]) + hi(o[0]) + lo(o[1]) + hi(o[1])) - 131070
    d[..., 1] = (lo(o[2]) + hi(o[2]) + lo(o[3]) + hi(o[3])) - 131070
    return d


def rows(row_lo, row_hi, H):
    """(idx uint32 [H], wt float32 [H]) of mcrt_mmode_rows, in double"""
    idx = np.zeros(H, np.uint32); wt = np.zeros(H, f32)
    for y in range(H):
        p = float(row_lo) + (y + 0.5) * float(row_hi - row_lo) / float(H) - 0.5
        f = math.floor(p)
        if f < row_lo:
            idx[y], wt[y] = row_lo, 0.0
        elif f > row_hi - 1:
            idx[y], wt[y] = row_hi - 1, 0.0
        else:
            idx[y], wt[y] = f, min(f32(1.0), max(f32(0.0), f32(p - f)))
    return idx, wt


def displacement(tissue_line, dil_q24, w_q16, bulk_q24):
    """U int64 [T][R] of THE INTEGERS for one line's labels [R]"""
    table = np.zeros(256, np.int64); table[:len(dil_q24)] = np.asarray(dil_q24, np.int64)
    d = table[np.asarray(tissue_line).astype(np.int64)]
    D = np.cumsum(d) - d                                                                 # D[q] = the dilations above q
    u = ((D[None, :] * np.asarray(w_q16, np.int64)[:, None]) >> 16) + np.asarray(bulk_q24, np.int64)[:, None]
    return np.clip(u, -SATURATION, SATURATION)


def lines(iq, tissue, which, dil_q24, w_q16, bulk_q24, cycles_per_row, sigma=0.0, seed=COUNTER, first_image_id=0):
    """dict(env, truth_disp float32 [n_lines][T][R], iq_out float32 [n_lines][T][R][2], truth_label uint8 [n_lines][T][R]) of
    mcrt_mmode_lines_frames; which: [n_lines][2] (image, line); sigma: a number or [F]"""
    iq = np.asarray(iq, f32); tissue = np.asarray(tissue, np.uint8)
    F, E, R, _ = iq.shape
    T = len(w_q16)
    which = np.asarray(which, np.int64).reshape(-1, 2)
    carrier = int(np.rint(float(cycles_per_row) * 4294967296.0))
    lut = rotor()
    k = (np.broadcast_to(np.asarray(sigma, f32), (F,)) * INV_STD).astype(f32)
    q = np.arange(R, dtype=np.int64)
    out = dict(env=np.zeros((len(which), T, R), f32), iq_out=np.zeros((len(which), T, R, 2), f32), truth_disp=np.zeros((len(which), T, R), f32),
               truth_label=np.zeros((len(which), T, R), np.uint8))
    for j, (f, e) in enumerate(which):
        pre, lab = iq[f, e], tissue[f, e]
        U = displacement(lab, dil_q24, w_q16, bulk_q24)
        s0 = q[None, :] + (U >> 24); fr = U & 0xFFFFFF
        th0 = ((carrier * fr) >> 24) & 0xFFFFFFFF
        th1 = ((carrier * (fr - (1 << 24))) >> 24) & 0xFFFFFFFF

        def tap(at):
            ok = (at >= 0) & (at < R)
            return np.where(ok[..., None], pre[np.clip(at, 0, R - 1)], f32(0.0)).astype(f32)

        with np.errstate(**QUIET):
            w1 = (fr.astype(f32) * f32(2.0 ** -24)).astype(f32); w0 = (f32(1.0) - w1).astype(f32)
            ar, ai = _turn(tap(s0), th0, lut); br, bi = _turn(tap(s0 + 1), th1, lut)
            zr = ((w0 * ar).astype(f32) + (w1 * br).astype(f32)).astype(f32); zi = ((w0 * ai).astype(f32) + (w1 * bi).astype(f32)).astype(f32)
            if k[f] != 0:                                                                # no draw where k == 0
                d = draws(seed, first_image_id + int(f), int(e), R, T).astype(f32)
                zr = (zr + (k[f] * d[..., 0]).astype(f32)).astype(f32); zi = (zi + (k[f] * d[..., 1]).astype(f32)).astype(f32)
            out["env"][j] = np.sqrt(((zr * zr).astype(f32) + (zi * zi).astype(f32)).astype(f32)).astype(f32)
        out["iq_out"][j] = np.stack([zr, zi], axis=-1)
        out["truth_disp"][j] = (U.astype(np.int32).astype(f32) * f32(2.0 ** -24)).astype(f32)
        sr = s0 + (fr >> 23)
        out["truth_label"][j] = np.where((sr >= 0) & (sr < R), lab[np.clip(sr, 0, R - 1)], LABEL_NONE)
    return out


def picture(env, truth_label=None, truth_disp=None, hop=4, height=400, row_lo=0, row_hi=0, dynamic_range_db=60.0, gain_db=0.0, ref=0.0):
    """dict(out uint8 [n_lines][H][W], peak float32 [n_lines], mean float32 [n_lines][W][R], label_out uint8 and disp_out float32
    [n_lines][H][W] where their truths are given) of mcrt_mmode_picture_frames; log10 in float32 through numpy (the device's may differ
    by one level)"""
    env = np.asarray(env, f32)
    n, T, R = env.shape
    W, H = T // hop, height
    hi = row_hi if row_hi else R
    assert W >= 1 and 0 <= row_lo < hi <= R
    idx, wt = rows(row_lo, hi, H)
    i0 = idx.astype(np.int64); i1 = np.minimum(i0 + 1, hi - 1)
    rn = np.minimum(i0 + (wt >= f32(0.5)), hi - 1)
    with np.errstate(**QUIET):
        s = np.zeros((n, W, R), f32)
        for k in range(hop):                                                             # ascending from 0.0f
            s = (s + env[:, k:W * hop:hop]).astype(f32)
        mean = (s / f32(hop)).astype(f32)
        a = np.where(np.isfinite(mean) & (mean > 0), mean, f32(0.0)).astype(f32)
        peak = a[:, :, row_lo:hi].reshape(n, -1).max(axis=1).astype(f32)
        r = np.full(n, f32(ref), f32) if ref > 0 else peak
        qn = (a / r[:, None, None]).astype(f32)
        dr, gain = f32(dynamic_range_db), f32(gain_db)
        g = ((((f32(20.0) * np.log10(np.where(a > 0, qn, f32(1))).astype(f32)).astype(f32) + gain).astype(f32) + dr).astype(f32) / dr).astype(f32)
        g = np.where(a > 0, np.clip(g, f32(0.0), f32(1.0)), f32(0.0)).astype(f32)       # [n][W][R]
        v = (((f32(1.0) - wt).astype(f32)[None, None, :] * g[:, :, i0]).astype(f32) + (wt[None, None, :] * g[:, :, i1]).astype(f32)).astype(f32)   # [n][W][H]
        out = ((v * f32(255.0)).astype(f32) + f32(0.5)).astype(f32).astype(np.uint8).transpose(0, 2, 1)
    res = dict(out=np.ascontiguousarray(out), peak=peak, mean=mean)
    if truth_label is not None:
        res["label_out"] = np.ascontiguousarray(np.asarray(truth_label, np.uint8)[:, 0:W * hop:hop][:, :, rn].transpose(0, 2, 1))
    if truth_disp is not None:
        res["disp_out"] = np.ascontiguousarray(np.asarray(truth_disp, f32)[:, 0:W * hop:hop][:, :, rn].transpose(0, 2, 1))
    return res
