"""The contract of mcrt_recon_frames (include/mcrt.h) in numpy: float32 where the contract says float, one rounding per operation, int64 sums
through np.add.at.  It takes the product's own host floats (A, b from mcrt_recon_transform; row_u = float32(row_mm / unit_mm)) so that the
comparison is about the device's arithmetic and not about a matrix inverse."""
import numpy as np

f32 = np.float32
MEAN, MAX = 0, 1
DEFAULTS = dict(mode=MEAN, value_max=1024.0, fill_radius=1, fill_min=1, empty=0.0)


def positions(pos, dirs, R, row_u):
    """P [F][E][R][3], float32: pos + dir * ((float)r * row_u)"""
    t = (np.arange(R, dtype=f32) * f32(row_u)).astype(f32)
    return (pos[:, :, None, :].astype(f32) + (dirs[:, :, None, :].astype(f32) * t[None, None, :, None]).astype(f32)).astype(f32)


def indices(P, A, b):
    """i_c = floorf(x_c + 0.5f) as floats [..][3] (c = u, v, w), x_c = ((b_c + P_x A_c0) + P_y A_c1) + P_z A_c2"""
    A = np.asarray(A, f32).reshape(3, 3); b = np.asarray(b, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        out = np.empty(P.shape, f32)
        for c in range(3):
            x = (b[c] + (P[..., 0] * A[c, 0]).astype(f32)).astype(f32)
            x = (x + (P[..., 1] * A[c, 1]).astype(f32)).astype(f32)
            x = (x + (P[..., 2] * A[c, 2]).astype(f32)).astype(f32)
            out[..., c] = np.floor((x + f32(0.5)).astype(f32))
    return out


def splat(stack, pos, dirs, A, b, row_u, shape, mode=MEAN, value_max=1024.0):
    """-> (acc int64 [n], count uint32 [n], stats uint32 [2], voxel int64 [F][E][R] (-1: not binned)); shape = (nw, nv, nu)"""
    stack = np.ascontiguousarray(stack, f32)
    F, E, R = stack.shape
    nw, nv, nu = shape
    n = nw * nv * nu
    idx = indices(positions(np.asarray(pos, f32).reshape(F, E, 3), np.asarray(dirs, f32).reshape(F, E, 3), R, row_u), A, b)
    with np.errstate(invalid="ignore"):
        inside = np.ones(stack.shape, bool)
        for c, nc in enumerate((nu, nv, nw)):
            inside &= (idx[..., c] >= f32(0.0)) & (idx[..., c] < f32(nc))
        usable = np.isfinite(stack) & (np.abs(stack) < f32(value_max))
    take = inside & usable
    stats = np.array([(~inside).sum(), (inside & ~usable).sum()], np.uint32)
    ii = np.where(take[..., None], idx, 0).astype(np.int64)
    vox = (ii[..., 2] * nv + ii[..., 1]) * nu + ii[..., 0]
    qscale = 2.0 ** 31 / float(f32(value_max))
    q = np.trunc(np.where(take, stack, 0).astype(np.float64) * qscale).astype(np.int64)
    count = np.zeros(n, np.int64)
    np.add.at(count, vox[take], 1)
    if mode == MAX:
        acc = np.full(n, np.iinfo(np.int64).min, np.int64)
        np.maximum.at(acc, vox[take], q[take])
    else:
        acc = np.zeros(n, np.int64)
        np.add.at(acc, vox[take], q[take])
    return acc, count.astype(np.uint32), stats, np.where(take, vox, -1)


def resolve(acc, count, shape, mode=MEAN, value_max=1024.0, fill_radius=1, fill_min=1, empty=0.0):
    """-> out float32 [nw][nv][nu]: sampled voxels resolved, holes filled from SAMPLED voxels only"""
    nw, nv, nu = shape
    qscale = 2.0 ** 31 / float(f32(value_max))
    cnt = count.reshape(shape).astype(np.int64)
    sampled = cnt > 0
    a = acc.reshape(shape).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        val = (a / qscale if mode == MAX else a / (cnt.astype(np.float64) * qscale)).astype(f32)
    val = np.where(sampled, val, f32(0.0)).astype(f32)
    out = np.where(sampled, val, f32(empty)).astype(f32)
    H = int(fill_radius)
    todo = ~sampled
    pv = np.pad(val, H, constant_values=0) if H else val
    ps = np.pad(sampled, H, constant_values=False) if H else sampled
    for h in range(1, H + 1):
        s = np.zeros(shape, f32); n = np.zeros(shape, np.int64)
        for dw in range(-h, h + 1):
            for dv in range(-h, h + 1):
                for du in range(-h, h + 1):
                    sl = (slice(H + dw, H + dw + nw), slice(H + dv, H + dv + nv), slice(H + du, H + du + nu))
                    m = ps[sl]
                    s = np.where(m, (s + pv[sl]).astype(f32), s)
                    n += m
        ok = todo & (n >= int(fill_min))
        with np.errstate(invalid="ignore", divide="ignore"):
            out = np.where(ok, (s / n.astype(f32)).astype(f32), out)
        todo &= ~ok
    return out


def recon(stack, pos, dirs, A, b, row_u, shape, mode=MEAN, value_max=1024.0, fill_radius=1, fill_min=1, empty=0.0):
    """mcrt_recon_frames -> (out float32 [nw][nv][nu], count uint32 the same, stats uint32 [2])"""
    acc, count, stats, _ = splat(stack, pos, dirs, A, b, row_u, shape, mode, value_max)
    return resolve(acc, count, shape, mode, value_max, fill_radius, fill_min, empty), count.reshape(shape), stats
