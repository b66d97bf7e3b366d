"""numpy float32 mirror of mcrt_elevation_frames and mcrt_elevation_planes (include/mcrt.h) and a restatement of
mcrt_psf_elevation_kernels with Python's math module (glibc's exp and sqrt, as std::exp / std::sqrt): the references of
tests/test_elevation_contract.py and tests/test_gpu_elevation.py."""
import math
import numpy as np

f32 = np.float32


def plane_z_mm(n_planes, pitch_um):
    """z_k [mm], float32 [K]: centred, plane (K-1)//2 lies in the probe's own plane"""
    c = (n_planes - 1) // 2
    return np.array([f32((float(k) - float(c)) * float(pitch_um) / 1000.0) for k in range(n_planes)], f32)


def planes(pos, dirs, axis, n_planes, pitch_um):
    """mcrt_elevation_planes: (pos [K][E][3], dir [K][E][3], z_mm [K]); one float32 multiply and one float32 add per coordinate"""
    pos = np.ascontiguousarray(pos, f32).reshape(-1, 3); dirs = np.ascontiguousarray(dirs, f32).reshape(-1, 3)
    axis = np.ascontiguousarray(axis, f32)
    z = plane_z_mm(n_planes, pitch_um)
    po = np.empty((n_planes,) + pos.shape, f32); do = np.empty_like(po)
    for k in range(n_planes):
        o = f32(float(z[k]) / 10.0)
        shift = (o * axis).astype(f32)
        po[k] = (pos + shift[None, :]).astype(f32)
        do[k] = dirs
    return po, do, z


def psf_elevation_rows(var_z, pitch_um, n_rows, row_mm, focus_mm, focal_range_mm, n_planes, normalize):
    """mcrt_psf_elevation_kernels restated: float32 [n_rows][n_planes]"""
    z2 = [float(z) * float(z) for z in plane_z_mm(n_planes, pitch_um)]
    vz = float(f32(var_z))
    out = np.empty((n_rows, n_planes), f32)
    for r in range(n_rows):
        z = r * row_mm
        var, g = vz, 1.0
        if focus_mm:
            zf = min(focus_mm, key=lambda f: abs(z - float(f32(f))))          # min keeps the first (shallowest) of equals
            q = (z - float(f32(zf))) / float(f32(focal_range_mm))
            var = vz * (1.0 + q * q)
            g = math.sqrt(vz / var)
        v = [g * math.exp(-0.5 * (x / var)) for x in z2]
        s = 0.0
        for x in v:
            s += x
        for k, x in enumerate(v):
            out[r, k] = f32(x / s) if normalize else f32(x)
    return out


def fold(stack, w_rows):
    """stack [F][K][E][R] (the device layout), w_rows [R][K] -> [F][E][R]: the sum over k in order from 0.0f, one float32 rounding per
    multiply and per add.  A NaN or an infinity of a plane reaches the sum under any weight."""
    stack = np.ascontiguousarray(stack, f32); w = np.ascontiguousarray(w_rows, f32)
    F, K, E, R = stack.shape
    assert w.shape == (R, K)
    acc = np.zeros((F, E, R), f32)
    with np.errstate(all="ignore"):
        for k in range(K):
            acc = (acc + (stack[:, k] * w[None, None, :, k]).astype(f32)).astype(f32)
    return acc
