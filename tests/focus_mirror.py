"""numpy float32 mirror of mcrt_convolve_frames_depth (include/mcrt.h) and a restatement of mcrt_psf_focus_kernels with Python's math module
(glibc's exp and sqrt, as std::exp / std::sqrt): the references of tests/test_focus_contract.py and tests/test_gpu_focus.py."""
import math
import numpy as np

f32 = np.float32


def convolve_depth(img, ax, lat_rows):
    """img [E][R] (the device layout), ax [n_ax], lat_rows [R][n_lat] -> the image after both passes.  The reference's index ranges
    (rfimage.h:93-123): axial rows [n_ax, R-n_ax), lateral columns [n_lat/2, E-n_lat); sums sequential over k from 0, one float32 rounding per
    multiply and per add; pixels outside the window keep their bits."""
    img = np.ascontiguousarray(img, f32)
    ax = np.ascontiguousarray(ax, f32); lat = np.ascontiguousarray(lat_rows, f32)
    E, R = img.shape
    na, nl = ax.size, lat.shape[1]
    assert lat.shape[0] == R
    out = img.copy()
    if R <= 2 * na:
        return out
    rows = slice(na, R - na)
    tmp = np.zeros_like(img)
    with np.errstate(all="ignore"):
        conv = np.zeros((E, R - 2 * na), f32)
        for k in range(na):
            conv = (conv + (img[:, na + k:R - na + k] * ax[k]).astype(f32)).astype(f32)
        tmp[:, rows] = conv
        c0, c1 = nl // 2, E - nl
        if c1 <= c0:
            return out
        w = lat[rows].T                                        # [n_lat][rows]
        conv = np.zeros((c1 - c0, R - 2 * na), f32)
        for k in range(nl):
            conv = (conv + (tmp[c0 + k:c1 + k, rows] * w[k][None, :]).astype(f32)).astype(f32)
        out[c0:c1, rows] = conv
    return out


def psf_focus_rows(var_y, res_um, n_rows, row_mm, focus_mm, focal_range_mm, n_lat):
    """mcrt_psf_focus_kernels restated: float32 [n_rows][n_lat]"""
    res = f32(f32(res_um) / f32(1000.0))
    half = f32(f32(f32(n_lat * res_um) / f32(1000.0)) / f32(2.0))
    ys = [f32(f32(f32(i) * res) - half) for i in range(n_lat)]
    vy = float(f32(var_y))
    out = np.empty((n_rows, n_lat), f32)
    for r in range(n_rows):
        z = r * row_mm
        var, g = vy, 1.0
        if focus_mm:
            zf = min(focus_mm, key=lambda f: abs(z - float(f32(f))))          # min keeps the first (shallowest) of equals
            q = (z - float(f32(zf))) / float(f32(focal_range_mm))
            var = vy * (1.0 + q * q)
            g = math.sqrt(vy / var)
        for i, y in enumerate(ys):
            y2 = float(y) * float(y)
            out[r, i] = f32(g * math.exp(-0.5 * (y2 / var)))
    return out
