"""numpy float32 mirror of mcrt_convolve_bands_frames (include/mcrt.h) and a restatement of mcrt_psf_band_kernels with Python's math module
(glibc's exp and cos, as std::exp / std::cos): the references of tests/test_bands_contract.py and tests/test_gpu_bands.py.  The fold of the
band images is elevation_mirror.fold (mcrt_band_fold_frames is mcrt_elevation_frames' contract with K = B)."""
import math
import numpy as np

f32 = np.float32


def tap_positions(res_um, n_ax):
    """x_i of mcrt_psf_kernels: (float)i * res - half_ax in float32"""
    res = f32(f32(res_um) / f32(1000.0))
    half = f32(f32(f32(n_ax * res_um) / f32(1000.0)) / f32(2.0))
    return [f32(f32(f32(i) * res) - half) for i in range(n_ax)]


def band_frequency(band_mhz, downshift_mhz_per_mm, min_mhz, z_mm):
    """the centre frequency of a band at depth z_mm, in double from the struct's floats"""
    return max(float(f32(min_mhz)), float(f32(band_mhz)) - float(f32(downshift_mhz_per_mm)) * z_mm)


def axial_taps(freq, var_x, res_um, n_ax):
    """mcrt_psf_kernels' axial taps with a double frequency: float32 [n_ax]"""
    vx = float(f32(var_x))
    out = np.empty(n_ax, f32)
    for i, x in enumerate(tap_positions(res_um, n_ax)):
        x2 = float(x) * float(x)
        out[i] = f32(math.exp(-0.5 * (x2 / vx)) * math.cos(2 * 3.14159 * freq * float(x)))
    return out


def psf_band_rows(band_mhz, weights, var_x, downshift_mhz_per_mm, min_mhz, res_um, n_rows, row_mm, n_ax):
    """mcrt_psf_band_kernels restated: (ax_rows float32 [B][n_rows][n_ax], w_rows float32 [n_rows][B])"""
    B = len(band_mhz)
    weights = [1.0] * B if weights is None else weights
    ax = np.empty((B, n_rows, n_ax), f32)
    for b in range(B):
        last_f, last = None, None
        for r in range(n_rows):
            f = band_frequency(band_mhz[b], downshift_mhz_per_mm, min_mhz, r * row_mm)
            if f != last_f:                                    # (the same frequency gives the same taps: rows at the floor, no downshift)
                last_f, last = f, axial_taps(f, var_x, res_um, n_ax)
            ax[b, r] = last
    s = 0.0
    for x in weights:
        s += float(f32(x))
    w = np.empty((n_rows, B), f32)
    w[:] = np.array([f32(float(f32(x)) / s) for x in weights], f32)[None, :]
    return ax, w


def convolve_bands(img, ax_rows, lateral=None, lat_rows=None):
    """img [E][R] (the device layout), ax_rows [B][R][n_ax], and either lateral [n_lat] or lat_rows [R][n_lat] -> the band images [B][E][R].
    The reference's index ranges (rfimage.h:93-123): axial rows [n_ax, R-n_ax) with ROW r's own taps, lateral columns [n_lat/2, E-n_lat); sums
    sequential over k from 0, one float32 rounding per multiply and per add; pixels outside the windows hold the input's bits."""
    assert (lateral is None) != (lat_rows is None)
    img = np.ascontiguousarray(img, f32); ax = np.ascontiguousarray(ax_rows, f32)
    E, R = img.shape
    B, _, na = ax.shape
    assert ax.shape[1] == R
    lat = np.tile(np.ascontiguousarray(lateral, f32), (R, 1)) if lat_rows is None else np.ascontiguousarray(lat_rows, f32)
    nl = lat.shape[1]
    assert lat.shape[0] == R
    out = np.stack([img.copy() for _ in range(B)])
    if R <= 2 * na:
        return out
    rows = slice(na, R - na)
    c0, c1 = nl // 2, E - nl
    with np.errstate(all="ignore"):
        for b in range(B):
            tmp = np.zeros_like(img)
            conv = np.zeros((E, R - 2 * na), f32)
            for k in range(na):
                conv = (conv + (img[:, na + k:R - na + k] * ax[b, rows, k][None, :]).astype(f32)).astype(f32)
            tmp[:, rows] = conv
            if c1 <= c0:
                continue
            w = lat[rows].T                                    # [n_lat][rows]
            conv = np.zeros((c1 - c0, R - 2 * na), f32)
            for k in range(nl):
                conv = (conv + (tmp[c0 + k:c1 + k, rows] * w[k][None, :]).astype(f32)).astype(f32)
            out[b, c0:c1, rows] = conv
    return out
