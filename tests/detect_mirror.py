"""numpy mirror of quadrature detection (the contract is in include/mcrt.h: mcrt_detect_taps, mcrt_detect_gain, mcrt_psf_carrier,
mcrt_detect_frames): float32 arrays, one astype(np.float32) per rounded operation, the taps formula in double."""
import numpy as np

f32 = np.float32
PI = 3.141592653589793
N_TAPS = (3, 7, 11, 15, 19, 23, 27, 31, 35, 39, 43, 47, 51, 55, 59, 63)


def taps(n_taps=31):
    """the type-III FIR Hilbert transformer under a Hamming window, float32 [n_taps]: antisymmetric, every even offset +0.0"""
    assert n_taps in N_TAPS
    M = (n_taps - 1) // 2
    t = np.zeros(n_taps, f32)
    for m in range(1, M + 1, 2):
        v = f32((2.0 / (PI * m)) * (0.54 + 0.46 * np.cos(PI * m / (M + 1))))
        t[M + m] = v; t[M - m] = -v
    return t


def gain(t, cycles):
    """|2 * sum over odd m, ascending, of t_m * sin(2 pi f m)| in double"""
    M = (len(t) - 1) // 2
    s = 0.0
    for m in range(1, M + 1, 2):
        s += float(t[M + m]) * np.sin(2.0 * PI * cycles * m)
    return abs(2.0 * s)


def carrier(freq_mhz, res_um=145):
    c = float(f32(freq_mhz)) * (float(res_um) / 1000.0)
    return abs(c - np.rint(c))


def quadrature(x, n_taps=31):
    """q of the scan-lines x [..., R] (the last axis is the row): the sum over m = 1, 3, ... <= M in ascending order from 0.0f of
    (xz[r - m] - xz[r + m]) * t_m, the difference, the multiply and the add rounded once each; xz is x between zeros"""
    x = np.ascontiguousarray(x, f32)
    t = taps(n_taps)
    M = (n_taps - 1) // 2
    R = x.shape[-1]
    xz = np.zeros(x.shape[:-1] + (R + 2 * M,), f32)
    xz[..., M:M + R] = x
    q = np.zeros(x.shape, f32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for m in range(1, M + 1, 2):
            d = (xz[..., M - m:M - m + R] - xz[..., M + m:M + m + R]).astype(f32)
            q = (q + (d * t[M + m]).astype(f32)).astype(f32)
    return q


def magnitude(x, q):
    """sqrtf(x * x + q * q): the two squares and their sum rounded once each, the root correctly rounded"""
    x = np.asarray(x, f32); q = np.asarray(q, f32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return np.sqrt(((x * x).astype(f32) + (q * q).astype(f32)).astype(f32)).astype(f32)


def detect(x, n_taps=31):
    """(env, iq) of the scan-lines x [..., R]: env float32 [..., R], iq float32 [..., R, 2] = (x's own bits, q)"""
    x = np.ascontiguousarray(x, f32)
    q = quadrature(x, n_taps)
    return magnitude(x, q), np.stack([x, q], axis=-1)


def reached(r, R, n_taps):
    """the rows of a scan-line of R rows that a NaN at row r reaches: r itself and r +- m for odd m <= M"""
    M = (n_taps - 1) // 2
    return sorted({r} | {r + s * m for m in range(1, M + 1, 2) for s in (-1, 1) if 0 <= r + s * m < R})
