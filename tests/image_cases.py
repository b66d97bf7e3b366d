"""Inputs of the image-stage tests (tests/test_oracle_image_stages.py on the CPU, tests/test_gpu_image_stages.py on the MI355X): synthetic
RF columns for the envelope, random convolution taps, the scan-conversion geometries, and the one bit-for-bit comparison they all use."""
import math
import numpy as np

f32 = np.float32

# the envelope sweep: scan-lines x rows, around k_envelope's 64 lane chunks of ceil(R/64) rows and its 2048-row LDS column
ENV_E = (1, 3, 64, 129)
ENV_R = (2, 3, 5, 63, 64, 65, 127, 128, 129, 465, 2047, 2048)

# the convolution sweep: the API's tap counts (1..16 axial, 1..32 lateral) at and around the bounds of rfimage.h:93-123
CONV_AX = (1, 2, 7, 16)
CONV_LAT = (1, 2, 13, 31, 32)

# scan conversion: (radius_mm, total_angle, out_rows, out_cols) and the RF shapes (E, R) they are paired with
SCAN_GEOMETRIES = [(30.0, 1.0471975511965976, 400, 500), (10.0, math.pi / 2, 257, 333), (60.0, 0.3, 64, 48), (20.0, 3.6, 96, 160),
                   (30.0, 1.0471975511965976, 1, 1)]
SCAN_SHAPES = [(E, R) for E in (1, 3, 128) for R in (2, 2048)]


def assert_same_bits(got, want, what=""):
    """NaN exactly where the reference has NaN, every other float bit-identical (-0.0 is not 0.0); no tolerance"""
    got = np.ascontiguousarray(got, f32); want = np.ascontiguousarray(want, f32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    if not np.array_equal(gn, wn):
        i = np.argwhere(gn != wn)[0]
        raise AssertionError("%s: NaN positions differ (%d places, first %s: got %r, want %r)" % (what, int((gn != wn).sum()), tuple(i), got[tuple(i)], want[tuple(i)]))
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~wn
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError("%s: %d floats differ, first at %s: got %r (0x%08x), want %r (0x%08x)" % (
            what, int(bad.sum()), i, got[i], int(got.view(np.uint32)[i]), want[i], int(want.view(np.uint32)[i])))


def _thin(rows, R):
    """the rows of `rows` that can be peaks of one column (1 <= i <= R-2), at least two apart (neighbours cannot both be peaks)"""
    out = []
    for i in sorted(set(rows)):
        if 1 <= i <= R - 2 and (not out or i >= out[-1] + 2):
            out.append(i)
    return out


def _ramps(R, peaks):
    """a column that rises by 1 per row and drops back to 1 right after each of `peaks`: exactly those rows are peaks"""
    c = np.empty(R, f32)
    v = 0.0
    for i in range(R):
        v = 1.0 if (i == 0 or (i - 1) in peaks) else v + 1.0
        c[i] = v
    return c


def _noise(R, rng):
    return rng.standard_normal(R).astype(f32)


def _ascending(R, rng):
    return (np.arange(R, dtype=f32) * f32(0.5) - f32(3.0)).astype(f32)


def _descending(R, rng):
    return (f32(R) - np.arange(R, dtype=f32) * f32(1.25)).astype(f32)


def _constant(R, rng):
    return np.full(R, f32(-2.5))


def _stairs(R, rng):
    """plateaus of 1-5 equal values going up and down: every rise onto a plateau is a peak at the plateau's first row (!(c[i] < c[i+1]))"""
    out = []
    while len(out) < R:
        out += [float(rng.integers(-4, 5)) * 0.75] * int(rng.integers(1, 6))
    return np.asarray(out[:R], f32)


def _alternating(R, rng):
    return (np.where(np.arange(R) % 2 == 0, 1.0, -1.0) * (1.0 + 0.01 * np.arange(R))).astype(f32)


def _saw_on_chunk_starts(R, rng):
    per = -(-R // 64)
    return _ramps(R, _thin([k * per for k in range(1, 65)], R)) * f32(0.375)


def _saw_on_chunk_ends(R, rng):
    per = -(-R // 64)
    return _ramps(R, _thin([k * per - 1 for k in range(1, 65)], R)) * f32(-0.625)


def _edge_peaks(R, rng):
    """peaks at rows 1 and R-2, a flat floor between them"""
    c = np.full(R, f32(0.25))
    c[0] = f32(0.125)
    if R >= 3:
        c[1] = f32(2.0); c[R - 2] = f32(3.0)
    return c


def _negative_start(R, rng):
    """noise after a negative c[0]: the line before the first peak starts from the SIGNED c[0] (rfimage.h:64)"""
    c = _noise(R, rng)
    c[0] = f32(-5.5)
    return c


def _specials(R, rng):
    """noise with -0.0, subnormals, +-inf and NaN taps"""
    c = _noise(R, rng) * f32(1e-3)
    vals = np.array([-0.0, 1e-40, -3e-39, 1.4e-45, np.inf, -np.inf, np.nan, 0.0], f32)
    idx = rng.permutation(R)[:min(R, 3 * len(vals))]
    c[idx] = np.resize(vals, idx.size)
    return c


ENV_FAMILIES = [_noise, _ascending, _descending, _constant, _stairs, _alternating, _saw_on_chunk_starts, _saw_on_chunk_ends, _edge_peaks,
                _negative_start, _specials]


def envelope_image(E, R, seed=0):
    """[E][R] (the device layout): scan-line e is family (e + R) % len(ENV_FAMILIES), so narrow images meet every family across the sweep"""
    rng = np.random.default_rng(seed * 7919 + E * 4099 + R)
    img = np.empty((E, R), f32)
    for e in range(E):
        img[e] = ENV_FAMILIES[(e + R) % len(ENV_FAMILIES)](R, rng)
    return img


def conv_taps(n_ax, n_lat, seed=0):
    """seeded taps with both signs and zeros"""
    rng = np.random.default_rng(1000 + 37 * n_ax + n_lat + seed)
    ax = rng.standard_normal(n_ax).astype(f32); lat = rng.standard_normal(n_lat).astype(f32)
    ax[rng.random(n_ax) < 0.2] = 0.0; lat[rng.random(n_lat) < 0.2] = 0.0
    return ax, lat


def conv_shapes(n_ax, n_lat):
    """(E, R) at the bounds of the convolved window [n_ax, R-n_ax) x [n_lat/2, E-n_lat), and one full-size image"""
    Es = sorted({max(1, n_lat - 1), n_lat, n_lat + 1})
    Rs = sorted({max(1, n_ax), 2 * n_ax, 2 * n_ax + 1})
    return [(E, R) for E in Es for R in Rs] + [(129, 465)]


def conv_image(E, R, seed=0):
    """[E][R]: noise with a few -0.0, NaN and inf taps (the pixels outside the window must keep their bits, these included)"""
    rng = np.random.default_rng(5000 + 131 * E + R + seed)
    img = rng.standard_normal((E, R)).astype(f32)
    flat = img.reshape(-1)
    k = max(1, flat.size // 50)
    flat[rng.integers(0, flat.size, k)] = -0.0
    if flat.size > 8:
        flat[rng.integers(0, flat.size, 2)] = np.nan
        flat[rng.integers(0, flat.size, 1)] = np.inf
    return img


def scan_image(E, R, seed=0):
    """[E][R]: positive and negative noise with NaN and +-inf taps"""
    rng = np.random.default_rng(9000 + 17 * E + R + seed)
    img = rng.standard_normal((E, R)).astype(f32)
    flat = img.reshape(-1)
    n = flat.size
    if n < 8:
        return img
    flat[rng.integers(0, n, max(1, n // 97))] = np.nan
    flat[rng.integers(0, n, max(1, n // 113))] = np.inf
    flat[rng.integers(0, n, max(1, n // 127))] = -np.inf
    return img
