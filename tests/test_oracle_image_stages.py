"""The oracle's image stages pinned on their own (CPU only): orc.envelope and orc.convolve against a plain numpy reading of rfimage.h:54-123,
bit for bit, on the cases tests/test_gpu_image_stages.py sends to the GPU; the product's host scan-conversion maps (mcrt_scan_maps) against
the oracle's at every geometry of that sweep; and the rows < 2 guard of orc_envelope."""
import numpy as np
import pytest

import image_cases as ic

f32 = np.float32


def envelope_literal(img):
    """rfimage.h:54-91 written out: one sequential walk per column with `ascending` and the last peak, float32 throughout.  img is
    [rows][cols] (the reference's layout); a copy is returned."""
    out = np.array(img, f32, copy=True)
    rows, cols = out.shape
    if rows < 2:
        return out
    one = f32(1)
    for column in range(cols):
        c = out[:, column]
        ascending = c[0] < c[1]
        last_peak_pos = 0
        last_peak = c[0]
        for i in range(1, rows - 1):
            if c[i] < c[i + 1]:
                ascending = True
            elif ascending:
                ascending = False
                new_peak = np.abs(c[i])
                j = np.arange(last_peak_pos, i, dtype=f32)
                alpha = (j - f32(last_peak_pos)) / (f32(i) - f32(last_peak_pos))
                with np.errstate(invalid="ignore", over="ignore"):
                    c[last_peak_pos:i] = last_peak * (one - alpha) + new_peak * alpha
                last_peak_pos = i
                last_peak = new_peak
    return out


def convolve_literal(img, axial, lateral):
    """rfimage.h:93-123: float32 products summed from 0 in the reference's k order -- axial over rows [na, R-na) into tmp, then lateral
    over columns [nl/2, E-nl) back into the image.  img is [rows][cols]; a copy is returned."""
    out = np.array(img, f32, copy=True)
    rows, cols = out.shape
    na, nl = len(axial), len(lateral)
    r0, r1 = na, rows - na
    if r1 <= r0:
        return out
    tmp = np.zeros((r1 - r0, cols), f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(na):
            tmp = tmp + out[r0 + k:r1 + k, :] * f32(axial[k])
        c0, c1 = nl // 2, cols - nl
        if c1 > c0:
            conv = np.zeros((r1 - r0, c1 - c0), f32)
            for k in range(nl):
                conv = conv + tmp[:, c0 + k:c1 + k] * f32(lateral[k])
            out[r0:r1, c0:c1] = conv
    return out


def test_literal_readings_are_float32():
    """the numpy readings stay in float32 (a float64 intermediate would make them a different reference)"""
    img = ic.envelope_image(3, 65)
    assert envelope_literal(img.T).dtype == f32
    ax, lat = ic.conv_taps(7, 13)
    assert convolve_literal(ic.conv_image(14, 15).T, ax, lat).dtype == f32


@pytest.mark.parametrize("R", ic.ENV_R)
def test_envelope_oracle_is_the_sequential_walk(orc, R):
    """every column family at every row count of the GPU sweep (one column of each family, and the 3-wide image)"""
    for E in (len(ic.ENV_FAMILIES), 3):
        img = ic.envelope_image(E, R)                     # [E][R]
        ref = img.T.copy()                                # [R][E]
        ic.assert_same_bits(orc.envelope(ref), envelope_literal(ref), "envelope E=%d R=%d" % (E, R))


def test_envelope_families_do_what_they_say():
    """the sawtooth families put their peaks on k*ceil(R/64) and k*ceil(R/64)-1, the edge family on rows 1 and R-2"""
    def peaks(c):
        return [i for i in range(1, len(c) - 1) if c[i - 1] < c[i] and not (c[i] < c[i + 1])]
    rng = np.random.default_rng(0)
    for R in (129, 465, 2048):
        per = -(-R // 64)
        starts = peaks(ic._saw_on_chunk_starts(R, rng))
        assert starts and all(p % per == 0 for p in starts), R
        ends = peaks(-ic._saw_on_chunk_ends(R, rng))
        assert ends and all((p + 1) % per == 0 for p in ends), R
        assert peaks(ic._edge_peaks(R, rng)) == [1, R - 2]
    assert peaks(ic._stairs(465, rng)) and not peaks(ic._ascending(465, rng)) and not peaks(ic._descending(465, rng))


def test_envelope_of_fewer_than_two_rows_is_the_identity(orc):
    """rows == 1: the reference's first comparison would read row 1; the oracle (like the GPU) leaves the image alone"""
    img = np.array([[-1.5, 2.0, np.nan, -0.0, np.inf]], f32)
    assert np.array_equal(orc.envelope(img).view(np.uint32), img.view(np.uint32))


@pytest.mark.parametrize("n_ax", ic.CONV_AX)
@pytest.mark.parametrize("n_lat", ic.CONV_LAT)
def test_convolve_oracle_is_the_reference_loop(orc, n_ax, n_lat):
    ax, lat = ic.conv_taps(n_ax, n_lat)
    for E, R in ic.conv_shapes(n_ax, n_lat):
        ref = ic.conv_image(E, R).T.copy()                # [R][E]
        got = orc.convolve(ref, ax, lat)
        ic.assert_same_bits(got, convolve_literal(ref, ax, lat), "convolve %dx%d taps %d/%d" % (E, R, n_ax, n_lat))
        if R <= 2 * n_ax or E - n_lat <= n_lat // 2:          # an empty window: the image comes back bit for bit
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("geom", ic.SCAN_GEOMETRIES, ids=lambda g: "%gmm-%.3frad-%dx%d" % g)
def test_product_scan_maps_equal_the_oracle(mcrt, orc, geom):
    """mcrt_scan_maps (the product's host code) == orc_scan_maps, bit for bit and NaN where NaN, away from the three golden shapes"""
    radius, angle, orows, ocols = geom
    for E, R in ic.SCAN_SHAPES:
        pr, pc = mcrt.host_scan_maps(E, R, radius, angle, 100, 1500, orows, ocols)
        orr, occ = orc.scan_maps(R, E, radius, angle, 100, 1500, orows, ocols)
        ic.assert_same_bits(pr, orr, "map_row %s %dx%d" % (geom, E, R))
        ic.assert_same_bits(pc, occ, "map_col %s %dx%d" % (geom, E, R))
