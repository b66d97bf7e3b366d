"""Frequency compounding and the depth downshift, host side (no GPU): mcrt_psf_band_kernels against tests/bands_mirror.py bit for bit, its pin
on mcrt_psf_kernels, the floor, the struct's layout, the errors, and -- on the mirror alone -- the effect: the speckle contrast of the mean of
the detected band images against one band's."""
import ctypes as C
import numpy as np
import pytest

import bands_mirror as bm
import elevation_mirror as em
import image_cases as ic

f32 = np.float32
INVALID, LIMIT = -1, -5

BANDS = {1: (4.5,), 3: (3.5, 4.5, 5.5), 8: (6.0, 2.5, 3.0, 3.5, 4.0, 4.5, 5.0, 5.5)}          # (any order)
WEIGHTS = {1: None, 3: (1.0, 2.0, 0.5), 8: (1.0, 0.0, 3.0, 1.0, 0.25, 1.0, 1.0, 7.0)}


@pytest.mark.parametrize("R", [2, 465, 2048])
@pytest.mark.parametrize("n_ax", [1, 7, 16])
@pytest.mark.parametrize("B", [1, 3, 8])
def test_tables_match_the_mirror(mcrt, B, n_ax, R):
    """with a downshift that reaches the floor part way down (at 4.5, 0.02 per mm and a floor of 2.0: near row 388 at 0.322 mm)"""
    for shift, floor, var_x in ((0.0, 0.0, 0.05), (0.02, 2.0, 0.2)):
        b = mcrt.bands_struct(BANDS[B], WEIGHTS[B], var_x=var_x, downshift_mhz_per_mm=shift, min_mhz=floor)
        ax, w = mcrt.host_psf_bands(b, 145, R, 0.322, n_ax)
        wax, ww = bm.psf_band_rows(BANDS[B], WEIGHTS[B], var_x, shift, floor, 145, R, 0.322, n_ax)
        ic.assert_same_bits(ax, wax, "taps B=%d n_ax=%d R=%d shift=%g" % (B, n_ax, R, shift))
        ic.assert_same_bits(w, ww, "weights B=%d" % B)


def test_one_band_without_downshift_is_psf_kernels(mcrt):
    for freq, var_x, n_ax, res in ((4.5, 0.05, 7, 145), (3.3, 0.2, 16, 145), (7.0, 0.01, 1, 100)):
        b = mcrt.Bands()
        assert mcrt.load_library().mcrt_default_bands(C.byref(b), freq, var_x) == 0
        assert (b.n_bands, b.band_weight[0], b.downshift_mhz_per_mm, b.min_mhz) == (1, 1.0, 0.0, 0.0) and b.band_mhz[0] == f32(freq) and b.var_x == f32(var_x)
        for floor in (0.0, freq):                                # min_mhz <= freq
            b.min_mhz = floor
            ax, w = mcrt.host_psf_bands(b, res, 465, 0.322, n_ax)
            want = mcrt.host_psf(freq, var_x, 0.2, res, n_ax, 13)[0]
            ic.assert_same_bits(ax, np.tile(want, (1, 465, 1)), "pin %g" % freq)
            assert np.array_equal(w.view(np.uint32), np.ones((465, 1), f32).view(np.uint32))


def test_rows_at_the_floor_are_the_floor_frequencys_taps(mcrt):
    R, row_mm = 465, 0.322
    b = mcrt.bands_struct((4.5,), downshift_mhz_per_mm=0.02, min_mhz=2.0)
    ax, _ = mcrt.host_psf_bands(b, 145, R, row_mm, 7)
    first = next(r for r in range(R) if 4.5 - float(f32(0.02)) * (r * row_mm) <= 2.0)
    assert 380 < first < 395                                     # 2.5 MHz / 0.02 per mm = 125 mm = row 388
    floor = mcrt.host_psf(2.0, 0.05, 0.2, 145, 7, 13)[0]
    ic.assert_same_bits(ax[0, first:], np.tile(floor, (R - first, 1)), "floor")
    assert not np.array_equal(ax[0, first - 1], floor)
    ic.assert_same_bits(ax[0, 0], mcrt.host_psf(4.5, 0.05, 0.2, 145, 7, 13)[0], "row 0")
    # every frequency falls monotonically: the taps of the rows above the floor all differ from their neighbours'
    assert all(not np.array_equal(ax[0, r], ax[0, r + 1]) for r in range(first - 1))


def test_struct_layout(mcrt):
    B = mcrt.Bands
    assert C.sizeof(B) == 80
    assert (B.n_bands.offset, B.band_mhz.offset, B.band_weight.offset, B.var_x.offset, B.downshift_mhz_per_mm.offset, B.min_mhz.offset) == (0, 4, 36, 68, 72, 76)
    with pytest.raises(ValueError):
        mcrt.bands_struct((3.5, 4.5), weights=(1.0,))


def test_errors_leave_the_outputs_untouched(mcrt):
    L = mcrt.load_library()
    R, n_ax = 16, 7
    nan, inf = float("nan"), float("inf")

    def call(b, res_um=145, n_rows=R, row_mm=0.322, n=n_ax, null_ax=False, null_b=False):
        ax = np.full((8, max(n_rows, 1), 16), 7.0, f32); w = np.full((max(n_rows, 1), 8), 7.0, f32)
        rc = L.mcrt_psf_band_kernels(None if null_b else C.byref(b), res_um, n_rows, row_mm, None if null_ax else ax.ctypes.data_as(C.c_void_p), n,
                                     w.ctypes.data_as(C.c_void_p))
        assert (ax == 7.0).all() and (w == 7.0).all()
        return rc

    ok = lambda **kw: mcrt.bands_struct(kw.pop("band_mhz", (3.5, 4.5, 5.5)), **kw)
    assert call(ok(), null_b=True) == INVALID and call(ok(), null_ax=True) == INVALID
    zero, nine = ok(), ok()
    zero.n_bands, nine.n_bands = 0, 9
    assert call(zero) == INVALID and call(nine) == INVALID
    for bad in (0.0, -1.0, nan, inf):
        assert call(ok(band_mhz=(3.5, bad, 5.5))) == INVALID, bad
        assert call(ok(var_x=bad)) == INVALID, bad
        assert call(ok(), row_mm=bad) == INVALID, bad
    for bad in (-1.0, nan, inf):
        assert call(ok(weights=(1.0, bad, 1.0))) == INVALID, bad
        assert call(ok(downshift_mhz_per_mm=bad)) == INVALID, bad
        assert call(ok(min_mhz=bad)) == INVALID, bad
    assert call(ok(weights=(0.0, 0.0, 0.0))) == INVALID
    assert call(ok(), res_um=0) == INVALID
    assert call(ok(), n=0) == INVALID and call(ok(), n=17) == INVALID
    assert call(ok(), n_rows=2049) == LIMIT
    assert L.mcrt_default_bands(None, 4.5, 0.05) == INVALID
    # the entries past n_bands are not looked at, and a null w_rows is allowed
    b = ok(band_mhz=(4.5,))
    b.band_mhz[1], b.band_weight[1] = nan, -1.0
    ax = np.zeros((1, R, n_ax), f32)
    assert L.mcrt_psf_band_kernels(C.byref(b), 145, R, 0.322, ax.ctypes.data_as(C.c_void_p), n_ax, None) == 0
    assert call(ok(weights=(0.0, 1.0, 0.0)), n_rows=0) == 0


def _cv(img, R):
    a = img[:, 30:R - 30].astype(np.float64)
    return a.std() / a.mean()


@pytest.mark.parametrize("n_ax,var_x,bands,bound", [(7, 0.05, (3.5, 4.5, 5.5), 0.85), (15, 0.2, (3.5, 4.5, 5.5), 0.72)])
def test_the_effect_on_the_mirror(orc, n_ax, var_x, bands, bound):
    """dense Gaussian RF of 64 x 465, the mirror's band convolution (axial taps alone: one lateral tap of 1), the reference's envelope of every
    band image and their mean: the speckle's coefficient of variation (std / mean over rows 30 .. R-30) falls to at most `bound` of the 4.5
    band's own.  The bounds are the issue's: 0.79-0.80 measured at 7 taps and 0.65 at 15 taps / var_x 0.2, +-0.01 over the seeds."""
    E, R = 64, 465
    ax, w = bm.psf_band_rows(bands, None, var_x, 0.0, 0.0, 145, R, 0.322, n_ax)
    for seed in (1, 2, 3):
        rf = np.random.default_rng(seed).standard_normal((E, R)).astype(f32)
        imgs = bm.convolve_bands(rf, ax, lateral=np.ones(1, f32))
        env = np.stack([orc.envelope(np.ascontiguousarray(im.T)).T for im in imgs])
        fold = em.fold(env[None], w)[0]
        one, mean = _cv(env[bands.index(4.5)][:E - 1], R), _cv(fold[:E - 1], R)        # (one lateral tap leaves the last column unconvolved)
        print("n_ax %d seed %d: CV(4.5) %.4f CV(fold) %.4f ratio %.4f" % (n_ax, seed, one, mean, mean / one))
        assert mean / one <= bound
