"""Focal zones on the CPU (no GPU): mcrt_psf_focus_kernels against a restatement of the model in include/mcrt.h with Python's math module,
bit for bit; its focal rows against mcrt_psf_kernels; its argument errors; and the numpy mirror of mcrt_convolve_frames_depth
(tests/focus_mirror.py) tied to the pinned oracle's convolution when every row has the same taps."""
import ctypes as C
import math
import numpy as np
import pytest

import focus_mirror as fm
import image_cases as ic

INVALID, LIMIT = -1, -5
VAR_Y, RES_UM = 0.2, 145


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("focus,row_mm,n_rows,n_lat", [
    ((40.0,), 0.322, 465, 13),                   # one focus, the context's row pitch at 4.5 MHz
    ((30.0, 60.0, 90.0), 0.322, 465, 13),        # three zones
    ((10.0, 20.0), 0.25, 200, 13),               # row 60 lies exactly between the foci (15 mm): the shallower one is taken
    ((500.0,), 0.322, 465, 7),                   # a focus deeper than the image
    ((0.0,), 0.1, 300, 32),                      # focus at the probe
    ((0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0), 0.05, 2048, 1),   # eight foci, the row limit, one tap
])
def test_table_matches_the_restatement(mcrt, focus, row_mm, n_rows, n_lat):
    got = mcrt.host_psf_focus(VAR_Y, RES_UM, n_rows, row_mm, focus, 20.0, n_lat)
    want = fm.psf_focus_rows(VAR_Y, RES_UM, n_rows, row_mm, focus, 20.0, n_lat)
    assert np.array_equal(bits(got), bits(want))
    assert np.isfinite(got).all() and (got > 0).all()


@pytest.mark.parametrize("n_lat", [1, 2, 13, 32])
def test_without_foci_every_row_is_the_constant_kernel(mcrt, n_lat):
    _, lat = mcrt.host_psf(4.5, 0.05, VAR_Y, RES_UM, 7, n_lat)
    got = mcrt.host_psf_focus(VAR_Y, RES_UM, 465, 0.322, (), 20.0, n_lat)
    assert np.array_equal(bits(got), np.tile(bits(lat), (465, 1)))


def test_focal_rows_are_the_constant_kernel(mcrt):
    _, lat = mcrt.host_psf(4.5, 0.05, VAR_Y, RES_UM, 7, 13)
    got = mcrt.host_psf_focus(VAR_Y, RES_UM, 465, 0.25, (40.0,), 20.0, 13)
    assert np.array_equal(bits(got[160]), bits(lat))                     # 160 * 0.25 = 40.0 exactly
    assert not np.array_equal(bits(got[159]), bits(lat)) and not np.array_equal(bits(got[161]), bits(lat))
    got = mcrt.host_psf_focus(VAR_Y, RES_UM, 465, 0.25, (10.0, 50.0, 100.0), 7.5, 13)
    for r in (40, 200, 400):
        assert np.array_equal(bits(got[r]), bits(lat)), r
    # away from a focus the beam is wider and its gain keeps the area: the centre taps drop, the outer ones rise
    assert got[300, 6] < lat[6] and got[300, 0] > lat[0]


def _call(mcrt, out, var_y=VAR_Y, res_um=RES_UM, focus=(40.0,), focal_range=20.0, n_rows=None, row_mm=0.322, n_lat=None, null_focus=False, null_out=False):
    L = mcrt.load_library()
    f = mcrt.focus_struct(focus, focal_range)
    n_rows = out.shape[0] if n_rows is None else n_rows
    n_lat = out.shape[1] if n_lat is None else n_lat
    return L.mcrt_psf_focus_kernels(var_y, res_um, None if null_focus else C.byref(f), n_rows, row_mm, None if null_out else out.ctypes.data_as(C.c_void_p), n_lat)


@pytest.mark.parametrize("kw,code", [
    (dict(null_focus=True), INVALID), (dict(null_out=True), INVALID),
    (dict(focus=tuple(float(i) for i in range(1, 10))), INVALID),          # nine foci
    (dict(focus=(40.0, 30.0)), INVALID), (dict(focus=(30.0, 30.0)), INVALID),
    (dict(focus=(math.nan,)), INVALID), (dict(focus=(10.0, math.inf)), INVALID), (dict(focus=(-1.0,)), INVALID),
    (dict(focal_range=0.0), INVALID), (dict(focal_range=-5.0), INVALID), (dict(focal_range=math.nan), INVALID), (dict(focal_range=math.inf), INVALID),
    (dict(row_mm=0.0), INVALID), (dict(row_mm=-0.322), INVALID), (dict(row_mm=math.nan), INVALID), (dict(row_mm=math.inf), INVALID),
    (dict(n_lat=0), INVALID), (dict(n_lat=33), INVALID),
    (dict(var_y=0.0), INVALID), (dict(var_y=math.nan), INVALID),
    (dict(n_rows=2049), LIMIT),
])
def test_argument_errors_leave_the_output_untouched(mcrt, kw, code):
    out = np.full((2049, 33), -7.25, np.float32)
    assert _call(mcrt, out, **({"n_rows": 465, "n_lat": 13} | kw)) == code
    assert (out == np.float32(-7.25)).all()
    assert mcrt.load_library().mcrt_last_error()


def test_a_focal_range_is_only_needed_with_foci(mcrt):
    out = np.full((10, 13), -7.25, np.float32)
    assert _call(mcrt, out, focus=(), focal_range=0.0) == 0
    _, lat = mcrt.host_psf(4.5, 0.05, VAR_Y, RES_UM, 7, 13)
    assert np.array_equal(bits(out), np.tile(bits(lat), (10, 1)))
    assert _call(mcrt, out, n_rows=0) == 0


@pytest.mark.parametrize("n_lat", ic.CONV_LAT)
@pytest.mark.parametrize("n_ax", ic.CONV_AX)
def test_mirror_with_equal_rows_is_the_oracle(orc, n_ax, n_lat):
    ax, lat = ic.conv_taps(n_ax, n_lat)
    for E, R in ic.conv_shapes(n_ax, n_lat):
        img = ic.conv_image(E, R)
        got = fm.convolve_depth(img, ax, np.tile(lat, (R, 1)))
        ic.assert_same_bits(got, orc.convolve(img.T, ax, lat).T, "mirror %dx%d taps %d/%d" % (E, R, n_ax, n_lat))
