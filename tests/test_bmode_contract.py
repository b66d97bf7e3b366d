"""mcrt_bmode_frames without a GPU: the parameter block and its defaults, the null-context failure, and the numpy mirror of the contract
(tests/bmode_mirror.py) against grey levels computed by hand."""
import ctypes as C
import math
import numpy as np

import bmode_mirror as bm


def test_default_bmode_and_layout(mcrt):
    L = mcrt.load_library()
    p = mcrt.BmodeParams()
    p.mode = 7
    assert L.mcrt_default_bmode(C.byref(p)) == 0
    assert (p.mode, p.dynamic_range_db, p.gain_db, p.ref, p.persistence, p.reset_state) == (0, 60.0, 0.0, 0.0, 0.0, 1)
    assert (p.out_rows, p.out_cols, p.radius_mm, p.total_angle_rad) == (400, 500, 30.0, math.pi / 3)
    assert C.sizeof(mcrt.BmodeParams) == 48
    assert mcrt.BmodeParams.radius_mm.offset == 32 and mcrt.BmodeParams.total_angle_rad.offset == 40
    assert L.mcrt_default_bmode(None) != 0


def test_bmode_frames_without_context_fails_cleanly(mcrt):
    L = mcrt.load_library()
    p = mcrt.bmode_params()
    assert L.mcrt_bmode_frames(None, None, 1, 128, 465, C.byref(p), None, None, None, None) == -1
    assert b"null context" in L.mcrt_last_error()


def staircase(E=128, R=465, steps=12):
    """RF rows in `steps` depth bands, band k at amplitude 2^-k (-6.02 dB per band), the sign alternating over the scan-lines"""
    band = np.minimum(np.arange(R) // (R // steps), steps - 1)
    img = np.ldexp(np.float32(1.0), -band).astype(np.float32)[None, :].repeat(E, 0)
    img[1::2] *= -1
    return img, band


def test_mirror_reproduces_a_hand_computed_staircase(mcrt, orc):
    E, R, steps = 128, 465, 12
    img, band = staircase(E, R, steps)
    out, refs, _ = bm.bmode(orc, img[None], dynamic_range_db=60.0)
    assert refs[0] == 1.0
    # grey of band k: 255 * (60 - 20 k log10 2) / 60, rounded half up, 0 below the range
    want = [max(0, int(math.floor(255.0 * (60.0 - 20.0 * k * math.log10(2.0)) / 60.0 + 0.5))) for k in range(steps)]
    assert want == [255, 229, 204, 178, 153, 127, 101, 76, 50, 25, 0, 0]
    y0, x0, all_in, none_in = bm.tap_boxes(mcrt.host_scan_maps(E, R), E, R)
    same = all_in & (band[np.clip(y0, 0, R - 1)] == band[np.clip(y0 + 1, 0, R - 1)])
    got_bands = band[np.clip(y0, 0, R - 1)]
    for k in range(steps):
        m = same & (got_bands == k)
        assert m.sum() > 500, k
        assert np.all(out[0][m] == want[k]), (k, np.unique(out[0][m]))
    assert np.all(out[0][none_in] == 0) and none_in.sum() > 10000
    # with +6 dB gain every band moves up by 6 dB; in REF_LOG mode band 0 is white
    g6, _, _ = bm.bmode(orc, img[None], gain_db=6.0206)
    m1 = same & (got_bands == 1)
    assert np.all(g6[0][m1] == 255)
    rl, _, _ = bm.bmode(orc, img[None], mode="ref_log")
    m0 = same & (got_bands == 0)
    assert np.all(rl[0][m0] == 255)
    want1 = int(math.floor(255.0 * math.log10(1.5) / math.log10(2.0) + 0.5))
    assert np.all(np.abs(rl[0][m1].astype(int) - want1) <= 1)
