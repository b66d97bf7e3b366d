"""Automatic gain without a GPU (include/mcrt.h: mcrt_autogain_opts, mcrt_default_autogain_opts, mcrt_autogain_curve,
mcrt_autogain_frames): the struct and its defaults, the symbols, every refusal that needs no device, the host's curve against the numpy
mirror of tests/autogain_mirror.py exactly -- on random histograms and on histograms built for each branch of the rule --, the compiler's
report for the three kernels, and the mirror's own sanity, which holds tests/test_gpu_autogain.py honest."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest

import autogain_mirror as am

f32 = np.float32
INVALID, LIMIT = -1, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ struct, defaults, header, errors
def test_struct_defaults_and_header(mcrt):
    O = mcrt.AutogainOpts
    names = ("band_rows", "min_permille", "floor", "floor_scale", "max_gain", "apply")
    assert C.sizeof(O) == 24 and [getattr(O, n).offset for n in names] == [0, 4, 8, 12, 16, 20]
    L = mcrt.load_library()
    o = O()
    C.memset(C.byref(o), 0xA5, 24)
    assert L.mcrt_default_autogain_opts(C.byref(o)) == 0
    assert {n: getattr(o, n) for n in names} == am.DEFAULTS == dict(band_rows=16, min_permille=250, floor=0.0, floor_scale=3.0, max_gain=1000.0, apply=1)
    assert L.mcrt_default_autogain_opts(None) == INVALID and b"null" in L.mcrt_last_error()
    d = mcrt.autogain_opts_struct()
    assert [getattr(d, n) for n in names] == [getattr(o, n) for n in names]
    a = mcrt.autogain_opts_struct(band_rows=7, min_permille=10, floor=0.5, floor_scale=2.0, max_gain=4.0, apply=False)
    assert [getattr(a, n) for n in names] == [7, 10, 0.5, 2.0, 4.0, 0]
    assert mcrt.autogain_opts_struct(max_gain_db=40).max_gain == 100.0
    assert mcrt.autogain_opts_struct(max_gain_db=30).max_gain == f32(10.0 ** 1.5)
    with pytest.raises(ValueError):
        mcrt.autogain_opts_struct(max_gain=2.0, max_gain_db=6.0)
    with pytest.raises(TypeError):
        mcrt.autogain_opts_struct(rows=4)
    src = open(os.path.join(ROOT, "include", "mcrt.h")).read()
    assert "#define MCRT_VERSION 109 " in src and L.mcrt_version() == 109
    block = src[src.index("#define MCRT_VERSION"):src.index("typedef enum")]
    added = block[block.index("mcrt_autogain_opts"):]
    for name in ("mcrt_autogain_opts", "mcrt_default_autogain_opts", "mcrt_autogain_curve", "mcrt_autogain_frames", "automatic gain", "additive"):
        assert name in added, name
    for name in ("mcrt_default_autogain_opts", "mcrt_autogain_curve", "mcrt_autogain_frames"):
        assert re.search(r"\bint " + name + r"\(", src) and hasattr(L, name) and name in mcrt._lib.SYMBOLS, name
    exported = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "mcray-tracing_amd", "libmcrt_hip.so")], capture_output=True, text=True).stdout
    for name in ("mcrt_default_autogain_opts", "mcrt_autogain_curve", "mcrt_autogain_frames"):
        assert re.search(r" T " + name + r"\b", exported), name
    assert "no measurement backs" in src[src.index("---- automatic gain"):src.index("} mcrt_autogain_opts;")]
    # the call without a context is refused before anything else is looked at
    assert L.mcrt_autogain_frames(None, None, 1, 1, 1, 1, None, None, None, None, None) == INVALID and b"null context" in L.mcrt_last_error()


def test_curve_errors_write_nothing(mcrt):
    L = mcrt.load_library()
    hist = np.zeros((2, 2048), np.uint32); hist[:, 900] = 50
    k = np.full(32, -7.0, f32); band = np.full(2, -7, np.int32); pen = C.c_uint32(77)
    hp, kp, bp = (x.ctypes.data_as(C.c_void_p) for x in (hist, k, band))

    def call(h=hp, lines=4, R=32, floor=0.0, **kw):
        return L.mcrt_autogain_curve(h, lines, R, f32(floor), C.byref(mcrt.autogain_opts_struct(**kw)), kp, bp, C.byref(pen))

    for kw, code, word in ((dict(h=None), INVALID, b"null hist"), (dict(lines=0), INVALID, b"n_lines"), (dict(R=0), INVALID, b"n_rows"),
                           (dict(floor=-1.0), INVALID, b"floor_f"), (dict(floor=np.nan), INVALID, b"floor_f"), (dict(floor=np.inf), INVALID, b"floor_f"),
                           (dict(band_rows=3), INVALID, b"band_rows"), (dict(band_rows=257), INVALID, b"band_rows"), (dict(band_rows=0), INVALID, b"band_rows"),
                           (dict(min_permille=1001), INVALID, b"min_permille"),
                           (dict(floor=0.0, floor_scale=-1.0), INVALID, b"floor_scale"), (dict(floor_scale=np.nan), INVALID, b"floor_scale"),
                           (dict(floor_scale=np.inf), INVALID, b"floor_scale"),
                           (dict(max_gain=0.5), INVALID, b"max_gain"), (dict(max_gain=np.inf), INVALID, b"max_gain"), (dict(max_gain=np.nan), INVALID, b"max_gain"),
                           (dict(R=2049), LIMIT, b"n_rows")):
        assert call(**kw) == code, kw
        assert word in L.mcrt_last_error(), (kw, L.mcrt_last_error())
    o = mcrt.autogain_opts_struct(); o.floor = -1.0                 # the options' own floor is checked too, though floor_f is what counts
    assert L.mcrt_autogain_curve(hp, 4, 32, f32(0.0), C.byref(o), kp, bp, C.byref(pen)) == INVALID and b"floor" in L.mcrt_last_error()
    assert (k == -7.0).all() and (band == -7).all() and pen.value == 77
    assert call() == 0 and pen.value == 32 and (band == 900).all() and (k == 1.0).all()
    assert L.mcrt_autogain_curve(hp, 4, 32, f32(0.0), None, None, None, None) == 0          # defaults, and every output is optional


# ------------------------------------------------------------------ the host's curve against the mirror
def _check(mcrt, hist, lines, R, floor=0.0, **opts):
    k, band, pen = mcrt.host_autogain_curve(hist, lines, R, floor=floor, **opts)
    mk, mband, mpen = am.curve(hist, lines, R, floor, opts)
    assert np.array_equal(band, mband), (band, mband)
    assert pen == mpen
    assert np.array_equal(k.view(np.uint32), mk.view(np.uint32)), np.flatnonzero(k.view(np.uint32) != mk.view(np.uint32))[:8]
    return k, band, pen


def _hist(R, B, levels, lines=8, spread=3):
    """band histograms with every sample of band b around the bin levels[b] (None: an empty band, all in bin 0)"""
    nB = am.n_bands(R, B)
    assert len(levels) == nB
    h = np.zeros((nB, 2048), np.uint32)
    for b, lv in enumerate(levels):
        n = lines * (min((b + 1) * B, R) - b * B)
        if lv is None:
            h[b, 0] = n
        else:
            for i in range(n):
                h[b, lv - spread + i % (2 * spread + 1)] += 1
    return h


@pytest.mark.parametrize("R,B", [(1, 16), (5, 4), (17, 4), (64, 16), (255, 16), (256, 16), (257, 16), (465, 16), (465, 7), (2048, 4), (2048, 256), (100, 256)])
def test_curve_equals_the_mirror_on_random_histograms(mcrt, R, B):
    rng = np.random.default_rng(R * 1000 + B)
    nB = am.n_bands(R, B)
    lines = 33
    for trial in range(4):
        h = np.zeros((nB, 2048), np.uint32)
        for b in range(nB):
            n = lines * (min((b + 1) * B, R) - b * B)
            centre_bin = int(rng.integers(700, 1100)) - 3 * b * 465 // max(R, 1) // max(nB, 1)
            echo = int(n * rng.uniform(0.0, 1.0)) if trial != 3 else n
            bins = np.clip(np.rint(rng.normal(centre_bin, 6.0, echo)).astype(np.int64), 1, 2039)
            h[b] = np.bincount(bins, minlength=2048)
            h[b, 0] = n - echo
        floor = [0.0, 1e-4, 0.002, 0.0][trial]
        _check(mcrt, h, lines, R, floor=floor, band_rows=B, min_permille=[250, 0, 500, 1000][trial], max_gain=[1000.0, 2.0, 1000.0, 1.0][trial])


def test_curve_on_built_histograms(mcrt):
    R, B = 100, 16                                                   # seven bands, the last one ragged (4 rows)
    # no valid band: gains 1, penetration 0
    k, band, pen = _check(mcrt, _hist(R, B, [None] * 7), 8, R, band_rows=B)
    assert (k == 1.0).all() and (band == -1).all() and pen == 0
    k, band, pen = _check(mcrt, _hist(R, B, [900] * 7), 8, R, floor=1e30, band_rows=B)        # everything under the floor
    assert (k == 1.0).all() and (band == -1).all() and pen == 0
    # only the last band valid: the bands before it hold its gain (1: it is the target), the penetration is R
    k, band, pen = _check(mcrt, _hist(R, B, [None] * 6 + [950]), 8, R, band_rows=B)
    assert list(band) == [-1] * 6 + [950] and pen == R and (k == 1.0).all()
    # an invalid span in the middle holds the gain of the band before it; the target is the lower median of 960, 940, 920, 900 = 920
    k, band, pen = _check(mcrt, _hist(R, B, [960, 940, None, None, 920, 900, None]), 8, R, band_rows=B)
    assert list(band) == [960, 940, -1, -1, 920, 900, -1] and pen == 96
    g940 = am.centre(920) / am.centre(940)
    assert k[0] == am.centre(920) / am.centre(960) and (k[24:56] == g940).all() and k[56] != g940       # (band centres: rows 23.5 .. 55.5)
    assert (k[88:] == am.centre(920) / am.centre(900)).all()        # past the last valid band: its gain, no further
    # ties in the target: 900, 900, 940, 940 -> element 1 = 900; and an odd count 900, 940, 940 -> 940
    k, _, _ = _check(mcrt, _hist(64, 16, [940, 900, 940, 900]), 8, 64, band_rows=16)
    assert k[0] == am.centre(900) / am.centre(940) == 2.0 ** -5 and k[63] == 1.0
    k, _, _ = _check(mcrt, _hist(48, 16, [940, 900, 940]), 8, 48, band_rows=16)
    assert k[0] == 1.0 and k[47] == 1.0 and 31.0 < k.max() < 32.0
    # the clamp at both ends: 40 bins are five octaves (x 32), max_gain 4
    k, _, _ = _check(mcrt, _hist(48, 16, [940, 900, 860]), 8, 48, band_rows=16, max_gain=4.0)
    assert k[0] == 0.25 and k[47] == 4.0 and k.min() == 0.25 and k.max() == 4.0
    # band_rows larger than R: one band, one gain
    k, band, pen = _check(mcrt, _hist(100, 256, [880]), 8, 100, band_rows=256)
    assert (k == 1.0).all() and list(band) == [880] and pen == 100
    # min_permille: a band with 3 of 8 scan-lines' samples in tissue is valid at 375, not at 376
    h = _hist(32, 16, [900, 900]); h[1] = 0; h[1, 0] = 80; h[1, 870] = 48
    assert list(_check(mcrt, h, 8, 32, band_rows=16, min_permille=375)[1]) == [900, 870]
    assert list(_check(mcrt, h, 8, 32, band_rows=16, min_permille=376)[1]) == [900, -1]
    # the floor: thr = 0.002 * 3 has bin 956; a level of 956 is noise, 957 is tissue
    assert am.threshold_bin(0.002, 3.0) == 956
    assert list(_check(mcrt, _hist(32, 16, [956, 957], spread=0), 8, 32, floor=0.002, band_rows=16)[1]) == [-1, 957]
    # the row gains between two band centres, rows 7.5 and 23.5 (the target is the lower level, 892: gains 0.5 and 1): row 8 is 1/32 of the way
    k, _, _ = _check(mcrt, _hist(32, 16, [900, 892]), 8, 32, band_rows=16)
    assert (k[:8] == 0.5).all() and (k[24:] == 1.0).all() and k[8] == f32(0.5 + 0.5 / 32.0) and k[23] == f32(0.5 + 0.5 * 31.0 / 32.0)


# ------------------------------------------------------------------ the kernels' resources
def test_kernels_use_no_scratch_and_spill_nothing():
    """the compiler's own report for the three kernels (their translation unit alone)"""
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "mcray-tracing_amd"), "resources", "KERNELS=mcrt_autogain"], capture_output=True, text=True).stderr
    blocks = [b for b in out.split("Function Name: ") if b.startswith("_ZN4mcrt")]
    seen = set()
    for b in blocks:
        val = lambda key: int(re.search(key + r": (\d+)", b).group(1))
        assert val("VGPRs Spill") == 0 and val("SGPRs Spill") == 0 and val(r"ScratchSize \[bytes/lane\]") == 0, b[:900]
        seen.add(re.match(r"_ZN4mcrt\d+(k_autogain_[a-z]+)", b).group(1))
    assert seen == {"k_autogain_hist", "k_autogain_curve", "k_autogain_apply"}, out[-2000:]


# ------------------------------------------------------------------ the mirror's own sanity
def test_mirror_flattens_decaying_speckle_and_holds_past_the_penetration():
    """Rayleigh speckle decaying as exp(-r / 60), 33 scan-lines x 465 rows over a Gaussian floor of 0.002 (enveloped: a Rayleigh floor).
    The spread of the valid bands' median bins falls below a quarter of what it was, and the bands past the penetration depth keep the last
    valid gain"""
    rng = np.random.default_rng(7)
    E, R = 33, 465
    decay = np.exp(-np.arange(R) / 60.0)
    echo = np.hypot(rng.standard_normal((E, R)), rng.standard_normal((E, R))) * decay
    floor = np.hypot(rng.standard_normal((E, R)), rng.standard_normal((E, R))) * 0.002
    x = (echo + floor).astype(f32).reshape(1, 1, E, R)
    out, gain, band, pen = am.autogain(x, dict(floor=0.002))
    valid = np.flatnonzero(band[0] >= 0)
    assert valid.size >= 10 and 0 < pen[0] < R and pen[0] == (valid[-1] + 1) * 16
    before = int(band[0][valid].max() - band[0][valid].min())
    # the levels after the gain, measured on the same bands with the floor out of the way (the gained noise would count as tissue)
    after_bins = [int(np.median(am.bins_of(out[0, 0][:, b * 16:(b + 1) * 16]))) for b in valid]
    after = max(after_bins) - min(after_bins)
    print("spread of the valid bands' median bins: %d before, %d after; penetration %d rows of %d" % (before, after, pen[0], R))
    assert after * 4 < before
    last = gain[0][valid[-1] * 16 + 8]
    assert (gain[0][pen[0]:] == last).all() and (gain[0] <= last).all()
    assert np.array_equal(out.view(np.uint32), (x * gain[0]).astype(f32).view(np.uint32))
    # apply == 0 keeps every bit; an all-zero frame has gains 1 and no penetration
    keep, g0, _, _ = am.autogain(x, dict(floor=0.002, apply=0))
    assert np.array_equal(keep.view(np.uint32), x.view(np.uint32)) and np.array_equal(g0, gain)
    z = np.zeros((1, 2, 3, 17), f32); z[0, 0, 0, 0] = -0.0; z[0, 1, 2, 5] = np.nan; z[0, 1, 2, 6] = np.inf
    out, g, b, p = am.autogain(z)
    assert (g == 1.0).all() and (b == -1).all() and p[0] == 0
    assert np.array_equal(out.view(np.uint32), z.view(np.uint32))
