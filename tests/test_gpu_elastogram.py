"""The strain overlay on the MI355X: mcrt_elastogram_frames (k_elastogram) against the integer mirror (tests/strain_mirror.py) byte for byte
-- at pictures of one pixel, around a wavefront's 64 lanes and its tile of 256 pixels, at an odd picture and past one workgroup, for one
frame and three; with every threshold deciding pixels at equality, NaN pixels, both ends of the colour table, alpha 0 and 256, a negative
reference strain, a table of the caller's own; behind sentinels and at every alignment; the refusals."""
import ctypes as C
import numpy as np
import pytest

import strain_mirror as sm

pytestmark = pytest.mark.gpu

f32 = np.float32
INVALID, LIMIT = -1, -5
OPTS = dict(ref_strain=0.01, rho_min=0.75, grey_min=20, alpha=160)


@pytest.fixture(scope="module")
def ctx(mcrt):
    c = mcrt.Context(0)
    yield c
    c.close()


@pytest.fixture
def dev(ctx):
    bufs = []

    def upload(arr, skew=0):
        arr = np.ascontiguousarray(arr)
        p = ctx.alloc(max(arr.nbytes, 4) + skew)
        bufs.append(p)
        ctx.h2d(p + skew, arr)
        return p + skew
    yield upload
    for p in bufs:
        ctx.free(p)


#            strain            rho          grey
PINS = [(0.01, 1.0, 100),                   # shown: the reference strain, entry 128
        (0.01, 0.75, 100),                  # rho == rho_min: shown
        (0.01, float(np.nextafter(f32(0.75), f32(0))), 100),      # just under it: grey
        (0.01, 1.0, 20),                    # grey == grey_min: shown
        (0.01, 1.0, 19),                    # darker: grey
        (np.nan, 1.0, 101), (0.01, np.nan, 102), (np.inf, 1.0, 103), (-np.inf, 1.0, 104), (0.01, np.inf, 105),
        (0.0, 1.0, 106), (-0.0, 1.0, 107),  # no strain: entry 0
        (-0.003, 1.0, 108),                 # a negative strain: clamped to entry 0
        (0.5, 1.0, 109),                    # far above twice the reference: entry 255
        (0.002, 1.0, 110)]                  # a fifth of the reference: 25.6, entry 26


def picture(F, H, W, seed=0):
    """(strain, rho [F][H][W] floats, grey [F][H][W] bytes): strains from under 0 to past twice the reference, coefficients about the
    threshold, every grey level; then, where the picture has room, the pins"""
    rng = np.random.default_rng(seed * 101 + F * 17 + H * 3 + W)
    strain = rng.uniform(-0.004, 0.026, (F, H, W)).astype(f32); rho = rng.uniform(0.5, 1.0, (F, H, W)).astype(f32)
    grey = rng.integers(0, 256, (F, H, W)).astype(np.uint8)
    if H * W >= len(PINS):
        for f in range(F):
            for i, (s, r, g) in enumerate(PINS):
                strain.reshape(F, -1)[f, i] = s; rho.reshape(F, -1)[f, i] = r; grey.reshape(F, -1)[f, i] = g
    return strain, rho, grey


def run(ctx, dev, strain, rho, grey, lut=None, skew=0, **opts):
    F, H, W = grey.shape
    n = F * H * W
    p_s = dev(strain, 4 * (skew % 4)); p_r = dev(rho); p_g = dev(grey, skew)
    p_rgb = dev(np.full(3 * n + 16, 0xA5, np.uint8), skew)
    ctx.elastogram_frames(p_s, p_r, p_g, F, H, W, p_rgb, lut=lut, **opts)
    rgb = ctx.d2h(p_rgb, (3 * n + 16,), np.uint8)
    assert (rgb[3 * n:] == 0xA5).all(), "the sentinel behind rgb_dev was overwritten"
    for p, x, name in ((p_s, strain, "strain_img_dev"), (p_r, rho, "rho_img_dev")):
        assert np.array_equal(ctx.d2h(p, x.shape).view(np.uint32), x.view(np.uint32)), "%s is read only" % name
    assert np.array_equal(ctx.d2h(p_g, grey.shape, np.uint8), grey), "grey_dev is read only"
    return rgb[:3 * n].reshape(F, H, W, 3)


@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 63), (1, 64), (1, 65), (3, 5), (16, 16), (4, 65), (37, 41), (32, 80)])
def test_pictures_match_the_mirror(mcrt, ctx, dev, H, W, F):
    strain, rho, grey = picture(F, H, W)
    lut = mcrt.host_strain_map()
    want = sm.elastogram(strain, rho, grey, lut, **OPTS)
    rgb = run(ctx, dev, strain, rho, grey, **OPTS)
    assert np.array_equal(rgb, want), "rgb %dx%d F=%d: %d bytes differ" % (H, W, F, int((rgb != want).sum()))
    if H * W >= len(PINS):
        flat = rgb.reshape(F, -1, 3).astype(int); g = grey.reshape(F, -1).astype(int)
        mix = lambda level, entry: tuple((level * 96 + int(c) * 160 + 128) >> 8 for c in lut[entry])
        for f in range(F):
            for i in (0, 1, 3):
                assert tuple(flat[f, i]) == mix(g[f, i], 128), i            # thresholds at equality are shown
            for i in (2, 4, 5, 6):
                assert tuple(flat[f, i]) == (g[f, i],) * 3, i              # under a threshold, NaN: grey
            assert tuple(flat[f, 7]) == mix(103, 255) and tuple(flat[f, 8]) == mix(104, 0) and tuple(flat[f, 9]) == mix(105, 128)
            assert tuple(flat[f, 10]) == mix(106, 0) and tuple(flat[f, 11]) == mix(107, 0) and tuple(flat[f, 12]) == mix(108, 0)
            assert tuple(flat[f, 13]) == mix(109, 255) and tuple(flat[f, 14]) == mix(110, 26)


@pytest.mark.parametrize("alpha", [0, 1, 255, 256])
def test_alpha(mcrt, ctx, dev, alpha):
    """alpha 0 leaves the grey picture, 256 the table's colours alone"""
    strain, rho, grey = picture(2, 16, 20, seed=alpha)
    lut = mcrt.host_strain_map()
    opts = dict(OPTS, alpha=alpha)
    want = sm.elastogram(strain, rho, grey, lut, **opts)
    rgb = run(ctx, dev, strain, rho, grey, **opts)
    assert np.array_equal(rgb, want)
    if alpha == 0:
        assert (rgb == grey[..., None]).all()
    if alpha == 256:
        assert tuple(rgb.reshape(2, -1, 3)[0, 0]) == tuple(lut[128]) and tuple(rgb.reshape(2, -1, 3)[1, 13]) == tuple(lut[255])


@pytest.mark.parametrize("skew", [1, 2, 3])
@pytest.mark.parametrize("H,W", [(16, 16), (7, 9)])
def test_pointers_off_a_word_boundary(mcrt, ctx, dev, H, W, skew):
    strain, rho, grey = picture(2, H, W, seed=skew)
    want = sm.elastogram(strain, rho, grey, mcrt.host_strain_map(), **OPTS)
    assert np.array_equal(run(ctx, dev, strain, rho, grey, skew=skew, **OPTS), want)


def test_defaults_negative_reference_and_own_table(mcrt, ctx, dev):
    strain, rho, grey = picture(1, 20, 30, seed=5)
    lut = mcrt.host_strain_map()
    assert np.array_equal(run(ctx, dev, strain, rho, grey), sm.elastogram(strain, rho, grey, lut))
    # a decompression: the strains and the reference are negative together
    want = sm.elastogram(-strain, rho, grey, lut, **dict(OPTS, ref_strain=-0.01))
    assert np.array_equal(run(ctx, dev, -strain, rho, grey, **dict(OPTS, ref_strain=-0.01)), want)
    assert np.array_equal(want, sm.elastogram(strain, rho, grey, lut, **OPTS))
    own = np.random.default_rng(3).integers(0, 256, (256, 3)).astype(np.uint8)
    for table in (own, lut, own[::-1]):                                    # the table lives in the context and is replaced when it changes
        assert np.array_equal(run(ctx, dev, strain, rho, grey, lut=table, **OPTS), sm.elastogram(strain, rho, grey, table, **OPTS))
    with pytest.raises(ValueError):
        run(ctx, dev, strain, rho, grey, lut=own[:255])


def test_refusals_leave_the_picture_untouched(mcrt, ctx, dev):
    L = mcrt.load_library()
    F, H, W = 2, 5, 8
    n = F * H * W
    strain, rho, grey = picture(F, H, W)
    lut = mcrt.host_strain_map()
    lut_p = lut.ctypes.data_as(C.c_void_p)
    opts = mcrt.elastogram_opts_struct(**OPTS)
    # one allocation, in bytes: strain [0, 4n), rho [4n, 8n), grey [8n, 9n), then room for rgb (3n)
    head = np.concatenate([strain.reshape(-1).view(np.uint8), rho.reshape(-1).view(np.uint8), grey.reshape(-1)])

    def call(s=0, r=4 * n, g=8 * n, frames=F, h=H, w=W, table=lut_p, o=opts, rgb=9 * n, null_ctx=False):
        big = dev(np.concatenate([head, np.full(4 * n, 0xA5, np.uint8)]))
        at = lambda b: None if b is None else C.c_void_p(big + b)
        rc = L.mcrt_elastogram_frames(None if null_ctx else ctx.h, at(s), at(r), at(g), frames, h, w, table, None if o is None else C.byref(o), at(rgb))
        got = ctx.d2h(big, (13 * n,), np.uint8)
        assert np.array_equal(got[:9 * n], head) and (got[9 * n:] == 0xA5).all()
        return rc

    assert call(null_ctx=True) == INVALID and call(s=None) == INVALID and call(r=None) == INVALID and call(g=None) == INVALID
    assert call(table=None) == INVALID and call(o=None) == INVALID and call(rgb=None) == INVALID
    assert call(frames=0) == INVALID and call(h=0) == INVALID and call(w=0) == INVALID
    assert call(frames=1 << 11, h=1 << 10, w=1 << 10) == LIMIT                             # 2^31 pixels
    for kw in (dict(ref_strain=0.0), dict(ref_strain=-0.0), dict(ref_strain=np.nan), dict(ref_strain=np.inf), dict(rho_min=np.nan), dict(rho_min=np.inf),
               dict(grey_min=256), dict(alpha=257)):
        assert call(o=mcrt.elastogram_opts_struct(**kw)) == INVALID, kw
    assert call(rgb=4 * n - 1) == INVALID and call(rgb=8 * n - 1) == INVALID and call(rgb=9 * n - 1) == INVALID      # rgb_dev overlaps each input
    assert call(rgb=0) == INVALID


def test_call_with_nothing_wrong_writes(mcrt, ctx, dev):
    """the refusal test's shape with nothing wrong is accepted: its sentinels are not a kernel that does nothing"""
    strain, rho, grey = picture(2, 5, 8)
    rgb = run(ctx, dev, strain, rho, grey, **OPTS)
    assert np.array_equal(rgb, sm.elastogram(strain, rho, grey, mcrt.host_strain_map(), **OPTS)) and (rgb != 0xA5).any()
