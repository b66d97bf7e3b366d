"""The flow overlay on the MI355X: mcrt_colour_frames (k_colour) against the numpy mirror (tests/flow_mirror.py) byte for byte and bit for
bit -- at pictures of one pixel, of less than a wavefront's tile, past one workgroup and at the display size, for one frame and three; with
every threshold deciding pixels of the case, NaN pixels, both ends of the colour table, a table of the caller's own; behind sentinels; the
refusals."""
import ctypes as C
import math
import numpy as np
import pytest

import flow_mirror as fm
import image_cases as ic

pytestmark = pytest.mark.gpu

f32 = np.float32
INVALID, LIMIT = -1, -5
V_NYQ = 333.3333333333333
OPTS = dict(power_thr=0.5, vel_thr_mm_s=40.0, grey_max=180)


@pytest.fixture(scope="module")
def ctx(mcrt):
    c = mcrt.Context(0)
    yield c
    c.close()


@pytest.fixture
def dev(ctx):
    bufs = []

    def upload(arr):
        arr = np.ascontiguousarray(arr)
        p = ctx.alloc(max(arr.nbytes, 4))
        bufs.append(p)
        ctx.h2d(p, arr)
        return p
    yield upload
    for p in bufs:
        ctx.free(p)


def picture(F, H, W, seed=0):
    """(corr_img [F][3][H][W], grey [F][H][W]): powers about the threshold, phase steps over the whole circle (velocities about the
    threshold), every grey level; then, where the picture has room, pixels that pin one condition each, NaN and infinite pixels, and the
    two ends of the colour table"""
    rng = np.random.default_rng(seed * 101 + F * 17 + H * 3 + W)
    r0 = rng.uniform(0.0, 2.0, (F, H, W))
    ang = rng.uniform(-math.pi, math.pi, (F, H, W)); mag = rng.uniform(0.1, 1.0, (F, H, W))
    x = np.stack([r0, mag * np.cos(ang), mag * np.sin(ang)], axis=1).astype(f32)
    grey = rng.integers(0, 256, (F, H, W)).astype(np.uint8)
    flat = x.reshape(F, 3, -1); g = grey.reshape(F, -1)
    if H * W >= 15:
        #            r0    re     im     grey
        pins = [(2.0, 1.0, 1.0, 100),        # shown: an eighth of a turn towards the probe
                (0.5, 1.0, 1.0, 100),        # r0 == power_thr: not above it
                (2.0, 1.0, 0.1, 100),        # |v| = 10.6 mm/s: under the velocity threshold
                (2.0, 1.0, 1.0, 181),        # brighter than grey_max
                (2.0, 1.0, 1.0, 180),        # grey_max itself: shown
                (np.nan, 0.0, 1.0, 7), (2.0, np.nan, 1.0, 8), (2.0, 1.0, np.nan, 9), (2.0, np.inf, np.inf, 10), (np.inf, 1.0, -1.0, 11),
                (2.0, -1.0, 1e-7, 12),       # ang = +pi: the table's entry 255
                (2.0, -1.0, -1e-7, 13),      # ang = -pi: entry 1
                (2.0, -1.0, 0.0, 14), (2.0, -1.0, -0.0, 15),
                (2.0, 0.0, 0.0, 16)]         # no phase at all: ang = +0, v = 0, under the velocity threshold
        for f in range(F):
            for i, (a, b, c, level) in enumerate(pins):
                flat[f, :, i] = (a, b, c); g[f, i] = level
    return x, grey


def run_colour(ctx, dev, x, grey, want_vel=True, lut=None, **opts):
    F, _, H, W = x.shape
    n = F * H * W
    p_x = dev(x); p_g = dev(grey)
    p_rgb = dev(np.full(3 * n + 16, 0xA5, np.uint8))
    p_vel = dev(np.full(n + 8, f32(-77.25))) if want_vel else None
    ctx.colour_frames(p_x, p_g, F, H, W, V_NYQ, p_rgb, vel_img_dev=p_vel, lut=lut, **opts)
    rgb = ctx.d2h(p_rgb, (3 * n + 16,), np.uint8)
    assert (rgb[3 * n:] == 0xA5).all(), "the sentinel behind rgb_dev was overwritten"
    vel = None
    if want_vel:
        vel = ctx.d2h(p_vel, (n + 8,))
        assert (vel[n:] == f32(-77.25)).all(), "the sentinel behind vel_img_dev was overwritten"
        vel = vel[:n].reshape(F, H, W)
    ic.assert_same_bits(ctx.d2h(p_x, x.shape), x, "corr_img_dev is read only")
    assert np.array_equal(ctx.d2h(p_g, grey.shape, np.uint8), grey), "grey_dev is read only"
    return rgb[:3 * n].reshape(F, H, W, 3), vel


@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (64, 65), (400, 500)])
def test_pictures_match_the_mirror(mcrt, ctx, dev, H, W, F):
    x, grey = picture(F, H, W)
    lut = mcrt.host_colour_map()
    want_rgb, want_vel = fm.colour(x, grey, lut, V_NYQ, **OPTS)
    rgb, vel = run_colour(ctx, dev, x, grey, **OPTS)
    assert np.array_equal(rgb, want_rgb), "rgb %dx%d F=%d: %d bytes differ" % (H, W, F, int((rgb != want_rgb).sum()))
    ic.assert_same_bits(vel, want_vel, "vel_img %dx%d F=%d" % (H, W, F))
    rgb2, none = run_colour(ctx, dev, x, grey, want_vel=False, **OPTS)
    assert none is None and np.array_equal(rgb2, want_rgb)
    if H * W >= 15:
        # each of the three conditions decides pixels: it alone is false there, and the pixel is grey
        r0, ang = x[:, 0], fm.atan2f(x[:, 2], x[:, 1])
        v = (ang * f32(V_NYQ / fm.PI)).astype(f32)
        with np.errstate(invalid="ignore"):
            c = [r0 > f32(OPTS["power_thr"]), np.abs(v) >= f32(OPTS["vel_thr_mm_s"]), grey <= OPTS["grey_max"]]
        shown = c[0] & c[1] & c[2]
        assert shown.any() and np.array_equal(shown, want_vel != 0)
        for k in range(3):
            alone = ~c[k] & c[(k + 1) % 3] & c[(k + 2) % 3]
            assert alone.any(), "condition %d decides no pixel" % k
            assert (rgb[alone] == grey[alone][:, None]).all() and not vel[alone].view(np.uint32).any()
        flat = rgb.reshape(F, -1, 3); fv = vel.reshape(F, -1); g = grey.reshape(F, -1)
        for f in range(F):
            assert tuple(flat[f, 0]) == tuple(lut[128 + 32]) and tuple(flat[f, 4]) == tuple(lut[128 + 32])          # pi / 4 is 31.75 levels: entry 160
            for i in (1, 2, 3, 5, 6, 7, 8, 14):                                                                      # thresholds, NaN, inf / inf, no phase
                assert tuple(flat[f, i]) == (g[f, i],) * 3 and fv[f, i].view(np.uint32) == 0, i
            assert tuple(flat[f, 9]) == tuple(lut[128 - 32])                                                         # infinite power, an eighth of a turn away
            assert tuple(flat[f, 10]) == tuple(lut[255]) and tuple(flat[f, 12]) == tuple(lut[255]) and tuple(flat[f, 11]) == tuple(lut[1])
            assert tuple(flat[f, 13]) == tuple(lut[255])                                                             # im = -0.0 is not < 0: +pi


def test_defaults_show_everything_that_has_power(mcrt, ctx, dev):
    """thresholds 0, 0 and 255: a pixel is coloured exactly where r0 > 0 and the estimate is a number"""
    x, grey = picture(2, 20, 31, seed=3)
    x[:, 0, ::3, ::2] = 0.0; x[:, 0, 1::4, 1::3] = -1.0
    lut = mcrt.host_colour_map()
    rgb, vel = run_colour(ctx, dev, x, grey)
    want_rgb, want_vel = fm.colour(x, grey, lut, V_NYQ)
    assert np.array_equal(rgb, want_rgb)
    ic.assert_same_bits(vel, want_vel, "vel_img")
    with np.errstate(invalid="ignore"):
        coloured = (x[:, 0] > 0) & ~np.isnan(fm.atan2f(x[:, 2], x[:, 1]))
    assert (rgb[~coloured] == grey[~coloured][:, None]).all() and not vel[~coloured].view(np.uint32).any() and coloured.any() and (~coloured).any()


def test_a_table_of_the_callers_own(mcrt, ctx, dev):
    """any 256 x 3 bytes: every index of the table is reached by its own angle, and a second call with another table reads that one"""
    k = np.arange(-127, 128)
    ang = k * (math.pi / 127.0)
    x = np.stack([np.full(255, 1.0), np.cos(ang), np.sin(ang)]).astype(f32).reshape(1, 3, 1, 255)
    grey = np.zeros((1, 1, 255), np.uint8)
    for seed in (1, 2):
        lut = np.random.default_rng(seed).integers(0, 256, (256, 3)).astype(np.uint8)
        rgb, _ = run_colour(ctx, dev, x, grey, lut=lut)
        assert np.array_equal(rgb, fm.colour(x, grey, lut, V_NYQ)[0])
        assert np.array_equal(rgb[0, 0, 1:-1], lut[128 + k[1:-1]])                 # (the two ends sit on the cut at +-pi)
    with pytest.raises(ValueError):
        ctx.colour_frames(dev(x), dev(grey), 1, 1, 255, V_NYQ, dev(np.zeros(3 * 255, np.uint8)), lut=np.zeros((255, 3), np.uint8))


def test_refusals(mcrt, ctx, dev):
    L = mcrt.load_library()
    F, H, W = 2, 4, 6
    n = F * H * W
    x, grey = picture(F, H, W)
    lut = mcrt.host_colour_map()
    lp = lut.ctypes.data_as(C.c_void_p)
    opts = mcrt.colour_opts_struct()
    SENT = f32(-77.25)
    # one allocation, in floats: corr_img [0, 3n), grey [3n, 3n + n / 4), room for rgb (3n / 4 floats) at 4n and vel (n) at 5n
    head = np.concatenate([x.reshape(-1).view(np.uint8), grey.reshape(-1)])

    def call(corr=0, g=3 * n, frames=F, h=H, w=W, lut_=lp, o=opts, nyq=V_NYQ, rgb=4 * n, vel=5 * n, null_ctx=False):
        big = dev(np.concatenate([head, np.full(7 * n - head.size // 4, SENT).view(np.uint8)]))
        at = lambda floats: None if floats is None else C.c_void_p(big + 4 * floats)
        rc = L.mcrt_colour_frames(None if null_ctx else ctx.h, at(corr), at(g), frames, h, w, lut_, None if o is None else C.byref(o), nyq, at(rgb), at(vel))
        got = ctx.d2h(big, (7 * n * 4,), np.uint8)
        assert np.array_equal(got[:head.size], head) and (got[head.size:].view(f32) == SENT).all()
        return rc

    assert call(null_ctx=True) == INVALID and call(corr=None) == INVALID and call(g=None) == INVALID and call(lut_=None) == INVALID
    assert call(o=None) == INVALID and call(rgb=None) == INVALID
    assert call(frames=0) == INVALID and call(h=0) == INVALID and call(w=0) == INVALID
    for kw in (dict(power_thr=np.nan), dict(power_thr=np.inf), dict(vel_thr_mm_s=-1.0), dict(vel_thr_mm_s=np.nan), dict(grey_max=256)):
        assert call(o=mcrt.colour_opts_struct(**kw)) == INVALID, kw
    for nyq in (0.0, -5.0, float("nan"), float("inf")):
        assert call(nyq=nyq) == INVALID
    assert call(frames=1 << 11, h=1 << 10, w=1 << 10) == LIMIT                            # 2^31 pixels
    assert call(rgb=3 * n - 1) == INVALID and call(rgb=3 * n) == INVALID                  # rgb_dev overlaps corr_img_dev, grey_dev
    assert call(vel=0) == INVALID and call(vel=3 * n) == INVALID and call(vel=4 * n) == INVALID and call(vel=4 * n + n // 2) == INVALID      # ... corr_img_dev, grey_dev, rgb_dev


def test_a_call_with_nothing_wrong_writes(mcrt, ctx, dev):
    """the refusal test's shape, accepted: every byte and every float is written"""
    x, grey = picture(2, 4, 6)
    rgb, vel = run_colour(ctx, dev, x, grey)
    assert np.array_equal(rgb, fm.colour(x, grey, mcrt.host_colour_map(), V_NYQ)[0]) and not (vel == f32(-77.25)).any()
