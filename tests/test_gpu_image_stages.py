"""The image stages on the MI355X at the shapes, taps, geometries and alignments the traced-frame tests never reach: k_envelope,
k_conv_axial / k_conv_lateral, k_remap and its map cache, the B-mode kernels' scalar paths, tails, chunking and peak grid-stride, and the
float4 instance of k_blocks_to_frames.  Every input is a synthetic device image (no tracing, except the group test); every image is compared
with the oracle bit for bit (tests/image_cases.assert_same_bits), the 8-bit B-mode frames with the contract's mirror (tests/bmode_mirror.py,
one grey level of log10f allowance) and their peaks bit for bit."""
import math
import numpy as np
import pytest

import bmode_mirror as bm
import compound_mirror as cm
import image_cases as ic
import volume_mirror as vm

pytestmark = pytest.mark.gpu

f32 = np.float32
LIMIT = -5          # MCRT_ERR_LIMIT


@pytest.fixture(scope="module")
def ctx(mcrt):
    c = mcrt.Context(0)
    yield c
    c.close()


class Dev:
    """device buffers of one test, freed at the end"""
    def __init__(self, ctx):
        self.ctx, self.bufs = ctx, []

    def __call__(self, nbytes, fill=None):
        p = self.ctx.alloc(nbytes)
        self.bufs.append(p)
        if fill is not None:
            self.ctx.h2d(p, np.full(nbytes, fill, np.uint8))
        return p

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self(arr.nbytes)
        self.ctx.h2d(p, arr)
        return p

    def close(self):
        for p in self.bufs:
            self.ctx.free(p)


@pytest.fixture
def dev(ctx):
    d = Dev(ctx)
    yield d
    d.close()


# ------------------------------------------------------------------ envelope (rfimage.h:54-91)
@pytest.mark.parametrize("R", ic.ENV_R)
@pytest.mark.parametrize("E", ic.ENV_E)
def test_envelope_sweep(ctx, orc, dev, E, R):
    img = ic.envelope_image(E, R)
    p = dev.upload(img)
    ctx.envelope(p, E, R)
    got = ctx.d2h(p, (E, R))
    ic.assert_same_bits(got, orc.envelope(img.T).T, "envelope %dx%d" % (E, R))


@pytest.mark.parametrize("E,R", [(3, 2), (64, 465), (129, 2048)])
def test_envelope_frames_equal_the_per_image_calls(ctx, orc, dev, E, R):
    F = 3
    frames = np.stack([ic.envelope_image(E, R, seed=1 + f) for f in range(F)])
    p = dev.upload(frames)
    ctx.envelope_frames(p, F, E, R)
    got = ctx.d2h(p, (F, E, R))
    one = dev(frames[0].nbytes)
    for f in range(F):
        ctx.h2d(one, frames[f])
        ctx.envelope(one, E, R)
        assert np.array_equal(got[f].view(np.uint32), ctx.d2h(one, (E, R)).view(np.uint32)), f
        ic.assert_same_bits(got[f], orc.envelope(frames[f].T).T, "envelope_frames %d" % f)


def test_envelope_row_limits_leave_the_image_untouched(mcrt, ctx, orc, dev):
    """R = 1: nothing to find, the image stays (GPU and oracle); R = 2049: MCRT_ERR_LIMIT and the image stays"""
    img = np.array([[-1.5], [2.0], [np.nan], [-0.0], [np.inf]], f32)          # [E=5][R=1]
    p = dev.upload(img)
    ctx.envelope(p, 5, 1)
    ctx.envelope_frames(p, 5, 1, 1)
    assert np.array_equal(ctx.d2h(p, (5, 1)).view(np.uint32), img.view(np.uint32))
    assert np.array_equal(orc.envelope(img.T).view(np.uint32), img.T.view(np.uint32))
    big = ic.envelope_image(2, 2049)
    q = dev.upload(big)
    for call in (lambda: ctx.envelope(q, 2, 2049), lambda: ctx.envelope_frames(q, 1, 2, 2049)):
        with pytest.raises(mcrt.McrtError) as e:
            call()
        assert e.value.code == LIMIT
    ctx.synchronize()
    assert np.array_equal(ctx.d2h(q, (2, 2049)).view(np.uint32), big.view(np.uint32))


# ------------------------------------------------------------------ convolution (rfimage.h:93-123)
@pytest.mark.parametrize("n_lat", ic.CONV_LAT)
@pytest.mark.parametrize("n_ax", ic.CONV_AX)
def test_convolve_sweep(ctx, orc, dev, n_ax, n_lat):
    """every pixel compared: inside the window the oracle's sums, outside it the input's own bits"""
    ax, lat = ic.conv_taps(n_ax, n_lat)
    for E, R in ic.conv_shapes(n_ax, n_lat):
        img = ic.conv_image(E, R)
        p = dev.upload(img)
        ctx.convolve(p, E, R, ax, lat)
        ic.assert_same_bits(ctx.d2h(p, (E, R)), orc.convolve(img.T, ax, lat).T, "convolve %dx%d taps %d/%d" % (E, R, n_ax, n_lat))


@pytest.mark.parametrize("n_ax,n_lat", [(1, 1), (7, 13), (16, 32)])
def test_convolve_frames_equal_the_per_image_calls(ctx, orc, dev, n_ax, n_lat):
    F, E, R = 3, 129, 465
    ax, lat = ic.conv_taps(n_ax, n_lat, seed=3)
    frames = np.stack([ic.conv_image(E, R, seed=f) for f in range(F)])
    p = dev.upload(frames)
    ctx.convolve_frames(p, F, E, R, ax, lat)
    got = ctx.d2h(p, (F, E, R))
    one = dev(frames[0].nbytes)
    for f in range(F):
        ctx.h2d(one, frames[f])
        ctx.convolve(one, E, R, ax, lat)
        assert np.array_equal(got[f].view(np.uint32), ctx.d2h(one, (E, R)).view(np.uint32)), f
        ic.assert_same_bits(got[f], orc.convolve(frames[f].T, ax, lat).T, "convolve_frames %d" % f)


def test_convolve_tap_limits_leave_the_image_untouched(mcrt, ctx, dev):
    E, R = 40, 60
    img = ic.conv_image(E, R)
    p = dev.upload(img)
    for n_ax, n_lat in ((17, 13), (7, 33)):
        ax, lat = ic.conv_taps(n_ax, n_lat)
        for call in (lambda: ctx.convolve(p, E, R, ax, lat), lambda: ctx.convolve_frames(p, 1, E, R, ax, lat)):
            with pytest.raises(mcrt.McrtError) as e:
                call()
            assert e.value.code == LIMIT
    ctx.synchronize()
    assert np.array_equal(ctx.d2h(p, (E, R)).view(np.uint32), img.view(np.uint32))


# ------------------------------------------------------------------ scan conversion (rfimage.h:125-140,183-215)
def _scan(ctx, dev, img, geom, F=None):
    radius, angle, orows, ocols = geom
    E, R = img.shape[-2:]
    p = dev.upload(img)
    n = orows * ocols
    if F is None:
        out = dev(4 * n)
        ctx.scan_convert(p, E, R, out, radius_mm=radius, total_angle=angle, out_rows=orows, out_cols=ocols)
        return ctx.d2h(out, (orows, ocols))
    out = dev(4 * n * F)
    ctx.scan_convert_frames(p, F, E, R, out, radius_mm=radius, total_angle=angle, out_rows=orows, out_cols=ocols)
    return ctx.d2h(out, (F, orows, ocols))


def _want(orc, img, geom):
    radius, angle, orows, ocols = geom
    return orc.scan_convert(img.T, radius_mm=radius, total_angle=angle, out_rows=orows, out_cols=ocols)


@pytest.mark.parametrize("geom", ic.SCAN_GEOMETRIES, ids=lambda g: "%gmm-%.3frad-%dx%d" % g)
def test_scan_convert_sweep(ctx, orc, dev, geom):
    for E, R in ic.SCAN_SHAPES:
        img = ic.scan_image(E, R)
        ic.assert_same_bits(_scan(ctx, dev, img, geom), _want(orc, img, geom), "scan_convert %s %dx%d" % (geom, E, R))
    for E, R in ((3, 2), (128, 2048)):
        frames = np.stack([ic.scan_image(E, R, seed=f) for f in range(3)])
        got = _scan(ctx, dev, frames, geom, F=3)
        for f in range(3):
            ic.assert_same_bits(got[f], _want(orc, frames[f], geom), "scan_convert_frames %s %dx%d frame %d" % (geom, E, R, f))


# (30 mm, 1 rad) and (29.999999 mm, 2 rad): the same radius_mm * 1e6 + total_angle, the map cache's old key
COLLIDING = ((30.0, 1.0), (29.999999, 2.0))


def test_map_cache_follows_the_geometry(mcrt, orc):
    """A, B, A and then the colliding pair on one context: each image equals the oracle's for its own geometry"""
    assert COLLIDING[0][0] * 1e6 + COLLIDING[0][1] == COLLIDING[1][0] * 1e6 + COLLIDING[1][1]
    c = mcrt.Context(0)
    d = Dev(c)
    try:
        E, R, orows, ocols = 64, 300, 200, 240
        img = ic.scan_image(E, R)
        A, B = (30.0, math.pi / 3), (10.0, math.pi / 2)
        for radius, angle in (A, B, A) + COLLIDING:
            geom = (radius, angle, orows, ocols)
            ic.assert_same_bits(_scan(c, d, img, geom), _want(orc, img, geom), "map cache at %s" % (geom,))
    finally:
        d.close()
        c.close()


def test_bmode_shares_the_map_cache(mcrt, orc):
    """the same through mcrt_bmode_frames, which draws on the same cached maps: scan_convert then bmode_frames, and bmode_frames twice"""
    c = mcrt.Context(0)
    d = Dev(c)
    try:
        E, R, orows, ocols = 64, 300, 200, 240
        rng = np.random.default_rng(21)
        frames = (rng.rayleigh(1.0, (1, E, R)) * np.where(rng.random((1, E, R)) < 0.5, -1, 1)).astype(f32)
        rf = d.upload(frames)
        out = d(orows * ocols)
        img = frames[0]
        for first, second in ((COLLIDING[0], COLLIDING[1]), (COLLIDING[1], COLLIDING[0])):
            g1 = first + (orows, ocols)
            ic.assert_same_bits(_scan(c, d, img, g1), _want(orc, img, g1), "scan_convert at %s" % (g1,))
            for radius, angle in (second, first):
                c.bmode_frames(rf, 1, E, R, out, radius_mm=radius, total_angle=angle, out_rows=orows, out_cols=ocols)
                got = c.d2h(out, (1, orows, ocols), np.uint8)
                want, _, _ = bm.bmode(orc, frames, radius_mm=radius, total_angle=angle, out_rows=orows, out_cols=ocols)
                bm.assert_close(got[0], want[0])
    finally:
        d.close()
        c.close()


def test_the_three_map_caches_do_not_evict_each_other(mcrt, orc):
    """scan conversion, a two-view compound, a volume of two planes and a B-mode frame in turn on one context, twice round, nothing waited
    for between the calls: the plain, the compound and the volume maps live in three caches of one type, and every output of both rounds
    equals its mirror (merged into one pool of slots, a later call's maps would replace an earlier call's)"""
    c = mcrt.Context(0)
    d = Dev(c)
    try:
        E, R, rows, cols, K = 16, 64, 20, 24, 2                # 480 pixels: one whole wavefront of 256 and a tail
        radius, angle = ic.SCAN_GEOMETRIES[0][:2]
        geom = dict(radius_mm=radius, total_angle=angle, out_rows=rows, out_cols=cols)
        steers, sweep = (0.0, 0.1), (K, vm.STEP, 0.0)
        g = vm.grid_for(mcrt, (9, 7, 2), E, R, K, 0.0)
        img = ic.scan_image(E, R)
        views = np.stack([ic.scan_image(E, R, seed=1 + n) for n in range(2)])[None]
        planes = np.stack([ic.scan_image(E, R, seed=3 + k) for k in range(K)])[None]
        frames = bmode_frames(E, R, 1)
        p_img, p_views, p_planes, p_frames = d.upload(img), d.upload(views), d.upload(planes), d.upload(frames)
        n, nv = rows * cols, g.nu * g.nv * g.nw
        outs = [(d(4 * n, 0xA5), d(4 * n, 0xA5), d(4 * nv, 0xA5), d(n, 0xA5)) for _ in range(2)]
        for scan, comp, vol, grey in outs:
            c.scan_convert_frames(p_img, 1, E, R, scan, **geom)
            c.compound_frames(p_views, 1, E, R, steers, comp, **geom)
            c.volume_frames(p_planes, 1, E, R, sweep, g, vol, radius_mm=radius, total_angle=angle)
            c.bmode_frames(p_frames, 1, E, R, grey, **geom)
        c.synchronize()
        want_scan = _want(orc, img, (radius, angle, rows, cols))
        want_comp = cm.compound_frames(views, [mcrt.host_compound_maps(E, R, s, radius, angle, out_rows=rows, out_cols=cols) for s in steers])
        want_vol = vm.volume_frames(planes, mcrt.host_volume_maps(E, R, sweep, g, radius_mm=radius, total_angle=angle))
        want_grey, _, _ = bm.bmode(orc, frames, **geom)
        for i, (scan, comp, vol, grey) in enumerate(outs):
            ic.assert_same_bits(c.d2h(scan, (rows, cols)), want_scan, "scan conversion, round %d" % i)
            ic.assert_same_bits(c.d2h(comp, (1, rows, cols)), want_comp, "compound, round %d" % i)
            ic.assert_same_bits(c.d2h(vol, (1, g.nw, g.nv, g.nu)), want_vol, "volume, round %d" % i)
            bm.assert_close(c.d2h(grey, (1, rows, cols), np.uint8)[0], want_grey[0])
    finally:
        d.close()
        c.close()


# ------------------------------------------------------------------ B-mode (include/mcrt.h, mcrt_bmode_frames): every kernel branch
def bmode_frames(E, R, F, seed=0):
    """[F][E][R]: signed Rayleigh speckle with a NaN stretch, an inf tap and a zero scan-line"""
    rng = np.random.default_rng(300 + seed)
    fr = (rng.rayleigh(1.0, (F, E, R)) * np.where(rng.random((F, E, R)) < 0.5, -1.0, 1.0)).astype(f32)
    for f in range(F):
        e = f % E
        fr[f, e, : max(1, R // 3)] = np.nan
        fr[f, (e + 1) % E, R // 2] = np.inf
        if E > 2:
            fr[f, (e + 2) % E] = 0.0
    return fr


def run_bmode(ctx, dev, frames, out_shape, rf_off=0, out_off=0, **kw):
    """frames [F][E][R] at rf_dev + rf_off bytes -> (bytes [F][rows][cols] written at out_dev + out_off, peaks [F]); the bytes around
    the output are checked to be untouched"""
    F, E, R = frames.shape
    n = out_shape[0] * out_shape[1]
    rf = dev(frames.nbytes + 16)
    ctx.h2d(rf + rf_off, frames)
    out = dev(F * n + 16, 0xA5)
    peak = dev(4 * F, 0xA5)
    ctx.bmode_frames(rf + rf_off, F, E, R, out + out_off, peak_dev=peak, out_rows=out_shape[0], out_cols=out_shape[1], **kw)
    ctx.synchronize()
    raw = ctx.d2h(out, (F * n + 16,), np.uint8)
    assert np.all(raw[:out_off] == 0xA5) and np.all(raw[out_off + F * n:] == 0xA5), "bytes outside the output written"
    return raw[out_off:out_off + F * n].reshape((F,) + tuple(out_shape)), ctx.d2h(peak, (F,), np.float32)


def check_bmode(orc, got, peaks, frames, out_shape, **kw):
    want, refs, _ = bm.bmode(orc, frames, out_rows=out_shape[0], out_cols=out_shape[1], **kw)
    for f in range(frames.shape[0]):
        bm.assert_close(got[f], want[f])
    assert np.array_equal(peaks.view(np.uint32), refs.view(np.uint32)), (peaks, refs)
    return want


# (id, E, R, F, out shape, rf_dev offset, out_dev offset)
BMODE_CASES = [("ER-3x7", 3, 7, 2, (40, 50), 0, 0),                 # E*R % 4 != 0: scalar k_bmode_peak / k_bmode_grey
               ("ER-5x465", 5, 465, 2, (64, 80), 0, 0),
               ("rf+4", 128, 465, 2, (100, 120), 4, 0),             # rf_dev not 16-byte aligned: the scalar peak / grey too
               ("out-401x499", 128, 465, 1, (401, 499), 0, 0),      # n % 4 != 0: scalar k_bmode and its < 4-pixel tail
               ("out-7x9", 16, 64, 3, (7, 9), 0, 0),
               ("out+1", 128, 465, 2, (400, 500), 0, 1)]            # out_dev not 4-byte aligned: scalar k_bmode
DISPLAY = [("db", None, False), ("db", 2.5, True), ("ref_log", None, True), ("ref_log", 2.5, False)]


@pytest.mark.parametrize("mode,ref,with_tgc", DISPLAY, ids=["%s-%s-%s" % (m, "auto" if r is None else "fixed", "tgc" if t else "flat") for m, r, t in DISPLAY])
@pytest.mark.parametrize("case", BMODE_CASES, ids=[c[0] for c in BMODE_CASES])
def test_bmode_branches(ctx, orc, dev, case, mode, ref, with_tgc):
    _, E, R, F, out_shape, rf_off, out_off = case
    frames = bmode_frames(E, R, F)
    tgc = (0.03 * np.arange(R)).astype(f32) if with_tgc else None
    kw = dict(mode=mode, ref=ref, tgc_db=tgc, dynamic_range_db=50.0, gain_db=3.0)
    got, peaks = run_bmode(ctx, dev, frames, out_shape, rf_off, out_off, **kw)
    check_bmode(orc, got, peaks, frames, out_shape, **kw)
    assert got.any()


@pytest.mark.parametrize("with_tgc", [False, True])
def test_bmode_peak_beyond_the_block_cap(ctx, orc, dev, with_tgc):
    """512 x 2048 taps = 128 blocks' worth: k_bmode_peak is capped at 64 blocks per frame and grid-strides; the one bright tap sits in
    the last stretch of the frame (a different one per frame) and must be each frame's peak, bit for bit"""
    E, R, F = 512, 2048, 2
    rng = np.random.default_rng(77)
    frames = (rng.random((F, E, R)) * 0.5).astype(f32)
    spots = [(E - 1, R - 2), (E - 3, R - 700)]
    for f, (e, r) in enumerate(spots):
        frames[f, e, r] = f32(-1.0e4 * (f + 1))
    tgc = (0.02 * np.arange(R)).astype(f32) if with_tgc else None
    for mode in ("db", "ref_log"):
        got, peaks = run_bmode(ctx, dev, frames, (200, 240), mode=mode, tgc_db=tgc)
        check_bmode(orc, got, peaks, frames, (200, 240), mode=mode, tgc_db=tgc)
        k = bm.tgc_factors(tgc, R)
        for f, (e, r) in enumerate(spots):
            assert peaks[f] == np.abs(frames[f, e, r]) * k[r], f


@pytest.mark.parametrize("mode,ref", [("db", None), ("ref_log", 2.5)])
def test_bmode_frames_in_chunks(ctx, orc, dev, mode, ref):
    """F = 44 at 400 x 500 without persistence: frames_per_chunk = 3, 15 chunks, the last one of 2 frames"""
    E, R, F = 32, 100, 44
    frames = bmode_frames(E, R, F, seed=5)
    tgc = (0.05 * np.arange(R)).astype(f32)
    got, peaks = run_bmode(ctx, dev, frames, (400, 500), mode=mode, ref=ref, tgc_db=tgc)
    check_bmode(orc, got, peaks, frames, (400, 500), mode=mode, ref=ref, tgc_db=tgc)
    one = dev(400 * 500)
    rf = dev.upload(frames)
    for f in (0, 2, 3, 41, 42, 43):                          # chunk edges: the per-frame calls give the same bytes
        ctx.bmode_frames(rf + f * E * R * 4, 1, E, R, one, mode=mode, ref=ref, tgc_db=tgc)
        assert np.array_equal(ctx.d2h(one, (400, 500), np.uint8), got[f]), f


def test_bmode_persistence_on_an_odd_output(ctx, orc, dev):
    """401 x 499 (scalar k_bmode, a 3-pixel tail) with persistence: 2 + 3 frames chained through state_dev == one call of 5, bit for bit"""
    E, R, F, shape = 64, 465, 5, (401, 499)
    n = shape[0] * shape[1]
    frames = bmode_frames(E, R, F, seed=9)
    rf = dev.upload(frames)
    st = dev(4 * n)
    five = dev(F * n, 0)
    kw = dict(persistence=0.5, out_rows=shape[0], out_cols=shape[1], tgc_db=(0.02 * np.arange(R)).astype(f32))
    ctx.bmode_frames(rf, F, E, R, five, state_dev=st, reset_state=True, **kw)
    g5 = ctx.d2h(five, (F,) + shape, np.uint8)
    s5 = ctx.d2h(st, shape)
    want, _, ys = bm.bmode(orc, frames, persistence=0.5, out_rows=shape[0], out_cols=shape[1], tgc_db=kw["tgc_db"])
    for f in range(F):
        bm.assert_close(g5[f], want[f])
    assert np.abs(s5 - ys).max() < 1e-5
    ctx.h2d(st, np.full(shape, np.nan, f32))
    split = dev(F * n, 0)
    ctx.bmode_frames(rf, 2, E, R, split, state_dev=st, reset_state=True, **kw)
    ctx.bmode_frames(rf + 2 * E * R * 4, 3, E, R, split + 2 * n, state_dev=st, reset_state=False, **kw)
    assert np.array_equal(ctx.d2h(split, (F,) + shape, np.uint8), g5)
    assert np.array_equal(ctx.d2h(st, shape).view(np.uint32), s5.view(np.uint32))


# ------------------------------------------------------------------ the group's gather, float4 instance (R % 4 == 0)
def test_group_gather_float4_equals_single_context(mcrt, sphere):
    cfg, sd = sphere
    E, S, F, R = 16, 32, 3, 464
    tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    tex = mcrt.host_texture(32)
    one = mcrt.Context(0)
    grp = mcrt.Group([0, 0, 0])
    try:
        for obj in (one, grp):
            obj.set_params(n_elements=E, n_samples=S, frequency=tr.frequency, n_rows=R, tex_n=32)
            obj.upload_scene(sd); obj.upload_texture(tex, 32); obj.set_transducer(tr.pos, tr.dir)
        assert one.params.n_rows == R and grp.root.params.n_rows == R
        a, b = one.alloc(F * E * R * 4), grp.root.alloc(F * E * R * 4)
        one.trace_frames(4, F, a)
        grp.trace_frames(4, F, b)
        grp.synchronize()
        want, got = one.d2h(a, (F, E, R)), grp.root.d2h(b, (F, E, R))
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert np.abs(np.nan_to_num(want)).sum() > 0 and not np.array_equal(want[0], want[1])
        one.free(a); grp.root.free(b)
    finally:
        grp.close()
        one.close()
