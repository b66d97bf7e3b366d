"""Frequency compounding on the MI355X: mcrt_convolve_bands_frames (k_conv_axial_bands + the lateral kernels) against the numpy mirror
(tests/bands_mirror.py) bit for bit on synthetic device images, constant tables against mcrt_convolve_frames / mcrt_convolve_frames_depth,
passes against single calls, table uploads between back-to-back calls, mcrt_band_fold_frames against elevation_mirror's fold, argument
errors, an impulse column, the Simulator, the C++ shim and the CLI."""
import ctypes as C
import json
import os
import subprocess
import numpy as np
import pytest

import bands_mirror as bm
import elevation_mirror as em
import image_cases as ic
import noise_mirror as nm

pytestmark = pytest.mark.gpu

f32 = np.float32
INVALID, LIMIT = -1, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx(mcrt):
    c = mcrt.Context(0)
    yield c
    c.close()


class Dev:
    """device buffers of one test, freed at the end"""
    def __init__(self, ctx):
        self.ctx, self.bufs = ctx, []

    def __call__(self, nbytes):
        p = self.ctx.alloc(max(nbytes, 4))
        self.bufs.append(p)
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


def table(shape, seed=0):
    """random taps with both signs, zeros and -0.0"""
    rng = np.random.default_rng(900 + 31 * shape[-2] + shape[-1] + 7 * len(shape) + seed)
    t = rng.standard_normal(shape).astype(f32)
    t[rng.random(shape) < 0.1] = 0.0
    t[rng.random(shape) < 0.02] = -0.0
    return t


SENTINEL = f32(-77.25)


def run_bands(ctx, dev, frames, ax_rows, lateral=None, lat_rows=None):
    """the call on frames [F][E][R] -> (bands [F][B][E][R], the input as the device holds it afterwards); the output starts as a sentinel"""
    F, E, R = frames.shape
    B = ax_rows.shape[0]
    p = dev.upload(frames)
    q = dev.upload(np.full((F, B, E, R), SENTINEL, f32))
    ctx.convolve_bands_frames(p, F, E, R, ax_rows, q, lateral=lateral, lat_rows=lat_rows)
    return ctx.d2h(q, (F, B, E, R)), ctx.d2h(p, (F, E, R))


@pytest.mark.parametrize("n_lat", [1, 13, 32])
@pytest.mark.parametrize("n_ax", ic.CONV_AX)
@pytest.mark.parametrize("B", [1, 3, 8])
def test_random_tables_match_the_mirror(ctx, dev, B, n_ax, n_lat):
    """every pixel compared: inside the windows the mirror's sums, outside them the input's own bits (NaN, inf and -0.0 included); both lateral
    forms; F = 1 and 3; the input is unchanged afterwards"""
    shapes = ic.conv_shapes(n_ax, n_lat) + [(3, 2048), (37, 1001), (130, 2047)]
    for i, (E, R) in enumerate(shapes):
        F = 3 if i % 2 else 1
        frames = np.stack([ic.conv_image(E, R, seed=f) for f in range(F)])
        ax = table((B, R, n_ax), seed=i)
        depth = i % 2 == 0 or (E, R) == (129, 465)
        lat = table((R, n_lat), seed=i) if depth else table((1, n_lat), seed=i)[0]
        kw = dict(lat_rows=lat) if depth else dict(lateral=lat)
        got, after = run_bands(ctx, dev, frames, ax, **kw)
        assert np.array_equal(after.view(np.uint32), frames.view(np.uint32)), "rf_dev changed"
        for f in range(F):
            ic.assert_same_bits(got[f], bm.convolve_bands(frames[f], ax, **kw), "bands %dx%d B %d taps %d/%d frame %d" % (E, R, B, n_ax, n_lat, f))
        dev.close(); dev.bufs = []


@pytest.mark.parametrize("n_ax,n_lat", [(1, 1), (7, 13), (16, 32)])
def test_constant_tables_are_the_plain_calls(ctx, dev, n_ax, n_lat):
    F, E, R, B = 2, 129, 465, 3
    frames = np.stack([ic.conv_image(E, R, seed=f) for f in range(F)])
    axs = [ic.conv_taps(n_ax, n_lat, seed=s)[0] for s in range(B)]
    lat = ic.conv_taps(n_ax, n_lat, seed=2)[1]
    rows = table((R, n_lat), seed=1)
    ax_rows = np.stack([np.tile(a, (R, 1)) for a in axs])
    plain, _ = run_bands(ctx, dev, frames, ax_rows, lateral=lat)
    depth, _ = run_bands(ctx, dev, frames, ax_rows, lat_rows=rows)
    for b in range(B):
        a, d = dev.upload(frames), dev.upload(frames)
        ctx.convolve_frames(a, F, E, R, axs[b], lat)
        ctx.convolve_frames_depth(d, F, E, R, axs[b], rows)
        assert np.array_equal(plain[:, b].view(np.uint32), ctx.d2h(a, (F, E, R)).view(np.uint32)), b
        assert np.array_equal(depth[:, b].view(np.uint32), ctx.d2h(d, (F, E, R)).view(np.uint32)), b


def test_a_nan_and_an_inf_spread_as_the_mirror_says(ctx, dev):
    E, R, n_ax, n_lat, B = 40, 120, 7, 13, 3
    img = np.zeros((1, E, R), f32)
    img[0, 20, 60] = np.nan
    img[0, 5, 30] = np.inf
    ax = table((B, R, n_ax), seed=5)
    ax[1, 50:70, 2] = 0.0                                  # 0 * NaN is NaN too
    lat = table((R, n_lat), seed=5)
    got, _ = run_bands(ctx, dev, img, ax, lat_rows=lat)
    want = bm.convolve_bands(img[0], ax, lat_rows=lat)
    ic.assert_same_bits(got[0], want, "nan")
    for b in range(B):
        assert 20 < np.isnan(want[b]).sum() < E * R // 4   # the NaN reached a patch of every band image, not all of it


@pytest.mark.parametrize("E,R", [(129, 465), (3, 2048)])
def test_a_pass_equals_the_per_image_calls(ctx, dev, E, R):
    F, n_ax, n_lat, B = 4, 7, 13, 3
    ax = table((B, R, n_ax), seed=3)
    lat = table((1, n_lat), seed=3)[0]
    frames = np.stack([ic.conv_image(E, R, seed=10 + f) for f in range(F)])
    got, _ = run_bands(ctx, dev, frames, ax, lateral=lat)
    for f in range(F):
        one, _ = run_bands(ctx, dev, frames[f:f + 1], ax, lateral=lat)
        assert np.array_equal(got[f].view(np.uint32), one[0].view(np.uint32)), f


def test_back_to_back_calls_each_get_their_own_tables(ctx, dev):
    """four calls with different tables and shapes, no synchronisation between them, the caller's arrays overwritten as soon as each returns"""
    n_ax, n_lat = 7, 13
    shapes = [(96, 465, 3), (96, 465, 3), (40, 2048, 8), (96, 465, 3)]
    axs = [table((B, R, n_ax), seed=s) for (E, R, B), s in zip(shapes, (11, 12, 13, 11))]
    lats = [table((R, n_lat), seed=s) for (E, R, B), s in zip(shapes, (21, 21, 22, 23))]
    imgs = [ic.conv_image(E, R, seed=30 + i)[None] for i, (E, R, B) in enumerate(shapes)]
    ps = [dev.upload(im) for im in imgs]
    qs = [dev.upload(np.full((B, E, R), SENTINEL, f32)) for E, R, B in shapes]
    ctx.synchronize()
    for p, q, a, l, (E, R, B) in zip(ps, qs, axs, lats, shapes):
        abuf, lbuf = a.copy(), l.copy()
        ctx.convolve_bands_frames(p, 1, E, R, abuf, q, lat_rows=lbuf)
        abuf[:] = np.nan; lbuf[:] = np.nan                 # the call has returned: the tables are the caller's again
    ctx.synchronize()
    for i, (q, a, l, im, (E, R, B)) in enumerate(zip(qs, axs, lats, imgs, shapes)):
        ic.assert_same_bits(ctx.d2h(q, (B, E, R)), bm.convolve_bands(im[0], a, lat_rows=l), "call %d" % i)


@pytest.mark.parametrize("B", [1, 3, 8])
def test_the_fold_matches_the_mirror(ctx, dev, B):
    for F, E, R in ((1, 5, 7), (3, 129, 465), (2, 3, 2047)):          # R % 4 != 0: rows wrap inside a float4, or the scalar form
        rng = np.random.default_rng(40 + B + R)
        stack = np.stack([np.stack([ic.conv_image(E, R, seed=f * 8 + b) for b in range(B)]) for f in range(F)])
        w = table((R, B), seed=B)
        w[rng.random((R, B)) < 0.2] = 0.0                              # a NaN reaches the output under a zero weight
        p = dev.upload(stack)
        q = dev.upload(np.full((F, E, R), SENTINEL, f32))
        ctx.band_fold_frames(p, F, B, E, R, w, q)
        ic.assert_same_bits(ctx.d2h(q, (F, E, R)), em.fold(stack, w), "fold B %d %dx%dx%d" % (B, F, E, R))
        assert np.array_equal(ctx.d2h(p, stack.shape).view(np.uint32), stack.view(np.uint32))


def test_one_band_of_weight_one_copies(ctx, dev):
    E, R = 33, 465
    img = ic.conv_image(E, R, seed=9)
    img[0, :3] = (-0.0, 0.0, -1.5)
    p, q = dev.upload(img), dev(img.nbytes)
    ctx.band_fold_frames(p, 1, 1, E, R, np.ones((R, 1), f32), q)
    got = ctx.d2h(q, (E, R))
    want = img.copy()
    want[(img == 0) & ~np.isnan(img)] = 0.0                             # a -0.0 becomes +0.0 (0.0f + -0.0f * 1.0f)
    ic.assert_same_bits(got, want, "copy")
    assert got.view(np.uint32)[0, 0] == 0


def test_errors_leave_the_device_memory_untouched(mcrt, ctx, dev):
    E, R, B, n_ax, n_lat = 40, 60, 3, 7, 13
    img = ic.conv_image(E, R)[None]
    p = dev.upload(img)
    out = np.full((B, E, R), SENTINEL, f32)
    q = dev.upload(out)
    big = dev.upload(np.full((2, 2049), SENTINEL, f32))
    ax, lat, rows, w = table((B, R, n_ax)), table((1, n_lat))[0], table((R, n_lat)), table((R, B))
    cases = [(lambda: ctx.convolve_bands_frames(p, 1, E, R, ax, q, lateral=lat, lat_rows=rows), INVALID),          # both
             (lambda: ctx.convolve_bands_frames(p, 1, E, R, ax, q), INVALID),                                      # neither
             (lambda: ctx.convolve_bands_frames(p, 1, E, R, table((9, R, n_ax)), q, lateral=lat), INVALID),
             (lambda: ctx.convolve_bands_frames(p, 1, E, R, table((B, R, 17)), q, lateral=lat), LIMIT),
             (lambda: ctx.convolve_bands_frames(p, 1, E, R, ax, q, lateral=table((1, 33))[0]), LIMIT),
             (lambda: ctx.convolve_bands_frames(big, 1, 1, 2049, table((1, 2049, n_ax)), big + 4 * 2049, lateral=lat), LIMIT),
             (lambda: ctx.convolve_bands_frames(p, 1, E, R, ax[:1], p, lateral=lat), INVALID),                     # overlap: the same buffer
             (lambda: ctx.convolve_bands_frames(q + 4 * E * R, 1, E, R, ax[:2], q, lateral=lat), INVALID),          # overlap: the input inside the output
             (lambda: ctx.band_fold_frames(q, 1, B, E, R, w, q + 4 * 2 * E * R), INVALID),                          # overlap
             (lambda: ctx.band_fold_frames(q, 1, 9, E, R, table((R, 9)), p), INVALID),
             (lambda: ctx.band_fold_frames(big, 1, 1, 1, 2049, table((2049, 1)), big + 4 * 2049), LIMIT)]
    for i, (call, code) in enumerate(cases):
        with pytest.raises(mcrt.McrtError) as e:
            call()
        assert e.value.code == code, i
    L = ctx.L
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    pv, qv = C.c_void_p(p), C.c_void_p(q)
    conv = L.mcrt_convolve_bands_frames
    assert conv(ctx.h, pv, 1, E, R, 0, vp(ax), n_ax, vp(lat), None, n_lat, qv) == INVALID                         # B = 0
    assert conv(ctx.h, None, 1, E, R, B, vp(ax), n_ax, vp(lat), None, n_lat, qv) == INVALID
    assert conv(ctx.h, pv, 1, E, R, B, None, n_ax, vp(lat), None, n_lat, qv) == INVALID
    assert conv(ctx.h, pv, 1, E, R, B, vp(ax), n_ax, vp(lat), None, n_lat, None) == INVALID
    assert conv(None, pv, 1, E, R, B, vp(ax), n_ax, vp(lat), None, n_lat, qv) == INVALID
    assert conv(ctx.h, pv, 0, E, R, B, vp(ax), n_ax, vp(lat), None, n_lat, qv) == INVALID
    assert conv(ctx.h, pv, 1, E, R, B, vp(ax), 0, vp(lat), None, n_lat, qv) == LIMIT
    fold = L.mcrt_band_fold_frames
    assert fold(ctx.h, qv, 1, 0, E, R, vp(w), pv) == INVALID
    assert fold(ctx.h, None, 1, B, E, R, vp(w), pv) == INVALID
    assert fold(ctx.h, qv, 1, B, E, R, None, pv) == INVALID
    assert fold(ctx.h, qv, 1, B, E, R, vp(w), None) == INVALID
    with pytest.raises(ValueError):
        ctx.convolve_bands_frames(p, 1, E, R, table((B, R + 1, n_ax)), q, lateral=lat)
    with pytest.raises(ValueError):
        ctx.band_fold_frames(q, 1, B, E, R, table((R, B + 1)), p)
    ctx.synchronize()
    assert np.array_equal(ctx.d2h(p, img.shape).view(np.uint32), img.view(np.uint32))
    assert np.array_equal(ctx.d2h(q, out.shape).view(np.uint32), out.view(np.uint32))
    assert (ctx.d2h(big, (2, 2049)) == SENTINEL).all()


def test_an_impulse_column_shows_each_rows_taps(mcrt, ctx, dev):
    """img[e0][r0] = 1: bands[b][e0][r0 - k] = ax_rows[b][r0 - k][k] for every k whose row stays inside the window -- row r0 - k's OWN tap k, under
    a downshift a different number on every row"""
    E, R, n_ax, e0, B = 8, 465, 7, 3, 3
    ax, _ = mcrt.host_psf_bands(mcrt.bands_struct((3.5, 4.5, 5.5), downshift_mhz_per_mm=0.02, min_mhz=2.0), 145, R, 0.322, n_ax)
    for r0 in (n_ax, n_ax + 3, 200, R - n_ax - 1, R - n_ax + 3, R - 1):
        img = np.zeros((1, E, R), f32)
        img[0, e0, r0] = 1.0
        got, _ = run_bands(ctx, dev, img, ax, lateral=np.ones(1, f32))
        seen = 0
        for b in range(B):
            for k in range(n_ax):
                r = r0 - k
                if n_ax <= r < R - n_ax:
                    assert got[0, b, e0, r].view(np.uint32) == ax[b, r, k].view(np.uint32), (b, r0, k)
                    seen += 1
        assert seen == B * sum(1 for k in range(n_ax) if n_ax <= r0 - k < R - n_ax)
        dev.close(); dev.bufs = []


def _chain(orc, raw, psf, R, row_mm, noise=None):
    """the mirror's chain from a raw host frame [R][E]: band convolution, (noise,) the oracle's envelope, the fold -> [R][E]"""
    ax, w = psf.axial_rows(R, row_mm), psf.band_weights(R, row_mm)
    imgs = bm.convolve_bands(np.ascontiguousarray(raw.T), ax, lateral=psf.lateral_kernel)
    if noise is not None:
        imgs = noise(imgs)
    env = np.stack([orc.envelope(np.ascontiguousarray(im.T)).T for im in imgs])
    return imgs, em.fold(env[None], w)[0].T


def test_simulator(mcrt, orc, sphere, tex256):
    """Psf(bands=None) is today's frame; bands=(3.5, 4.5, 5.5) equals the mirror's chain from the same raw frame (band convolution, the oracle's
    envelope, the fold); without the envelope the fold is the coherent sum; a downshift alone differs from the plain frame only below row n_ax;
    with noise= the band images carry noise_mirror's draws under the id rule (frame_id * n + i) * B + b"""
    cfg, sd = sphere
    tr = mcrt.Transducer(48, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    plain = mcrt.Simulator(sd, tr, n_samples=16, texture=tex256, psf=mcrt.Psf(freq=tr.frequency, bands=None))
    try:
        raw = plain.frame(0, convolve=False)
        got = plain.frame(0)
        assert not plain.psf.has_bands and plain._band_buf.dev is None
        ic.assert_same_bits(got, orc.convolve(raw, plain.psf.axial_kernel, plain.psf.lateral_kernel), "no bands")
        plain._run(0)
        plain_env = plain.ctx.d2h(plain.rf_dev, (plain.E, plain.R)).T
        R, E, row_mm = plain.R, plain.E, plain.row_mm
    finally:
        plain.close()

    psf = mcrt.Psf(freq=tr.frequency, bands=(3.5, 4.5, 5.5))
    assert psf.has_bands and psf.bands.n_bands == 3 and psf.axial_rows(R, row_mm).shape == (3, R, 7) and psf.axial_rows(R, row_mm) is psf.axial_rows(R, row_mm)
    sim = mcrt.Simulator(sd, tr, n_samples=16, texture=tex256, psf=psf)
    try:
        assert np.array_equal(sim.frame(0, convolve=False).view(np.uint32), raw.view(np.uint32))
        imgs, want = _chain(orc, raw, psf, R, row_mm)
        sim._run(0)
        ic.assert_same_bits(sim.ctx.d2h(sim.rf_dev, (E, R)).T, want, "three bands")
        assert not np.array_equal(want.view(np.uint32), plain_env.view(np.uint32))
        ic.assert_same_bits(sim.frame(0), em.fold(imgs[None], psf.band_weights(R, row_mm))[0].T, "the coherent sum")
        img = sim.bmode(0, dynamic_range_db=50.0)
        assert img.shape == (400, 500) and img.max() > 200
    finally:
        sim.close()

    shifted = mcrt.Simulator(sd, tr, n_samples=16, texture=tex256, psf=mcrt.Psf(freq=tr.frequency, downshift_mhz_per_mm=0.02, min_mhz=2.0))
    try:
        assert shifted.psf.has_bands and shifted.psf.bands.n_bands == 1
        down = shifted.frame(0)
        n_ax = 7
        ic.assert_same_bits(down[:n_ax], got[:n_ax], "the rows above the window")
        ic.assert_same_bits(down[R - n_ax:], got[R - n_ax:], "the rows past the window")
        differ = (down[n_ax:R - n_ax].view(np.uint32) != got[n_ax:R - n_ax].view(np.uint32)).any(axis=1)
        assert differ.any()                                 # from row n_ax down the pulse is another one (rows without an echo stay 0 in both)
    finally:
        shifted.close()

    noisy = mcrt.Simulator(sd, tr, n_samples=16, texture=tex256, psf=psf, noise=dict(snr_db=30.0, seed=77))
    try:
        fid, opts = 2, dict(snr_db=30.0, seed=77)
        raw2 = _raw_of(noisy, fid)
        noisy.convolve()
        clean = noisy.ctx.d2h(noisy._band_buf.dev, (3, E, R))
        noisy.add_noise(fid)
        want_bands, _ = nm.noise(clean[None], (fid * 1 + 0) * 3, opts)          # one receiver, one peak; image 0's band b has the id (fid * 1 + 0) * 3 + b
        ic.assert_same_bits(noisy.ctx.d2h(noisy._band_buf.dev, (3, E, R)), want_bands[0], "noise on the band images")
        _, want = _chain(orc, raw2, psf, R, row_mm, noise=lambda x: nm.noise(x[None], fid * 3, opts)[0][0])
        noisy._run(fid)
        ic.assert_same_bits(noisy.ctx.d2h(noisy.rf_dev, (E, R)).T, want, "noisy bands")
    finally:
        noisy.close()


def _raw_of(sim, frame_id):
    """the traced frame [R][E] before every image stage"""
    sim.trace(frame_id)
    return sim.ctx.d2h(sim.rf_dev, (sim.E, sim.R)).T.copy()


def test_simulator_with_compound(mcrt, sphere, tex256):
    """bands combine with compound=: the stack keeps its shape, and the picture differs from the plain psf's"""
    cfg, sd = sphere
    tr = mcrt.Transducer(48, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    pics = []
    for bands in (None, (3.5, 4.5, 5.5)):
        sim = mcrt.Simulator(sd, tr, n_samples=8, texture=tex256, psf=mcrt.Psf(freq=tr.frequency, bands=bands), compound=(-0.1, 0.0, 0.1))
        try:
            pics.append(sim.compound_image(0, out_rows=100, out_cols=120))
            assert sim._stack == (sim.views_dev, 3)
            assert (sim._band_buf.nbytes == 3 * 3 * sim.E * sim.R * 4) if bands else sim._band_buf.dev is None
        finally:
            sim.close()
    assert pics[0].shape == pics[1].shape == (100, 120) and np.isfinite(pics[1]).all() and pics[1].max() > 0
    assert not np.array_equal(pics[0], pics[1])


def _build_driver(tmp_path):
    pkg = os.path.join(ROOT, "mcray-tracing_amd")
    exe = str(tmp_path / "bands_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(pkg, "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "bands_driver.cpp"), "-L", pkg, "-lmcrt_hip", "-Wl,-rpath," + pkg])
    return exe


@pytest.mark.parametrize("bands,shift,floor,var_x", [((3.5, 4.5, 5.5), 0.0, 0.0, 0.05), ((5.0, 3.0), 0.02, 2.0, 0.2), ((4.5,), 0.03, 1.0, 0.05), ((), 0.0, 0.0, 0.05)])
def test_host_shim(mcrt, ctx, dev, tmp_path, bands, shift, floor, var_x):
    """the shim driver's images -- before, convolve + envelope, convolve + fold_bands, convolve + add_noise + envelope -- against the Python path"""
    exe = _build_driver(tmp_path)
    out = tmp_path / "bands.bin"
    r = subprocess.run([exe, str(out), str(shift), str(floor), str(var_x)] + [str(f) for f in bands], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    E, R, B = 64, 465, len(bands)
    imgs = np.fromfile(str(out), f32).reshape(4, R, E)
    before = np.ascontiguousarray(imgs[0].T)
    assert np.count_nonzero(before) > 1000
    psf = mcrt.Psf(bands=dict(band_mhz=bands, weights=tuple(range(1, B + 1)), var_x=var_x) if B else None, downshift_mhz_per_mm=shift, min_mhz=floor)
    nopts = dict(snr_db=30.0, seed=77)
    p = dev.upload(before)
    if not B:
        ctx.convolve(p, E, R, psf.axial_kernel, psf.lateral_kernel)
        coherent = ctx.d2h(p, (E, R))
        ctx.envelope(p, E, R)
        ic.assert_same_bits(imgs[1].T, ctx.d2h(p, (E, R)), "plain: envelope")
        ic.assert_same_bits(imgs[2].T, coherent, "plain: fold_bands does nothing")
        ctx.h2d(p, coherent)
        ctx.noise_frames(p, 1, 1, E, R, **nopts)
        ctx.envelope(p, E, R)
        ic.assert_same_bits(imgs[3].T, ctx.d2h(p, (E, R)), "plain: noise")
        return
    ax, w = psf.axial_rows(R, 0.322), psf.band_weights(R, 0.322)
    q, o = dev(B * E * R * 4), dev(E * R * 4)

    def chain(envelope, noise):
        ctx.convolve_bands_frames(p, 1, E, R, ax, q, lateral=psf.lateral_kernel)
        if noise:
            ctx.noise_frames(q, 1, B, E, R, first_image_id=0, **nopts)
        if envelope:
            ctx.envelope_frames(q, B, E, R)
        ctx.band_fold_frames(q, 1, B, E, R, w, o)
        return ctx.d2h(o, (E, R))

    ic.assert_same_bits(imgs[1].T, chain(True, False), "shim vs python: compounded")
    ic.assert_same_bits(imgs[2].T, chain(False, False), "shim vs python: coherent")
    ic.assert_same_bits(imgs[3].T, chain(True, True), "shim vs python: noisy")
    want = em.fold(bm.convolve_bands(before, ax, lateral=psf.lateral_kernel)[None], w)[0]
    ic.assert_same_bits(imgs[2].T, want, "shim vs mirror: coherent")
    assert not np.array_equal(imgs[1], imgs[2]) and not np.array_equal(imgs[1], imgs[3])


def test_cli_options(mcrt, tmp_path):
    exe = os.path.join(ROOT, "mcray-tracing_amd", "mattausch_hip")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "mcray-tracing_amd"), "mattausch_hip"])
    cfg, meshes = mcrt.synth.sphere_scene(3)
    cfg["workingDirectory"] = str(tmp_path) + "/"
    for f, (V, F) in meshes.items():
        mcrt.scene_io.save_obj(str(tmp_path / f), V, F)
    (tmp_path / "sphere.scene").write_text(json.dumps(cfg))
    scene = str(tmp_path / "sphere.scene")

    def run(name, *opts):
        r = subprocess.run([exe, scene, "2", "5", str(tmp_path / (name + ".pgm")), str(tmp_path / (name + ".bin"))] + list(opts),
                           capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout + r.stderr
        return (tmp_path / (name + ".pgm")).read_bytes(), (tmp_path / (name + ".bin")).read_bytes()

    plain = run("plain")
    assert run("one", "--freq-compound", "1") == plain                    # one band is the plain run, byte for byte
    three = run("three", "--freq-compound", "3", "--freq-span-mhz", "2")
    assert len(three[0]) == len(plain[0]) and three[0] != plain[0] and three[1] != plain[1]
    down = run("down", "--downshift-mhz-per-mm", "0.02", "--downshift-min-mhz", "2")
    assert down[1] != plain[1] and down[1] != three[1]
    for bad, word in ((["--freq-compound", "9"], "1..8"), (["--freq-compound", "0"], "1..8"), (["--freq-span-mhz", "2"], "--freq-compound"),
                      (["--downshift-min-mhz", "2"], "--downshift-mhz-per-mm"), (["--downshift-mhz-per-mm", "-1"], "downshift")):
        r = subprocess.run([exe, scene, "1", "5"] + bad, capture_output=True, text=True, timeout=240)
        assert r.returncode == 1 and word in r.stdout, (bad, r.stdout)
