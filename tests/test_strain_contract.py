"""Strain elastography without a GPU (include/mcrt.h: mcrt_strain_opts, mcrt_default_strain_opts, mcrt_strain_table, mcrt_strain_draws,
mcrt_strain_map, mcrt_elastogram_opts, mcrt_default_elastogram_opts): the host helpers against tests/strain_mirror.py bit for bit, the
structs and their defaults, every refusal that needs no device, and the properties of the model on the float32 mirror: the zero-strain
identity, what the tracker recovers of a uniform medium and of a stiff inclusion, and its correlation coefficient."""
import ctypes as C
import numpy as np
import pytest

import detect_mirror as dm
import strain_mirror as sm

f32 = np.float32
INVALID, LIMIT = -1, -5
CARRIER = 0.3475


# ------------------------------------------------------------------ structs and defaults
def test_structs_and_defaults(mcrt):
    L = mcrt.load_library()
    o = mcrt.StrainOpts()
    assert C.sizeof(o) == 20
    assert [getattr(mcrt.StrainOpts, n).offset for n in ("window_rows", "search_rows", "lsq_rows", "sigma", "seed")] == list(range(0, 20, 4))
    assert L.mcrt_default_strain_opts(C.byref(o)) == 0
    assert (o.window_rows, o.search_rows, o.lsq_rows, o.sigma, o.seed) == (16, 8, 12, 0.0, 0x5354524E)
    assert L.mcrt_default_strain_opts(None) == INVALID
    e = mcrt.ElastogramOpts()
    assert C.sizeof(e) == 16 and [getattr(mcrt.ElastogramOpts, n).offset for n in ("ref_strain", "rho_min", "grey_min", "alpha")] == [0, 4, 8, 12]
    assert L.mcrt_default_elastogram_opts(C.byref(e)) == 0
    assert (e.ref_strain, e.rho_min, e.grey_min, e.alpha) == (float(f32(0.01)), float(f32(0.7)), 0, 160)
    assert L.mcrt_default_elastogram_opts(None) == INVALID
    o = mcrt.strain_opts_struct(window_rows=32, search_rows=0, lsq_rows=1, sigma=0.5, seed=9)
    assert (o.window_rows, o.search_rows, o.lsq_rows, o.sigma, o.seed) == (32, 0, 1, 0.5, 9)
    e = mcrt.elastogram_opts_struct(ref_strain=-0.02, rho_min=0.5, grey_min=3, alpha=256)
    assert (e.ref_strain, e.rho_min, e.grey_min, e.alpha) == (float(f32(-0.02)), 0.5, 3, 256)


# ------------------------------------------------------------------ the strain table
def test_table_equals_the_mirrors(mcrt):
    mod = [1.0, 5.0, 0.0, 0.32, 1e30, 3.0, 7.7]
    for applied, ref in ((0.01, 1.0), (-0.01, 1.0), (0.005, 1.5), (0.003, 3.0), (0.0, 1.0)):
        got = mcrt.host_strain_table(mod, applied, ref)
        assert got.dtype == np.int32 and np.array_equal(got, sm.strain_table(mod, applied, ref)), (applied, ref)
    eps = mcrt.host_strain_table([1.0, 5.0, 0.0], 0.01, 1.0)
    assert list(eps) == [167772, 33554, 0]                               # 1 %, 0.2 %, rigid
    assert list(mcrt.host_strain_table([1.0, 0.32], 0.01, 1.0)) == [167772, 524288]       # 0.32: exactly the cap, 1/32
    assert list(mcrt.host_strain_table([1.0], -0.03125, 1.0)) == [-524288]


def test_table_refuses(mcrt):
    L = mcrt.load_library()
    mod = np.array([1.0, 5.0], np.float64)
    out = np.full(2, -7, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    call = lambda m=mod, n=2, applied=0.01, ref=1.0, o=out: L.mcrt_strain_table(None if m is None else p(m), n, applied, ref, None if o is None else p(o))
    assert call(m=None) == INVALID and call(o=None) == INVALID and call(n=0) == INVALID
    assert L.mcrt_strain_table(p(np.ones(255)), 255, 0.01, 1.0, p(np.zeros(255, np.int32))) == LIMIT
    for bad in (np.nan, np.inf, -np.inf):
        assert call(applied=bad) == INVALID and call(ref=bad) == INVALID
        assert call(m=np.array([1.0, bad])) == INVALID
    assert call(ref=0.0) == INVALID and call(ref=-1.0) == INVALID and call(m=np.array([1.0, -2.0])) == INVALID
    assert call(applied=0.04) == INVALID and call(m=np.array([1.0, 0.3199])) == INVALID and call(applied=-0.04) == INVALID      # above 1/32
    assert call(m=np.array([1.0, 1e-300])) == INVALID                    # (the quotient overflows every integer)
    assert (out == -7).all()
    assert call() == 0 and (out != -7).all()


# ------------------------------------------------------------------ the draws
@pytest.mark.parametrize("E,R", [(1, 1), (3, 65), (2, 2048)])
def test_draws_equal_the_mirrors(mcrt, E, R):
    for seed, image in ((0x5354524E, 0), (7, 0xFFFFFFFF)):
        got = mcrt.host_strain_draws(seed, image, E, R)
        assert got.shape == (E, R, 2) and np.array_equal(got, sm.draws(seed, image, E, R))


def test_draws_are_a_stream_of_their_own(mcrt):
    """counter word 2 differs from the noise stage's, flow's and spectral's: the same key gives other draws"""
    import flow_mirror as fm
    d = mcrt.host_strain_draws(5, 3, 4, 33)
    assert not np.array_equal(d, fm.draws(5, 3, 4, 33, 2)[0])
    assert not np.array_equal(d[0, 0], mcrt.host_spectral_draws(5, 3, 0, 0, 1)[0])
    assert sm.COUNTER not in (0x4E4F4953, 0x464C4F57, 0x53504543) and sm.COUNTER >= 16


def test_draws_refuse(mcrt):
    L = mcrt.load_library()
    d = np.full((2, 3, 2), -7, np.int32)
    p = d.ctypes.data_as(C.c_void_p)
    assert L.mcrt_strain_draws(1, 2, 2, 3, None) == INVALID and L.mcrt_strain_draws(1, 2, 0, 3, p) == INVALID and L.mcrt_strain_draws(1, 2, 2, 0, p) == INVALID
    assert L.mcrt_strain_draws(1, 2, 1, 2049, p) == LIMIT
    assert (d == -7).all()


# ------------------------------------------------------------------ the colour table
def test_map(mcrt):
    lut = mcrt.host_strain_map()
    assert lut.dtype == np.uint8 and np.array_equal(lut, sm.strain_map())
    assert tuple(lut[0]) == (0, 0, 255) and tuple(lut[128]) == (0, 255, 0) and tuple(lut[255]) == (254, 1, 0)      # stiff blue, green at the reference, soft red
    assert (lut[:129, 0] == 0).all() and (lut[129:, 2] == 0).all() and (np.diff(lut[128:, 0].astype(int)) > 0).all() and (np.diff(lut[:129, 2].astype(int)) <= 0).all()
    L = mcrt.load_library()
    buf = np.full((256, 3), 9, np.uint8)
    assert L.mcrt_strain_map(0, None) == INVALID and L.mcrt_strain_map(1, buf.ctypes.data_as(C.c_void_p)) == INVALID and (buf == 9).all()
    assert L.mcrt_colour_map(1, buf.ctypes.data_as(C.c_void_p)) == INVALID          # mcrt_colour_map keeps its one kind


# ------------------------------------------------------------------ the model, on the mirror
def speckle(mcrt, E, R, seed):
    """fully developed speckle: white scatterers under the reference's 7-tap axial pulse at 4.5 MHz, through the 31-tap Hilbert transformer"""
    ax = np.asarray(mcrt.host_psf()[0], np.float64).reshape(-1)
    x = np.random.default_rng(seed).standard_normal((E, R + len(ax) - 1))
    rf = np.stack([np.convolve(x[e], ax, mode="valid") for e in range(E)])[None].astype(f32)
    return dm.detect(rf)[1]


@pytest.fixture(scope="module")
def medium(mcrt):
    """8 scan-lines of 465 rows and what the defaults track of them: at zero strain, uniformly at 1 %, and around a 100-row inclusion five
    times as stiff; computed once"""
    E, R = 8, 465
    assert abs(mcrt.host_psf_carrier(4.5) - CARRIER) < 1e-12
    iq = speckle(mcrt, E, R, 1)
    eps = sm.strain_table([1.0, 5.0], 0.01, 1.0)
    uniform = np.zeros((1, E, R), np.uint8)
    lesion = uniform.copy(); lesion[..., 180:280] = 1
    out = dict(iq=iq, R=R)
    for name, tissue, table in (("zero", uniform, [0]), ("uniform", uniform, eps), ("lesion", lesion, eps)):
        c = sm.compress(iq, tissue, table, CARRIER)
        out[name] = dict(c, **sm.track(iq, c["post"], CARRIER))
    return out


def test_zero_strain_is_the_identity(medium):
    z = medium["zero"]
    assert np.array_equal(z["post"], medium["iq"])                        # as floats
    assert not z["truth_disp"].view(np.uint32).any() and not z["truth_strain"].view(np.uint32).any()
    assert (z["disp"] == 0.0).all() and (z["rho"] == 1.0).all() and (z["strain"] == 0.0).all()


def test_uniform_medium_reads_its_strain(medium):
    """the mean strain over rows 40 .. R - 40 within 5 % of the truth (a float64 prototype read 2.2 % low, this mirror 0.9 % low)"""
    u = medium["uniform"]
    R = medium["R"]
    truth = float(u["truth_strain"][0, 0, 0])
    assert abs(truth - 0.01) < 1e-7 and (u["truth_strain"] == u["truth_strain"][0, 0, 0]).all()
    assert np.array_equal(u["truth_disp"][0, 0], (np.arange(R, dtype=np.int64) * 167772).astype(np.int32).astype(f32) * f32(2.0 ** -24))
    mean = float(u["strain"][..., 40:R - 40].astype(np.float64).mean())
    err = np.abs(u["disp"].astype(np.float64) - u["truth_disp"])[..., 40:R - 40]
    print("uniform 1 %%: mean strain %.6f (truth %.6f), displacement error median %.4f rows, 99th percentile %.4f" % (mean, truth, np.median(err), np.percentile(err, 99)))
    assert abs(mean - truth) <= 0.05 * truth


def test_inclusion_contrast(medium):
    """background 1 %, inclusion 0.2 %: the ratio of the mean strains between 4 and 6 (the prototype read 4.9).  The means are taken a
    search-and-slope window (20 rows) inside each region: the least-squares slope of 25 rows smears the step over its own length"""
    t = medium["lesion"]
    R = medium["R"]
    s = t["strain"].astype(np.float64)
    inside = s[..., 200:260].mean()
    outside = np.concatenate([s[..., 40:160].ravel(), s[..., 300:R - 40].ravel()]).mean()
    print("inclusion: mean strain inside %.6f, outside %.6f, ratio %.3f" % (inside, outside, outside / inside))
    assert 4.0 <= outside / inside <= 6.0
    assert (t["truth_strain"][..., 180:280] == f32(33554) * f32(2.0 ** -24)).all() and (t["truth_strain"][..., :180] == f32(167772) * f32(2.0 ** -24)).all()


def test_correlation_stays_high(medium):
    """rho >= 0.9 on 99 % of the interior samples at 1 % (the prototype's smallest was 0.93)"""
    R = medium["R"]
    for name in ("uniform", "lesion"):
        rho = medium[name]["rho"][..., 40:R - 40]
        print("%s: smallest rho %.4f, share >= 0.9: %.4f" % (name, rho.min(), (rho >= 0.9).mean()))
        assert (rho >= 0.9).mean() >= 0.99 and (rho <= 1.0 + 1e-6).all()


def test_decompression_is_negative(mcrt):
    """a negative applied strain reads as a negative strain of the same size.  The bound is three standard errors of the mean: the
    prototype's 0.0023 per sample, correlated over the 25 rows of the slope window, over 4 x 220 samples is 3.9e-4 -- 12 % of 1 % at 3 SE"""
    iq = speckle(mcrt, 4, 300, 2)
    tissue = np.zeros((1, 4, 300), np.uint8)
    c = sm.compress(iq, tissue, sm.strain_table([1.0], -0.01), CARRIER)
    t = sm.track(iq, c["post"], CARRIER)
    mean = float(t["strain"][..., 40:260].astype(np.float64).mean())
    assert (c["truth_disp"] <= 0).all() and abs(mean + 0.01) <= 0.12 * 0.01
