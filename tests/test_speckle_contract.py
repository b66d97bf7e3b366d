"""Speckle reduction without a GPU (include/mcrt.h: mcrt_speckle_opts, mcrt_default_speckle_opts, mcrt_speckle_tables, mcrt_speckle_frames):
the struct and its defaults, the host tables against their formulas in numpy double, every refusal that needs no device, and the properties
of the numpy mirror (tests/speckle_mirror.py) that hold tests/test_gpu_speckle.py honest -- conservation, the convex combination, the constant
frame, exact power-of-two scaling, the degenerate patches -- and that the filter does what it is for."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest

import speckle_mirror as sm

f32 = np.float32
INVALID, LIMIT = -1, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mcray-tracing_amd")


# ------------------------------------------------------------------ struct, defaults, header
def test_struct_defaults_and_header(mcrt):
    O = mcrt.SpeckleOpts
    assert C.sizeof(O) == 16 and [getattr(O, n).offset for n in ("n_iter", "q0", "rho", "lambda_")] == [0, 4, 8, 12]
    L = mcrt.load_library()
    o = O()
    C.memset(C.byref(o), 0xA5, 16)
    assert L.mcrt_default_speckle_opts(C.byref(o)) == 0
    assert (o.n_iter, o.q0, o.rho, o.lambda_) == (20, float(f32(0.5227232)), float(f32(1.0 / 6.0)), 0.5)
    assert abs(o.q0 - np.sqrt(4.0 / np.pi - 1.0)) < 3e-8                     # the Rayleigh amplitude's coefficient of variation
    assert sm.DEFAULTS == dict(n_iter=o.n_iter, q0=o.q0, rho=o.rho, lambda_=o.lambda_)
    assert L.mcrt_default_speckle_opts(None) == INVALID and b"null" in L.mcrt_last_error()
    d = mcrt.speckle_opts_struct()
    assert (d.n_iter, d.q0, d.rho, d.lambda_) == (o.n_iter, o.q0, o.rho, o.lambda_)
    e = mcrt.speckle_opts_struct(n_iter=3, q0=0.25, rho=0.0, **{"lambda": 1.0})
    assert (e.n_iter, e.q0, e.rho, e.lambda_) == (3, 0.25, 0.0, 1.0)
    with pytest.raises(TypeError):
        mcrt.speckle_opts_struct(iterations=3)
    src = open(os.path.join(ROOT, "include", "mcrt.h")).read()
    block = src[src.index("#define MCRT_VERSION"):src.index("typedef enum")]
    added = block[block.index("mcrt_speckle_opts"):]
    for name in ("mcrt_speckle_opts", "mcrt_default_speckle_opts", "mcrt_speckle_tables", "mcrt_speckle_frames", "additive"):
        assert name in added, name
    for name in ("mcrt_default_speckle_opts", "mcrt_speckle_tables", "mcrt_speckle_frames"):
        assert re.search(r"\bint " + name + r"\(", src) and hasattr(L, name), name
    # the call without a context is refused before anything else is looked at
    assert L.mcrt_speckle_frames(None, None, 1, 1, 1, None, None) == INVALID and b"null context" in L.mcrt_last_error()


# ------------------------------------------------------------------ the tables
def _ulps(got, want64):
    return np.abs(got.astype(np.float64) - want64) / np.spacing(np.abs(want64).astype(f32)).astype(np.float64)


@pytest.mark.parametrize("opts", [dict(), dict(n_iter=256), dict(n_iter=1), dict(n_iter=64, q0=1.0, rho=0.0), dict(n_iter=40, q0=0.3, rho=0.5, lambda_=1.0),
                                  dict(n_iter=17, q0=3.0, rho=0.01, lambda_=0.1)])
def test_tables_match_their_formulas(mcrt, opts):
    """q0sq, kq and lam4 against numpy's evaluation of the same double formulas, each float within 1 ulp: two libms' exp may differ in the
    last place of the double, and a double that lies next to a float rounding boundary then rounds to the neighbouring float"""
    o = mcrt.speckle_opts_struct(**opts)
    q0sq, kq, lam4 = mcrt.host_speckle_tables(o)
    assert q0sq.shape == kq.shape == (o.n_iter,) and q0sq.dtype == kq.dtype == f32
    q = np.float64(o.q0) * np.exp(-np.float64(o.rho) * np.arange(o.n_iter, dtype=np.float64))
    assert _ulps(q0sq, q * q).max() <= 1.0 and _ulps(kq, 1.0 / (q * q * (1.0 + q * q))).max() <= 1.0
    assert lam4 == f32(0.25 * np.float64(o.lambda_))                                   # (no libm in it: exact)
    m = sm.tables(o.n_iter, o.q0, o.rho, o.lambda_)
    assert _ulps(q0sq, m[0].astype(np.float64)).max() <= 1.0 and _ulps(kq, m[1].astype(np.float64)).max() <= 1.0 and lam4 == m[2]


def test_tables_n_iter_zero(mcrt):
    L = mcrt.load_library()
    o = mcrt.speckle_opts_struct(n_iter=0)
    lam4 = np.full(1, 7.0, f32)
    assert L.mcrt_speckle_tables(C.byref(o), None, None, lam4.ctypes.data_as(C.c_void_p)) == 0 and lam4[0] == f32(0.125)
    q0sq, kq, l4 = mcrt.host_speckle_tables(n_iter=0)
    assert q0sq.size == 0 and kq.size == 0 and l4 == f32(0.125)
    x = np.array([[np.nan, -1.0], [-0.0, np.inf]], f32)
    assert np.array_equal(sm.srad(x, q0sq, kq, l4).view(np.uint32), x.view(np.uint32))      # n_iter = 0: the input's bits


REFUSED = [(dict(n_iter=257), LIMIT, b"n_iter"), (dict(n_iter=0xffffffff), LIMIT, b"n_iter"),
           (dict(q0=0.0), INVALID, b"q0"), (dict(q0=-0.5), INVALID, b"q0"), (dict(q0=np.nan), INVALID, b"q0"), (dict(q0=np.inf), INVALID, b"q0"),
           (dict(rho=-0.1), INVALID, b"rho"), (dict(rho=np.nan), INVALID, b"rho"), (dict(rho=np.inf), INVALID, b"rho"),
           (dict(lambda_=0.0), INVALID, b"lambda"), (dict(lambda_=-0.5), INVALID, b"lambda"), (dict(lambda_=1.0001), INVALID, b"lambda"), (dict(lambda_=np.nan), INVALID, b"lambda"),
           (dict(lambda_=1e-45), INVALID, b"lambda"),                      # 0.25 * lambda rounds to 0
           (dict(n_iter=256, rho=1.0), INVALID, b"iteration"),             # q_t has decayed to nothing: q0sq[t] = 0, kq[t] = inf
           (dict(n_iter=2, q0=1e-30), INVALID, b"iteration"),              # q_t^2 is no float above 0
           (dict(n_iter=2, q0=3e19), INVALID, b"iteration")]               # q_t^2 overflows


@pytest.mark.parametrize("case", range(len(REFUSED)))
def test_tables_refuse_and_write_nothing(mcrt, case):
    opts, code, word = REFUSED[case]
    L = mcrt.load_library()
    o = mcrt.speckle_opts_struct(**opts)
    q0sq = np.full(256, 7.0, f32); kq = np.full(256, 7.0, f32); lam4 = np.full(1, 7.0, f32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.mcrt_speckle_tables(C.byref(o), p(q0sq), p(kq), p(lam4)) == code, opts
    assert word in L.mcrt_last_error(), (opts, L.mcrt_last_error())
    assert (q0sq == 7.0).all() and (kq == 7.0).all() and lam4[0] == 7.0


def test_tables_refuse_null_pointers(mcrt):
    L = mcrt.load_library()
    o = mcrt.speckle_opts_struct(n_iter=2)
    buf = np.zeros(4, f32); p = buf.ctypes.data_as(C.c_void_p)
    for args in ((None, p, p, p), (C.byref(o), None, p, p), (C.byref(o), p, None, p), (C.byref(o), p, p, None)):
        assert L.mcrt_speckle_tables(*args) == INVALID and b"null" in L.mcrt_last_error()


# ------------------------------------------------------------------ the mirror's properties
def _speckle(shape, seed):
    return np.random.default_rng(seed).rayleigh(1.0, shape).astype(f32)


@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1), (2, 2), (37, 41), (3, 64, 48)])
def test_mirror_keeps_the_sum_and_the_range(shape):
    """the flux across every interior edge is antisymmetric and the clamped border has none: the frame's sum is kept up to rounding; with
    lambda <= 1 and c in [0,1] every X' is a convex combination of X and its neighbours"""
    x = _speckle(shape, 3) * f32(2.5)
    for lam in (0.5, 1.0):
        y = sm.srad(x, *sm.tables(20, lambda_=lam))
        s0, s1 = x.astype(np.float64).sum((-2, -1)), y.astype(np.float64).sum((-2, -1))
        assert (np.abs(s1 - s0) <= 1e-5 * s0).all(), (shape, lam, s0, s1)
        assert y.min() >= x.min() and y.max() <= x.max() and np.isfinite(y).all()


def test_mirror_constant_frame_keeps_its_bits():
    for v in (0.0, 1.0, 0.1, 3.3e-5, 1e25, 1e-30):
        x = np.full((7, 9), v, f32)
        assert np.array_equal(sm.srad(x, *sm.tables()).view(np.uint32), x.view(np.uint32)), v


def test_mirror_scaling_by_a_power_of_two_is_exact():
    x = _speckle((33, 29), 5)
    t = sm.tables()
    y = sm.srad(x, *t)
    for k in (f32(1024.0), f32(1.0 / 1024.0)):
        assert np.array_equal(sm.srad(x * k, *t).view(np.uint32), (y * k).view(np.uint32)), k


def test_mirror_step_zero_and_signs():
    """X = |v| where v is finite, else 0: a NaN scan-line is no echo and does not spread"""
    x = _speckle((12, 10), 7)
    z = x.copy(); z[5, :] = np.nan; z[0, 0] = np.inf; z[11, 9] = -np.inf
    w = x.copy(); w[5, :] = 0.0; w[0, 0] = 0.0; w[11, 9] = 0.0
    t = sm.tables(5)
    y = sm.srad(z, *t)
    assert np.isfinite(y).all() and np.array_equal(y.view(np.uint32), sm.srad(w, *t).view(np.uint32))
    assert np.array_equal(sm.srad(-x, *t).view(np.uint32), sm.srad(x, *t).view(np.uint32))


def test_mirror_degenerate_patches():
    """a 5 x 7 zero frame with one spike: 0/0 in the flat zero patch (c = 0, moot), x/0 beside the spike (q2 = inf, c = 0) -- the frame stays
    finite and the spike is an edge the filter keeps, within 5 % after 3 iterations; a frame of 1e25 (m*m overflows) stays finite"""
    x = np.zeros((5, 7), f32); x[2, 3] = 10.0
    y = sm.srad(x, *sm.tables(3))
    assert np.isfinite(y).all() and abs(float(y[2, 3]) - 10.0) <= 0.5, y[2, 3]
    big = np.full((6, 5), 1e25, f32); big[2, 2] = 3e25; big[4, 1] = 0.0
    assert np.isfinite(sm.srad(big, *sm.tables())).all()


def test_mirror_does_its_job():
    """fully developed speckle over a disc four times as bright as its background, with a shadow: at the defaults the background's
    coefficient of variation falls below 0.6 of the input's (prototype: 0.617 -> 0.313), the disc's contrast to the background moves by
    less than 2 % (0.1 %), and the shadow's columns 0..4 stay below 1 % of the background mean (0.5 %): conditions, not tolerances"""
    i, j = np.mgrid[0:96, 0:80]
    mean = np.where((i - 48) ** 2 + (j - 40) ** 2 <= 20 ** 2, 4.0, 1.0)
    x = (np.random.default_rng(1).rayleigh(1.0, (96, 80)) * mean).astype(f32)
    x[:, 0:6] = 0.0
    y = sm.srad(x, *sm.tables())
    bg, disc = (slice(4, 30), slice(40, 76)), (slice(40, 56), slice(32, 48))
    cv = lambda a: float(a.astype(np.float64).std() / a.astype(np.float64).mean())
    mu = lambda a: float(a.astype(np.float64).mean())
    print("cv %.4f -> %.4f, contrast %.4f -> %.4f, shadow %.5f of the background" % (cv(x[bg]), cv(y[bg]), mu(x[disc]) / mu(x[bg]), mu(y[disc]) / mu(y[bg]),
                                                                                   y[:, 0:5].max() / mu(y[bg])))
    assert cv(y[bg]) < 0.6 * cv(x[bg])
    assert abs(mu(y[disc]) / mu(y[bg]) / (mu(x[disc]) / mu(x[bg])) - 1.0) < 0.02
    assert y[:, 0:5].max() < 0.01 * mu(y[bg])


# ------------------------------------------------------------------ the kernels' resources
def test_srad_kernels_use_no_scratch_and_leave_two_workgroups_per_cu():
    """the compiler's own report for k_srad<2> and <4>: nothing spilled, no scratch, and an LDS block of which at least two fit a CU's
    160 KB (a gfx950 workgroup may have 64 KB)"""
    out = subprocess.run(["make", "-C", PKG, "resources"], capture_output=True, text=True).stderr
    blocks = [b for b in out.split("Function Name: ") if b.startswith("_ZN4mcrt6k_sradILi")]
    assert len(blocks) == 2, out[-2000:]
    for b in blocks:
        val = lambda key: int(re.search(key + r": (\d+)", b).group(1))
        assert val("VGPRs Spill") == 0 and val("SGPRs Spill") == 0 and val(r"ScratchSize \[bytes/lane\]") == 0, b[:900]
        assert 2 * val(r"LDS Size \[bytes/block\]") <= 160 * 1024 and val(r"Occupancy \[waves/SIMD\]") >= 4, b[:900]
