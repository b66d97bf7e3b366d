"""The sonogram on the MI355X: mcrt_sonogram_frames (k_sonogram_peak, k_sonogram) against the numpy mirror (tests/spectral_mirror.py) --
the bytes within one grey level (the device's log10f is not correctly rounded), the peaks exact, row 0 the highest velocity, NaN and
infinite powers black, a given ref against the automatic one, behind sentinels and at every alignment; the refusals."""
import ctypes as C
import numpy as np
import pytest

import spectral_mirror as sm

pytestmark = pytest.mark.gpu

f32 = np.float32
INVALID, LIMIT = -1, -5
TAIL = 16
SHAPES = [(1, 1, 32), (3, 7, 128), (2, 65, 512)]


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
        p = ctx.alloc(arr.nbytes + skew)
        bufs.append(p)
        ctx.h2d(p + skew, arr)
        return p + skew

    yield upload
    for p in bufs:
        ctx.free(p)


def spectra(n_gates, n_cols, N, seed=0, special=True):
    """powers over 90 dB, each gate at its own level, with zeros, NaN, infinities and negative values sprinkled in"""
    rng = np.random.default_rng(seed + N)
    p = (10.0 ** rng.uniform(-9.0, 0.0, (n_gates, n_cols, N)) * (10.0 ** np.arange(n_gates))[:, None, None]).astype(f32)
    if special:
        at = rng.choice(p.size, size=max(p.size // 9, 4), replace=False)
        p.reshape(-1)[at] = rng.choice(np.array([0.0, -0.0, np.nan, np.inf, -np.inf, -3.0, 1e-42], f32), size=at.size)
    return p


def run(ctx, dev, p, with_peak=True, skew=0, **opts):
    n_gates, n_cols, N = p.shape
    p_in = dev(p, skew)
    p_out = dev(np.full(p.size + TAIL, 0xA5, np.uint8), skew)
    p_peak = dev(np.full(n_gates + TAIL, f32(-77.25)), skew) if with_peak else None
    ctx.sonogram_frames(p_in, n_gates, n_cols, N, p_out, peak_dev=p_peak, **opts)
    flat = ctx.d2h(p_out, (p.size + TAIL,), np.uint8)
    assert (flat[p.size:] == 0xA5).all(), "the sentinel behind out_dev was overwritten"
    peak = None
    if with_peak:
        pk = ctx.d2h(p_peak, (n_gates + TAIL,))
        assert (pk[n_gates:] == f32(-77.25)).all(), "the sentinel behind peak_dev was overwritten"
        peak = pk[:n_gates]
    assert np.array_equal(ctx.d2h(p_in, p.shape).view(np.uint32), p.view(np.uint32)), "power_dev is read only"
    return flat[:p.size].reshape(n_gates, N, n_cols), peak


@pytest.mark.parametrize("skew", [0, 4, 8])
@pytest.mark.parametrize("n_gates,n_cols,N", SHAPES)
def test_bytes_and_peaks_match_the_mirror(ctx, dev, n_gates, n_cols, N, skew):
    p = spectra(n_gates, n_cols, N, seed=skew)
    for opts in (dict(), dict(dynamic_range_db=60.0, gain_db=-7.5), dict(dynamic_range_db=25.0, gain_db=6.0)):
        got, peak = run(ctx, dev, p, skew=skew, **opts)
        want, want_peak = sm.sonogram(p, **opts)
        assert np.array_equal(peak.view(np.uint32), want_peak.view(np.uint32)), "the peaks are exact"
        d = np.abs(got.astype(np.int32) - want.astype(np.int32))
        assert d.max() <= 1, "bytes differ by %d levels (%s)" % (d.max(), opts)
        bad = ~(np.isfinite(p) & (p > 0))
        assert not got.transpose(0, 2, 1)[:, :, ::-1][bad].any(), "NaN, infinite, zero and negative powers are black"
        without, _ = run(ctx, dev, p, with_peak=False, skew=skew, **opts)
        assert np.array_equal(without, got), "the bytes do not depend on whether the peaks are asked for"


def test_row_0_is_the_highest_velocity(ctx, dev):
    """one bright bin per column, climbing with time: its picture row is N - 1 - bin, and everything else is black at 40 dB"""
    n_cols, N = 20, 32
    p = np.full((1, n_cols, N), f32(1e-9)); bins = (np.arange(n_cols) * 3 + 1) % N
    p[0, np.arange(n_cols), bins] = 1.0
    got, peak = run(ctx, dev, p)
    assert peak[0] == 1.0
    assert (got[0, N - 1 - bins, np.arange(n_cols)] == 255).all() and got.sum() == 255 * n_cols


def test_a_given_ref_against_the_automatic_one(ctx, dev):
    """ref = the gate's own peak gives the automatic picture; a ref 20 dB above it is the automatic picture under a gain of -20 dB to
    within a level; the peaks are reported whatever ref is"""
    p = spectra(1, 33, 64, special=False)
    auto, peak = run(ctx, dev, p)
    same, peak2 = run(ctx, dev, p, ref=float(peak[0]))
    assert np.array_equal(auto, same) and peak2[0] == peak[0] == p.max()
    dim, _ = run(ctx, dev, p, ref=float(peak[0]) * 100.0)
    low, _ = run(ctx, dev, p, gain_db=-20.0)
    assert np.abs(dim.astype(np.int32) - low.astype(np.int32)).max() <= 1 and dim.sum() < auto.sum()
    want, _ = sm.sonogram(p, ref=float(peak[0]) * 100.0)
    assert np.abs(dim.astype(np.int32) - want.astype(np.int32)).max() <= 1


def test_a_gate_without_a_finite_power_is_black(ctx, dev):
    p = np.zeros((2, 5, 32), f32); p[0] = np.nan; p[1, :, ::2] = np.inf; p[1, :, 1::2] = -1.0
    got, peak = run(ctx, dev, p)
    assert not got.any() and not peak.view(np.uint32).any()


def test_refusals(mcrt, ctx, dev):
    L = mcrt.load_library()
    NG, NC, N = 2, 9, 32
    p = spectra(NG, NC, N)
    n = p.size
    o = mcrt.sonogram_opts_struct()

    def call(power=0, ng=NG, nc=NC, nfft=N, opts=o, peak=n, out=n + NG, null_ctx=False):
        big = dev(np.concatenate([p.reshape(-1), np.full(NG + n // 4 + 4, f32(-77.25))]))      # floats: power, then room for the peaks and the bytes
        at = lambda floats: None if floats is None else C.c_void_p(big + 4 * floats)
        rc = L.mcrt_sonogram_frames(None if null_ctx else ctx.h, at(power), ng, nc, nfft, None if opts is None else C.byref(opts), at(peak), at(out))
        got = ctx.d2h(big, (n + NG + n // 4 + 4,))
        assert np.array_equal(got[:n].view(np.uint32), p.reshape(-1).view(np.uint32)) and (got[n:] == f32(-77.25)).all()
        return rc

    assert call(null_ctx=True) == INVALID and call(power=None) == INVALID and call(opts=None) == INVALID and call(out=None) == INVALID
    assert call(ng=0) == INVALID and call(nc=0) == INVALID
    for nfft in (0, 16, 48, 1024):
        assert call(nfft=nfft) == INVALID
    for kw in (dict(dynamic_range_db=0.0), dict(dynamic_range_db=-40.0), dict(dynamic_range_db=float("nan")), dict(gain_db=float("inf")), dict(ref=float("nan"))):
        assert call(opts=mcrt.sonogram_opts_struct(**kw)) == INVALID, kw
    assert call(ng=65536) == LIMIT and call(ng=16384, nc=16384) == LIMIT
    assert call(out=n - 1) == INVALID and call(peak=0) == INVALID and call(peak=n + NG) == INVALID      # overlaps
