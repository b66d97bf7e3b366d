"""Spectral Doppler on the MI355X: mcrt_spectral_series_frames (k_gate_series) and mcrt_spectral_frames (k_spectrum<N>) against the numpy
mirror (tests/spectral_mirror.py) bit for bit -- at the shapes around a wavefront's 64 pulses, for every gate length class and FFT size,
with and without the static stack and the noise, on special values, with every output left out in turn, behind sentinels and at every
alignment; the refusals; and two properties read on the device itself: a gate where nothing moves has no power at all under mean
removal, and a rotor that steps by whole bins puts its power into one bin."""
import ctypes as C
import numpy as np
import pytest

import spectral_mirror as sm
import image_cases as ic

pytestmark = pytest.mark.gpu

f32 = np.float32
INVALID, LIMIT = -1, -5
SENTINEL = f32(-77.25)
V_NYQ = 333.3333333333333
TAIL = 8


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

    def upload(self, arr, skew=0):
        """arr on the device, `skew` bytes past a fresh allocation's start (allocations are at least 256-byte aligned)"""
        arr = np.ascontiguousarray(arr)
        p = self(arr.nbytes + skew) + skew
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


def images(F, E, R, seed=0):
    """(iq_static, iq_moving [F][E][R][2]): every family of image_cases' scan-lines in both components (noise, ramps, saws, subnormals,
    infinities, NaN, -0.0)"""
    st = np.stack([np.stack([ic.envelope_image(E, R, seed=seed + 5 * f + c) for c in range(2)], axis=-1) for f in range(F)])
    mv = np.stack([np.stack([ic.envelope_image(E, R, seed=seed + 5 * f + c + 2) for c in range(2)], axis=-1) for f in range(F)])
    return st.astype(f32), mv.astype(f32)


def gate_list(F, E, R, G, n_gates, rng):
    """n_gates gates: the first ends exactly at row R, the last two lie on the same rows"""
    g = [[F - 1, E - 1, R - G]]
    while len(g) < n_gates:
        g.append([int(rng.integers(F)), int(rng.integers(E)), int(rng.integers(R - G + 1))])
    if n_gates > 1:
        g[-1] = list(g[-2])
    return np.array(g, np.uint32)


def rate_table(n_gates, G, rng):
    """gate 0 stands still, gate 1 turns at +65536, gate 2 at -65536, the others (and the last row of each) mixed"""
    r = rng.integers(-65536, 65537, size=(n_gates, G)).astype(np.int32)
    for j, v in enumerate((0, 65536, -65536)[:n_gates]):
        r[j, :max(G - 1, 1)] = v
    return r


def phase_table(T, kind, rng):
    """Python ints [T].  "negative": speeds away from the probe, the phase falls below zero; "alias": speeds of 1.2 .. 1.9 v_nyq"""
    speed = {"negative": -rng.uniform(10.0, 300.0, T), "alias": rng.uniform(1.2, 1.9, T) * V_NYQ, "mixed": rng.uniform(-660.0, 660.0, T)}[kind]
    return sm.phase(V_NYQ, speed.astype(f32))


def run_series(ctx, dev, st, mv, gates, weight, rate, ph, sigma_from="opts", sigma=0.0, first_image_id=0, skew=0, **opts):
    """the call -> series [n_gates][T][2].  The output starts as a sentinel, has TAIL sentinel floats behind it that must survive, and starts
    `skew` bytes off a 256-byte boundary, as the inputs do; the inputs must come back unchanged"""
    F, E, R, _ = mv.shape
    n_out = 2 * len(gates) * len(ph)
    p_st = None if st is None else dev.upload(st, skew)
    p_mv = dev.upload(mv, skew)
    sig = np.broadcast_to(np.asarray(sigma, f32), (F,)).copy()
    p_sig = dev.upload(sig, skew) if sigma_from == "dev" else None
    p_out = dev.upload(np.full(n_out + TAIL, SENTINEL), skew)
    kw = dict(opts)
    if sigma_from == "opts":
        assert np.all(sig == sig[0])
        kw["sigma"] = float(sig[0])
    ctx.spectral_series_frames(p_st, p_mv, F, E, R, gates, weight, rate, np.array(ph, np.int64), p_out, first_image_id=first_image_id, sigma_dev=p_sig, **kw)
    flat = ctx.d2h(p_out, (n_out + TAIL,))
    assert (flat[n_out:] == SENTINEL).all(), "the sentinel behind series_dev was overwritten"
    for p, a, name in ((p_st, st, "iq_static_dev"), (p_mv, mv, "iq_moving_dev"), (p_sig, sig, "sigma_dev")):
        if p is not None:
            assert np.array_equal(ctx.d2h(p, a.shape).view(np.uint32), a.view(np.uint32)), name + " is read only"
    return flat[:n_out].reshape(len(gates), len(ph), 2)


SERIES_SHAPES = [(1, 1, 1, 1), (2, 3, 65, 1), (2, 3, 65, 3), (2, 3, 65, 64), (1, 2, 2048, 1), (1, 2, 2048, 3), (1, 2, 2048, 64)]


@pytest.mark.parametrize("T", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("F,E,R,G", SERIES_SHAPES)
def test_series_matches_the_mirror(ctx, dev, F, E, R, G, T):
    """every shape x gate length x series length; the number of gates, the static stack, the phase table and where sigma comes from
    rotate with the case"""
    i = SERIES_SHAPES.index((F, E, R, G)) + T
    rng = np.random.default_rng(i)
    n_gates = (1, 5)[i % 2]
    with_static = i % 3 != 0
    sigma_from, sigma = (("opts", 0.0), ("opts", 0.375), ("dev", [0.5, 0.0][:F] if F == 2 else [0.25]))[(i // 2) % 3]
    st, mv = images(F, E, R, seed=T)
    st = st if with_static else None
    gates = gate_list(F, E, R, G, n_gates, rng); rate = rate_table(n_gates, G, rng)
    weight = rng.uniform(0.25, 1.0, G).astype(f32)
    ph = phase_table(T, ("negative", "alias", "mixed")[i % 3], rng)
    what = "F=%d E=%d R=%d G=%d T=%d gates=%d static=%s sigma=%s from %s" % (F, E, R, G, T, n_gates, with_static, sigma, sigma_from)
    want = sm.series(st, mv, gates, weight, rate, ph, sigma=sigma, seed=11, first_image_id=5)
    got = run_series(ctx, dev, st, mv, gates, weight, rate, ph, sigma_from=sigma_from, sigma=sigma, first_image_id=5, seed=11)
    ic.assert_same_bits(got, want, what)


def clean_case(F=2, E=3, R=65, G=3, T=130, n_gates=5, seed=0):
    """finite images (no special values), so that a comparison covers every element's bits"""
    rng = np.random.default_rng(seed)
    st = rng.standard_normal((F, E, R, 2)).astype(f32) * f32(40.0); mv = rng.standard_normal((F, E, R, 2)).astype(f32)
    return st, mv, gate_list(F, E, R, G, n_gates, rng), rng.uniform(0.25, 1.0, G).astype(f32), rate_table(n_gates, G, rng), phase_table(T, "mixed", rng)


@pytest.mark.parametrize("skew", [4, 8])
def test_series_pointers_off_a_16_byte_boundary(ctx, dev, skew):
    st, mv, gates, weight, rate, ph = clean_case(seed=skew)
    want = sm.series(st, mv, gates, weight, rate, ph, sigma=[0.5, 0.25])
    got = run_series(ctx, dev, st, mv, gates, weight, rate, ph, sigma_from="dev", sigma=[0.5, 0.25], skew=skew)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_series_defaults_and_image_ids(ctx, dev):
    """the default seed; the image id of a gate is first_image_id + image, up to 2^32 - 1; the noise of G rows is one receiver's"""
    st, mv, gates, weight, rate, ph = clean_case(seed=1)
    got = run_series(ctx, dev, st, mv, gates, weight, rate, ph, sigma=0.5, first_image_id=0xFFFFFFFE)
    assert np.array_equal(got.view(np.uint32), sm.series(st, mv, gates, weight, rate, ph, sigma=0.5, first_image_id=0xFFFFFFFE).view(np.uint32))
    quiet = run_series(ctx, dev, st, mv, gates, weight, rate, ph, first_image_id=0xFFFFFFFE)
    assert not np.array_equal(got, quiet)


def test_series_tables_are_replaced_when_they_change(ctx, dev):
    """the host tables live in the context and are copied only when they differ: calls with other, smaller and larger tables read their own"""
    for seed, G, T, n_gates in ((0, 3, 130, 5), (1, 3, 130, 5), (2, 1, 64, 1), (3, 64, 200, 5), (0, 3, 130, 5)):
        st, mv, gates, weight, rate, ph = clean_case(G=G, T=T, n_gates=n_gates, seed=seed)
        got = run_series(ctx, dev, st, mv, gates, weight, rate, ph)
        assert np.array_equal(got.view(np.uint32), sm.series(st, mv, gates, weight, rate, ph).view(np.uint32)), (seed, G, T, n_gates)


def series_input(n_gates, T, seed, special=False):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n_gates, T, 2)).astype(f32)
    z[..., 0] += f32(25.0)                                           # clutter: a mean that the wall filter has to remove
    if special:
        vals = np.array([-0.0, 1e-40, -3e-39, 1.4e-45, np.inf, -np.inf, np.nan, 0.0, 3e38, -3e38], f32)
        at = rng.choice(z.size, size=min(z.size // 7 + 1, 40), replace=False)
        z.reshape(-1)[at] = rng.choice(vals, size=at.size)
    return z


def run_spectrum(ctx, dev, z, outputs=("power", "mean"), window="hann", skew=0, **opts):
    """the call -> dict of the outputs asked for, each behind a sentinel tail; the series must come back unchanged"""
    n_gates, T, _ = z.shape
    N, hop = opts.get("n_fft", 128), opts.get("hop", 32)
    cols = sm.n_cols(T, N, hop)
    sizes = dict(power=n_gates * cols * N, mean=n_gates * cols)
    p_z = dev.upload(z, skew)
    outs = {k: dev.upload(np.full(sizes[k] + TAIL, SENTINEL), skew) for k in outputs}
    ctx.spectral_frames(p_z, n_gates, V_NYQ, window=window, n_pulses=T, **{k + "_dev": p for k, p in outs.items()}, **opts)
    got = {}
    for k, p in outs.items():
        flat = ctx.d2h(p, (sizes[k] + TAIL,))
        assert (flat[sizes[k]:] == SENTINEL).all(), "the sentinel behind %s_dev was overwritten" % k
        got[k] = flat[:sizes[k]].reshape((n_gates, cols, N) if k == "power" else (n_gates, cols))
    assert np.array_equal(ctx.d2h(p_z, z.shape).view(np.uint32), z.view(np.uint32)), "series_dev is read only"
    return got


def check_spectrum(got, z, what, window=1, **opts):
    N = opts.get("n_fft", 128)
    h = sm.window(window, N) if isinstance(window, int) else window
    power, mean = sm.spectrum(z, h, V_NYQ, N=N, hop=opts.get("hop", 32), wall=opts.get("wall", sm.WALL_MEAN), wall_bins=opts.get("wall_bins", 2))
    want = dict(power=power, mean=mean)
    for k, v in got.items():
        ic.assert_same_bits(v, want[k], "%s %s" % (k, what))


@pytest.mark.parametrize("hop_of", ["1", "N/2", "N"])
@pytest.mark.parametrize("N", sm.FFT_SIZES)
def test_spectrum_matches_the_mirror(ctx, dev, N, hop_of):
    """every FFT size x hop, at T = N (one column), T = N + hop - 1 (the last partial window dropped) and a series of several columns;
    the wall filter, wall_bins, the window and the number of gates rotate with the case"""
    hop = {"1": 1, "N/2": N // 2, "N": N}[hop_of]
    for k, T in enumerate((N, N + hop - 1, 2 * N + 3 if hop > 1 else N + 70)):
        i = sm.FFT_SIZES.index(N) + hop + k
        n_gates = (1, 5)[i % 2]
        wall = (sm.WALL_MEAN, sm.WALL_NONE)[(i // 2) % 2]
        wall_bins = (0, N // 4, 2)[i % 3]
        kind = i % 2
        z = series_input(n_gates, T, seed=i)
        got = run_spectrum(ctx, dev, z, window=("rect", "hann")[kind], n_fft=N, hop=hop, wall=wall, wall_bins=wall_bins)
        assert (got["power"].shape[1] == 1) == (k < 2)
        check_spectrum(got, z, "N=%d hop=%d T=%d gates=%d wall=%d bins=%d window=%d" % (N, hop, T, n_gates, wall, wall_bins, kind), window=kind,
                       n_fft=N, hop=hop, wall=wall, wall_bins=wall_bins)


@pytest.mark.parametrize("N", sm.FFT_SIZES)
@pytest.mark.parametrize("wall", [sm.WALL_NONE, sm.WALL_MEAN])
def test_spectrum_special_values(ctx, dev, N, wall):
    """NaN, infinities, subnormals, -0.0 and values whose squares overflow, sprinkled over the series"""
    z = series_input(2, N + 2 * (N // 4), seed=N + wall, special=True)
    got = run_spectrum(ctx, dev, z, n_fft=N, hop=N // 4, wall=wall, wall_bins=1)
    check_spectrum(got, z, "special values N=%d wall=%d" % (N, wall), n_fft=N, hop=N // 4, wall=wall, wall_bins=1)


@pytest.mark.parametrize("only", ["power", "mean"])
@pytest.mark.parametrize("skew", [0, 4, 8])
def test_spectrum_each_output_alone_and_skewed(ctx, dev, only, skew):
    z = series_input(3, 300, seed=skew)
    got = run_spectrum(ctx, dev, z, outputs=(only,), skew=skew)
    assert sorted(got) == [only]
    check_spectrum(got, z, "only %s, skew %d" % (only, skew))
    own = np.linspace(0.0, 2.0, 128).astype(f32)                     # a caller's own window
    got = run_spectrum(ctx, dev, z, window=own, skew=skew)
    check_spectrum(got, z, "own window, skew %d" % skew, window=own)


def test_series_refusals_leave_the_output_untouched(mcrt, ctx, dev):
    L = mcrt.load_library()
    F, E, R, G, T, NG = 2, 3, 20, 4, 70, 3
    n = F * E * R
    st, mv, gates, weight, rate, ph = clean_case(F, E, R, G, T, NG)
    ph = np.array(ph, np.int64)
    opts = mcrt.spectral_opts_struct(n_pulses=T, gate_rows=G)
    # one allocation, in floats: iq_static [0, 2n), iq_moving [2n, 4n), then room for the series (2 NG T) and sigma (F)
    TOTAL = 4 * n + 2 * NG * T + 16
    head = np.concatenate([st.reshape(-1), mv.reshape(-1)])
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(st_=0, mv_=2 * n, frames=F, lines=E, rows=R, g=gates, ng=NG, w=weight, rt=rate, p=ph, o=opts, first=0, sig=None, out=4 * n, null_ctx=False):
        big = dev.upload(np.concatenate([head, np.full(TOTAL - 4 * n, SENTINEL)]))
        at = lambda floats: None if floats is None else C.c_void_p(big + 4 * floats)
        rc = L.mcrt_spectral_series_frames(None if null_ctx else ctx.h, at(st_), at(mv_), frames, lines, rows, None if g is None else vp(g), ng,
                                           None if w is None else vp(w), None if rt is None else vp(rt), None if p is None else vp(p),
                                           None if o is None else C.byref(o), first, at(sig), at(out))
        got = ctx.d2h(big, (TOTAL,))
        assert np.array_equal(got[:4 * n].view(np.uint32), head.view(np.uint32)) and (got[4 * n:] == SENTINEL).all()
        return rc

    assert call(null_ctx=True) == INVALID and call(mv_=None) == INVALID and call(g=None) == INVALID and call(w=None) == INVALID
    assert call(rt=None) == INVALID and call(p=None) == INVALID and call(o=None) == INVALID and call(out=None) == INVALID
    assert call(frames=0) == INVALID and call(lines=0) == INVALID and call(rows=0) == INVALID and call(ng=0) == INVALID
    for kw in (dict(n_pulses=0), dict(n_pulses=16385), dict(gate_rows=0), dict(gate_rows=65), dict(n_fft=100), dict(n_fft=1024), dict(hop=0), dict(hop=129),
               dict(wall=2), dict(wall_bins=33), dict(sigma=-0.5), dict(sigma=float("nan"))):
        assert call(o=mcrt.spectral_opts_struct(**dict(dict(n_pulses=T, gate_rows=G), **kw))) == INVALID, kw
    for bad in (np.nan, np.inf):
        w2 = weight.copy(); w2[1] = bad
        assert call(w=w2) == INVALID
    for bad in (65537, -65537):
        r2 = rate.copy(); r2[2, 3] = bad
        assert call(rt=r2) == INVALID
    for field, bad in ((0, F), (1, E), (2, R - G + 1)):
        g2 = gates.copy(); g2[1, field] = bad
        assert call(g=g2) == INVALID
    assert call(ng=65536) == LIMIT                                                          # (refused before any table is read)
    assert call(o=mcrt.spectral_opts_struct(n_pulses=16384, gate_rows=G), ng=16384) == LIMIT      # n_gates * T = 2^28
    assert call(frames=1 << 11, lines=1 << 10, rows=1 << 10) == LIMIT                       # 2^31 samples
    assert call(first=0xFFFFFFFF) == LIMIT                                                  # the second image's id would pass 2^32
    assert call(out=4 * n - 1) == INVALID and call(out=0) == INVALID and call(out=2 * n) == INVALID      # the series overlaps an input
    assert call(sig=4 * n + 3) == INVALID                                                   # sigma_dev inside the series
    with pytest.raises(ValueError):
        ctx.spectral_series_frames(None, dev(8 * n), F, E, R, gates, weight, rate[:, :2], ph, dev(8 * NG * T))


def test_spectrum_refusals_leave_the_outputs_untouched(mcrt, ctx, dev):
    L = mcrt.load_library()
    NG, T, N, hop = 2, 200, 64, 16
    cols = sm.n_cols(T, N, hop)
    z = series_input(NG, T, seed=3)
    opts = mcrt.spectral_opts_struct(n_pulses=T, n_fft=N, hop=hop)
    h = sm.window(1, N)
    nz, npw = 2 * NG * T, NG * cols * N
    TOTAL = nz + npw + NG * cols + 16                                 # floats: the series, then room for power and mean
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(z_=0, ng=NG, w=h, o=opts, nyq=V_NYQ, power=nz, mean=nz + npw, null_ctx=False):
        big = dev.upload(np.concatenate([z.reshape(-1), np.full(TOTAL - nz, SENTINEL)]))
        at = lambda floats: None if floats is None else C.c_void_p(big + 4 * floats)
        rc = L.mcrt_spectral_frames(None if null_ctx else ctx.h, at(z_), ng, None if w is None else vp(w), None if o is None else C.byref(o), nyq, at(power), at(mean))
        got = ctx.d2h(big, (TOTAL,))
        assert np.array_equal(got[:nz].view(np.uint32), z.reshape(-1).view(np.uint32)) and (got[nz:] == SENTINEL).all()
        return rc

    assert call(null_ctx=True) == INVALID and call(z_=None) == INVALID and call(w=None) == INVALID and call(o=None) == INVALID and call(ng=0) == INVALID
    assert call(power=None, mean=None) == INVALID                                          # no output
    for kw in (dict(n_pulses=N - 1), dict(n_pulses=0), dict(n_fft=48), dict(hop=0), dict(hop=N + 1), dict(wall=2), dict(wall_bins=N // 4 + 1), dict(gate_rows=0)):
        assert call(o=mcrt.spectral_opts_struct(**dict(dict(n_pulses=T, n_fft=N, hop=hop), **kw))) == INVALID, kw
    for nyq in (0.0, -1.0, float("nan"), float("inf")):
        assert call(nyq=nyq) == INVALID
    for bad in (np.nan, np.inf):
        h2 = h.copy(); h2[5] = bad
        assert call(w=h2) == INVALID
    assert call(ng=65536) == LIMIT and call(o=mcrt.spectral_opts_struct(n_pulses=16384, n_fft=N, hop=hop), ng=16384) == LIMIT
    assert call(power=nz - 1) == INVALID and call(mean=0) == INVALID and call(mean=nz + npw - 1) == INVALID      # overlaps
    with pytest.raises(ValueError):
        ctx.spectral_frames(dev(8 * NG * T), NG, V_NYQ, power_dev=dev(4 * npw), window=h[:10], n_pulses=T, n_fft=N, hop=hop)


def test_calls_with_nothing_wrong_write(ctx, dev):
    """the refusal tests' shapes with nothing wrong are accepted and write every element: their sentinels are not kernels that do nothing"""
    st, mv, gates, weight, rate, ph = clean_case(2, 3, 20, 4, 70, 3)
    got = run_series(ctx, dev, st, mv, gates, weight, rate, ph)
    assert (got != SENTINEL).all()
    got = run_spectrum(ctx, dev, series_input(2, 200, seed=3), n_fft=64, hop=16)
    assert all((v != SENTINEL).all() for v in got.values())


@pytest.mark.parametrize("N", sm.FFT_SIZES)
def test_a_gate_where_nothing_moves_has_no_power(ctx, dev, N):
    """on the device: without noise the series of a gate whose rows stand still (rate 0, with a moving part or without) is one value, the
    pairwise mean of N equal floats is that value exactly, and every power and every mean velocity is +0.0f"""
    F, E, R, G, T = 1, 2, 40, 8, N + 96
    rng = np.random.default_rng(N)
    st = (rng.standard_normal((F, E, R, 2)) * 1000.0).astype(f32); mv = rng.standard_normal((F, E, R, 2)).astype(f32)
    mv[0, 1] = 0.0
    gates = np.array([[0, 0, 5], [0, 1, 30]], np.uint32)
    rate = np.zeros((2, G), np.int32)
    z = run_series(ctx, dev, st, mv, gates, np.ones(G, f32), rate, phase_table(T, "mixed", rng))
    assert (z == z[:, :1]).all() and np.abs(z).min() > 0
    got = run_spectrum(ctx, dev, z, n_fft=N, hop=32, wall=sm.WALL_MEAN, wall_bins=0)
    assert not got["power"].view(np.uint32).any() and not got["mean"].view(np.uint32).any()


@pytest.mark.parametrize("N,m", [(32, 5), (64, -9), (128, 19), (256, -100), (512, 255)])
def test_a_whole_bin_rotor_fills_one_bin(ctx, dev, N, m):
    """on the device: a one-row gate at rate 65536 under a constant step of exactly m * 2^32 / N turns by whole table entries, so under the
    rectangular window all its power falls into bin N/2 + m.  What leaks is the float rounding of the table's entries and of the FFT: the
    mirror's own leakage, total outside the bin over the bin, is 6.3e-15 (N = 32), 7.1e-15, 6.2e-15, 7.1e-15, 9.9e-15 (N = 512); the bound
    is 4e-14, four times the worst of them and 134 dB below the line."""
    T = N + 5
    step = (m * (1 << 32)) // N
    ph = [t * step for t in range(T)]
    mv = np.zeros((1, 1, 3, 2), f32); mv[0, 0, 1] = (0.75, -1.5)
    gates = np.array([[0, 0, 1]], np.uint32)
    z = run_series(ctx, dev, None, mv, gates, np.ones(1, f32), np.array([[65536]], np.int32), ph)
    got = run_spectrum(ctx, dev, z, window="rect", n_fft=N, hop=1, wall=sm.WALL_NONE, wall_bins=0)
    p = got["power"][0].astype(np.float64)
    line = p[:, N // 2 + m]
    leak = (p.sum(axis=1) - line) / line
    want_p, _ = sm.spectrum(sm.series(None, mv, gates, np.ones(1, f32), np.array([[65536]], np.int32), ph), sm.window(0, N), V_NYQ, N=N, hop=1, wall=sm.WALL_NONE, wall_bins=0)
    ic.assert_same_bits(got["power"], want_p, "whole-bin rotor N=%d" % N)
    wp = want_p[0].astype(np.float64)
    print("N=%d m=%d: device leakage %.2e, mirror leakage %.2e" % (N, m, leak.max(), ((wp.sum(axis=1) - wp[:, N // 2 + m]) / wp[:, N // 2 + m]).max()))
    assert (leak < 4e-14).all()
    assert np.allclose(line, (N * np.hypot(0.75, 1.5)) ** 2, rtol=1e-5)
    assert np.allclose(got["mean"][0], m * 2.0 * V_NYQ / N, rtol=1e-5)
