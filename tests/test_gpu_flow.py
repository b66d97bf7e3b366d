"""Colour Doppler on the MI355X: mcrt_flow_split_frames (k_flow_split) and mcrt_flow_frames (k_flow<N, WALL>, k_flow_avg) against the numpy
mirror (tests/flow_mirror.py) bit for bit -- at the shapes around a wavefront's 64 rows, for every ensemble length class and wall filter,
windows up to larger than the image, with and without the static stack and the noise, on special values, with every output left out in
turn, behind sentinels and at every alignment; the refusals; and two properties read on the device itself: what stands still cancels
exactly under mean removal, and a uniform moving region reads its ground truth."""
import ctypes as C
import math
import numpy as np
import pytest

import flow_mirror as fm
import image_cases as ic

pytestmark = pytest.mark.gpu

f32 = np.float32
INVALID, LIMIT = -1, -5
SENTINEL = f32(-77.25)
V_NYQ = 333.3333333333333

SHAPES = [(1, 1, 1), (1, 2, 3), (2, 3, 63), (1, 5, 65), (2, 4, 465), (1, 2, 2048)]
WINDOWS = [(0, 0), (1, 1), (2, 1), (8, 4)]
N_LABELS = 3
OUTPUTS = ("corr", "vel", "var", "truth")


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


def case(F, E, R, seed=0):
    """(iq_static, iq_moving [F][E][R][2], tissue [F][E][R], phasor, truth): every family of image_cases' scan-lines in both components
    (noise, ramps, saws, subnormals, infinities, NaN), labels 0 .. N_LABELS - 1, one past the table and MCRT_LABEL_NONE"""
    st = np.stack([np.stack([ic.envelope_image(E, R, seed=seed + 5 * f + c) for c in range(2)], axis=-1) for f in range(F)])
    mv = np.stack([np.stack([ic.envelope_image(E, R, seed=seed + 5 * f + c + 2) for c in range(2)], axis=-1) for f in range(F)])
    rng = np.random.default_rng(seed * 31 + F * 7 + E * 3 + R)
    tissue = rng.choice(np.array([0, 1, 2, N_LABELS, 255], np.uint8), size=(F, E, R))
    vel = np.array([[0.0, 0.0, 0.0], [30.0, -120.0, 60.0], [-400.0, 10.0, 500.0]], f32)       # at rest; slow; beyond the Nyquist velocity
    d = rng.standard_normal((E, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    ph, tr = fm.phasors(V_NYQ, vel, d.astype(f32))
    return st.astype(f32), mv.astype(f32), tissue, ph, tr


def run_flow(ctx, dev, st, mv, tissue, ph, tr, outputs=OUTPUTS, sigma_from="opts", sigma=0.0, first_image_id=0, skew=0, tail=8, **opts):
    """the call -> (dict of the outputs asked for, the inputs as the device holds them afterwards).  Every output starts as a sentinel, has
    `tail` sentinel floats behind it that must survive, and starts `skew` bytes off a 256-byte boundary, as the inputs do"""
    F, E, R = tissue.shape
    n = F * E * R
    p_st = None if st is None else dev.upload(st, skew)
    p_mv = dev.upload(mv, skew); p_ti = dev.upload(tissue, skew)
    sig = np.broadcast_to(np.asarray(sigma, f32), (F,)).copy()
    p_sig = dev.upload(sig, skew) if sigma_from == "dev" else None
    sizes = dict(corr=3 * n, vel=n, var=n, truth=n)
    outs = {k: dev.upload(np.full(sizes[k] + tail, SENTINEL), skew) for k in outputs}
    kw = dict(opts)
    if sigma_from == "opts":
        assert np.all(sig == sig[0])
        kw["sigma"] = float(sig[0])
    ctx.flow_frames(p_st, p_mv, p_ti, F, E, R, V_NYQ, ph, tr, first_image_id=first_image_id, sigma_dev=p_sig,
                    **{k + "_dev": p for k, p in outs.items()}, **kw)
    got = {}
    for k, p in outs.items():
        flat = ctx.d2h(p, (sizes[k] + tail,))
        assert (flat[sizes[k]:] == SENTINEL).all(), "the sentinel behind %s_dev was overwritten" % k
        got[k] = flat[:sizes[k]].reshape((F, 3, E, R) if k == "corr" else (F, E, R))
    after = (None if st is None else ctx.d2h(p_st, st.shape), ctx.d2h(p_mv, mv.shape), ctx.d2h(p_ti, tissue.shape, np.uint8))
    if p_sig is not None:
        assert np.array_equal(ctx.d2h(p_sig, (F,)).view(np.uint32), sig.view(np.uint32)), "sigma_dev is read only"
    return got, after


def check(got, want, what, after=None, before=None):
    for k, v in got.items():
        ic.assert_same_bits(v, want[k], "%s %s" % (k, what))
    if after is not None:
        for a, b, name in zip(after, before, ("iq_static_dev", "iq_moving_dev", "tissue_dev")):
            if b is not None:
                assert np.array_equal(a.view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), "%s is read only (%s)" % (name, what)


WALLS = {"none": 0, "mean": 1, "linear": 2}


@pytest.mark.parametrize("wall", sorted(WALLS))
@pytest.mark.parametrize("N", [2, 3, 8, 16])
@pytest.mark.parametrize("F,E,R", SHAPES)
def test_shapes_match_the_mirror(ctx, dev, F, E, R, N, wall):
    """every shape x ensemble length x wall filter; the window, the static stack and where sigma comes from rotate with the case"""
    i = SHAPES.index((F, E, R)) + N + WALLS[wall]
    a, b = WINDOWS[i % 4]
    with_static = i % 2 == 0
    sigma_from, sigma = (("opts", 0.0), ("opts", 0.375), ("dev", [0.5, 0.0][:F] if F == 2 else [0.25]))[i % 3]
    st, mv, tissue, ph, tr = case(F, E, R, seed=N)
    st = st if with_static else None
    what = "F=%d E=%d R=%d N=%d wall=%s window=(%d, %d) static=%s sigma=%s from %s" % (F, E, R, N, wall, a, b, with_static, sigma, sigma_from)
    want = fm.flow(st, mv, tissue, ph, tr, V_NYQ, N=N, wall=WALLS[wall], avg_rows=a, avg_lines=b, sigma=sigma, seed=11, first_image_id=5)
    got, after = run_flow(ctx, dev, st, mv, tissue, ph, tr, sigma_from=sigma_from, sigma=sigma, first_image_id=5,
                          n_packets=N, wall=wall, avg_rows=a, avg_lines=b, seed=11)
    check(got, want, what, after, (st, mv, tissue))


@pytest.mark.parametrize("sigma_from,sigma", [("opts", 0.0), ("opts", 0.75), ("dev", [0.0, 1.5]), ("dev", [0.125, 0.125])])
@pytest.mark.parametrize("with_static", [False, True])
@pytest.mark.parametrize("a,b", WINDOWS)
def test_windows_static_and_sigma(ctx, dev, a, b, with_static, sigma_from, sigma):
    """every window (up to larger than the image: 3 lines, 63 rows under (8, 4) clips on every side) with and without the static stack, and
    sigma 0 and > 0 from the options and from the device -- a frame with sigma 0 beside one with noise"""
    F, E, R = 2, 3, 63
    st, mv, tissue, ph, tr = case(F, E, R, seed=a + b)
    st = st if with_static else None
    want = fm.flow(st, mv, tissue, ph, tr, V_NYQ, N=8, wall=fm.WALL_MEAN, avg_rows=a, avg_lines=b, sigma=sigma, first_image_id=0xFFFFFFFE)
    got, after = run_flow(ctx, dev, st, mv, tissue, ph, tr, sigma_from=sigma_from, sigma=sigma, first_image_id=0xFFFFFFFE, avg_rows=a, avg_lines=b)
    check(got, want, "window=(%d, %d) static=%s sigma=%s from %s" % (a, b, with_static, sigma, sigma_from), after, (st, mv, tissue))


def test_defaults(ctx, dev):
    """no options: N = 8, mean removal, window (2, 1), sigma 0, the default seed"""
    st, mv, tissue, ph, tr = case(1, 4, 70)
    got, _ = run_flow(ctx, dev, st, mv, tissue, ph, tr)
    check(got, fm.flow(st, mv, tissue, ph, tr, V_NYQ), "defaults")
    got, _ = run_flow(ctx, dev, st, mv, tissue, ph, tr, sigma=0.5)
    check(got, fm.flow(st, mv, tissue, ph, tr, V_NYQ, sigma=0.5), "the default seed")


@pytest.mark.parametrize("left_out", OUTPUTS)
def test_each_output_left_out(ctx, dev, left_out):
    st, mv, tissue, ph, tr = case(2, 5, 65, seed=3)
    want = fm.flow(st, mv, tissue, ph, tr, V_NYQ, N=3, wall=fm.WALL_LINEAR, sigma=0.25)
    outputs = tuple(k for k in OUTPUTS if k != left_out)
    got, after = run_flow(ctx, dev, st, mv, tissue, ph, tr, outputs=outputs, sigma=0.25, n_packets=3, wall="linear")
    assert sorted(got) == sorted(outputs)
    check(got, want, "without " + left_out, after, (st, mv, tissue))
    got, _ = run_flow(ctx, dev, st, mv, tissue, ph, tr, outputs=(left_out,), sigma=0.25, n_packets=3, wall="linear")
    check(got, want, "only " + left_out)


@pytest.mark.parametrize("skew", [4, 8, 12])
def test_pointers_off_a_16_byte_boundary(ctx, dev, skew):
    st, mv, tissue, ph, tr = case(1, 5, 65, seed=skew)
    want = fm.flow(st, mv, tissue, ph, tr, V_NYQ, sigma=0.5)
    got, after = run_flow(ctx, dev, st, mv, tissue, ph, tr, sigma_from="dev", sigma=[0.5], skew=skew)
    check(got, want, "skew %d" % skew, after, (st, mv, tissue))


def test_labels_outside_the_table(ctx, dev):
    """labels >= n_labels and MCRT_LABEL_NONE take the phasor (1, 0) and the truth 0: a line of each beside a line of a moving label"""
    F, E, R = 1, 3, 40
    st, mv, _, ph, tr = case(F, E, R, seed=9)
    tissue = np.empty((F, E, R), np.uint8); tissue[0, 0] = N_LABELS; tissue[0, 1] = 255; tissue[0, 2] = 1
    got, _ = run_flow(ctx, dev, None, mv, tissue, ph, tr, wall="none", avg_rows=0, avg_lines=0)
    check(got, fm.flow(None, mv, tissue, ph, tr, V_NYQ, wall=fm.WALL_NONE, avg_rows=0, avg_lines=0), "labels outside")
    assert not got["truth"][0, :2].view(np.uint32).any() and (got["truth"][0, 2] == tr[1, 2]).all()
    rest = fm.flow(None, mv, np.zeros_like(tissue), ph, tr, V_NYQ, wall=fm.WALL_NONE, avg_rows=0, avg_lines=0)      # label 0 is at rest: the same phasor
    ic.assert_same_bits(got["corr"][0, :, :2], rest["corr"][0, :, :2], "labels outside the table stand still")


def test_tables_are_replaced_when_they_change(ctx, dev):
    """the phasors and the truth live in the context and are copied only when they differ: a second call with other tables, then with a
    smaller and a larger table, reads its own"""
    st, mv, tissue, ph, tr = case(1, 4, 33, seed=2)
    for scale, labels in ((1.0, 3), (0.5, 3), (0.5, 2), (2.0, 3), (1.0, 3)):
        vel = np.array([[0.0, 0.0, 0.0], [30.0, -120.0, 60.0], [-400.0, 10.0, 500.0]], f32)[:labels] * f32(scale)
        d = np.random.default_rng(labels).standard_normal((4, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
        ph2, tr2 = fm.phasors(V_NYQ, vel, d.astype(f32))
        got, _ = run_flow(ctx, dev, st, mv, tissue, ph2, tr2, outputs=("vel", "truth"))
        check(got, fm.flow(st, mv, tissue, ph2, tr2, V_NYQ), "tables x %g, %d labels" % (scale, labels))


@pytest.mark.parametrize("F,E,R", [(1, 1, 1), (2, 3, 63), (1, 5, 65), (2, 4, 465)])
def test_split_matches_the_mirror(ctx, dev, F, E, R):
    rf = np.stack([ic.envelope_image(E, R, seed=f) for f in range(F)])
    rng = np.random.default_rng(R)
    tissue = rng.choice(np.array([0, 1, 2, 3, 4, 200, 253, 254, 255], np.uint8), size=(F, E, R))
    for moving in ([0, 1, 1], [1], [0] * 253 + [1], [1, 0, 0, 1, 1]):
        for skew in (0, 4):
            p_rf = dev.upload(rf, skew); p_ti = dev.upload(tissue, skew)
            p_out = dev.upload(np.full(2 * rf.size + 8, SENTINEL), skew)
            ctx.flow_split_frames(p_rf, p_ti, F, E, R, moving, p_out)
            flat = ctx.d2h(p_out, (2 * rf.size + 8,))
            assert (flat[2 * rf.size:] == SENTINEL).all()
            want = fm.split(rf, tissue, moving)
            got = flat[:2 * rf.size].reshape(F, 2, E, R)
            ic.assert_same_bits(got, want, "split %s" % (moving[:5],))
            assert np.array_equal(got.view(np.uint32)[~np.isnan(want)], want.view(np.uint32)[~np.isnan(want)])
            ic.assert_same_bits(ctx.d2h(p_rf, rf.shape), rf, "rf_dev is read only")
            assert np.array_equal(ctx.d2h(p_ti, tissue.shape, np.uint8), tissue)


def test_split_refusals(mcrt, ctx, dev):
    L = mcrt.load_library()
    F, E, R = 2, 3, 10
    n = F * E * R
    rf = np.arange(n, dtype=f32).reshape(F, E, R); tissue = np.ones((F, E, R), np.uint8)
    moving = np.array([0, 1], np.uint8)
    pm = moving.ctypes.data_as(C.c_void_p)
    big = dev.upload(np.concatenate([rf.reshape(-1), np.full(3 * n, SENTINEL)]))
    p_ti = dev.upload(tissue)
    at = lambda floats: None if floats is None else C.c_void_p(big + 4 * floats)

    def call(rf_=0, out=n, ti=p_ti, frames=F, lines=E, rows=R, mv=pm, labels=2, null_ctx=False):
        rc = L.mcrt_flow_split_frames(None if null_ctx else ctx.h, at(rf_), None if ti is None else C.c_void_p(ti), frames, lines, rows, mv, labels, at(out))
        got = ctx.d2h(big, (4 * n,))
        assert np.array_equal(got[:n], rf.reshape(-1)) and (got[n:] == SENTINEL).all()
        return rc

    assert call(null_ctx=True) == INVALID and call(rf_=None) == INVALID and call(out=None) == INVALID and call(ti=None) == INVALID and call(mv=None) == INVALID
    assert call(frames=0) == INVALID and call(lines=0) == INVALID and call(rows=0) == INVALID and call(labels=0) == INVALID
    assert call(labels=255) == LIMIT
    assert call(out=n - 1) == INVALID and call(out=0) == INVALID                           # out_dev overlaps rf_dev
    assert call(frames=1 << 11, lines=1 << 10, rows=1 << 10) == LIMIT                      # 2^31 samples
    tis = dev.upload(np.ones(4 * n, np.uint8))
    assert L.mcrt_flow_split_frames(ctx.h, at(0), C.c_void_p(tis), F, E, R, pm, 2, C.c_void_p(tis)) == INVALID     # out_dev overlaps tissue_dev


def test_refusals_leave_the_outputs_untouched(mcrt, ctx, dev):
    L = mcrt.load_library()
    F, E, R = 2, 3, 20
    n = F * E * R
    st, mv, tissue, ph, tr = case(F, E, R)
    opts = mcrt.flow_opts_struct()
    # one allocation, in floats: iq_static [0, 2n), iq_moving [2n, 4n), then room for corr (3n), vel, var, truth (n each) and sigma (F)
    TOTAL = 12 * n
    head = np.concatenate([st.reshape(-1), mv.reshape(-1)])
    p_ti = dev.upload(tissue)
    ph_p, tr_p = ph.ctypes.data_as(C.c_void_p), tr.ctypes.data_as(C.c_void_p)

    def call(st_=0, mv_=2 * n, ti=p_ti, frames=F, lines=E, rows=R, o=opts, nyq=V_NYQ, ph_=ph_p, tr_=tr_p, labels=N_LABELS, first=0, sig=None,
             corr=4 * n, vel=7 * n, var=8 * n, truth=9 * n, null_ctx=False):
        big = dev.upload(np.concatenate([head, np.full(TOTAL - 4 * n, SENTINEL)]))
        at = lambda floats: None if floats is None else C.c_void_p(big + 4 * floats)
        rc = L.mcrt_flow_frames(None if null_ctx else ctx.h, at(st_), at(mv_), None if ti is None else C.c_void_p(ti), frames, lines, rows,
                                None if o is None else C.byref(o), nyq, ph_, tr_, labels, first, at(sig), at(corr), at(vel), at(var), at(truth))
        got = ctx.d2h(big, (TOTAL,))
        assert np.array_equal(got[:4 * n].view(np.uint32), head.view(np.uint32)) and (got[4 * n:] == SENTINEL).all()
        return rc

    assert call(null_ctx=True) == INVALID and call(mv_=None) == INVALID and call(ti=None) == INVALID and call(o=None) == INVALID
    assert call(ph_=None) == INVALID and call(tr_=None) == INVALID
    assert call(frames=0) == INVALID and call(lines=0) == INVALID and call(rows=0) == INVALID and call(labels=0) == INVALID
    assert call(corr=None, vel=None, var=None, truth=None) == INVALID                      # no output
    assert call(rows=2049, frames=1, lines=1) == LIMIT and call(labels=255) == LIMIT
    assert call(frames=1 << 11, lines=1 << 10, rows=1 << 10) == LIMIT                      # 2^31 samples
    assert call(first=0xFFFFFFFF) == LIMIT                                                 # the second frame's id would pass 2^32
    for nyq in (0.0, -1.0, float("nan"), float("inf")):
        assert call(nyq=nyq) == INVALID
    for kw in (dict(n_packets=1), dict(n_packets=17), dict(wall=3), dict(avg_rows=9), dict(avg_lines=5), dict(sigma=-0.5), dict(sigma=float("nan")),
               dict(prf_hz=0.0)):
        assert call(o=mcrt.flow_opts_struct(**kw)) == INVALID, kw
    for bad in (np.nan, np.inf):
        p2 = ph.copy(); p2[2, 1, 0] = bad
        assert call(ph_=p2.ctypes.data_as(C.c_void_p)) == INVALID
        t2 = tr.copy(); t2[0, 0] = bad
        assert call(tr_=t2.ctypes.data_as(C.c_void_p)) == INVALID
    # overlaps: an output with an input, and two outputs with each other
    assert call(corr=4 * n - 1) == INVALID and call(vel=0) == INVALID and call(var=2 * n) == INVALID and call(truth=n) == INVALID
    assert call(vel=7 * n - 1) == INVALID and call(var=7 * n + 1) == INVALID and call(truth=9 * n - 1) == INVALID
    assert call(sig=7 * n) == INVALID and call(sig=4 * n + 1) == INVALID                   # sigma_dev inside vel_dev, inside corr_dev
    tis = dev.upload(np.ones(4 * n, np.uint8))
    assert L.mcrt_flow_frames(ctx.h, None, C.c_void_p(dev.upload(mv)), C.c_void_p(tis), F, E, R, C.byref(opts), V_NYQ, ph_p, tr_p, N_LABELS, 0, None,
                              None, C.c_void_p(tis), None, None) == INVALID                # vel_dev is tissue_dev
    with pytest.raises(ValueError):
        ctx.flow_frames(None, dev(8 * n), p_ti, F, E, R, V_NYQ, ph[:, :2], tr, vel_dev=dev(4 * n))


def test_call_with_nothing_wrong_writes(ctx, dev):
    """the refusal test's shape with nothing wrong is accepted and writes every element: its sentinels are not a kernel that does nothing"""
    st, mv, tissue, ph, tr = case(2, 3, 20)
    got, _ = run_flow(ctx, dev, st, mv, tissue, ph, tr)
    assert all((v != SENTINEL).all() for v in got.values())


@pytest.mark.parametrize("N", [2, 4, 8, 16])
@pytest.mark.parametrize("wall", ["mean", "linear"])
def test_what_stands_still_cancels_exactly(ctx, dev, N, wall):
    """on the device: at sigma 0 a sample whose label is at rest (or outside the table) has r0, Re r1 and Im r1 exactly +0.0 under mean
    removal where N is a power of two -- the pairwise sum of N equal floats and its division by N are exact there (not at N = 3)"""
    F, E, R = 1, 4, 130
    rng = np.random.default_rng(N)
    st = (rng.standard_normal((F, E, R, 2)) * 1000.0).astype(f32); mv = rng.standard_normal((F, E, R, 2)).astype(f32)
    st[0, 0, :5] = 0.0; mv[0, 0, :5, 0] = (1e-40, -1e-38, 1e37, -0.0, 1.0000001)             # (16 x 1e37 is still finite)
    tissue = rng.choice(np.array([0, N_LABELS, 255], np.uint8), size=(F, E, R))
    _, _, _, ph, tr = case(F, E, R)
    got, _ = run_flow(ctx, dev, st, mv, tissue, ph, tr, n_packets=N, wall=wall, avg_rows=0, avg_lines=0)
    assert not got["corr"].view(np.uint32).any() and not got["vel"].view(np.uint32).any() and not got["var"].view(np.uint32).any()


def test_uniform_moving_region_reads_its_truth(ctx, dev):
    """on the device: a region of one amplitude that moves, at sigma 0 and without a wall filter, reads its ground truth.  The bound, in
    radians of phase step: det_atan2f's 1e-5, plus 32 * 2^-24 for the float rounding of p^n -- each of the N - 1 = 7 rotations rounds its
    four products and two sums (under 3 ulp of phase), the phasor's own two components are rounded once (1 ulp), and the seven products
    of the autocorrelation and their sum add under 2 ulp each -- times v_nyq / pi; plus 4 * 2^-24 of the truth itself for its float
    rounding and the scale's.  The mirror's own worst case is printed beside it."""
    F, E, R = 1, 6, 100
    d = np.random.default_rng(1).standard_normal((E, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    ph, tr = fm.phasors(V_NYQ, [[0.0, 0.0, 0.0], [80.0, -250.0, 120.0]], d.astype(f32))
    mv = np.empty((F, E, R, 2), f32); mv[..., 0] = 0.75; mv[..., 1] = -1.5
    tissue = np.ones((F, E, R), np.uint8)
    # (the scan-lines point in unrelated directions here, so the window stays within a line: averaged across such lines the estimate is
    # a mean of different velocities, not an error of the estimator)
    got, _ = run_flow(ctx, dev, None, mv, tissue, ph, tr, outputs=("vel", "truth"), wall="none", avg_rows=2, avg_lines=0)
    assert np.abs(tr[1]).max() < V_NYQ                                                       # nothing aliases
    bound = (1e-5 + 32 * 2.0 ** -24) * V_NYQ / math.pi + 4 * 2.0 ** -24 * np.abs(got["truth"]).astype(np.float64)
    err = np.abs(got["vel"].astype(np.float64) - got["truth"].astype(np.float64))
    mirror = fm.flow(None, mv, tissue, ph, tr, V_NYQ, wall=fm.WALL_NONE, avg_rows=2, avg_lines=0)
    print("uniform region: device worst %.3e mm/s, mirror worst %.3e mm/s, bound %.3e mm/s"
          % (err.max(), np.abs(mirror["vel"].astype(np.float64) - mirror["truth"]).max(), bound.min()))
    assert (got["truth"][0] == tr[1][:, None]).all() and (err <= bound).all()
