"""Strain elastography on the MI355X: mcrt_strain_compress_frames (k_strain_warp) and mcrt_strain_frames (k_strain_track, k_strain_slope)
against the numpy mirror (tests/strain_mirror.py) bit for bit -- at the shapes around a wavefront's 64 rows, for the smallest, the default
and the largest windows, with and without noise from the options and from the device, on special values and labels outside the table,
with every output left out in turn, behind sentinels and at every alignment; the refusals; and the zero-strain identity read on the
device itself."""
import ctypes as C
import numpy as np
import pytest

import image_cases as ic
import strain_mirror as sm

pytestmark = pytest.mark.gpu

f32 = np.float32
INVALID, LIMIT = -1, -5
SENTINEL = f32(-77.25)
CARRIER = 0.3475

SHAPES = [(1, 1, 1), (1, 2, 3), (2, 3, 63), (1, 5, 65), (2, 4, 465), (1, 2, 2048)]
WINDOWS = [(0, 0, 1), (1, 1, 1), (16, 8, 12), (32, 16, 32)]
# a rigid label, 1 %, the cap -- and the same under decompression
TABLES = [np.array([0, 167772, 524288], np.int32), np.array([-167772, 0, -524288], np.int32), np.array([33554, -524288, 167772], np.int32)]
N_LABELS = 3
COMPRESS_OUT = ("post_iq", "truth_disp", "truth_strain")
TRACK_OUT = ("disp", "rho", "strain")


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
    """(iq [F][E][R][2], tissue [F][E][R]): every family of image_cases' scan-lines in both components (noise, ramps, saws, subnormals,
    infinities, NaN), labels 0 .. N_LABELS - 1, one past the table and MCRT_LABEL_NONE, in runs and row by row"""
    iq = np.stack([np.stack([ic.envelope_image(E, R, seed=seed + 5 * f + c) for c in range(2)], axis=-1) for f in range(F)]).astype(f32)
    rng = np.random.default_rng(seed * 31 + F * 7 + E * 3 + R)
    tissue = rng.choice(np.array([0, 1, 2, N_LABELS, 255], np.uint8), size=(F, E, R))
    for e in range(1, E, 2):                                    # every other scan-line in runs of one label, as anatomy has them
        tissue[:, e] = np.repeat(rng.choice(np.array([0, 1, 2, N_LABELS, 255], np.uint8), size=(F, R // 37 + 1)), 37, axis=1)[:, :R]
    return iq, tissue


def speckle(F, E, R, seed=0):
    """finite speckle-like pairs: a carrier at CARRIER cycles per row under a smooth random envelope"""
    rng = np.random.default_rng(seed)
    b = rng.standard_normal((F, E, R + 6, 2))
    b = sum(b[:, :, i:i + R] for i in range(7)) / 7.0
    ph = 2.0 * np.pi * CARRIER * np.arange(R)
    z = (b[..., 0] + 1j * b[..., 1]) * np.exp(1j * ph)
    return np.stack([z.real, z.imag], axis=-1).astype(f32)


def run_compress(ctx, dev, iq, tissue, eps, outputs=COMPRESS_OUT, sigma_from="opts", sigma=0.0, first_image_id=0, skew=0, tail=8, **opts):
    """the call -> (dict of the outputs asked for).  Every output starts as a sentinel, has `tail` sentinel floats behind it that must
    survive, and starts `skew` bytes off a 256-byte boundary, as the inputs do; the inputs must come back as they went"""
    F, E, R = tissue.shape
    n = F * E * R
    p_iq = dev.upload(iq, skew); p_ti = dev.upload(tissue, skew)
    sig = np.broadcast_to(np.asarray(sigma, f32), (F,)).copy()
    p_sig = dev.upload(sig, skew) if sigma_from == "dev" else None
    sizes = dict(post_iq=2 * n, truth_disp=n, truth_strain=n)
    outs = {k: dev.upload(np.full(sizes[k] + tail, SENTINEL), skew) for k in outputs}
    kw = dict(opts)
    if sigma_from == "opts":
        assert np.all(sig == sig[0])
        kw["sigma"] = float(sig[0])
    ctx.strain_compress_frames(p_iq, p_ti, F, E, R, eps, CARRIER, first_image_id=first_image_id, sigma_dev=p_sig,
                               **{k + "_dev": p for k, p in outs.items()}, **kw)
    got = {}
    for k, p in outs.items():
        flat = ctx.d2h(p, (sizes[k] + tail,))
        assert (flat[sizes[k]:] == SENTINEL).all(), "the sentinel behind %s_dev was overwritten" % k
        got[k] = flat[:sizes[k]].reshape((F, E, R, 2) if k == "post_iq" else (F, E, R))
    assert np.array_equal(ctx.d2h(p_iq, iq.shape).view(np.uint32), iq.view(np.uint32)), "iq_dev is read only"
    assert np.array_equal(ctx.d2h(p_ti, tissue.shape, np.uint8), tissue), "tissue_dev is read only"
    if p_sig is not None:
        assert np.array_equal(ctx.d2h(p_sig, (F,)).view(np.uint32), sig.view(np.uint32)), "sigma_dev is read only"
    return got


def run_track(ctx, dev, pre, post, outputs=TRACK_OUT, skew=0, tail=8, **opts):
    F, E, R, _ = pre.shape
    n = F * E * R
    p_pre = dev.upload(pre, skew); p_post = dev.upload(post, skew)
    outs = {k: dev.upload(np.full(n + tail, SENTINEL), skew) for k in outputs}
    ctx.strain_frames(p_pre, p_post, F, E, R, CARRIER, **{k + "_dev": p for k, p in outs.items()}, **opts)
    got = {}
    for k, p in outs.items():
        flat = ctx.d2h(p, (n + tail,))
        assert (flat[n:] == SENTINEL).all(), "the sentinel behind %s_dev was overwritten" % k
        got[k] = flat[:n].reshape(F, E, R)
    for p, x, name in ((p_pre, pre, "pre_iq_dev"), (p_post, post, "post_iq_dev")):
        assert np.array_equal(ctx.d2h(p, x.shape).view(np.uint32), x.view(np.uint32)), "%s is read only" % name
    return got


def check(got, want, what):
    for k, v in got.items():
        ic.assert_same_bits(v, want["post" if k == "post_iq" else k], "%s %s" % (k, what))


def sigma_of(i, F):
    return (("opts", 0.0), ("opts", 0.375), ("dev", [0.5, 0.0][:F] if F == 2 else [0.25]))[i % 3]


@pytest.mark.parametrize("a,L,g", WINDOWS)
@pytest.mark.parametrize("F,E,R", SHAPES)
def test_shapes_match_the_mirror(ctx, dev, F, E, R, a, L, g):
    """every shape x window, both calls: the strain table and where sigma comes from rotate with the case; the tracker reads the
    mirror's post-compression pairs, so that neither call's result depends on the other's"""
    i = SHAPES.index((F, E, R)) + WINDOWS.index((a, L, g))
    eps = TABLES[i % 3]
    sigma_from, sigma = sigma_of(i, F)
    iq, tissue = case(F, E, R, seed=a)
    what = "F=%d E=%d R=%d a=%d L=%d g=%d table=%s sigma=%s from %s" % (F, E, R, a, L, g, list(eps), sigma, sigma_from)
    want = sm.compress(iq, tissue, eps, CARRIER, sigma=sigma, seed=11, first_image_id=5)
    got = run_compress(ctx, dev, iq, tissue, eps, sigma_from=sigma_from, sigma=sigma, first_image_id=5, seed=11, window_rows=a, search_rows=L, lsq_rows=g)
    check(got, want, what)
    post = want["post"]
    check(run_track(ctx, dev, iq, post, window_rows=a, search_rows=L, lsq_rows=g), sm.track(iq, post, CARRIER, a, L, g), what)


@pytest.mark.parametrize("a,L,g", WINDOWS)
@pytest.mark.parametrize("F,E,R", [(1, 2, 65), (1, 3, 465), (1, 1, 2048)])
def test_speckle_tracks_like_the_mirror(ctx, dev, F, E, R, a, L, g):
    """finite speckle under a real compression -- the lags move, the windows correlate: 1 % everywhere, a rigid band, and the noise"""
    iq = speckle(F, E, R, seed=R + a)
    tissue = np.ones((F, E, R), np.uint8); tissue[..., R // 3:R // 2] = 0
    eps = TABLES[0]
    want = sm.compress(iq, tissue, eps, CARRIER, sigma=0.05)
    got = run_compress(ctx, dev, iq, tissue, eps, sigma=0.05)
    check(got, want, "speckle")
    t = sm.track(iq, want["post"], CARRIER, a, L, g)
    check(run_track(ctx, dev, iq, want["post"], window_rows=a, search_rows=L, lsq_rows=g), t, "speckle a=%d L=%d g=%d R=%d" % (a, L, g, R))
    if L >= 8 and R >= 465:
        assert len(np.unique(np.rint(t["disp"]))) > 2                    # more than one lag wins


def test_defaults(ctx, dev):
    """no options: window 16, search 8, slope 12, sigma 0, the default seed"""
    iq, tissue = case(1, 4, 70)
    check(run_compress(ctx, dev, iq, tissue, TABLES[0]), sm.compress(iq, tissue, TABLES[0], CARRIER), "defaults")
    want = sm.compress(iq, tissue, TABLES[0], CARRIER, sigma=0.5)
    check(run_compress(ctx, dev, iq, tissue, TABLES[0], sigma=0.5), want, "the default seed")
    check(run_track(ctx, dev, iq, want["post"]), sm.track(iq, want["post"], CARRIER), "defaults")


@pytest.mark.parametrize("sigma_from,sigma", [("opts", 0.0), ("opts", 0.75), ("dev", [0.0, 1.5]), ("dev", [0.125, 0.125])])
def test_sigma(ctx, dev, sigma_from, sigma):
    """sigma 0 and > 0 from the options and from the device -- a frame with sigma 0 beside one with noise; ids at the end of their range"""
    iq, tissue = case(2, 3, 63, seed=4)
    want = sm.compress(iq, tissue, TABLES[1], CARRIER, sigma=sigma, first_image_id=0xFFFFFFFE)
    check(run_compress(ctx, dev, iq, tissue, TABLES[1], sigma_from=sigma_from, sigma=sigma, first_image_id=0xFFFFFFFE), want, "sigma=%s from %s" % (sigma, sigma_from))


@pytest.mark.parametrize("left_out", COMPRESS_OUT)
def test_each_compress_output_left_out(ctx, dev, left_out):
    iq, tissue = case(2, 5, 65, seed=3)
    want = sm.compress(iq, tissue, TABLES[2], CARRIER, sigma=0.25)
    outputs = tuple(k for k in COMPRESS_OUT if k != left_out)
    got = run_compress(ctx, dev, iq, tissue, TABLES[2], outputs=outputs, sigma=0.25)
    assert sorted(got) == sorted(outputs)
    check(got, want, "without " + left_out)
    check(run_compress(ctx, dev, iq, tissue, TABLES[2], outputs=(left_out,), sigma=0.25), want, "only " + left_out)


@pytest.mark.parametrize("left_out", TRACK_OUT)
def test_each_track_output_left_out(ctx, dev, left_out):
    """(without disp_dev the displacement lives in the context's buffer: the strain is the same)"""
    iq, tissue = case(2, 5, 65, seed=6)
    post = sm.compress(iq, tissue, TABLES[0], CARRIER)["post"]
    want = sm.track(iq, post, CARRIER, 3, 2, 4)
    outputs = tuple(k for k in TRACK_OUT if k != left_out)
    got = run_track(ctx, dev, iq, post, outputs=outputs, window_rows=3, search_rows=2, lsq_rows=4)
    assert sorted(got) == sorted(outputs)
    check(got, want, "without " + left_out)
    check(run_track(ctx, dev, iq, post, outputs=(left_out,), window_rows=3, search_rows=2, lsq_rows=4), want, "only " + left_out)


@pytest.mark.parametrize("skew", [4, 8, 12])
def test_pointers_off_a_16_byte_boundary(ctx, dev, skew):
    iq, tissue = case(1, 5, 65, seed=skew)
    want = sm.compress(iq, tissue, TABLES[0], CARRIER, sigma=0.5)
    check(run_compress(ctx, dev, iq, tissue, TABLES[0], sigma_from="dev", sigma=[0.5], skew=skew), want, "skew %d" % skew)
    check(run_track(ctx, dev, iq, want["post"], skew=skew), sm.track(iq, want["post"], CARRIER), "skew %d" % skew)


def test_labels_outside_the_table(ctx, dev):
    """labels >= n_labels and MCRT_LABEL_NONE do not strain: a line of each beside a line of a straining label"""
    F, E, R = 1, 3, 140
    iq, _ = case(F, E, R, seed=9)
    tissue = np.empty((F, E, R), np.uint8); tissue[0, 0] = N_LABELS; tissue[0, 1] = 255; tissue[0, 2] = 1
    got = run_compress(ctx, dev, iq, tissue, TABLES[0])
    check(got, sm.compress(iq, tissue, TABLES[0], CARRIER), "labels outside")
    assert not got["truth_disp"][0, :2].view(np.uint32).any() and not got["truth_strain"][0, :2].view(np.uint32).any()
    assert (got["truth_strain"][0, 2] == f32(167772) * f32(2.0 ** -24)).all() and got["truth_disp"][0, 2, 100] == f32(16777200) * f32(2.0 ** -24)


def test_table_is_replaced_when_it_changes(ctx, dev):
    """the strain table lives in the context and is copied only when it differs: other values, then a shorter and a longer table"""
    iq, tissue = case(1, 4, 33, seed=2)
    for eps in (TABLES[0], TABLES[1], TABLES[1][:2], TABLES[2], np.array([5, 6, 7, 8, 9], np.int32), TABLES[0]):
        got = run_compress(ctx, dev, iq, tissue, eps, outputs=("post_iq", "truth_disp"))
        check(got, sm.compress(iq, tissue, eps, CARRIER), "table %s" % list(eps))


def test_zero_strain_is_the_identity_on_the_device(ctx, dev):
    """on the device: with every strain 0 and no noise, post equals pre as floats, and the tracker reads a displacement of exactly 0, a
    correlation coefficient of exactly 1 and a strain of exactly 0 on finite speckle"""
    F, E, R = 2, 3, 200
    iq = speckle(F, E, R, seed=1)
    tissue = np.random.default_rng(0).choice(np.array([0, 1, N_LABELS, 255], np.uint8), size=(F, E, R))
    c = run_compress(ctx, dev, iq, tissue, np.zeros(2, np.int32))
    assert np.array_equal(c["post_iq"], iq) and not c["truth_disp"].view(np.uint32).any() and not c["truth_strain"].view(np.uint32).any()
    t = run_track(ctx, dev, iq, c["post_iq"])
    assert (t["disp"] == 0.0).all() and (t["rho"] == 1.0).all() and (t["strain"] == 0.0).all()


def test_compress_refusals_leave_the_outputs_untouched(mcrt, ctx, dev):
    L = mcrt.load_library()
    F, E, R = 2, 3, 20
    n = F * E * R
    iq, tissue = case(F, E, R)
    opts = mcrt.strain_opts_struct()
    eps = TABLES[0]
    eps_p = eps.ctypes.data_as(C.c_void_p)
    # one allocation, in floats: iq [0, 2n), then room for post (2n), truth_disp, truth_strain (n each) and sigma (F)
    TOTAL = 8 * n
    head = iq.reshape(-1)
    p_ti = dev.upload(tissue)

    def call(iq_=0, ti=p_ti, frames=F, lines=E, rows=R, eps_=eps_p, labels=N_LABELS, cyc=CARRIER, o=opts, first=0, sig=None,
             post=2 * n, td=4 * n, ts=5 * n, null_ctx=False):
        big = dev.upload(np.concatenate([head, np.full(TOTAL - 2 * n, SENTINEL)]))
        at = lambda floats: None if floats is None else C.c_void_p(big + 4 * floats)
        rc = L.mcrt_strain_compress_frames(None if null_ctx else ctx.h, at(iq_), None if ti is None else C.c_void_p(ti), frames, lines, rows, eps_, labels, cyc,
                                           None if o is None else C.byref(o), first, at(sig), at(post), at(td), at(ts))
        got = ctx.d2h(big, (TOTAL,))
        assert np.array_equal(got[:2 * n].view(np.uint32), head.view(np.uint32)) and (got[2 * n:] == SENTINEL).all()
        return rc

    assert call(null_ctx=True) == INVALID and call(iq_=None) == INVALID and call(ti=None) == INVALID and call(o=None) == INVALID and call(eps_=None) == INVALID
    assert call(frames=0) == INVALID and call(lines=0) == INVALID and call(rows=0) == INVALID and call(labels=0) == INVALID
    assert call(post=None, td=None, ts=None) == INVALID                                    # no output
    assert call(rows=2049, frames=1, lines=1) == LIMIT and call(labels=255) == LIMIT
    assert call(frames=1 << 11, lines=1 << 10, rows=1 << 10) == LIMIT                      # 2^31 samples
    assert call(first=0xFFFFFFFF) == LIMIT                                                 # the second frame's id would pass 2^32
    for cyc in (0.0, -0.1, 0.5000001, float("nan"), float("inf")):
        assert call(cyc=cyc) == INVALID
    for kw in (dict(window_rows=33), dict(search_rows=17), dict(lsq_rows=0), dict(lsq_rows=33), dict(sigma=-0.5), dict(sigma=float("nan"))):
        assert call(o=mcrt.strain_opts_struct(**kw)) == INVALID, kw
    for bad in (524289, -524289):
        e2 = eps.copy(); e2[1] = bad
        assert call(eps_=e2.ctypes.data_as(C.c_void_p)) == INVALID
    # overlaps: an output with an input, and two outputs with each other
    assert call(post=2 * n - 1) == INVALID and call(td=0) == INVALID and call(ts=n) == INVALID
    assert call(td=4 * n - 1) == INVALID and call(ts=5 * n - 1) == INVALID and call(ts=3 * n) == INVALID
    assert call(sig=4 * n) == INVALID and call(sig=2 * n + 1) == INVALID                   # sigma_dev inside truth_disp_dev, inside post_iq_dev
    tis = dev.upload(np.ones(4 * n, np.uint8))
    assert L.mcrt_strain_compress_frames(ctx.h, C.c_void_p(dev.upload(iq)), C.c_void_p(tis), F, E, R, eps_p, N_LABELS, CARRIER, C.byref(opts), 0, None,
                                         None, C.c_void_p(tis), None) == INVALID            # truth_disp_dev is tissue_dev


def test_track_refusals_leave_the_outputs_untouched(mcrt, ctx, dev):
    L = mcrt.load_library()
    F, E, R = 2, 3, 20
    n = F * E * R
    iq, tissue = case(F, E, R)
    post = sm.compress(iq, tissue, TABLES[0], CARRIER)["post"]
    opts = mcrt.strain_opts_struct()
    # one allocation, in floats: pre [0, 2n), post [2n, 4n), then room for disp, rho, strain (n each)
    TOTAL = 8 * n
    head = np.concatenate([iq.reshape(-1), post.reshape(-1)])

    def call(pre_=0, post_=2 * n, frames=F, lines=E, rows=R, o=opts, cyc=CARRIER, disp=4 * n, rho=5 * n, strain=6 * n, null_ctx=False):
        big = dev.upload(np.concatenate([head, np.full(TOTAL - 4 * n, SENTINEL)]))
        at = lambda floats: None if floats is None else C.c_void_p(big + 4 * floats)
        rc = L.mcrt_strain_frames(None if null_ctx else ctx.h, at(pre_), at(post_), frames, lines, rows, None if o is None else C.byref(o), cyc,
                                  at(disp), at(rho), at(strain))
        got = ctx.d2h(big, (TOTAL,))
        assert np.array_equal(got[:4 * n].view(np.uint32), head.view(np.uint32)) and (got[4 * n:] == SENTINEL).all()
        return rc

    assert call(null_ctx=True) == INVALID and call(pre_=None) == INVALID and call(post_=None) == INVALID and call(o=None) == INVALID
    assert call(frames=0) == INVALID and call(lines=0) == INVALID and call(rows=0) == INVALID
    assert call(disp=None, rho=None, strain=None) == INVALID                               # no output
    assert call(rows=2049, frames=1, lines=1) == LIMIT
    assert call(frames=1 << 11, lines=1 << 10, rows=1 << 10) == LIMIT                      # 2^31 samples
    for cyc in (0.0, -0.1, 0.5000001, float("nan"), float("inf")):
        assert call(cyc=cyc) == INVALID
    for kw in (dict(window_rows=33), dict(search_rows=17), dict(lsq_rows=0), dict(lsq_rows=33), dict(sigma=-0.5)):
        assert call(o=mcrt.strain_opts_struct(**kw)) == INVALID, kw
    assert call(disp=2 * n - 1) == INVALID and call(rho=0) == INVALID and call(strain=4 * n - 1) == INVALID      # an output with an input
    assert call(rho=5 * n - 1) == INVALID and call(strain=4 * n + 1) == INVALID and call(strain=5 * n) == INVALID  # two outputs


def test_calls_with_nothing_wrong_write(ctx, dev):
    """the refusal tests' shape with nothing wrong is accepted and writes every element: their sentinels are not kernels that do nothing"""
    iq, tissue = case(2, 3, 20)
    c = run_compress(ctx, dev, iq, tissue, TABLES[0])
    assert all((v != SENTINEL).all() for v in c.values())
    t = run_track(ctx, dev, iq, sm.compress(iq, tissue, TABLES[0], CARRIER)["post"])
    assert all((v != SENTINEL).all() for v in t.values())
