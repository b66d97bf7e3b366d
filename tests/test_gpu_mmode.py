"""M-mode on the MI355X: mcrt_mmode_lines_frames (k_mmode_lines) and mcrt_mmode_picture_frames (k_mmode_peak, k_mmode_picture) against the
numpy mirror (tests/mmode_mirror.py) -- every float and label output and mean_dev bit for bit, the picture's bytes within one level (the
device's log10f) -- at the shapes around a wavefront's 64 rows and a workgroup's 256, with pulse counts on either side of a workgroup's
chunk of 16 pulses, lines on the first, the last and a middle scan-line, two lines of one image and one line named twice, dilations of
both signs, labels inside the table, one past it and MCRT_LABEL_NONE in runs and strewn, a waveform that reaches +-65536, a bulk that
reaches +-32 rows, a case that saturates, noise from the options, from the device and none, special values beside speckle, every output
left out in turn, behind sentinels and off a 256-byte boundary; every hop, height and row window of the display; the refusals; and that
nothing is allocated after the first call at a size."""
import ctypes as C
import numpy as np
import pytest

import image_cases as ic
import mmode_mirror as mm

pytestmark = pytest.mark.gpu

f32 = np.float32
INVALID, LIMIT = -1, -5
SENTINEL = f32(-77.25)
BYTE = 0xA5                                                        # the sentinel of the byte outputs
CARRIER = 0.3475

SHAPES = [(1, 1, 1, 1), (1, 2, 3, 4), (2, 3, 63, 5), (1, 5, 65, 8), (1, 3, 130, 33), (2, 4, 465, 16), (1, 2, 2048, 4)]
DIL = mm.mmode_table([0.03, -0.05, 0.25])                          # label 1 widens; label 2 at the cap
N_LABELS = 3
LINE_OUT = ("env", "iq_out", "truth_disp", "truth_label")
PICTURE_OUT = ("peak", "mean", "label_out", "disp_out")


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


def speckle(F, E, R, seed=0):
    """finite speckle-like pairs: a carrier at CARRIER cycles per row under a smooth random envelope"""
    rng = np.random.default_rng(seed)
    b = rng.standard_normal((F, E, R + 6, 2))
    b = sum(b[:, :, i:i + R] for i in range(7)) / 7.0
    z = (b[..., 0] + 1j * b[..., 1]) * np.exp(2j * np.pi * CARRIER * np.arange(R))
    return np.stack([z.real, z.imag], axis=-1).astype(f32)


def case(F, E, R, seed=0):
    """(iq [F][E][R][2], tissue [F][E][R]): image_cases' scan-lines in both components (noise, ramps, saws, subnormals, infinities, NaN)
    with speckle on every other scan-line from the second on; labels of the three materials with one past the table and
    MCRT_LABEL_NONE strewn in, and every other scan-line in runs of one label, as anatomy has them"""
    iq = np.stack([np.stack([ic.envelope_image(E, R, seed=seed + 5 * f + c) for c in range(2)], axis=-1) for f in range(F)]).astype(f32)
    iq[:, 1::2] = speckle(F, E, R, seed)[:, 1::2]
    rng = np.random.default_rng(seed * 31 + F * 7 + E * 3 + R)
    labels = np.array([0, 1, 2, N_LABELS, 255], np.uint8)
    tissue = rng.choice(labels, size=(F, E, R), p=[0.46, 0.03, 0.45, 0.03, 0.03])
    for e in range(1, E, 2):
        tissue[:, e] = np.repeat(rng.choice(labels, size=(F, R // 37 + 1), p=[0.4, 0.1, 0.4, 0.05, 0.05]), 37, axis=1)[:, :R]
    return iq, tissue


def lines_of(F, E):
    """the first, the last and a middle scan-line; two lines of one image; one line named twice"""
    return np.array([(0, 0), (F - 1, E - 1), (0, E // 2), (F - 1, 0), (0, 0)], np.uint32)


def motion(T, seed=0, small=False):
    """(w_q16, bulk_q24) [T]: a waveform that reaches +65536 and -65536 and a bulk that reaches +32 and -32 rows where there are pulses for
    them, fractions elsewhere; small: a fraction of a row of bulk and a tenth of the waveform, so that the lines stay in view"""
    rng = np.random.default_rng(100 + seed + T)
    w = rng.integers(-65536, 65537, T).astype(np.int32); b = rng.integers(-(3 << 24), (3 << 24) + 1, T).astype(np.int32)
    if small:
        return (w // 10).astype(np.int32), (b // 8).astype(np.int32)
    w[0] = 65536; b[0] = 32 << 24
    if T > 1:
        w[T - 1] = -65536; b[1] = -(32 << 24)
    if T > 2:
        w[T // 2] = 0; b[T // 2] = 0
    return w, b


def run_lines(ctx, dev, iq, tissue, which, w, b, dil=DIL, outputs=LINE_OUT, sigma_from="opts", sigma=0.0, first_image_id=0, skew=0, tail=8, **opts):
    """the call -> (dict of the outputs asked for).  Every output starts as a sentinel, has `tail` sentinel elements behind it that must
    survive, and starts `skew` bytes off a 256-byte boundary, as the inputs do; the inputs must come back as they went"""
    F, E, R = tissue.shape
    m = len(which) * len(w) * R
    p_iq = dev.upload(iq, skew); p_ti = dev.upload(tissue, skew)
    sig = np.broadcast_to(np.asarray(sigma, f32), (F,)).copy()
    p_sig = dev.upload(sig, skew) if sigma_from == "dev" else None
    sizes = dict(env=m, iq_out=2 * m, truth_disp=m, truth_label=m)
    fill = lambda k: np.full(sizes[k] + tail, BYTE, np.uint8) if k == "truth_label" else np.full(sizes[k] + tail, SENTINEL)
    outs = {k: dev.upload(fill(k), skew) for k in outputs}
    kw = dict(opts)
    if sigma_from == "opts":
        assert np.all(sig == sig[0])
        kw["sigma"] = float(sig[0])
    ctx.mmode_lines_frames(p_iq, p_ti, F, E, R, which, dil, w, b, CARRIER, first_image_id=first_image_id, sigma_dev=p_sig,
                           **{k + "_dev": p for k, p in outs.items()}, **kw)
    got = {}
    shape = (len(which), len(w), R)
    for k, p in outs.items():
        if k == "truth_label":
            flat = ctx.d2h(p, (m + tail,), np.uint8)
            assert (flat[m:] == BYTE).all(), "the sentinel behind truth_label_dev was overwritten"
            got[k] = flat[:m].reshape(shape)
        else:
            flat = ctx.d2h(p, (sizes[k] + tail,))
            assert (flat[sizes[k]:] == SENTINEL).all(), "the sentinel behind %s_dev was overwritten" % k
            got[k] = flat[:sizes[k]].reshape(shape + (2,) if k == "iq_out" else shape)
    assert np.array_equal(ctx.d2h(p_iq, iq.shape).view(np.uint32), iq.view(np.uint32)), "iq_dev is read only"
    assert np.array_equal(ctx.d2h(p_ti, tissue.shape, np.uint8), tissue), "tissue_dev is read only"
    if p_sig is not None:
        assert np.array_equal(ctx.d2h(p_sig, (F,)).view(np.uint32), sig.view(np.uint32)), "sigma_dev is read only"
    return got


def check_lines(got, want, what):
    for k, v in got.items():
        if k == "truth_label":
            assert np.array_equal(v, want[k]), "truth_label %s: %d labels differ" % (what, int((v != want[k]).sum()))
        else:
            ic.assert_same_bits(v, want[k], "%s %s" % (k, what))


def run_picture(ctx, dev, env, label=None, disp=None, outputs=PICTURE_OUT, skew=0, tail=8, **opts):
    """the display call -> dict(out, and the optional outputs asked for), behind sentinels as run_lines' are"""
    n, T, R = env.shape
    hop, H = opts.get("hop", 4), opts.get("height", 400)
    W = T // hop
    p_env = dev.upload(env, skew)
    p_lab = dev.upload(label, skew) if label is not None else None
    p_dis = dev.upload(disp, skew) if disp is not None else None
    sizes = dict(out=n * H * W, peak=n, mean=n * W * R, label_out=n * H * W, disp_out=n * H * W)
    is_byte = lambda k: k in ("out", "label_out")
    fill = lambda k: np.full(sizes[k] + tail, BYTE, np.uint8) if is_byte(k) else np.full(sizes[k] + tail, SENTINEL)
    outs = {k: dev.upload(fill(k), skew) for k in ("out",) + tuple(outputs)}
    ctx.mmode_picture_frames(p_env, n, T, R, outs["out"], truth_label_dev=p_lab, truth_disp_dev=p_dis,
                             **{k + "_dev": p for k, p in outs.items() if k != "out"}, **opts)
    shapes = dict(out=(n, H, W), peak=(n,), mean=(n, W, R), label_out=(n, H, W), disp_out=(n, H, W))
    got = {}
    for k, p in outs.items():
        flat = ctx.d2h(p, (sizes[k] + tail,), np.uint8 if is_byte(k) else f32)
        assert (flat[sizes[k]:] == (BYTE if is_byte(k) else SENTINEL)).all(), "the sentinel behind %s_dev was overwritten" % k
        got[k] = flat[:sizes[k]].reshape(shapes[k])
    assert np.array_equal(ctx.d2h(p_env, env.shape).view(np.uint32), env.view(np.uint32)), "env_dev is read only"
    return got


def check_picture(got, want, what):
    for k, v in got.items():
        if k == "out":
            d = np.abs(v.astype(np.int32) - want[k].astype(np.int32))
            assert d.max() <= 1, "out %s: %d bytes differ by more than one level (largest %d)" % (what, int((d > 1).sum()), int(d.max()))
        elif k == "label_out":
            assert np.array_equal(v, want[k]), "label_out %s" % what
        else:
            ic.assert_same_bits(v, want[k], "%s %s" % (k, what))


def sigma_of(i, F):
    return (("opts", 0.0), ("opts", 0.375), ("dev", [0.5, 0.0][:F] if F == 2 else [0.25]))[i % 3]


# ------------------------------------------------------------------ the M-lines
@pytest.mark.parametrize("F,E,R,T", SHAPES)
def test_shapes_match_the_mirror(ctx, dev, F, E, R, T):
    """every shape, both calls: where sigma comes from rotates with the case; the display reads the mirror's lines, so that neither
    call's result depends on the other's"""
    i = SHAPES.index((F, E, R, T))
    iq, tissue = case(F, E, R, seed=i)
    which = lines_of(F, E)
    w, b = motion(T, seed=i)
    sigma_from, sigma = sigma_of(i, F)
    what = "F=%d E=%d R=%d T=%d sigma=%s from %s" % (F, E, R, T, sigma, sigma_from)
    want = mm.lines(iq, tissue, which, DIL, w, b, CARRIER, sigma=sigma, seed=11, first_image_id=5)
    check_lines(run_lines(ctx, dev, iq, tissue, which, w, b, sigma_from=sigma_from, sigma=sigma, first_image_id=5, seed=11), want, what)
    assert np.array_equal(want["env"][0].view(np.uint32), want["env"][4].view(np.uint32))             # the line named twice
    o = dict(hop=min(T, (1, 3, 2)[i % 3]), height=(1, 7, 400)[i % 3], row_lo=(0, R // 3)[i % 2], row_hi=(0, R // 3 + 1)[i % 2])
    pw = mm.picture(want["env"], want["truth_label"], want["truth_disp"], **o)
    check_picture(run_picture(ctx, dev, want["env"], want["truth_label"], want["truth_disp"], **o), pw, what + " display %s" % o)


def test_the_largest_line_saturates(ctx, dev):
    """R = 2048 under the largest dilation and waveform: the displacement passes 127 rows and stays there, on the device as in the mirror"""
    F, E, R, T = 1, 2, 2048, 4
    iq, tissue = case(F, E, R, seed=6)
    w, b = motion(T, seed=6)
    got = run_lines(ctx, dev, iq, tissue, [[0, 0], [0, 1]], w, b, outputs=("truth_disp", "truth_label"))
    check_lines(got, mm.lines(iq, tissue, [[0, 0], [0, 1]], DIL, w, b, CARRIER), "saturation")
    assert got["truth_disp"].max() == 127.0 and got["truth_disp"].min() == -127.0
    assert (got["truth_label"] == 255).any()                             # samples read from beyond the line's ends


@pytest.mark.parametrize("T", [15, 16, 17, 32, 33, 49])
def test_pulse_chunks(ctx, dev, T):
    """pulse counts on either side of a workgroup's 16 pulses: every pulse written once, none beyond the last"""
    F, E, R = 1, 3, 70
    iq, tissue = case(F, E, R, seed=T)
    w, b = motion(T, seed=T, small=True)
    want = mm.lines(iq, tissue, [[0, 1], [0, 2]], DIL, w, b, CARRIER, sigma=0.125)
    check_lines(run_lines(ctx, dev, iq, tissue, [[0, 1], [0, 2]], w, b, sigma=0.125), want, "T=%d" % T)


def test_most_pulses(ctx, dev):
    F, E, R, T = 1, 1, 5, 16384
    iq, tissue = case(F, E, R, seed=2)
    iq[0, 0] = speckle(1, 1, R, seed=2)[0, 0]
    w, b = mm.waveform(1000.0, 72.0, T), mm.bulk(1000.0, 15.0, 1.5, T)
    check_lines(run_lines(ctx, dev, iq, tissue, [[0, 0]], w, b, sigma=0.25), mm.lines(iq, tissue, [[0, 0]], DIL, w, b, CARRIER, sigma=0.25), "T=16384")


def test_defaults(ctx, dev):
    """no options: sigma 0 and the default seed; the display's defaults: hop 4, 400 rows of the whole line, 60 dB, each line's own peak"""
    F, E, R, T = 1, 4, 130, 24
    iq, tissue = case(F, E, R)
    w, b = motion(T, small=True)
    want = mm.lines(iq, tissue, [[0, 1], [0, 3]], DIL, w, b, CARRIER)
    check_lines(run_lines(ctx, dev, iq, tissue, [[0, 1], [0, 3]], w, b), want, "defaults")
    noisy = mm.lines(iq, tissue, [[0, 1]], DIL, w, b, CARRIER, sigma=0.5)
    check_lines(run_lines(ctx, dev, iq, tissue, [[0, 1]], w, b, sigma=0.5, outputs=("env",)), noisy, "the default seed")
    check_picture(run_picture(ctx, dev, want["env"], want["truth_label"], want["truth_disp"]),
                  mm.picture(want["env"], want["truth_label"], want["truth_disp"]), "defaults")


@pytest.mark.parametrize("sigma_from,sigma", [("opts", 0.0), ("opts", 0.75), ("dev", [0.0, 1.5]), ("dev", [0.125, 0.125])])
def test_sigma(ctx, dev, sigma_from, sigma):
    """sigma 0 and > 0 from the options and from the device -- a line of an image with sigma 0 beside one with noise; ids at the end of their range"""
    iq, tissue = case(2, 3, 63, seed=4)
    which = [[0, 1], [1, 1], [1, 2]]
    w, b = motion(8, seed=4, small=True)
    want = mm.lines(iq, tissue, which, DIL, w, b, CARRIER, sigma=sigma, first_image_id=0xFFFFFFFE)
    check_lines(run_lines(ctx, dev, iq, tissue, which, w, b, sigma_from=sigma_from, sigma=sigma, first_image_id=0xFFFFFFFE), want, "sigma=%s from %s" % (sigma, sigma_from))


@pytest.mark.parametrize("left_out", LINE_OUT)
def test_each_line_output_left_out(ctx, dev, left_out):
    iq, tissue = case(2, 5, 65, seed=3)
    which = lines_of(2, 5)
    w, b = motion(6, seed=3, small=True)
    want = mm.lines(iq, tissue, which, DIL, w, b, CARRIER, sigma=0.25)
    outputs = tuple(k for k in LINE_OUT if k != left_out)
    got = run_lines(ctx, dev, iq, tissue, which, w, b, outputs=outputs, sigma=0.25)
    assert sorted(got) == sorted(outputs)
    check_lines(got, want, "without " + left_out)
    check_lines(run_lines(ctx, dev, iq, tissue, which, w, b, outputs=(left_out,), sigma=0.25), want, "only " + left_out)


@pytest.mark.parametrize("skew", [4, 8, 12, 1])
def test_pointers_off_a_256_byte_boundary(ctx, dev, skew):
    """(the byte outputs at any offset; the float buffers at multiples of 4)"""
    iq, tissue = case(1, 5, 65, seed=skew)
    w, b = motion(8, seed=skew, small=True)
    want = mm.lines(iq, tissue, [[0, 1], [0, 4]], DIL, w, b, CARRIER, sigma=[0.5])
    if skew % 4:
        F, E, R = tissue.shape
        p_iq = dev.upload(iq); p_ti = dev.upload(tissue, skew)
        p_lab = dev.upload(np.full(2 * 8 * R + 8, BYTE, np.uint8), skew)
        ctx.mmode_lines_frames(p_iq, p_ti, F, E, R, [[0, 1], [0, 4]], DIL, w, b, CARRIER, truth_label_dev=p_lab)
        flat = ctx.d2h(p_lab, (2 * 8 * R + 8,), np.uint8)
        assert (flat[2 * 8 * R:] == BYTE).all() and np.array_equal(flat[:2 * 8 * R].reshape(2, 8, R), want["truth_label"])
        return
    check_lines(run_lines(ctx, dev, iq, tissue, [[0, 1], [0, 4]], w, b, sigma_from="dev", sigma=[0.5], skew=skew), want, "skew %d" % skew)
    o = dict(hop=3, height=7)
    check_picture(run_picture(ctx, dev, want["env"], want["truth_label"], want["truth_disp"], skew=skew, **o),
                  mm.picture(want["env"], want["truth_label"], want["truth_disp"], **o), "skew %d" % skew)


def test_labels_that_do_not_move(ctx, dev):
    """a label past the table and MCRT_LABEL_NONE add nothing to the displacement; a line of them alone stays where it is"""
    F, E, R, T = 1, 2, 40, 3
    iq = speckle(F, E, R, seed=9)
    tissue = np.full((F, E, R), 255, np.uint8); tissue[0, 0, ::2] = N_LABELS; tissue[0, 1, :20] = 1
    w = np.array([65536, -65536, 30000], np.int32); b = np.zeros(T, np.int32)
    got = run_lines(ctx, dev, iq, tissue, [[0, 0], [0, 1]], w, b)
    check_lines(got, mm.lines(iq, tissue, [[0, 0], [0, 1]], DIL, w, b, CARRIER), "labels that do not move")
    assert not got["truth_disp"][0].view(np.uint32).any() and np.array_equal(got["iq_out"][0, 0], iq[0, 0])
    assert (got["truth_disp"][1, 0, 20:] == got["truth_disp"][1, 0, 20]).all() and got["truth_disp"][1, 0, 20] < 0


def test_tables_are_replaced_when_they_change(ctx, dev):
    """the host tables live in the context and are copied only when they differ: other values, then shorter and longer tables"""
    iq, tissue = case(1, 4, 33, seed=2)
    w, b = motion(8, seed=1, small=True)
    w2, b2 = motion(5, seed=2, small=True)
    variants = [dict(), dict(dil=mm.mmode_table([0.01])), dict(dil=mm.mmode_table([0.0, 0.1, -0.1, 0.2, 0.05])), dict(w=w2, b=b2), dict(which=[[0, 3]]),
                dict(which=[[0, 0], [0, 1], [0, 2], [0, 3]]), dict(b=np.zeros(8, np.int32)), dict()]
    for v in variants:
        a = dict(dict(which=[[0, 1], [0, 2]], w=w, b=b, dil=DIL), **v)
        got = run_lines(ctx, dev, iq, tissue, a["which"], a["w"], a["b"], dil=a["dil"])
        check_lines(got, mm.lines(iq, tissue, a["which"], a["dil"], a["w"], a["b"], CARRIER), "tables %s" % sorted(v))


def test_no_motion_is_the_identity_on_the_device(ctx, dev):
    """on the device: with all dilations 0, no bulk and no noise every pulse's line is the traced line and its envelope"""
    F, E, R, T = 2, 3, 200, 6
    iq = speckle(F, E, R, seed=1)
    tissue = np.random.default_rng(0).choice(np.array([0, 1, N_LABELS, 255], np.uint8), size=(F, E, R))
    got = run_lines(ctx, dev, iq, tissue, [[1, 2]], motion(T)[0], np.zeros(T, np.int32), dil=np.zeros(3, np.int32))
    re, im = iq[1, 2, :, 0], iq[1, 2, :, 1]
    env = np.sqrt(((re * re).astype(f32) + (im * im).astype(f32)).astype(f32)).astype(f32)
    for t in range(T):
        assert np.array_equal(got["env"][0, t].view(np.uint32), env.view(np.uint32)) and np.array_equal(got["iq_out"][0, t], iq[1, 2])
        assert np.array_equal(got["truth_label"][0, t], tissue[1, 2])
    assert not got["truth_disp"].view(np.uint32).any()


# ------------------------------------------------------------------ the display
def sweep(n, T, R, seed=0):
    """(env, truth_label, truth_disp) of the display's own: envelopes of several decades with zeros, subnormals, NaN and infinities strewn in"""
    rng = np.random.default_rng(seed + 17 * T + R)
    env = (np.abs(rng.standard_normal((n, T, R))) * 10.0 ** rng.uniform(-4, 1, (n, T, R))).astype(f32)
    for v, share in ((0.0, 0.05), (1e-41, 0.01), (np.nan, 0.01), (np.inf, 0.005)):
        env[rng.random((n, T, R)) < share] = v
    return env, rng.integers(0, 256, (n, T, R)).astype(np.uint8), rng.standard_normal((n, T, R)).astype(f32)


@pytest.mark.parametrize("H", [1, 7, 400])
@pytest.mark.parametrize("hop", [1, 3, 12])
def test_hops_and_heights(ctx, dev, hop, H):
    """hop 1, 3 and T (one column), with a last partial column to drop at 3 when T is 13"""
    n, T, R = 2, 12 if hop != 3 else 13, 130
    env, lab, dis = sweep(n, T, R, seed=hop + H)
    o = dict(hop=hop, height=H, dynamic_range_db=(60.0, 40.0)[H % 2], gain_db=(0.0, 6.0)[hop % 2])
    check_picture(run_picture(ctx, dev, env, lab, dis, **o), mm.picture(env, lab, dis, **o), "hop %d H %d" % (hop, H))


@pytest.mark.parametrize("lo,hi", [(0, 0), (0, 300), (0, 1), (299, 300), (150, 151), (7, 264), (64, 128)])
def test_row_windows(ctx, dev, lo, hi):
    """from the whole line down to a window of one row, at the line's ends and across the rows where a wavefront ends"""
    n, T, R = 1, 8, 300
    env, lab, dis = sweep(n, T, R, seed=lo)
    for H in (5, 300):
        o = dict(hop=2, height=H, row_lo=lo, row_hi=hi)
        got = run_picture(ctx, dev, env, lab, dis, **o)
        check_picture(got, mm.picture(env, lab, dis, **o), "rows [%d, %d) H %d" % (lo, hi, H))


def test_the_widest_line_and_the_tallest_picture(ctx, dev):
    n, T, R = 1, 4, 2048
    env, lab, dis = sweep(n, T, R)
    o = dict(hop=2, height=4096)
    check_picture(run_picture(ctx, dev, env, lab, dis, **o), mm.picture(env, lab, dis, **o), "R 2048 H 4096")


@pytest.mark.parametrize("ref", [0.0, 2.5, -1.0])
def test_ref_and_peak(ctx, dev, ref):
    """a ref of the caller's own and each line's peak (ref 0 or below); peak_dev is the line's largest mean whatever ref is; a line of
    nothing that counts is black and has a peak of 0"""
    n, T, R = 3, 6, 70
    env, lab, dis = sweep(n, T, R, seed=5)
    env[1] = np.where(np.isfinite(env[1]), f32(0.0), env[1])             # zeros, NaN and infinities alone
    o = dict(hop=2, height=33, ref=ref, row_lo=3, row_hi=60)
    want = mm.picture(env, lab, dis, **o)
    got = run_picture(ctx, dev, env, lab, dis, **o)
    check_picture(got, want, "ref %g" % ref)
    assert got["peak"][1] == 0.0 and not got["out"][1].any() and got["peak"][0] > 0
    for outputs in ((), ("peak",), ("mean",)):                           # without a peak_dev the peaks are the context's
        check_picture(run_picture(ctx, dev, env, outputs=outputs, **o), want, "ref %g outputs %s" % (ref, outputs))


@pytest.mark.parametrize("left_out", PICTURE_OUT)
def test_each_picture_output_left_out(ctx, dev, left_out):
    n, T, R = 2, 9, 65
    env, lab, dis = sweep(n, T, R, seed=8)
    o = dict(hop=2, height=50)
    want = mm.picture(env, lab, dis, **o)
    outputs = tuple(k for k in PICTURE_OUT if k != left_out)
    truths = dict(label=None if left_out == "label_out" else lab, disp=None if left_out == "disp_out" else dis)
    got = run_picture(ctx, dev, env, outputs=outputs, **truths, **o)
    assert sorted(got) == sorted(outputs + ("out",))
    check_picture(got, want, "without " + left_out)


def test_nothing_is_allocated_after_the_first_call_at_a_size(ctx, dev):
    """the tables and the peaks live in grow-only buffers of the context: the device's free memory stays where the first call left it"""
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(), C.c_size_t()

    def free_bytes():
        ctx.synchronize()
        assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
        return free.value

    F, E, R, T, H = 2, 7, 300, 24, 100
    iq, tissue = case(F, E, R)
    which = lines_of(F, E)
    w, b = motion(T, small=True)
    m = len(which) * T * R
    p_iq = dev.upload(iq); p_ti = dev.upload(tissue)
    env, lab, dis, out = dev(4 * m), dev(m), dev(4 * m), dev(len(which) * H * (T // 4))
    call = lambda: (ctx.mmode_lines_frames(p_iq, p_ti, F, E, R, which, DIL, w, b, CARRIER, env_dev=env, truth_label_dev=lab, truth_disp_dev=dis, sigma=0.1),
                    ctx.mmode_picture_frames(env, len(which), T, R, out, height=H))
    call()
    before = free_bytes()
    for _ in range(3):
        call()
    assert free_bytes() == before


# ------------------------------------------------------------------ the refusals
def test_lines_refusals_leave_the_outputs_untouched(mcrt, ctx, dev):
    L = mcrt.load_library()
    F, E, R, T = 2, 3, 20, 4
    n, nl = F * E * R, 3
    m = nl * T * R
    iq, tissue = case(F, E, R)
    which = np.array([(0, 0), (1, 2), (0, 1)], np.uint32)
    w, b = motion(T)
    opts = lambda **kw: mcrt.mmode_opts_struct(**dict(dict(n_pulses=T), **kw))
    hp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    # one allocation, in floats: iq [0, 2n), then room for env (m), iq_out (2 m), truth_disp (m), truth_label (m bytes in m floats) and sigma (F)
    TOTAL = 2 * n + 5 * m + F
    head = iq.reshape(-1)
    p_ti = dev.upload(tissue)

    def call(iq_=0, ti=p_ti, frames=F, lines=E, rows=R, ln=which, n_lines=nl, dil=DIL, labels=N_LABELS, w_=w, b_=b, cyc=CARRIER, o=opts(), first=0, sig=None,
             env=2 * n, io=2 * n + m, td=2 * n + 3 * m, tl=2 * n + 4 * m, null_ctx=False):
        big = dev.upload(np.concatenate([head, np.full(TOTAL - 2 * n, SENTINEL)]))
        at = lambda floats: None if floats is None else C.c_void_p(big + 4 * floats)
        rc = L.mcrt_mmode_lines_frames(None if null_ctx else ctx.h, at(iq_), None if ti is None else C.c_void_p(ti), frames, lines, rows, hp(ln), n_lines, hp(dil), labels,
                                       hp(w_), hp(b_), cyc, None if o is None else C.byref(o), first, at(sig), at(env), at(io), at(td), at(tl))
        got = ctx.d2h(big, (TOTAL,))
        assert np.array_equal(got[:2 * n].view(np.uint32), head.view(np.uint32)) and (got[2 * n:] == SENTINEL).all()
        return rc

    assert call(null_ctx=True) == INVALID and call(iq_=None) == INVALID and call(ti=None) == INVALID and call(o=None) == INVALID
    for k in ("ln", "dil", "w_", "b_"):
        assert call(**{k: None}) == INVALID, k
    assert call(frames=0) == INVALID and call(lines=0) == INVALID and call(rows=0) == INVALID and call(labels=0) == INVALID and call(n_lines=0) == INVALID
    assert call(env=None, io=None, td=None, tl=None) == INVALID                            # no output
    for cyc in (0.0, -0.1, 0.5000001, float("nan"), float("inf")):
        assert call(cyc=cyc) == INVALID
    for kw in (dict(n_pulses=0), dict(n_pulses=16385), dict(sigma=-0.5), dict(sigma=float("nan")), dict(sigma=float("inf"))):
        assert call(o=opts(**kw)) == INVALID, kw
    for bad in ((F, 0), (0, E), (0xFFFFFFFF, 0)):
        ln = which.copy(); ln[2] = bad
        assert call(ln=ln) == INVALID, bad
    for v in (4194305, -4194305):
        bad = DIL.copy(); bad[1] = v
        assert call(dil=bad) == INVALID
    for v in (65537, -65537):
        bad = w.copy(); bad[T - 1] = v
        assert call(w_=bad) == INVALID
    for v in ((32 << 24) + 1, -(32 << 24) - 1):
        bad = b.copy(); bad[T - 1] = v
        assert call(b_=bad) == INVALID
    assert call(rows=2049, frames=1, lines=1, ln=np.zeros((3, 2), np.uint32)) == LIMIT and call(labels=255, dil=np.zeros(255, np.int32)) == LIMIT
    assert call(n_lines=65536, ln=np.zeros((65536, 2), np.uint32)) == LIMIT
    assert call(frames=1 << 11, lines=1 << 10, rows=1 << 10) == LIMIT                      # a stack of 2^31 samples
    T2 = 16384
    assert call(n_lines=128, ln=np.zeros((128, 2), np.uint32), rows=1024, frames=1, lines=1, o=opts(n_pulses=T2), w_=np.zeros(T2, np.int32),
                b_=np.zeros(T2, np.int32)) == LIMIT                                        # 128 x 16384 x 1024 = 2^31 outputs
    assert call(first=0xFFFFFFFF) == LIMIT                                                 # the second frame's id would pass 2^32
    # overlaps: an output with an input, and two outputs with each other
    assert call(env=2 * n - 1) == INVALID and call(io=0) == INVALID and call(td=n) == INVALID and call(tl=2 * n - 1) == INVALID
    assert call(io=2 * n + m - 1) == INVALID and call(td=2 * n + 3 * m - 1) == INVALID and call(tl=2 * n + 4 * m - 1) == INVALID and call(td=2 * n + 1) == INVALID
    assert call(sig=2 * n + m) == INVALID and call(sig=2 * n + 1) == INVALID               # sigma_dev inside iq_out_dev, inside env_dev
    tis = dev.upload(np.ones(4 * m, np.uint8))
    o = opts()
    assert L.mcrt_mmode_lines_frames(ctx.h, C.c_void_p(dev.upload(iq)), C.c_void_p(tis), F, E, R, hp(which), nl, hp(DIL), N_LABELS, hp(w), hp(b), CARRIER, C.byref(o), 0,
                                     None, None, None, None, C.c_void_p(tis)) == INVALID    # truth_label_dev is tissue_dev


def test_picture_refusals_leave_the_outputs_untouched(mcrt, ctx, dev):
    L = mcrt.load_library()
    nl, T, R, H, hop = 2, 8, 20, 10, 2
    W = T // hop
    m, px = nl * T * R, nl * H * W
    env, lab, dis = sweep(nl, T, R)
    opts = lambda **kw: mcrt.mmode_display_opts_struct(**dict(dict(hop=hop, height=H), **kw))
    # one allocation, in floats: env [0, m), truth_disp [m, 2m), then room for peak (nl), mean (nl W R), out (px bytes in px floats), label_out (px), disp_out (px)
    TOTAL = 2 * m + nl + nl * W * R + 3 * px
    head = np.concatenate([env.reshape(-1), dis.reshape(-1)])
    p_lab = dev.upload(lab)
    base = 2 * m

    def call(env_=0, la=p_lab, di=m, lines=nl, pulses=T, rows=R, o=opts(), pk=base, mn=base + nl, out=base + nl + nl * W * R, lo=base + nl + nl * W * R + px,
             do=base + nl + nl * W * R + 2 * px, null_ctx=False):
        big = dev.upload(np.concatenate([head, np.full(TOTAL - 2 * m, SENTINEL)]))
        at = lambda floats: None if floats is None else C.c_void_p(big + 4 * floats)
        rc = L.mcrt_mmode_picture_frames(None if null_ctx else ctx.h, at(env_), None if la is None else C.c_void_p(la), at(di), lines, pulses, rows,
                                         None if o is None else C.byref(o), at(pk), at(mn), at(out), at(lo), at(do))
        got = ctx.d2h(big, (TOTAL,))
        assert np.array_equal(got[:2 * m].view(np.uint32), head.view(np.uint32)) and (got[2 * m:] == SENTINEL).all()
        return rc

    assert call(null_ctx=True) == INVALID and call(env_=None) == INVALID and call(o=None) == INVALID and call(out=None) == INVALID
    assert call(lines=0) == INVALID and call(pulses=0) == INVALID and call(rows=0) == INVALID
    assert call(la=None) == INVALID and call(di=None) == INVALID                           # a truth's picture without the truth
    for kw in (dict(hop=0), dict(hop=T + 1), dict(height=0), dict(height=4097), dict(row_lo=R), dict(row_lo=5, row_hi=5), dict(row_lo=6, row_hi=5), dict(row_hi=R + 1),
               dict(dynamic_range_db=0.0), dict(dynamic_range_db=-60.0), dict(dynamic_range_db=float("nan")), dict(dynamic_range_db=float("inf")),
               dict(gain_db=float("nan")), dict(gain_db=float("inf")), dict(ref=float("nan")), dict(ref=float("inf"))):
        assert call(o=opts(**kw)) == INVALID, kw
    assert call(rows=2049, lines=1, pulses=2) == LIMIT and call(pulses=16385, lines=1, rows=1) == LIMIT and call(lines=65536, pulses=2, rows=1) == LIMIT
    assert call(lines=128, pulses=16384, rows=1024) == LIMIT                               # 2^31 samples
    assert call(lines=32768, pulses=16384, rows=2, o=opts(hop=1, height=4096)) == LIMIT    # pictures of 2^31 pixels or more
    # overlaps: an output with an input, and two outputs with each other
    assert call(pk=m - 1) == INVALID and call(mn=0) == INVALID and call(out=2 * m - 1) == INVALID and call(lo=m) == INVALID and call(do=1) == INVALID
    assert call(mn=base) == INVALID and call(out=base + nl) == INVALID and call(lo=base + nl + nl * W * R) == INVALID and call(do=base + nl + nl * W * R + px) == INVALID
    assert L.mcrt_mmode_picture_frames(ctx.h, C.c_void_p(dev.upload(env)), C.c_void_p(p_lab), None, nl, T, R, C.byref(opts()), None, None, C.c_void_p(p_lab), None,
                                       None) == INVALID                                    # out_dev is truth_label_dev


def test_calls_with_nothing_wrong_write(ctx, dev):
    """the refusal tests' shapes with nothing wrong are accepted and write every element: their sentinels are not kernels that do nothing"""
    iq, tissue = case(2, 3, 20)
    w, b = motion(4)
    got = run_lines(ctx, dev, iq, tissue, [[0, 0], [1, 2], [0, 1]], w, b, sigma=0.5)
    assert all((v != SENTINEL).all() for k, v in got.items() if k != "truth_label")
    env, lab, dis = sweep(2, 8, 20)
    pic = run_picture(ctx, dev, np.where(np.isnan(env), f32(1.0), env), lab, dis, hop=2, height=10)
    assert all((v != SENTINEL).all() for k, v in pic.items() if k in ("peak", "mean", "disp_out"))
