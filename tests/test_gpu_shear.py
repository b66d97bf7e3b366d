"""Shear-wave elastography on the MI355X: mcrt_shear_wave_frames (k_shear_arrival, k_shear_track) and mcrt_shear_speed_frames
(k_shear_speed) against the numpy mirror (tests/shear_mirror.py) bit for bit -- at the shapes around a wavefront's 64 rows, for the
smallest, the default and the largest windows, pushes on the first, the last and a middle scan-line over rows that start at 0, end at R
and straddle a tile's 64th row, with and without noise from the options and from the device, on special values and speckle, labels
inside the table, one past it, MCRT_LABEL_NONE and a fluid, with every output left out in turn, behind sentinels and at every alignment;
the refusals; and that nothing is allocated after the first call at a size."""
import ctypes as C
import numpy as np
import pytest

import image_cases as ic
import shear_mirror as sh

pytestmark = pytest.mark.gpu

f32 = np.float32
INVALID, LIMIT = -1, -5
SENTINEL = f32(-77.25)
CARRIER = 0.3475

SHAPES = [(1, 1, 1, 4), (1, 2, 3, 4), (2, 3, 63, 5), (1, 5, 65, 8), (1, 9, 130, 32), (2, 4, 465, 16), (1, 2, 2048, 4)]
WINDOWS = [0, 1, 8, 16]
SPEEDS = [2.0, 0.0, 3.5]                                          # label 1 is a fluid
N_LABELS = 3
WAVE_OUT = ("peak_time", "peak_disp", "disp", "truth_arrival", "truth_speed")
SPEED_OUT = ("speed", "modulus", "quality")


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
    ph = 2.0 * np.pi * CARRIER * np.arange(R)
    z = (b[..., 0] + 1j * b[..., 1]) * np.exp(1j * ph)
    return np.stack([z.real, z.imag], axis=-1).astype(f32)


def case(F, E, R, seed=0):
    """(iq [F][E][R][2], tissue [F][E][R]): image_cases' scan-lines in both components (noise, ramps, saws, subnormals, infinities, NaN)
    with speckle on every other scan-line from the second on; labels mostly of the two materials the wave passes, with a fluid, one
    past the table and MCRT_LABEL_NONE strewn in, and every other scan-line in runs of one label, as anatomy has them"""
    iq = np.stack([np.stack([ic.envelope_image(E, R, seed=seed + 5 * f + c) for c in range(2)], axis=-1) for f in range(F)]).astype(f32)
    iq[:, 1::2] = speckle(F, E, R, seed)[:, 1::2]
    rng = np.random.default_rng(seed * 31 + F * 7 + E * 3 + R)
    labels = np.array([0, 1, 2, N_LABELS, 255], np.uint8)
    tissue = rng.choice(labels, size=(F, E, R), p=[0.46, 0.03, 0.45, 0.03, 0.03])
    for e in range(1, E, 2):
        tissue[:, e] = np.repeat(rng.choice(labels, size=(F, R // 37 + 1), p=[0.4, 0.1, 0.4, 0.05, 0.05]), 37, axis=1)[:, :R]
    return iq, tissue


def tables(E, R, T):
    """the host tables of a case: the speeds at 10 kHz, the pitch of a 128-line sector at R rows, a raised cosine of about a third of
    the pulses and the default decay"""
    slow, spf = sh.shear_table(SPEEDS, 10000.0)
    pitch_q8, pitch_mm = sh.shear_pitch(128, R, 30.0, 1.0471975511965976)
    return dict(slow_q16=slow, speed_f=spf, pitch_q8=pitch_q8, shape_q16=sh.shear_shape(max(2, T // 3)), amp_q16=sh.shear_decay(E, 8.0)), pitch_mm


def pushes(E, R):
    """(push_line, push_row0, push_rows): the first, the last and a middle line; rows that start at 0, end at R (push_rows 0 and
    spelled out) and straddle the 64th row of a tile where there is one"""
    rows = [(0, max(1, R // 2)), (R // 3, 0), (R // 3, R - R // 3)]
    if R > 70:
        rows.append((60, 10))
    return [(line, r0, n) for line in sorted({0, E - 1, E // 2}) for (r0, n) in rows]


def run_wave(ctx, dev, iq, tissue, tab, outputs=WAVE_OUT, sigma_from="opts", sigma=0.0, first_image_id=0, skew=0, tail=8, **opts):
    """the call -> (dict of the outputs asked for).  Every output starts as a sentinel, has `tail` sentinel floats behind it that must
    survive, and starts `skew` bytes off a 256-byte boundary, as the inputs do; the inputs must come back as they went"""
    F, E, R = tissue.shape
    n = F * E * R
    T = opts.get("n_pulses", 64)
    p_iq = dev.upload(iq, skew); p_ti = dev.upload(tissue, skew)
    sig = np.broadcast_to(np.asarray(sigma, f32), (F,)).copy()
    p_sig = dev.upload(sig, skew) if sigma_from == "dev" else None
    sizes = dict(peak_time=n, peak_disp=n, disp=n * T, truth_arrival=n, truth_speed=n)
    outs = {k: dev.upload(np.full(sizes[k] + tail, SENTINEL), skew) for k in outputs}
    kw = dict(opts)
    if sigma_from == "opts":
        assert np.all(sig == sig[0])
        kw["sigma"] = float(sig[0])
    ctx.shear_wave_frames(p_iq, p_ti, F, E, R, cycles_per_row=CARRIER, first_image_id=first_image_id, sigma_dev=p_sig,
                          **tab, **{k + "_dev": p for k, p in outs.items()}, **kw)
    got = {}
    for k, p in outs.items():
        flat = ctx.d2h(p, (sizes[k] + tail,))
        assert (flat[sizes[k]:] == SENTINEL).all(), "the sentinel behind %s_dev was overwritten" % k
        got[k] = flat[:sizes[k]].reshape((F, T, E, R) if k == "disp" else (F, E, R))
    assert np.array_equal(ctx.d2h(p_iq, iq.shape).view(np.uint32), iq.view(np.uint32)), "iq_dev is read only"
    assert np.array_equal(ctx.d2h(p_ti, tissue.shape, np.uint8), tissue), "tissue_dev is read only"
    if p_sig is not None:
        assert np.array_equal(ctx.d2h(p_sig, (F,)).view(np.uint32), sig.view(np.uint32)), "sigma_dev is read only"
    return got


def run_speed(ctx, dev, peak_time, pitch_mm, outputs=SPEED_OUT, skew=0, tail=8, **opts):
    F, E, R = peak_time.shape
    n = F * E * R
    p_pt = dev.upload(peak_time, skew)
    outs = {k: dev.upload(np.full(n + tail, SENTINEL), skew) for k in outputs}
    ctx.shear_speed_frames(p_pt, F, E, R, pitch_mm, **{k + "_dev": p for k, p in outs.items()}, **opts)
    got = {}
    for k, p in outs.items():
        flat = ctx.d2h(p, (n + tail,))
        assert (flat[n:] == SENTINEL).all(), "the sentinel behind %s_dev was overwritten" % k
        got[k] = flat[:n].reshape(F, E, R)
    assert np.array_equal(ctx.d2h(p_pt, peak_time.shape).view(np.uint32), peak_time.view(np.uint32)), "peak_time_dev is read only"
    return got


def check(got, want, what):
    for k, v in got.items():
        ic.assert_same_bits(v, want[k], "%s %s" % (k, what))


def sigma_of(i, F):
    return (("opts", 0.0), ("opts", 0.375), ("dev", [0.5, 0.0][:F] if F == 2 else [0.25]))[i % 3]


def peak_times(F, E, R, seed=0):
    """an input of the speed call of its own: arrival-like ramps away from line E // 2 with jitter, NaN strewn in and a few infinities"""
    rng = np.random.default_rng(seed + E * 13 + R)
    pt = (1.3 * np.abs(np.arange(E) - E // 2)[None, :, None] + rng.normal(0.0, 0.2, (F, E, R))).astype(f32)
    pt[rng.random((F, E, R)) < 0.08] = np.nan
    pt[rng.random((F, E, R)) < 0.005] = np.inf
    return pt


@pytest.mark.parametrize("a", WINDOWS)
@pytest.mark.parametrize("F,E,R,T", SHAPES)
def test_shapes_match_the_mirror(ctx, dev, F, E, R, T, a):
    """every shape x window, both calls: the push, where sigma comes from and the peak's sign rotate with the case; the speed call reads
    the mirror's peak times, so that neither call's result depends on the other's"""
    i = SHAPES.index((F, E, R, T)) + WINDOWS.index(a)
    ps = pushes(E, R)
    line, row0, rows = ps[(5 * i + a) % len(ps)]
    sigma_from, sigma = sigma_of(i, F)
    iq, tissue = case(F, E, R, seed=a)
    tab, pitch_mm = tables(E, R, T)
    o = dict(n_pulses=T, window_rows=a, push_line=line, push_row0=row0, push_rows=rows, peak_q24=(1677722, -3000000, 8388608)[i % 3], seed=11)
    what = "F=%d E=%d R=%d T=%d a=%d push=%s sigma=%s from %s" % (F, E, R, T, a, (line, row0, rows), sigma, sigma_from)
    want = sh.wave(iq, tissue, cycles_per_row=CARRIER, sigma=sigma, first_image_id=5, **tab, **o)
    check(run_wave(ctx, dev, iq, tissue, tab, sigma_from=sigma_from, sigma=sigma, first_image_id=5, **o), want, what)
    so = dict(push_line=line, speed_lines=1 + i % 2, avg_rows=(0, 2, 16)[i % 3], prf_hz=(10000.0, 7000.0)[i % 2], density=(1.0, 1.06)[i % 2])
    for pt in (want["peak_time"], peak_times(F, E, R, seed=a)):
        check(run_speed(ctx, dev, pt, pitch_mm, **so), sh.speed(pt, pitch_mm, **so), what + " speed %s" % so)


@pytest.mark.parametrize("line,row0,rows", pushes(9, 130))
def test_every_push(ctx, dev, line, row0, rows):
    """speckle under a real wave at every push line and row range: the wave arrives, peaks inside the observation and is found"""
    F, E, R, T = 1, 9, 130, 32
    iq = speckle(F, E, R, seed=line + row0)
    tissue = np.zeros((F, E, R), np.uint8); tissue[:, :, R // 2:] = 2
    tab, pitch_mm = tables(E, R, T)
    tab["shape_q16"] = sh.shear_shape(6)
    o = dict(n_pulses=T, push_line=line, push_row0=row0, push_rows=rows)
    want = sh.wave(iq, tissue, cycles_per_row=CARRIER, sigma=0.01, **tab, **o)
    check(run_wave(ctx, dev, iq, tissue, tab, sigma=0.01, **o), want, "push %s" % ((line, row0, rows),))
    assert np.isfinite(want["peak_time"]).sum() > 20                     # the case has peaks to find
    so = dict(push_line=line, speed_lines=1, avg_rows=1)
    s = sh.speed(want["peak_time"], pitch_mm, **so)
    check(run_speed(ctx, dev, want["peak_time"], pitch_mm, **so), s, "push %s speed" % ((line, row0, rows),))
    assert (s["quality"] > 0).any()


@pytest.mark.parametrize("b", [1, 16])
def test_windows_wider_than_the_image(ctx, dev, b):
    """E < 2 b + 1: the window is not clipped, so every sample is NaN with quality 0"""
    E = 2 * b
    pt = peak_times(1, E, 70, seed=b)
    got = run_speed(ctx, dev, pt, sh.shear_pitch(128, 70, 30.0, 1.0)[1], push_line=0, speed_lines=b)
    check(got, sh.speed(pt, sh.shear_pitch(128, 70, 30.0, 1.0)[1], push_line=0, speed_lines=b), "b=%d" % b)
    assert np.isnan(got["speed"]).all() and np.isnan(got["modulus"]).all() and not got["quality"].view(np.uint32).any()


@pytest.mark.parametrize("b,v", [(1, 0), (4, 2), (16, 16)])
def test_speed_windows(ctx, dev, b, v):
    """the smallest, the default and the largest fit on an image wide enough for them, pushes at both ends and in the middle"""
    F, E, R = 2, 4 * b + 8, 67                                           # (a push in the middle leaves whole windows on either side)
    pitch_mm = sh.shear_pitch(128, R, 30.0, 1.0471975511965976)[1]
    for line in (0, E - 1, E // 2):
        pt = (np.abs(np.arange(E) - line)[None, :, None] * f32(1.4) + peak_times(F, E, R, seed=line) * f32(0.05)).astype(f32)
        so = dict(push_line=line, speed_lines=b, avg_rows=v)
        s = sh.speed(pt, pitch_mm, **so)
        check(run_speed(ctx, dev, pt, pitch_mm, **so), s, "b=%d v=%d push=%d" % (b, v, line))
        assert np.isfinite(s["speed"]).any()


@pytest.mark.parametrize("T", [4, 256])
def test_fewest_and_most_pulses(ctx, dev, T):
    F, E, R = 1, 3, 40
    iq, tissue = case(F, E, R, seed=T)
    tab, _ = tables(E, R, T)
    o = dict(n_pulses=T, push_line=1, window_rows=3)
    check(run_wave(ctx, dev, iq, tissue, tab, sigma=0.125, **o), sh.wave(iq, tissue, cycles_per_row=CARRIER, sigma=0.125, **tab, **o), "T=%d" % T)


def test_defaults(ctx, dev):
    """no options: 64 pulses, window 8, a push on line 0 over every row, 0.1 row, sigma 0, the default seed; b 4 over +- 2 rows"""
    iq, tissue = case(1, 10, 70)
    tab, pitch_mm = tables(10, 70, 64)
    want = sh.wave(iq, tissue, cycles_per_row=CARRIER, **tab)
    check(run_wave(ctx, dev, iq, tissue, tab), want, "defaults")
    check(run_wave(ctx, dev, iq, tissue, tab, sigma=0.5, outputs=("peak_time", "peak_disp")), sh.wave(iq, tissue, cycles_per_row=CARRIER, sigma=0.5, **tab), "the default seed")
    check(run_speed(ctx, dev, want["peak_time"], pitch_mm), sh.speed(want["peak_time"], pitch_mm), "defaults")


@pytest.mark.parametrize("sigma_from,sigma", [("opts", 0.0), ("opts", 0.75), ("dev", [0.0, 1.5]), ("dev", [0.125, 0.125])])
def test_sigma(ctx, dev, sigma_from, sigma):
    """sigma 0 and > 0 from the options and from the device -- a frame with sigma 0 beside one with noise; ids at the end of their range"""
    iq, tissue = case(2, 3, 63, seed=4)
    tab, _ = tables(3, 63, 8)
    o = dict(n_pulses=8, push_line=1)
    want = sh.wave(iq, tissue, cycles_per_row=CARRIER, sigma=sigma, first_image_id=0xFFFFFFFE, **tab, **o)
    check(run_wave(ctx, dev, iq, tissue, tab, sigma_from=sigma_from, sigma=sigma, first_image_id=0xFFFFFFFE, **o), want, "sigma=%s from %s" % (sigma, sigma_from))


@pytest.mark.parametrize("left_out", WAVE_OUT)
def test_each_wave_output_left_out(ctx, dev, left_out):
    """(with the truths alone the tracker is not launched)"""
    iq, tissue = case(2, 5, 65, seed=3)
    tab, _ = tables(5, 65, 6)
    o = dict(n_pulses=6, push_line=2, window_rows=4)
    want = sh.wave(iq, tissue, cycles_per_row=CARRIER, sigma=0.25, **tab, **o)
    outputs = tuple(k for k in WAVE_OUT if k != left_out)
    got = run_wave(ctx, dev, iq, tissue, tab, outputs=outputs, sigma=0.25, **o)
    assert sorted(got) == sorted(outputs)
    check(got, want, "without " + left_out)
    check(run_wave(ctx, dev, iq, tissue, tab, outputs=(left_out,), sigma=0.25, **o), want, "only " + left_out)


@pytest.mark.parametrize("left_out", SPEED_OUT)
def test_each_speed_output_left_out(ctx, dev, left_out):
    pt = peak_times(2, 9, 65, seed=6)
    pitch_mm = sh.shear_pitch(128, 65, 30.0, 1.0)[1]
    so = dict(push_line=8, speed_lines=2, avg_rows=1)
    want = sh.speed(pt, pitch_mm, **so)
    outputs = tuple(k for k in SPEED_OUT if k != left_out)
    got = run_speed(ctx, dev, pt, pitch_mm, outputs=outputs, **so)
    assert sorted(got) == sorted(outputs)
    check(got, want, "without " + left_out)
    check(run_speed(ctx, dev, pt, pitch_mm, outputs=(left_out,), **so), want, "only " + left_out)


@pytest.mark.parametrize("skew", [4, 8, 12])
def test_pointers_off_a_16_byte_boundary(ctx, dev, skew):
    iq, tissue = case(1, 5, 65, seed=skew)
    tab, pitch_mm = tables(5, 65, 8)
    o = dict(n_pulses=8, push_line=2)
    want = sh.wave(iq, tissue, cycles_per_row=CARRIER, sigma=[0.5], **tab, **o)
    check(run_wave(ctx, dev, iq, tissue, tab, sigma_from="dev", sigma=[0.5], skew=skew, **o), want, "skew %d" % skew)
    so = dict(push_line=2, speed_lines=1)
    check(run_speed(ctx, dev, want["peak_time"], pitch_mm, skew=skew, **so), sh.speed(want["peak_time"], pitch_mm, **so), "skew %d" % skew)


def test_labels_that_block(ctx, dev):
    """a label past the table, MCRT_LABEL_NONE and a fluid each stop the wave: a row of each beside a row the wave passes"""
    F, E, R, T = 1, 6, 4, 16
    iq = speckle(F, E, R, seed=9)
    tissue = np.zeros((F, E, R), np.uint8); tissue[0, 3, 0] = N_LABELS; tissue[0, 3, 1] = 255; tissue[0, 3, 2] = 1
    tab, _ = tables(E, R, T)
    o = dict(n_pulses=T, push_line=0, window_rows=0)
    got = run_wave(ctx, dev, iq, tissue, tab, **o)
    check(got, sh.wave(iq, tissue, cycles_per_row=CARRIER, **tab, **o), "blocking labels")
    assert np.isposinf(got["truth_arrival"][0, 4:, :3]).all() and np.isfinite(got["truth_arrival"][0, :4]).all() and np.isfinite(got["truth_arrival"][0, :, 3]).all()
    assert not got["truth_speed"][0, 3, :3].view(np.uint32).any() and (got["truth_speed"][0, :3] == 2.0).all()
    assert not got["disp"][0, :, 4:, :3].view(np.uint32).any()           # nothing ever moves behind them


def test_tables_are_replaced_when_they_change(ctx, dev):
    """the host tables live in the context and are copied only when they differ: other values, then shorter and longer tables"""
    iq, tissue = case(1, 4, 33, seed=2)
    base, pitch_mm = tables(4, 33, 8)
    o = dict(n_pulses=8, push_line=1)
    variants = [dict(), dict(shape_q16=sh.shear_shape(5)), dict(amp_q16=sh.shear_decay(2, 1.0)), dict(pitch_q8=base["pitch_q8"] + np.uint32(777)),
                dict(slow_q16=sh.shear_table([3.0, 1.0], 9000.0)[0], speed_f=sh.shear_table([3.0, 1.0], 9000.0)[1]),
                dict(slow_q16=sh.shear_table([1.0, 2.0, 0.0, 4.0, 5.0])[0], speed_f=sh.shear_table([1.0, 2.0, 0.0, 4.0, 5.0])[1]), dict()]
    for v in variants:
        tab = dict(base, **v)
        check(run_wave(ctx, dev, iq, tissue, tab, **o), sh.wave(iq, tissue, cycles_per_row=CARRIER, **tab, **o), "tables %s" % sorted(v))
    pt = peak_times(1, 5, 33)
    for mm in (pitch_mm, (pitch_mm * f32(2.0)).astype(f32), pitch_mm):
        check(run_speed(ctx, dev, pt, mm, push_line=0, speed_lines=1), sh.speed(pt, mm, push_line=0, speed_lines=1), "pitch_mm")


def test_no_push_is_the_identity_on_the_device(ctx, dev):
    """on the device: with peak_q24 = 0 and no noise every frame of the movie is +0.0f on finite speckle, and there is no peak to time"""
    F, E, R, T = 2, 3, 200, 6
    iq = speckle(F, E, R, seed=1)
    tissue = np.random.default_rng(0).choice(np.array([0, 1, N_LABELS, 255], np.uint8), size=(F, E, R))
    tab, _ = tables(E, R, T)
    got = run_wave(ctx, dev, iq, tissue, tab, n_pulses=T, push_line=1, peak_q24=0)
    assert not got["disp"].view(np.uint32).any() and not got["peak_disp"].view(np.uint32).any() and np.isnan(got["peak_time"]).all()


def test_nothing_is_allocated_after_the_first_call_at_a_size(ctx, dev):
    """the arrival ticks and the tables live in grow-only buffers of the context: the device's free memory stays where the first call left it"""
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(), C.c_size_t()

    def free_bytes():
        ctx.synchronize()
        assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
        return free.value

    F, E, R, T = 2, 7, 300, 8
    iq, tissue = case(F, E, R)
    tab, pitch_mm = tables(E, R, T)
    n = F * E * R
    p_iq = dev.upload(iq); p_ti = dev.upload(tissue)
    outs = [dev(4 * n) for _ in range(4)]
    o = dict(n_pulses=T, push_line=3)
    call = lambda: (ctx.shear_wave_frames(p_iq, p_ti, F, E, R, cycles_per_row=CARRIER, peak_time_dev=outs[0], truth_arrival_dev=outs[1], **tab, **o),
                    ctx.shear_speed_frames(outs[0], F, E, R, pitch_mm, speed_dev=outs[2], quality_dev=outs[3], push_line=3))
    call()
    before = free_bytes()
    for _ in range(3):
        call()
    assert free_bytes() == before


def test_wave_refusals_leave_the_outputs_untouched(mcrt, ctx, dev):
    L = mcrt.load_library()
    F, E, R, T = 2, 3, 20, 4
    n = F * E * R
    iq, tissue = case(F, E, R)
    tab, _ = tables(E, R, T)
    opts = lambda **kw: mcrt.shear_opts_struct(**dict(dict(n_pulses=T, push_line=1), **kw))
    hp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    # one allocation, in floats: iq [0, 2n), then room for peak_time, peak_disp (n each), the movie (T n), the truths (n each) and sigma (F)
    TOTAL = (7 + T) * n
    head = iq.reshape(-1)
    p_ti = dev.upload(tissue)

    def call(iq_=0, ti=p_ti, frames=F, lines=E, rows=R, slow=tab["slow_q16"], spf=tab["speed_f"], labels=N_LABELS, pitch=tab["pitch_q8"], shape=tab["shape_q16"],
             n_shape=None, amp=tab["amp_q16"], n_amp=None, cyc=CARRIER, o=opts(), first=0, sig=None, pt=2 * n, pd=3 * n, mv=4 * n, ta=(4 + T) * n, ts=(5 + T) * n,
             null_ctx=False):
        big = dev.upload(np.concatenate([head, np.full(TOTAL - 2 * n, SENTINEL)]))
        at = lambda floats: None if floats is None else C.c_void_p(big + 4 * floats)
        rc = L.mcrt_shear_wave_frames(None if null_ctx else ctx.h, at(iq_), None if ti is None else C.c_void_p(ti), frames, lines, rows, hp(slow), hp(spf), labels,
                                      hp(pitch), hp(shape), len(shape) if n_shape is None else n_shape, hp(amp), len(amp) if n_amp is None else n_amp, cyc,
                                      None if o is None else C.byref(o), first, at(sig), at(pt), at(pd), at(mv), at(ta), at(ts))
        got = ctx.d2h(big, (TOTAL,))
        assert np.array_equal(got[:2 * n].view(np.uint32), head.view(np.uint32)) and (got[2 * n:] == SENTINEL).all()
        return rc

    assert call(null_ctx=True) == INVALID and call(iq_=None) == INVALID and call(ti=None) == INVALID and call(o=None) == INVALID
    big_shape = np.zeros(16385, np.uint32); big_amp = np.zeros(65537, np.uint32)
    for k in ("slow", "spf", "pitch"):
        assert call(**{k: None}) == INVALID, k
    assert call(shape=None, n_shape=4) == INVALID and call(amp=None, n_amp=4) == INVALID
    assert call(frames=0) == INVALID and call(lines=0) == INVALID and call(rows=0) == INVALID
    assert call(labels=0) == INVALID and call(n_shape=0) == INVALID and call(n_amp=0) == INVALID
    assert call(pt=None, pd=None, mv=None, ta=None, ts=None) == INVALID                    # no output
    for cyc in (0.0, -0.1, 0.5000001, float("nan"), float("inf")):
        assert call(cyc=cyc) == INVALID
    for kw in (dict(n_pulses=3), dict(n_pulses=257), dict(window_rows=17), dict(prf_hz=0.0), dict(prf_hz=float("nan")), dict(sigma=-0.5), dict(sigma=float("nan")),
               dict(peak_q24=8388609), dict(peak_q24=-8388609), dict(push_line=E), dict(push_row0=R), dict(push_row0=R - 1, push_rows=2), dict(push_rows=R + 1),
               dict(speed_lines=0), dict(speed_lines=17), dict(avg_rows=17), dict(density=0.0), dict(density=float("inf"))):
        assert call(o=opts(**kw)) == INVALID, kw
    bad = tab["slow_q16"].copy(); bad[2] = -1
    assert call(slow=bad) == INVALID
    bad[2] = (1 << 38) + 1
    assert call(slow=bad) == INVALID
    for v in (0, 1 << 24):
        bad = tab["pitch_q8"].copy(); bad[R - 1] = v
        assert call(pitch=bad) == INVALID
    bad = tab["shape_q16"].copy(); bad[-1] = 65537
    assert call(shape=bad) == INVALID
    bad = tab["amp_q16"].copy(); bad[-1] = 65537
    assert call(amp=bad) == INVALID
    assert call(rows=2049, frames=1, lines=1, pitch=np.ones(2049, np.uint32)) == LIMIT and call(labels=255) == LIMIT
    assert call(shape=big_shape) == LIMIT and call(amp=big_amp) == LIMIT
    assert call(frames=1 << 11, lines=1 << 10, rows=1 << 10, pitch=np.ones(1024, np.uint32)) == LIMIT      # 2^31 samples
    assert call(frames=1 << 9, lines=1 << 10, rows=1 << 10, pitch=np.ones(1024, np.uint32), o=opts(n_pulses=4)) == LIMIT     # a movie of 2^31 samples
    assert call(first=0xFFFFFFFF) == LIMIT                                                 # the second frame's id would pass 2^32
    # overlaps: an output with an input, and two outputs with each other
    assert call(pt=2 * n - 1) == INVALID and call(pd=0) == INVALID and call(mv=n) == INVALID and call(ta=1) == INVALID and call(ts=2 * n - 1) == INVALID
    assert call(pd=3 * n - 1) == INVALID and call(mv=4 * n - 1) == INVALID and call(ta=(4 + T) * n - 1) == INVALID and call(ts=(5 + T) * n - 1) == INVALID
    assert call(ts=4 * n + 1) == INVALID                                                   # a truth inside the movie
    assert call(sig=4 * n) == INVALID and call(sig=2 * n + 1) == INVALID                   # sigma_dev inside the movie, inside peak_time_dev
    tis = dev.upload(np.ones(4 * n, np.uint8))
    o = opts()
    assert L.mcrt_shear_wave_frames(ctx.h, C.c_void_p(dev.upload(iq)), C.c_void_p(tis), F, E, R, hp(tab["slow_q16"]), hp(tab["speed_f"]), N_LABELS, hp(tab["pitch_q8"]),
                                    hp(tab["shape_q16"]), len(tab["shape_q16"]), hp(tab["amp_q16"]), len(tab["amp_q16"]), CARRIER, C.byref(o), 0, None,
                                    None, C.c_void_p(tis), None, None, None) == INVALID      # peak_disp_dev is tissue_dev


def test_speed_refusals_leave_the_outputs_untouched(mcrt, ctx, dev):
    L = mcrt.load_library()
    F, E, R = 2, 5, 20
    n = F * E * R
    pt = peak_times(F, E, R)
    pitch_mm = sh.shear_pitch(128, R, 30.0, 1.0)[1]
    opts = lambda **kw: mcrt.shear_opts_struct(**dict(dict(push_line=1, speed_lines=1), **kw))
    hp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    # one allocation, in floats: peak_time [0, n), then room for speed, modulus and quality (n each)
    TOTAL = 4 * n
    head = pt.reshape(-1)

    def call(pt_=0, frames=F, lines=E, rows=R, pitch=pitch_mm, o=opts(), sp=n, mo=2 * n, qu=3 * n, null_ctx=False):
        big = dev.upload(np.concatenate([head, np.full(TOTAL - n, SENTINEL)]))
        at = lambda floats: None if floats is None else C.c_void_p(big + 4 * floats)
        rc = L.mcrt_shear_speed_frames(None if null_ctx else ctx.h, at(pt_), frames, lines, rows, hp(pitch), None if o is None else C.byref(o), at(sp), at(mo), at(qu))
        got = ctx.d2h(big, (TOTAL,))
        assert np.array_equal(got[:n].view(np.uint32), head.view(np.uint32)) and (got[n:] == SENTINEL).all()
        return rc

    assert call(null_ctx=True) == INVALID and call(pt_=None) == INVALID and call(pitch=None) == INVALID and call(o=None) == INVALID
    assert call(frames=0) == INVALID and call(lines=0) == INVALID and call(rows=0) == INVALID
    assert call(sp=None, mo=None, qu=None) == INVALID                                      # no output
    for kw in (dict(n_pulses=3), dict(window_rows=17), dict(prf_hz=-1.0), dict(sigma=-0.5), dict(peak_q24=8388609), dict(push_line=E), dict(push_row0=R),
               dict(push_rows=R + 1), dict(speed_lines=0), dict(speed_lines=17), dict(avg_rows=17), dict(density=-1.0), dict(density=float("nan"))):
        assert call(o=opts(**kw)) == INVALID, kw
    for v in (0.0, -0.3, float("nan"), float("inf")):
        bad = pitch_mm.copy(); bad[R - 1] = v
        assert call(pitch=bad) == INVALID
    assert call(rows=2049, frames=1, lines=2, pitch=np.ones(2049, f32)) == LIMIT
    assert call(frames=1 << 11, lines=1 << 10, rows=1 << 10, pitch=np.ones(1024, f32)) == LIMIT      # 2^31 samples
    assert call(sp=n - 1) == INVALID and call(mo=0) == INVALID and call(qu=n - 1) == INVALID         # an output with the input
    assert call(mo=2 * n - 1) == INVALID and call(qu=n + 1) == INVALID and call(qu=2 * n) == INVALID  # two outputs


def test_calls_with_nothing_wrong_write(ctx, dev):
    """the refusal tests' shapes with nothing wrong are accepted and write every element: their sentinels are not kernels that do nothing"""
    iq, tissue = case(2, 3, 20)
    tab, _ = tables(3, 20, 4)
    w = run_wave(ctx, dev, iq, tissue, tab, n_pulses=4, push_line=1)
    assert all((v != SENTINEL).all() for v in w.values())
    s = run_speed(ctx, dev, peak_times(2, 5, 20), sh.shear_pitch(128, 20, 30.0, 1.0)[1], push_line=1, speed_lines=1)
    assert all((v != SENTINEL).all() for v in s.values())
