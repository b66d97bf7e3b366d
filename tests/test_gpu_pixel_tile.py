"""The pixel tile the gather kernels share (csrc/mcrt_pixels.h) at its edges, on the MI355X: the 8-bit forms of k_compound, k_volume and
k_label_gather at 257 points (a whole tile and one ragged point, byte stores), 260 points (a whole tile storing words beside a ragged one
storing bytes), 260 points with the output one byte into its allocation (byte stores by alignment), fewer than 64 points, and a pass whose
chunks hold two frames and whose last chunk holds one; k_bmode's and k_compound's persistence over three calls at 257 pixels.
The stacks hold 0 and 1 only and the reference is 1: every grey level is exactly 0 or 1 (log10f(1) = 0), so the bytes are the mirrors' bit
for bit."""
import numpy as np
import pytest

import bmode_mirror as bm
import compound_mirror as cm
import label_mirror as lm
import volume_mirror as vm
from test_gpu_focus import Dev

pytestmark = pytest.mark.gpu

f32 = np.float32
E, R, K = 8, 16, 2
STEERS = (0.1, -0.1)
RADIUS, ANGLE = 30.0, vm.DEFAULT_ANGLE
PIVOT = 10.0
SWEEP = (K, vm.STEP, PIVOT)
# n -> the picture (rows, cols) and the grid (nu, nv, nw)
SHAPES = {257: ((257, 1), (257, 1, 1)), 260: ((4, 65), (65, 4, 1)), 21: ((3, 7), (7, 3, 1))}
# (n, the output's offset into its allocation): word stores only at 260 points on a word boundary
CASES = [(257, 0), (260, 0), (260, 1), (21, 0)]
GUARD = 8
BMODE = dict(ref=1.0, dynamic_range_db=48.0)


@pytest.fixture(scope="module")
def ctx(mcrt):
    c = mcrt.Context(0)
    yield c
    c.close()


@pytest.fixture
def dev(ctx):
    d = Dev(ctx)
    yield d
    d.close()


def binary(shape, seed):
    """0 and +-1 in equal parts"""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 2, shape) * rng.choice([-1.0, 1.0], shape)).astype(f32)


def tissue(shape, seed):
    return np.random.default_rng(seed).integers(0, 200, shape).astype(np.uint8)


def guarded(ctx, dev, F, n, off, call):
    """call(out) writes [F][n] bytes at out, `off` bytes past a word boundary -> those bytes; the GUARD bytes on either side stay as they were"""
    buf = dev.upload(np.full(GUARD + off + F * n + GUARD, 0xA5, np.uint8))
    call(buf + GUARD + off)
    ctx.synchronize()
    raw = ctx.d2h(buf, (GUARD + off + F * n + GUARD,), np.uint8)
    assert np.all(raw[:GUARD + off] == 0xA5) and np.all(raw[GUARD + off + F * n:] == 0xA5), "bytes beside the output were written"
    return raw[GUARD + off:GUARD + off + F * n].reshape(F, n)


def same_bytes(got, want, what):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    print("%s: %d of %d bytes differ" % (what, int((got != want).sum()), got.size))
    assert np.array_equal(got, want), what


def compound_maps(mcrt, rows, cols):
    return [mcrt.host_compound_maps(E, R, s, RADIUS, ANGLE, out_rows=rows, out_cols=cols) for s in STEERS]


# ------------------------------------------------------------------ the ragged end, the word store and its alignment
@pytest.mark.parametrize("n,off", CASES)
def test_compound_bytes(mcrt, ctx, dev, n, off):
    rows, cols = SHAPES[n][0]
    F = 2
    st = binary((F, len(STEERS), E, R), n + off)
    p = dev.upload(st)
    got = guarded(ctx, dev, F, n, off, lambda out: ctx.bmode_compound_frames(p, F, E, R, STEERS, out, radius_mm=RADIUS, total_angle=ANGLE, out_rows=rows,
                                                                             out_cols=cols, **BMODE))
    want, _, _ = cm.bmode_compound(st, compound_maps(mcrt, rows, cols), **BMODE)
    same_bytes(got, want, "k_compound n %d offset %d" % (n, off))
    assert len(np.unique(got)) > 2


@pytest.mark.parametrize("n,off", CASES)
def test_volume_bytes(mcrt, ctx, dev, n, off):
    g = vm.grid_for(mcrt, SHAPES[n][1], E, R, K, PIVOT)
    F = 2
    st = binary((F, K, E, R), 10 + n + off)
    p = dev.upload(st)
    got = guarded(ctx, dev, F, n, off, lambda out: ctx.bmode_volume_frames(p, F, E, R, SWEEP, g, out, **BMODE))
    want, _ = vm.bmode_volume(st, mcrt.host_volume_maps(E, R, SWEEP, g), **BMODE)
    same_bytes(got, want, "k_volume n %d offset %d" % (n, off))
    assert len(np.unique(got)) > 2


@pytest.mark.parametrize("n,off", CASES)
def test_label_bytes(mcrt, ctx, dev, n, off):
    (rows, cols), which = SHAPES[n]
    F = 2
    t = tissue((F, K, E, R), 20 + n + off)
    p = dev.upload(t)
    # one plane through the scan-conversion maps: the first plane of each frame, contiguous
    p1 = dev.upload(t[:, 0])
    got = guarded(ctx, dev, F, n, off, lambda out: ctx.label_scan_convert_frames(p1, F, E, R, out, RADIUS, ANGLE, rows, cols))
    mr, mc = mcrt.host_scan_maps(E, R, RADIUS, ANGLE, 100, 1500, rows, cols)
    same_bytes(got, np.stack([lm.scan_convert(t[f, 0], mr, mc) for f in range(F)]), "k_label_gather, two maps, n %d offset %d" % (n, off))
    g = vm.grid_for(mcrt, which, E, R, K, PIVOT)
    got = guarded(ctx, dev, F, n, off, lambda out: ctx.label_volume_frames(p, F, E, R, SWEEP, g, out))
    maps = mcrt.host_volume_maps(E, R, SWEEP, g)
    same_bytes(got, np.stack([lm.volume(t[f], maps) for f in range(F)]), "k_label_gather, three maps, n %d offset %d" % (n, off))
    assert len(np.unique(got)) > 2


# ------------------------------------------------------------------ chunks of two frames and a last chunk of one
def test_a_chunked_pass_equals_single_calls(mcrt, ctx, dev):
    """256 x 256 points, 65 frames: the pass is cut into 33 chunks of 2, 2, ..., 1 frames"""
    F, rows, cols = 65, 256, 256
    n = rows * cols
    st = binary((F, K, E, R), 30)                       # (K = the number of views)
    t = tissue((F, K, E, R), 31)
    p, pt = dev.upload(st), dev.upload(t)
    g = vm.grid_for(mcrt, (cols, rows, 1), E, R, K, PIVOT)
    calls = {
        "k_compound": lambda src, f, out: ctx.bmode_compound_frames(src, f, E, R, STEERS, out, radius_mm=RADIUS, total_angle=ANGLE, out_rows=rows, out_cols=cols, **BMODE),
        "k_volume": lambda src, f, out: ctx.bmode_volume_frames(src, f, E, R, SWEEP, g, out, **BMODE),
        "k_label_gather": lambda src, f, out: ctx.label_volume_frames(src, f, E, R, SWEEP, g, out),
    }
    last = {"k_compound": lambda: cm.bmode_compound(st[-1:], compound_maps(mcrt, rows, cols), **BMODE)[0],
            "k_volume": lambda: vm.bmode_volume(st[-1:], mcrt.host_volume_maps(E, R, SWEEP, g), **BMODE)[0],
            "k_label_gather": lambda: lm.volume(t[-1], mcrt.host_volume_maps(E, R, SWEEP, g))}
    for name, call in calls.items():
        src, item = (pt, K * E * R) if name == "k_label_gather" else (p, 4 * K * E * R)
        whole, single = dev.upload(np.full(F * n, 0xA5, np.uint8)), dev.upload(np.full(F * n, 0x5A, np.uint8))
        call(src, F, whole)
        for f in range(F):
            call(src + f * item, 1, single + f * n)
        ctx.synchronize()
        got = ctx.d2h(whole, (F, n), np.uint8)
        same_bytes(got, ctx.d2h(single, (F, n), np.uint8), name + ": 65 frames in one call and in 65")
        same_bytes(got[-1], last[name](), name + ": the last frame against the mirror")
        assert len(np.unique(got)) > 2


# ------------------------------------------------------------------ persistence carried through the state
def test_persistence_one_call_of_three_equals_three_calls(mcrt, orc, ctx, dev):
    rows, cols = SHAPES[257][0]
    n, F, alpha = rows * cols, 3, 0.6
    kw = dict(radius_mm=RADIUS, total_angle=ANGLE, out_rows=rows, out_cols=cols, **BMODE)
    st = binary((F, len(STEERS), E, R), 40)
    p = dev.upload(st)
    forms = {
        "k_bmode": (4 * len(STEERS) * E * R, lambda src, f, out, **o: ctx.bmode_frames(src, f, len(STEERS) * E, R, out, **kw, **o),
                    lambda: bm.bmode(orc, st.reshape(F, len(STEERS) * E, R), persistence=alpha, **kw)[0]),
        "k_compound": (4 * len(STEERS) * E * R, lambda src, f, out, **o: ctx.bmode_compound_frames(src, f, E, R, STEERS, out, **kw, **o),
                       lambda: cm.bmode_compound(st, compound_maps(mcrt, rows, cols), persistence=alpha, **BMODE)[0]),
    }
    for name, (item, call, mirror) in forms.items():
        s3, s1 = dev.upload(np.full(n, np.nan, f32)), dev.upload(np.full(n, np.nan, f32))        # (reset_state: what the state held is not read)
        whole = guarded(ctx, dev, F, n, 0, lambda out: call(p, F, out, persistence=alpha, state_dev=s3, reset_state=True))
        parts = [guarded(ctx, dev, 1, n, 0, lambda out: call(p + f * item, 1, out, persistence=alpha, state_dev=s1, reset_state=f == 0)) for f in range(F)]
        same_bytes(np.concatenate(parts), whole, name + ": three calls carrying the state and one call of three")
        a, b = ctx.d2h(s3, (n,)), ctx.d2h(s1, (n,))
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.isfinite(a).all(), name
        same_bytes(whole, mirror(), name + " against the mirror")
        plain = guarded(ctx, dev, F, n, 0, lambda out: call(p, F, out))
        assert np.array_equal(plain[0], whole[0]) and not np.array_equal(plain[2], whole[2]), name
