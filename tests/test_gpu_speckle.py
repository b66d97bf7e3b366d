"""mcrt_speckle_frames on the MI355X: k_srad in both forms (2 and 4 iterations per launch: the default, and the other through
MCRT_SPECKLE_FUSE, read when a context is made) against the numpy mirror of the contract (tests/speckle_mirror.py) fed with the product's own
table floats, bit for bit -- at the shapes where a tile or a halo can go wrong, at the iteration counts where the launches split, in place
and out of place, one frame and three; the argument errors; a traced scene through the Simulator, the C++ shim and mattausch_hip."""
import ctypes as C
import json
import os
import subprocess
import numpy as np
import pytest

import image_cases as ic
import speckle_mirror as sm
from test_gpu_focus import Dev

pytestmark = pytest.mark.gpu

f32 = np.float32
INVALID, LIMIT = -1, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TH, TW = 16, 64                 # k_srad's tile (SRAD_TH, SRAD_TW in csrc/mcrt_kernels.h)
FUSE = (2, 4)                   # the forms that are built (SRAD_FUSE_MAX = 4)
T = max(FUSE)
SHAPES = [(1, 1), (1, 37), (37, 1), (2, 2), (3, 300), (300, 3), (63, 65), (65, 63), (129, 130)] + \
         [(h, w) for h in (TH - 1, TH, TH + 1, 2 * TH + 1) for w in (TW - 1, TW, TW + 1, 2 * TW + 1)]
N_ITER = sorted({1, 2, 3, 20} | {n for t in FUSE for n in (t - 1, t, t + 1, 2 * t + 1)})      # 1, 2, 3, 4, 5, 9, 20
FILL = f32(-777.25)             # outputs are pre-filled: a pixel that is not written shows


def test_the_tile_is_the_kernels():
    src = open(os.path.join(ROOT, "mcray-tracing_amd", "csrc", "mcrt_kernels.h")).read()
    assert "#define SRAD_TH %d " % TH in src and "#define SRAD_TW %d " % TW in src and "#define SRAD_FUSE_MAX %d " % T in src


def _context_with(mcrt, fuse):
    """a context whose k_srad runs `fuse` iterations per launch (None: the default)"""
    saved = os.environ.get("MCRT_SPECKLE_FUSE")
    if fuse is not None:
        os.environ["MCRT_SPECKLE_FUSE"] = str(fuse)                 # (MCRT_TUNING=1 is the suite's: conftest.py)
    try:
        return mcrt.Context(0)
    finally:
        if saved is None:
            os.environ.pop("MCRT_SPECKLE_FUSE", None)
        else:
            os.environ["MCRT_SPECKLE_FUSE"] = saved


@pytest.fixture(scope="module")
def ctx(mcrt):
    c = _context_with(mcrt, None)
    yield c
    c.close()


@pytest.fixture(scope="module", params=["default"] + ["fuse%d" % t for t in FUSE])
def form(request, mcrt, ctx):
    if request.param == "default":
        yield ctx
        return
    c = _context_with(mcrt, int(request.param[4:]))
    yield c
    c.close()


@pytest.fixture
def dev(ctx):
    d = Dev(ctx)
    yield d
    d.close()


def stack(F, H, W, seed=0):
    """[F][H][W]: speckle with both signs, a flat zero patch, exact zeros, -0.0, NaN and +-inf"""
    rng = np.random.default_rng(4000 + 131 * H + W + seed)
    x = (rng.rayleigh(1.0, (F, H, W)) * np.where(rng.random((F, H, W)) < 0.3, -1.0, 1.0) * (1.0 + 3.0 * (rng.random((F, 1, 1)) < 0.5))).astype(f32)
    x[:, H // 3:H // 3 + 4, W // 4:W // 4 + 5] = 0.0
    flat = x.reshape(F, -1)
    n = flat.shape[1]
    if n >= 6:
        vals = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-30], f32)
        for f in range(F):
            k = max(len(vals), n // 40)
            idx = rng.permutation(n)[:k]
            flat[f, idx] = np.resize(vals, k)
    return x


_WANT = {}


def want(H, W, n_iter, mcrt, **opts):
    """the mirror's answer for stack(3, H, W) with the product's table floats, computed once and shared by the forms"""
    key = (H, W, n_iter, tuple(sorted(opts.items())))
    if key not in _WANT:
        _WANT[key] = sm.srad(stack(3, H, W), *mcrt.host_speckle_tables(n_iter=n_iter, **opts))
        _WANT[key].setflags(write=False)
    return _WANT[key]


@pytest.mark.parametrize("H,W", SHAPES)
def test_forms_shapes_and_iteration_counts(mcrt, form, H, W):
    """every form at every shape and iteration count: three frames out of place, the first alone (frame 0 of the three is the single
    one), and the three in place"""
    c = form
    d = Dev(c)
    try:
        x = stack(3, H, W)
        src = d.upload(x); out = d(x.nbytes); inp = d(x.nbytes)
        fill = np.full(x.shape, FILL)
        for n_iter in N_ITER:
            w = want(H, W, n_iter, mcrt)
            c.h2d(out, fill)
            c.speckle_frames(src, 3, H, W, out, n_iter=n_iter)
            c.synchronize()
            ic.assert_same_bits(c.d2h(out, x.shape), w, "out of place, F = 3, n_iter %d" % n_iter)
            c.h2d(out, fill)
            c.speckle_frames(src, 1, H, W, out, n_iter=n_iter)
            c.synchronize()
            got = c.d2h(out, x.shape)
            ic.assert_same_bits(got[0], w[0], "out of place, F = 1, n_iter %d" % n_iter)
            assert (got[1:] == FILL).all(), "F = 1 wrote past its frame"
            c.h2d(inp, x)
            c.speckle_frames(inp, 3, H, W, n_iter=n_iter)
            c.synchronize()
            ic.assert_same_bits(c.d2h(inp, x.shape), w, "in place, F = 3, n_iter %d" % n_iter)
        ic.assert_same_bits(c.d2h(src, x.shape), x, "the input of the out-of-place calls")
    finally:
        d.close()


def test_other_options_and_n_iter_zero(mcrt, form):
    """options away from the defaults (lambda = 1, another scale, no decay; 256 iterations), and n_iter = 0: the input's bits, untouched
    in place"""
    c = form
    d = Dev(c)
    try:
        H, W = 33, 70
        x = stack(3, H, W)
        src = d.upload(x); out = d(x.nbytes)
        for opts in (dict(n_iter=5, lambda_=1.0), dict(n_iter=7, q0=1.0, rho=0.0, lambda_=0.25), dict(n_iter=256, q0=2.0, rho=0.01)):
            c.h2d(out, np.full(x.shape, FILL))
            c.speckle_frames(src, 3, H, W, out, **opts)
            c.synchronize()
            n = opts.pop("n_iter")
            ic.assert_same_bits(c.d2h(out, x.shape), want(H, W, n, mcrt, **opts), str(opts))
        c.h2d(out, np.full(x.shape, FILL))
        c.speckle_frames(src, 3, H, W, out, n_iter=0)
        c.synchronize()
        ic.assert_same_bits(c.d2h(out, x.shape), x, "n_iter = 0, out of place")
        c.speckle_frames(src, 3, H, W, n_iter=0)
        c.synchronize()
        ic.assert_same_bits(c.d2h(src, x.shape), x, "n_iter = 0, in place")
    finally:
        d.close()


def test_a_pass_of_four_is_two_passes_of_two(mcrt, form):
    """with rho = 0 the tables' halves are the tables of two calls (q_2 = q0 exactly): 4 iterations equal 2 + 2, bit for bit.  With a decay
    the second call's q0 is (float)q_2, whose tables may differ from the pass's in the last place: the mirror decides what the two
    calls give, and they are held to the single pass only where the floats agree"""
    c = form
    d = Dev(c)
    try:
        H, W = 2 * TH + 1, TW + 1
        x = stack(3, H, W)
        src = d.upload(x); out = d(x.nbytes)
        for rho in (0.0, sm.DEFAULTS["rho"]):
            t4 = mcrt.host_speckle_tables(n_iter=4, rho=rho)
            q2 = float(f32(np.float64(f32(sm.DEFAULTS["q0"])) * np.exp(-np.float64(f32(rho)) * 2.0)))
            ta, tb = mcrt.host_speckle_tables(n_iter=2, rho=rho), mcrt.host_speckle_tables(n_iter=2, q0=q2, rho=rho)
            c.h2d(out, np.full(x.shape, FILL))
            c.speckle_frames(src, 3, H, W, out, n_iter=2, rho=rho)
            c.speckle_frames(out, 3, H, W, n_iter=2, q0=q2, rho=rho)
            c.synchronize()
            two = c.d2h(out, x.shape)
            ic.assert_same_bits(two, sm.srad(sm.srad(x, *ta), *tb), "2 + 2, rho %g" % rho)
            same = np.array_equal(np.concatenate([ta[0], tb[0]]), t4[0]) and np.array_equal(np.concatenate([ta[1], tb[1]]), t4[1])
            assert same or rho != 0.0
            if same:
                ic.assert_same_bits(two, sm.srad(x, *t4), "2 + 2 against 4, rho %g" % rho)
    finally:
        d.close()


def test_errors_leave_out_dev_untouched(mcrt, ctx, dev):
    L = ctx.L
    H, W = 9, 20
    x = stack(2, H, W)
    src = dev.upload(x)
    fill = np.full(x.shape, FILL)
    out = dev.upload(fill)
    good = mcrt.speckle_opts_struct(n_iter=3)

    def call(h=ctx.h, i=src, F=2, hh=H, ww=W, o=good, out_=out):
        return L.mcrt_speckle_frames(h, C.c_void_p(i) if i else None, F, hh, ww, C.byref(o) if o is not None else None, C.c_void_p(out_) if out_ else None)

    def err(code, word, **kw):
        assert call(**kw) == code, kw
        assert word in L.mcrt_last_error(), (kw, L.mcrt_last_error())

    err(INVALID, b"null context", h=None)
    err(INVALID, b"in_dev", i=None); err(INVALID, b"out_dev", out_=None)
    err(INVALID, b"zero", F=0); err(INVALID, b"zero", hh=0); err(INVALID, b"zero", ww=0)
    for opts, code, word in ((dict(n_iter=257), LIMIT, b"n_iter"), (dict(q0=0.0), INVALID, b"q0"), (dict(q0=np.nan), INVALID, b"q0"), (dict(rho=-1.0), INVALID, b"rho"),
                             (dict(rho=np.inf), INVALID, b"rho"), (dict(lambda_=0.0), INVALID, b"lambda"), (dict(lambda_=1.5), INVALID, b"lambda"),
                             (dict(n_iter=256, rho=1.0), INVALID, b"iteration")):
        err(code, word, o=mcrt.speckle_opts_struct(**opts))
    err(LIMIT, b"2^31", F=1 << 11, hh=1 << 10, ww=1 << 10); err(LIMIT, b"2^31", F=0xFFFFFFFF, hh=0xFFFFFFFF, ww=0xFFFFFFFF)
    # any overlap but the same buffer: a stack that starts one float, or one frame, into the other
    big = dev.upload(np.concatenate([fill, fill]))
    err(INVALID, b"overlap", i=big, out_=big + 4); err(INVALID, b"overlap", i=big + 4 * H * W, out_=big)
    ctx.synchronize()
    ic.assert_same_bits(ctx.d2h(out, x.shape), fill, "out_dev after the errors")
    ic.assert_same_bits(ctx.d2h(big, (4, H, W)), np.concatenate([fill, fill]), "the overlapping buffers after the errors")
    ic.assert_same_bits(ctx.d2h(src, x.shape), x, "in_dev after the errors")
    # the context still works; null options are the defaults
    assert call(o=None) == 0
    ctx.synchronize()
    ic.assert_same_bits(ctx.d2h(out, x.shape), sm.srad(x, *mcrt.host_speckle_tables()), "null options")
    # adjacent buffers do not overlap
    ctx.h2d(big, np.concatenate([x, fill]))
    assert call(i=big, out_=big + x.nbytes) == 0
    ctx.synchronize()
    ic.assert_same_bits(ctx.d2h(big, (4, H, W))[2:], sm.srad(x, *mcrt.host_speckle_tables(n_iter=3)), "adjacent buffers")


def test_the_scratch_is_shared_with_convolve_and_only_grows(mcrt, ctx, dev):
    """a large stack after a small one, a convolution between two filters: the ping-pong buffer is the context's scratch"""
    small, large = stack(3, 5, 9), stack(3, 40, 129)
    for x in (small, large, small):
        p = dev.upload(x)
        ctx.speckle_frames(p, 3, x.shape[1], x.shape[2], n_iter=6)
        ctx.synchronize()
        ic.assert_same_bits(ctx.d2h(p, x.shape), sm.srad(x, *mcrt.host_speckle_tables(n_iter=6)), str(x.shape))
        q = dev.upload(np.ones((3, 64, 128), f32))
        ctx.convolve_frames(q, 3, 64, 128, np.ones(3, f32), np.ones(3, f32))


# ------------------------------------------------------------------ end to end: a traced scene
def _write_scene(mcrt, tmp_path):
    cfg, meshes = mcrt.synth.sphere_scene(3)
    cfg["workingDirectory"] = str(tmp_path) + "/"
    for f, (V, F) in meshes.items():
        mcrt.scene_io.save_obj(str(tmp_path / f), V, F)
    (tmp_path / "sphere.scene").write_text(json.dumps(cfg))
    return cfg, str(tmp_path / "sphere.scene")


def test_simulator_pictures_are_the_filter_by_hand(mcrt, tmp_path):
    """Simulator(speckle=...) pictures equal Simulator() pictures pushed through Context.speckle_frames by hand: the plain B-mode frame,
    a compounded frame (the filter runs over the views) and a cut through a swept volume (over the planes); frame() returns RF and is
    left alone"""
    cfg, scene = _write_scene(mcrt, tmp_path)
    sd = mcrt.scene_io.load_scene_file(scene)
    E, S, frame = 16, 8, 3
    tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    size = dict(out_rows=80, out_cols=100)
    for kw, spk in ((dict(), True), (dict(compound=(-0.1, 0.0, 0.1)), dict(n_iter=5, lambda_=1.0)), (dict(sweep=(3, 0.05), sweep_pivot_mm=10.0), dict(n_iter=3, q0=1.0))):
        plain, filt = mcrt.Simulator(sd, tr, n_samples=S, **kw), mcrt.Simulator(sd, tr, n_samples=S, speckle=spk, **kw)
        try:
            assert plain.speckle is None and filt.speckle is not None
            o = filt.speckle
            by_hand = dict(n_iter=o.n_iter, q0=o.q0, rho=o.rho, lambda_=o.lambda_)
            assert o.n_iter == (20 if spk is True else spk["n_iter"])
            plain._run(frame)
            buf, n = plain._stack
            raw = plain.ctx.d2h(buf, (n, E, plain.R))
            plain.ctx.speckle_frames(buf, n, E, plain.R, **by_hand)
            plain.ctx.synchronize()
            ic.assert_same_bits(plain.ctx.d2h(buf, raw.shape), sm.srad(raw, *mcrt.host_speckle_tables(o)), "the stack by hand")
            with plain.ctx.temp(size["out_rows"] * size["out_cols"] * 4) as out:
                if "sweep" in kw:
                    g = mcrt.cplane_grid(80.0, nu=40, nv=8, pitch_mm=1.0)
                    plain.ctx.bmode_volume_frames(buf, 1, E, plain.R, plain.sweep, g, out)
                    want_pic = plain.ctx.d2h(out, (g.nw, g.nv, g.nu), np.uint8)
                    got_pic = filt.bmode_volume(frame, g)
                elif "compound" in kw:
                    plain.ctx.bmode_compound_frames(buf, 1, E, plain.R, plain.steers, out, **size)
                    want_pic = plain.ctx.d2h(out, (80, 100), np.uint8)
                    got_pic = filt.bmode(frame, **size)
                else:
                    plain.ctx.bmode_frames(buf, 1, E, plain.R, out, **size)
                    want_pic = plain.ctx.d2h(out, (80, 100), np.uint8)
                    got_pic = filt.bmode(frame, **size)
            assert np.array_equal(got_pic, want_pic), kw
            assert len(np.unique(got_pic)) > (4 if "sweep" in kw else 10)
            unfiltered = mcrt.Simulator(sd, tr, n_samples=S, **kw)
            try:
                other = unfiltered.bmode_volume(frame, g) if "sweep" in kw else unfiltered.bmode(frame, **size)
            finally:
                unfiltered.close()
            assert not np.array_equal(other, got_pic), "the filter changed nothing"
            if not kw:
                ic.assert_same_bits(filt.frame(frame), unfiltered_rf(mcrt, sd, tr, S, frame), "frame() is RF")
        finally:
            plain.close(); filt.close()


def unfiltered_rf(mcrt, sd, tr, S, frame):
    s = mcrt.Simulator(sd, tr, n_samples=S)
    try:
        return s.frame(frame)
    finally:
        s.close()


def test_cli_speckle_options(mcrt, tmp_path):
    """mattausch_hip --speckle: the PGM equals the Python bytes, rf.bin is the mirror's filter of the run without the option, and without
    --speckle the PGM is the picture of a Simulator that makes no new call; options that the library refuses end the program before it
    touches a device"""
    exe = os.path.join(ROOT, "mcray-tracing_amd", "mattausch_hip")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "mcray-tracing_amd"), "mattausch_hip"])
    cfg, scene = _write_scene(mcrt, tmp_path)
    run = lambda *a: subprocess.run([exe, scene, "1", "5"] + list(a), capture_output=True, text=True, timeout=240)
    r = run(str(tmp_path / "s.pgm"), str(tmp_path / "s.bin"), "--db", "50", "--speckle", "5", "--speckle-lambda", "1", "--speckle-q0", "0.75", "--speckle-rho", "0.125")
    assert r.returncode == 0, r.stdout + r.stderr
    r = run(str(tmp_path / "p.pgm"), str(tmp_path / "p.bin"), "--db", "50")
    assert r.returncode == 0, r.stdout + r.stderr
    head = b"P5\n500 400\n255\n"
    tr = mcrt.Transducer(512, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    sd = mcrt.scene_io.load_scene_file(scene)
    opts = dict(n_iter=5, lambda_=1.0, q0=0.75, rho=0.125)
    for name, spk in (("s", opts), ("p", None)):
        sim = mcrt.Simulator(sd, tr, n_samples=5, speckle=spk)
        try:
            pic = sim.bmode(0, dynamic_range_db=50.0)
        finally:
            sim.close()
        assert (tmp_path / (name + ".pgm")).read_bytes() == head + pic.tobytes(), name
    env = np.fromfile(str(tmp_path / "p.bin"), f32).reshape(465, 512)
    got = np.fromfile(str(tmp_path / "s.bin"), f32).reshape(465, 512)
    ic.assert_same_bits(got.T, sm.srad(np.ascontiguousarray(env.T), *mcrt.host_speckle_tables(**opts)), "rf.bin")
    assert (tmp_path / "s.pgm").read_bytes() != (tmp_path / "p.pgm").read_bytes()
    for bad, word in ((["--speckle-q0", "0.5"], "need --speckle"), (["--speckle", "257"], "0..256"), (["--speckle", "-1"], "0..256"),
                      (["--speckle", "3", "--speckle-lambda", "2"], "lambda"), (["--speckle", "3", "--speckle-q0", "0"], "q0"),
                      (["--speckle", "200", "--speckle-rho", "2"], "iteration")):
        r = subprocess.run([exe, scene, "1", "5"] + bad, capture_output=True, text=True, timeout=240)
        assert r.returncode == 1 and "--speckle" in r.stdout and word in r.stdout, (bad, word, r.stdout)
