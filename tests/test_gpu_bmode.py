"""mcrt_bmode_frames on the MI355X: log-compressed 8-bit B-mode frames (TGC, dynamic range, gain, persistence) against the numpy mirror
of the contract (tests/bmode_mirror.py, whose scan conversion is the oracle's), its invariances, a traced pass, the argument errors, a
group's root context and the mattausch_hip CLI."""
import json
import math
import os
import subprocess
import numpy as np
import pytest

import bmode_mirror as bm

pytestmark = pytest.mark.gpu

E, R = 128, 465
OUT = (400, 500)
N = OUT[0] * OUT[1]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def synthetic_frames():
    """[3][E][R]: depth plateaus (2^-k) with the sign alternating over the scan-lines and NaN / +inf / -inf scan-lines; ramps with zero and
    NaN stretches; an all-zero frame (black with the automatic reference)"""
    band = np.minimum(np.arange(R) // 40, 11)
    fr = np.zeros((3, E, R), np.float32)
    fr[0] = 3.0 * np.ldexp(np.float32(1.0), -band)[None, :]
    fr[0, 1::2] *= -1
    fr[0, 40] = np.nan; fr[0, 41] = np.inf; fr[0, 90] = -np.inf
    ramp = np.linspace(0.0, 2.0, R, dtype=np.float32)[None, :] * (1.0 + np.arange(E, dtype=np.float32) / E)[:, None]
    fr[1] = ramp ** 3
    fr[1, ::3] *= -1
    fr[1, 10:15] = 0.0
    fr[1, 60, 100:180] = np.nan
    fr[1, 61, 200:210] = np.inf
    return fr, band


@pytest.fixture(scope="module")
def ctx(mcrt):
    c = mcrt.Context(0)
    yield c
    c.close()


class Dev:
    """device buffers of one test, freed at the end"""
    def __init__(self, ctx):
        self.ctx, self.bufs = ctx, []

    def __call__(self, nbytes, fill=None):
        p = self.ctx.alloc(nbytes)
        self.bufs.append(p)
        if fill is not None:
            self.ctx.h2d(p, np.full(nbytes, fill, np.uint8))
        return p

    def close(self):
        for p in self.bufs:
            self.ctx.free(p)


def run(ctx, dev, frames, **kw):
    """frames [F][E][R] host -> (bytes [F][400][500], peaks [F])"""
    F, e, r = frames.shape
    rf = dev(frames.nbytes); ctx.h2d(rf, frames)
    out = dev(F * N, 0xA5); peak = dev(4 * F, 0xA5)
    ctx.bmode_frames(rf, F, e, r, out, peak_dev=peak, **kw)
    ctx.synchronize()
    return ctx.d2h(out, (F,) + OUT, np.uint8), ctx.d2h(peak, (F,), np.float32)


TGC = (0.02 * np.arange(R)).astype(np.float32)         # 0 .. 9.3 dB with depth


@pytest.mark.parametrize("mode", ["db", "ref_log"])
@pytest.mark.parametrize("ref,gain,tgc", [(None, 0.0, None), (None, 6.0, TGC), (2.5, 0.0, None), (2.5, -10.0, TGC)])
def test_synthetic_frames_match_the_mirror(mcrt, orc, ctx, mode, ref, gain, tgc):
    frames, band = synthetic_frames()
    dev = Dev(ctx)
    try:
        kw = dict(mode=mode, ref=ref, gain_db=gain, tgc_db=tgc, dynamic_range_db=48.0)
        got, peak = run(ctx, dev, frames, **kw)
        want, refs, _ = bm.bmode(orc, frames, mode=mode, ref=ref, gain_db=gain, tgc_db=tgc, dynamic_range_db=48.0)
        for f in range(3):
            bm.assert_close(got[f], want[f])
        assert np.array_equal(peak.view(np.uint32), refs.view(np.uint32))          # the reference each frame used, bit for bit
        y0, x0, all_in, none_in = bm.tap_boxes(mcrt.host_scan_maps(E, R), E, R)
        assert none_in.sum() > 10000 and np.all(got[:, none_in] == 0)              # outside the sector
        if ref is None:
            assert refs[2] == 0 and not got[2].any()                               # the all-zero frame is black
        else:
            assert refs[2] == np.float32(ref)
        # inside a plateau of frame 0, away from the non-finite scan-lines, every pixel has the plateau's exact grey
        bad_cols = {40, 41, 90}
        ok = all_in & (band[np.clip(y0, 0, R - 1)] == band[np.clip(y0 + 1, 0, R - 1)]) & ~np.isin(x0, [c - 1 for c in bad_cols] + list(bad_cols))
        if tgc is None:
            for b in range(12):
                m = ok & (band[np.clip(y0, 0, R - 1)] == b)
                if m.sum() == 0:
                    continue
                g = bm.grey(np.array([3.0 * 2.0 ** -b], np.float32), refs[0], mode, gain, 48.0)
                assert np.all(got[0][m] == bm.quantise(g)[0]), (b, np.unique(got[0][m]))
        assert got[0][ok].max() > 0
    finally:
        dev.close()


def test_invariances(mcrt, orc, ctx):
    frames, _ = synthetic_frames()
    dev = Dev(ctx)
    try:
        a, pa = run(ctx, dev, frames, tgc_db=TGC)
        b, pb = run(ctx, dev, frames * np.float32(4.0), tgc_db=TGC)
        assert np.array_equal(a, b) and np.array_equal(pb, pa * 4)           # a power-of-two scale leaves a / ref unchanged, bit for bit
        c, _ = run(ctx, dev, frames, ref=2.0, tgc_db=np.full(R, 6.0206, np.float32))
        d, _ = run(ctx, dev, frames, ref=1.0)                                  # +6.0206 dB everywhere == half the reference
        bm.assert_close(c, d)
    finally:
        dev.close()


def test_back_to_back_calls_each_get_their_own_tgc_curve(mcrt, orc, ctx):
    """five calls with no synchronisation between them -- curves A, B, A, C of one length, then a curve of another -- every curve handed over
    in ONE host array that is overwritten as soon as each call returns: every frame shows its own curve, and the peaks are its own bit for bit"""
    e, rows, cols = 16, 33, 35
    rng = np.random.default_rng(5)
    curves = [rng.uniform(-6.0, 12.0, r).astype(np.float32) for r in (64, 64, 64, 128)]
    order = [curves[0], curves[1], curves[0], curves[2], curves[3]]
    frames = [(rng.rayleigh(1.0, (1, e, c.size)) * rng.choice([-1.0, 1.0], (1, e, c.size))).astype(np.float32) for c in order]
    dev = Dev(ctx)
    try:
        rfs = []
        for fr in frames:
            rfs.append(dev(fr.nbytes)); ctx.h2d(rfs[-1], fr)
        outs = [dev(rows * cols, 0xA5) for _ in order]; peaks = [dev(4, 0xA5) for _ in order]
        ctx.synchronize()
        buf = np.empty(128, np.float32)
        for rf, c, out, peak in zip(rfs, order, outs, peaks):
            buf[:c.size] = c
            ctx.bmode_frames(rf, 1, e, c.size, out, peak_dev=peak, tgc_db=buf[:c.size], dynamic_range_db=48.0, out_rows=rows, out_cols=cols)
            buf[:] = np.nan                            # the call has returned: the curve is the caller's again
        ctx.synchronize()
        for i, (fr, c, out, peak) in enumerate(zip(frames, order, outs, peaks)):
            want, refs, _ = bm.bmode(orc, fr, tgc_db=c, dynamic_range_db=48.0, out_rows=rows, out_cols=cols)
            got = ctx.d2h(out, (rows, cols), np.uint8)
            print("call %d: %d of %d pixels differ from the mirror" % (i, np.count_nonzero(got != want[0]), got.size))
            bm.assert_close(got, want[0])
            assert got.any()
            assert np.array_equal(ctx.d2h(peak, (1,), np.float32).view(np.uint32), refs.view(np.uint32)), i
        assert not np.array_equal(bm.bmode(orc, frames[1], tgc_db=curves[0], dynamic_range_db=48.0, out_rows=rows, out_cols=cols)[0],
                                  bm.bmode(orc, frames[1], tgc_db=curves[1], dynamic_range_db=48.0, out_rows=rows, out_cols=cols)[0])   # (a wrong curve would show)
    finally:
        dev.close()


def _traced(mcrt, sphere, tex256, F, **kw):
    cfg, sd = sphere
    Es, S = 64, 48
    tr = mcrt.Transducer(Es, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    sim = mcrt.Simulator(sd, tr, n_samples=S, texture=tex256, **kw)
    dev = sim.ctx.alloc(F * Es * sim.R * 4)
    sim.ctx.trace_frames(3, F, dev)
    sim.ctx.convolve_frames(dev, F, Es, sim.R, sim.psf.axial_kernel, sim.psf.lateral_kernel)
    sim.ctx.envelope_frames(dev, F, Es, sim.R)
    return sim, dev, Es


@pytest.mark.parametrize("sanitize", [1, 0])
def test_a_traced_pass(mcrt, orc, sphere, tex256, sanitize):
    F = 4
    sim, rf, Es = _traced(mcrt, sphere, tex256, F, sanitize_tir=sanitize)
    ctx, Rr = sim.ctx, sim.R
    dev = Dev(ctx)
    try:
        if sanitize == 0:       # scan-lines the reference leaves NaN (total internal reflection), as whole stretches of an image
            env = ctx.d2h(rf, (F, Es, Rr))
            env[:, 20:23, 150:] = np.nan
            env[2, 40] = np.nan
            ctx.h2d(rf, env)
        env = ctx.d2h(rf, (F, Es, Rr))
        out = dev(F * N, 0)
        ctx.bmode_frames(rf, F, Es, Rr, out)
        got = ctx.d2h(out, (F,) + OUT, np.uint8)
        want, refs, _ = bm.bmode(orc, env)
        for f in range(F):
            bm.assert_close(got[f], want[f])
            assert np.count_nonzero(got[f]) > 1000
        one = dev(N, 0)
        for f in range(F):
            ctx.bmode_frames(rf + f * Es * Rr * 4, 1, Es, Rr, one)
            assert np.array_equal(ctx.d2h(one, OUT, np.uint8), got[f]), f
        if sanitize == 0:
            assert np.isnan(env).any()
            y0, x0, all_in, _ = bm.tap_boxes(mcrt.host_scan_maps(Es, Rr), Es, Rr)
            dead = all_in & np.isin(x0, [20, 21]) & (y0 >= 150)                 # all four taps NaN
            assert dead.sum() > 100 and np.all(got[:, dead] == 0)
        # a first look at the dynamic range of a traced frame: the peak over the median in-sector amplitude
        a = np.abs(env[0][np.isfinite(env[0])])
        print("dynamic range of a traced sphere frame: peak / median = %.3g (%.1f dB)" % (a.max() / np.median(a[a > 0]), 20 * math.log10(a.max() / np.median(a[a > 0]))))
    finally:
        dev.close()
        ctx.free(rf)
        sim.close()


def test_persistence(mcrt, orc, ctx):
    frames, _ = synthetic_frames()
    rng = np.random.default_rng(11)
    frames = np.concatenate([frames, (rng.rayleigh(1.0, (1, E, R)) * 2.0).astype(np.float32)])[[0, 1, 3, 2]]
    dev = Dev(ctx)
    try:
        rf = dev(frames.nbytes); ctx.h2d(rf, frames)
        st = dev(4 * N)
        four = dev(4 * N, 0)
        ctx.bmode_frames(rf, 4, E, R, four, persistence=0.5, state_dev=st, reset_state=True)
        g4 = ctx.d2h(four, (4,) + OUT, np.uint8)
        s4 = ctx.d2h(st, OUT)
        want, _, ys = bm.bmode(orc, frames, persistence=0.5)
        for f in range(4):
            bm.assert_close(g4[f], want[f])
        # two calls of two frames with the state == one call of four, bit for bit
        ctx.h2d(st, np.full(OUT, np.nan, np.float32))                         # ... and reset_state ignores what the state held
        two = dev(4 * N, 0)
        ctx.bmode_frames(rf, 2, E, R, two, persistence=0.5, state_dev=st, reset_state=True)
        ctx.bmode_frames(rf + 2 * E * R * 4, 2, E, R, two + 2 * N, persistence=0.5, state_dev=st, reset_state=False)
        assert np.array_equal(ctx.d2h(two, (4,) + OUT, np.uint8), g4)
        assert np.array_equal(ctx.d2h(st, OUT).view(np.uint32), s4.view(np.uint32))
        assert np.abs(s4 - ys).max() < 1e-5
        # a state carried in from before: the mirror's too
        carried = dev(4 * N, 0)
        ctx.bmode_frames(rf, 4, E, R, carried, persistence=0.5, state_dev=st, reset_state=False)
        w2, _, _ = bm.bmode(orc, frames, persistence=0.5, state=s4, reset_state=False)
        for f in range(4):
            bm.assert_close(ctx.d2h(carried, (4,) + OUT, np.uint8)[f], w2[f])
        # alpha = 0: the state is neither needed nor read
        a0, b0 = dev(4 * N, 0), dev(4 * N, 0)
        ctx.h2d(st, np.full(OUT, np.nan, np.float32))
        ctx.bmode_frames(rf, 4, E, R, a0, persistence=0.0, state_dev=st, reset_state=False)
        ctx.bmode_frames(rf, 4, E, R, b0)
        assert np.array_equal(ctx.d2h(a0, (4,) + OUT, np.uint8), ctx.d2h(b0, (4,) + OUT, np.uint8))
    finally:
        dev.close()


def test_invalid_arguments_leave_the_output_untouched(mcrt, ctx):
    frames, _ = synthetic_frames()
    dev = Dev(ctx)
    try:
        rf = dev(frames.nbytes); ctx.h2d(rf, frames)
        out = dev(3 * N, 0x5A)
        bad_tgc = TGC.copy(); bad_tgc[7] = np.inf
        cases = [(dict(rf_dev=None), "null rf_dev"), (dict(out_dev=None), "null out_dev"), (dict(mode=2), "unknown mode"),
                 (dict(dynamic_range_db=0.0), "dynamic_range_db"), (dict(dynamic_range_db=-3.0), "dynamic_range_db"),
                 (dict(dynamic_range_db=float("inf")), "dynamic_range_db"), (dict(dynamic_range_db=float("nan")), "dynamic_range_db"),
                 (dict(persistence=1.0), "persistence"), (dict(persistence=-0.25), "persistence"), (dict(persistence=float("nan")), "persistence"),
                 (dict(ref=float("nan")), "ref must be finite"), (dict(ref=float("inf")), "ref must be finite"),
                 (dict(tgc_db=bad_tgc), "tgc_db[7]")]
        for kw, msg in cases:
            args = dict(rf_dev=rf, out_dev=out)
            args.update(kw)
            rfd, outd = args.pop("rf_dev"), args.pop("out_dev")
            with pytest.raises(mcrt.McrtError) as e:
                ctx.bmode_frames(rfd, 3, E, R, outd, **args)
            assert e.value.code == -1 and msg in str(e.value), (kw, str(e.value))
        ctx.synchronize()
        assert np.all(ctx.d2h(out, (3 * N,), np.uint8) == 0x5A)
        with pytest.raises(mcrt.McrtError) as e:
            ctx.bmode_frames(rf, 65536, E, R, out)
        assert e.value.code == -5
    finally:
        dev.close()


def test_group_root_equals_single_context(mcrt, sphere, tex256):
    cfg, sd = sphere
    Es, S, F = 16, 64, 3
    tr = mcrt.Transducer(Es, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    psf = mcrt.Psf(freq=tr.frequency)
    one = mcrt.Context(0)
    grp = mcrt.Group([0, 0])
    try:
        for obj in (one, grp):
            obj.set_params(n_elements=Es, n_samples=S, frequency=tr.frequency)
            obj.upload_scene(sd); obj.upload_texture(tex256, 256); obj.set_transducer(tr.pos, tr.dir)
        Rr = one.params.n_rows
        got = []
        for c, trace in ((one, one.trace_frames), (grp.root, grp.trace_frames)):
            rf = c.alloc(F * Es * Rr * 4); out = c.alloc(F * N)
            trace(5, F, rf)
            c.convolve_frames(rf, F, Es, Rr, psf.axial_kernel, psf.lateral_kernel)
            c.envelope_frames(rf, F, Es, Rr)
            c.bmode_frames(rf, F, Es, Rr, out, tgc_db=TGC, persistence=0.25)
            got.append(c.d2h(out, (F,) + OUT, np.uint8))
            c.free(rf); c.free(out)
        grp.synchronize()
        assert np.array_equal(got[0], got[1]) and got[0].any()
    finally:
        grp.close()
        one.close()


def test_cli_display_options(mcrt, orc, tmp_path):
    exe = os.path.join(ROOT, "mcray-tracing_amd", "mattausch_hip")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "mcray-tracing_amd"), "mattausch_hip"])
    cfg, meshes = mcrt.synth.sphere_scene(3)
    cfg["workingDirectory"] = str(tmp_path) + "/"
    for f, (V, F) in meshes.items():
        mcrt.scene_io.save_obj(str(tmp_path / f), V, F)
    (tmp_path / "sphere.scene").write_text(json.dumps(cfg))
    scene = str(tmp_path / "sphere.scene")
    r = subprocess.run([exe, scene, "3", "5", str(tmp_path / "db.pgm"), str(tmp_path / "rf.bin"), "--db", "60"], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    pgm = (tmp_path / "db.pgm").read_bytes()
    assert len(pgm) == 15 + N and pgm[:15] == b"P5\n500 400\n255\n"
    env = np.fromfile(str(tmp_path / "rf.bin"), np.float32).reshape(465, 512)
    want, _, _ = bm.bmode(orc, np.ascontiguousarray(env.T)[None])
    bm.assert_close(np.frombuffer(pgm[15:], np.uint8).reshape(OUT), want[0])
    # without display options: today's linear file, (uint8)(v * 255) of the float scan conversion
    r = subprocess.run([exe, scene, "3", "5", str(tmp_path / "lin.pgm"), str(tmp_path / "rf2.bin")], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert (tmp_path / "rf2.bin").read_bytes() == (tmp_path / "rf.bin").read_bytes()
    x = orc.scan_convert(env) * np.float32(255.0)
    lin = np.where(np.isnan(x) | (x < 0), 0, np.where(x > 255, 255, np.nan_to_num(x))).astype(np.uint8)
    assert (tmp_path / "lin.pgm").read_bytes() == b"P5\n500 400\n255\n" + lin.tobytes()
    # the other options parse and run
    r = subprocess.run([exe, scene, "2", "5", str(tmp_path / "rl.pgm"), "--ref-log", "--gain", "3", "--persistence", "0.5"],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and len((tmp_path / "rl.pgm").read_bytes()) == 15 + N, r.stdout + r.stderr


def test_simulator_bmode(mcrt, sphere, tex256):
    cfg, sd = sphere
    tr = mcrt.Transducer(32, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    sim = mcrt.Simulator(sd, tr, n_samples=32, texture=tex256)
    try:
        img = sim.bmode(0, dynamic_range_db=50.0)
        assert img.dtype == np.uint8 and img.shape == OUT and img.max() > 200 and np.count_nonzero(img) > 1000
    finally:
        sim.close()
