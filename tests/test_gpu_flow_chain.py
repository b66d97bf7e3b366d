"""Colour Doppler end to end on the MI355X: a box of LIVER with a vascular sphere of BLOOD under 64 scan-lines.  Simulator.colour_flow()
against the same chain by hand through Context calls, byte for byte; where the colour lies against the ground-truth labels; no colour
without motion; the estimate against the registered truth; what flow= leaves alone; and what it refuses."""
import json
import os
import subprocess
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

f32 = np.float32
E, ROWS, COLS = 64, 200, 250
VEL = (-150.0, 40.0, 0.0)              # the probe looks along +x: the blood comes towards it


@pytest.fixture(scope="module")
def small(mcrt):
    cfg, meshes = mcrt.synth.sphere_scene(3)
    cfg["meshes"][1] = dict(cfg["meshes"][1], material="BLOOD", vascular=True)          # the sphere's record: a vessel's
    sd = mcrt.scene_io.build_scene(cfg, meshes)
    tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    return sd, tr, mcrt.host_texture(32)


def make_sim(mcrt, small, **kw):
    sd, tr, tex = small
    return mcrt.Simulator(sd, tr, n_samples=8, texture=tex, tex_n=32, **kw)


def by_hand(mcrt, sim, frame_id, flow, noise, out_rows, out_cols):
    """colour_flow()'s chain through Context calls alone, on sim's context and scene"""
    ctx, R = sim.ctx, sim.R
    n, npix = E * R, out_rows * out_cols
    names = sim.material_names
    vel = np.zeros((len(names), 3), f32); vel[names.index("BLOOD")] = flow["velocity_mm_s"]["BLOOD"]
    opts = mcrt.flow_opts_struct(**{k: v for k, v in flow.items() if k in ("n_packets", "wall", "avg_rows", "avg_lines", "prf_hz", "sigma", "seed")})
    v_nyq = mcrt.host_flow_nyquist(sim.tr.frequency, ctx.params.speed_of_sound, opts=opts)
    phasor, truth = mcrt.host_flow_phasors(v_nyq, vel, sim.tr.dir)
    bufs = [ctx.alloc(size) for size in (4 * n, n, 8 * n, 16 * n, 12 * n, 4 * n, 4, npix, 12 * npix, 3 * npix, 4 * npix)]
    rf, tissue, parts, iq, corr, truth_dev, sigma_dev, grey, img, rgb, velimg = bufs
    try:
        ctx.trace_frame(frame_id, rf)
        ctx.label_frames(tissue_dev=tissue)
        ctx.flow_split_frames(rf, tissue, 1, E, R, (vel != 0).any(axis=1), parts)
        ctx.convolve_frames(rf, 1, E, R, sim.psf.axial_kernel, sim.psf.lateral_kernel)
        if noise is not None:
            ctx.noise_frames(rf, 1, 1, E, R, first_image_id=frame_id, sigma_dev=sigma_dev, **noise)
        ctx.envelope_frames(rf, 1, E, R)
        ctx.convolve_frames(parts, 2, E, R, sim.psf.axial_kernel, sim.psf.lateral_kernel)
        ctx.detect_frames(parts, 2, E, R, iq_dev=iq)
        ctx.flow_frames(iq, iq + 8 * n, tissue, 1, E, R, v_nyq, phasor, truth, first_image_id=frame_id, sigma_dev=sigma_dev if noise is not None else None,
                        corr_dev=corr, truth_dev=truth_dev, opts=opts)
        sigma = float(ctx.d2h(sigma_dev, (1,))[0]) if noise is not None else float(opts.sigma)
        ctx.bmode_frames(rf, 1, E, R, grey, out_rows=out_rows, out_cols=out_cols)
        ctx.scan_convert_frames(corr, 3, E, R, img, out_rows=out_rows, out_cols=out_cols)
        ctx.colour_frames(img, grey, 1, out_rows, out_cols, v_nyq, rgb, vel_img_dev=velimg, power_thr=flow.get("power_scale", 4.0) * 2.0 * opts.n_packets * sigma * sigma,
                          vel_thr_mm_s=flow.get("vel_thr_mm_s"), grey_max=flow.get("grey_max"))
        return dict(rgb=ctx.d2h(rgb, (out_rows, out_cols, 3), np.uint8), grey=ctx.d2h(grey, (out_rows, out_cols), np.uint8),
                    velocity=ctx.d2h(velimg, (out_rows, out_cols)), truth=ctx.d2h(truth_dev, (E, R)), corr=ctx.d2h(corr, (3, E, R)))
    finally:
        for b in bufs:
            ctx.free(b)


@pytest.mark.parametrize("noise", [None, dict(snr_db=30.0, seed=7)])
def test_colour_flow_equals_the_chain_by_hand(mcrt, small, noise):
    flow = dict(velocity_mm_s={"BLOOD": VEL}, n_packets=8, wall="mean", avg_rows=2, avg_lines=1, sigma=0.0 if noise else 2e-4, seed=99, vel_thr_mm_s=5.0, grey_max=250)
    sim = make_sim(mcrt, small, flow=flow, noise=noise)
    try:
        got = sim.colour_flow(3, out_rows=ROWS, out_cols=COLS)
        want = by_hand(mcrt, sim, 3, flow, noise, ROWS, COLS)
        for k in ("rgb", "grey", "velocity", "truth", "corr"):
            assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
            assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), k
        coloured = (got["rgb"] != got["grey"][..., None]).any(axis=-1)
        assert coloured.any() and (got["velocity"][~coloured] == 0).all()
    finally:
        sim.close()


@pytest.fixture(scope="module")
def quiet(mcrt, small):
    """sigma 0, a window of the sample itself: a pixel has power exactly where a sample it gathers from has a moving echo"""
    sim = make_sim(mcrt, small, flow=dict(velocity_mm_s={"BLOOD": VEL}, avg_rows=0, avg_lines=0))
    try:
        yield sim, sim.colour_flow(1, out_rows=ROWS, out_cols=COLS), sim.labels(out_rows=ROWS, out_cols=COLS), sim.flow_velocity(1)
    finally:
        sim.close()


def test_colour_lies_where_the_blood_is(mcrt, small, quiet):
    """Coloured pixels against labels()["picture"].  The label picture is gathered nearest-neighbour and the autocorrelation bilinearly
    (mcrt_scan_convert_frames, the contract), so a pixel is reached by the blood of any of the four samples about it: asserted is that
    every coloured pixel has BLOOD among the samples it gathers from -- the bilinear gather of the samples' BLOOD indicator is > 0 there
    --, that no pixel whose four samples are all BLOOD-free is coloured, and that the coloured pixels the nearest-neighbour picture calls
    something else are that one-sample rim and no more (printed: their share)."""
    sim, pic, labels, _ = quiet
    blood = small[0].material_names.index("BLOOD")
    coloured = (pic["rgb"] != pic["grey"][..., None]).any(axis=-1)
    assert coloured.sum() > 100
    ind = (labels["tissue"] == blood).astype(f32)
    assert ind.any()
    p_in = sim.ctx.alloc(ind.nbytes); p_out = sim.ctx.alloc(ROWS * COLS * 4)
    try:
        sim.ctx.h2d(p_in, ind)
        sim.ctx.scan_convert_frames(p_in, 1, E, sim.R, p_out, out_rows=ROWS, out_cols=COLS)
        reach = sim.ctx.d2h(p_out, (ROWS, COLS))
    finally:
        sim.ctx.free(p_in); sim.ctx.free(p_out)
    assert not coloured[reach == 0].any(), "%d coloured pixels gather from no BLOOD sample" % int(coloured[reach == 0].sum())
    inside = labels["picture"] == blood
    rim = coloured & ~inside
    print("coloured %d pixels, %d of them (%.1f %%) on the rim the nearest-neighbour label picture calls another tissue"
          % (coloured.sum(), rim.sum(), 100.0 * rim.sum() / coloured.sum()))
    assert (reach[rim] > 0).all() and (reach[rim] < 1).all()                 # the rim is mixed pixels only
    assert (coloured & inside).any()                                         # and the lumen itself is coloured where the blood echoes
    # the blood comes towards the probe: the coloured pixels are red (a sample whose blood echo is lost in the rounding of the liver echo
    # the PSF leaked beside it has any phase; such samples are few)
    towards = pic["velocity"][coloured] > 0
    print("%.2f %% of the coloured pixels read towards the probe" % (100.0 * towards.mean()))
    assert towards.mean() > 0.9 and ((pic["rgb"][coloured][:, 0] >= 129) == towards).all()


def test_estimate_reads_the_truth_in_the_lumen(mcrt, small, quiet):
    """in beam space, at sigma 0 with mean removal: where the blood echoes, the Kasai velocity is the registered truth to within the wall
    filter's bias.  At this phase step (|phi| about 1.3 rad) mean removal over 8 pulses takes under 2 % of the blood's own power and
    biases the angle by under 0.05 rad where blood alone echoes; samples with leaked liver echo beside the wall are wider, so the
    median is asserted, at 0.05 rad * v_nyq / pi."""
    sim, pic, labels, beams = quiet
    blood = small[0].material_names.index("BLOOD")
    lumen = (labels["tissue"] == blood) & (pic["corr"][0] > 0)
    assert lumen.sum() > 50 and (beams["truth"][labels["tissue"] != blood] == 0).all() and (beams["truth"][lumen] > 0).all()
    assert np.array_equal(beams["truth"].view(np.uint32), pic["truth"].view(np.uint32))
    v_nyq = sim.flow["v_nyq"]
    err = np.abs(beams["vel"][lumen] - beams["truth"][lumen])
    print("lumen: %d samples, truth %.1f .. %.1f mm/s, median |vel - truth| %.3f mm/s, worst %.3f" % (lumen.sum(), beams["truth"][lumen].min(),
                                                                                                      beams["truth"][lumen].max(), np.median(err), err.max()))
    assert np.median(err) < 0.05 * v_nyq / np.pi
    assert (beams["var"] >= 0).all() and (beams["var"] <= 1).all()


def test_nothing_moves_nothing_is_coloured(mcrt, small):
    """velocity 0: every phasor is (1, 0), the mean filter takes everything at sigma 0, and the picture is bmode()'s own"""
    sim = make_sim(mcrt, small, flow={"BLOOD": (0.0, 0.0, 0.0)})
    try:
        pic = sim.colour_flow(2, out_rows=ROWS, out_cols=COLS)
        assert (pic["rgb"] == pic["grey"][..., None]).all() and not pic["velocity"].any() and not pic["corr"].view(np.uint32).any() and not pic["truth"].any()
        assert np.array_equal(pic["grey"], sim.bmode(2, out_rows=ROWS, out_cols=COLS))
    finally:
        sim.close()


def test_flow_leaves_bmode_alone(mcrt, small):
    """without flow= the simulator never heard of it; with flow= every other method gives the same bytes, before and after colour_flow()"""
    plain = make_sim(mcrt, small, noise=dict(snr_db=35.0))
    with_flow = make_sim(mcrt, small, noise=dict(snr_db=35.0), flow={"BLOOD": VEL})
    try:
        assert plain.flow is None
        want = plain.bmode(4, out_rows=ROWS, out_cols=COLS), plain.frame(4)
        assert np.array_equal(with_flow.bmode(4, out_rows=ROWS, out_cols=COLS), want[0])
        pic = with_flow.colour_flow(4, out_rows=ROWS, out_cols=COLS)
        assert np.array_equal(pic["grey"], want[0])                          # the underlay IS bmode()'s picture
        assert np.array_equal(with_flow.bmode(4, out_rows=ROWS, out_cols=COLS), want[0])
        assert np.array_equal(with_flow.frame(4).view(np.uint32), want[1].view(np.uint32))
        with pytest.raises(RuntimeError, match="flow="):
            plain.colour_flow()
        with pytest.raises(RuntimeError, match="flow="):
            plain.flow_velocity()
    finally:
        plain.close(); with_flow.close()


def test_what_flow_refuses(mcrt, small):
    sd, tr, tex = small
    with pytest.raises(ValueError, match="no material"):
        make_sim(mcrt, small, flow={"PLASMA": VEL})
    with pytest.raises(TypeError):
        make_sim(mcrt, small, flow=dict(velocity_mm_s={"BLOOD": VEL}, packets=8))
    with pytest.raises(mcrt.McrtError):
        make_sim(mcrt, small, flow=dict(velocity_mm_s={"BLOOD": VEL}, n_packets=17))
    for kw, word in ((dict(sweep=(3, 0.02)), "sweep="), (dict(compound=(-0.1, 0.1)), "compound="), (dict(elevation=True), "elevation="),
                     (dict(psf=mcrt.Psf(freq=tr.frequency, bands=(3.5, 4.5, 5.5))), "bands")):
        sim = make_sim(mcrt, small, flow={"BLOOD": VEL}, **kw)
        try:
            for call in (sim.colour_flow, sim.flow_velocity):
                with pytest.raises(RuntimeError, match=word):
                    call()
        finally:
            sim.close()


# ------------------------------------------------------------------ the C++ shim and the CLI
def _write_scene(mcrt, tmp_path):
    cfg, meshes = mcrt.synth.sphere_scene(3)
    cfg["meshes"][1] = dict(cfg["meshes"][1], material="BLOOD", vascular=True)
    cfg["workingDirectory"] = str(tmp_path) + "/"
    for f, (V, F) in meshes.items():
        mcrt.scene_io.save_obj(str(tmp_path / f), V, F)
    (tmp_path / "vessel.scene").write_text(json.dumps(cfg))
    return cfg, str(tmp_path / "vessel.scene")


@pytest.mark.parametrize("noise_db", [None, 30.0])
def test_host_shim(mcrt, tmp_path, noise_db):
    """tests/host/flow_driver.cpp -- trace, rf_image::flow_split, the B-mode chain, rf_image::colour_flow -- writes the Python path's bytes"""
    pkg = os.path.join(ROOT, "mcray-tracing_amd")
    exe = str(tmp_path / "flow_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(pkg, "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "flow_driver.cpp"), "-L", pkg, "-lmcrt_hip", "-Wl,-rpath," + pkg])
    cfg, scene = _write_scene(mcrt, tmp_path)
    sigma = 0.0 if noise_db else 1e-4
    out = tmp_path / "flow.bin"
    r = subprocess.run([exe, scene, str(out), "2", "BLOOD"] + [str(v) for v in VEL] + [str(sigma)] + ([str(noise_db)] if noise_db else []),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    blob = out.read_bytes()
    npix, R = ROWS * COLS, 465
    assert len(blob) == 3 * npix + npix + 4 * npix + 3 * 4 * E * R
    sd = mcrt.scene_io.load_scene_file(scene)
    tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    sim = mcrt.Simulator(sd, tr, n_samples=8, flow=dict(velocity_mm_s={"BLOOD": VEL}, sigma=sigma), noise=dict(snr_db=noise_db) if noise_db else None)
    try:
        pic = sim.colour_flow(2, out_rows=ROWS, out_cols=COLS)
        beams = sim.flow_velocity(2)
    finally:
        sim.close()
    assert (pic["rgb"] != pic["grey"][..., None]).any()
    at = 0
    for name, want in (("rgb", pic["rgb"]), ("grey", pic["grey"]), ("velocity", pic["velocity"]), ("vel", beams["vel"]), ("var", beams["var"]), ("truth", beams["truth"])):
        assert blob[at:at + want.nbytes] == want.tobytes(), name
        at += want.nbytes


def test_cli(mcrt, tmp_path):
    """mattausch_hip --colour-flow: the PPM and --flow-truth are the Python Simulator's bytes, the PGM beside it is bmode()'s; options that
    make no sense end the program before it touches a device"""
    exe = os.path.join(ROOT, "mcray-tracing_amd", "mattausch_hip")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "mcray-tracing_amd"), "mattausch_hip"])
    cfg, scene = _write_scene(mcrt, tmp_path)
    ppm, truth, pgm = tmp_path / "flow.ppm", tmp_path / "truth.raw", tmp_path / "b.pgm"
    r = subprocess.run([exe, scene, "1", "5", str(pgm), str(tmp_path / "rf.bin"), "--colour-flow", str(ppm), "--flow-velocity", "BLOOD:-150,40,0", "--flow-packets", "6",
                        "--flow-prf-hz", "3000", "--flow-wall", "linear", "--flow-avg", "1,2", "--flow-vel-thr", "8", "--flow-grey-max", "240", "--flow-truth", str(truth),
                        "--noise-db", "35"], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    sd = mcrt.scene_io.load_scene_file(scene)
    tr = mcrt.Transducer(512, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    sim = mcrt.Simulator(sd, tr, n_samples=5, noise=dict(snr_db=35.0),
                         flow=dict(velocity_mm_s={"BLOOD": VEL}, n_packets=6, prf_hz=3000.0, wall="linear", avg_rows=1, avg_lines=2, vel_thr_mm_s=8.0, grey_max=240))
    try:
        pic = sim.colour_flow(0)
    finally:
        sim.close()
    assert (pic["rgb"] != pic["grey"][..., None]).any()
    assert ppm.read_bytes() == b"P6\n500 400\n255\n" + pic["rgb"].tobytes()
    assert truth.read_bytes() == pic["truth"].tobytes()
    assert pgm.read_bytes() == b"P5\n500 400\n255\n" + pic["grey"].tobytes()
    for bad, word in ((["--flow-packets", "8"], "--colour-flow"), (["--colour-flow", "x.ppm"], "--flow-velocity"),
                      (["--colour-flow", "x.ppm", "--flow-velocity", "BLOOD:1,2"], "NAME:vx,vy,vz"), (["--colour-flow", "x.ppm", "--flow-velocity", "PLASMA:1,2,3"], "PLASMA"),
                      (["--colour-flow", "x.ppm", "--flow-velocity", "BLOOD:1,2,3", "--flow-packets", "17"], "n_packets"),
                      (["--colour-flow", "x.ppm", "--flow-velocity", "BLOOD:1,2,3", "--flow-wall", "median"], "none, mean or linear"),
                      (["--colour-flow", "x.ppm", "--flow-velocity", "BLOOD:1,2,3", "--compound", "3"], "--colour-flow"),
                      (["--colour-flow", "x.ppm", "--flow-velocity", "BLOOD:1,2,3", "--freq-compound", "3"], "--colour-flow"),
                      (["--colour-flow", "x.ppm", "--flow-velocity", "BLOOD:1,2,3", "--elevation", "3"], "--colour-flow")):
        r = subprocess.run([exe, scene, "1", "5"] + bad, capture_output=True, text=True, timeout=240, cwd=str(tmp_path))
        assert r.returncode == 1 and word in r.stdout, (bad, r.stdout)
