"""M-mode end to end on the MI355X: a box of LIVER with a sphere of KIDNEY that pulsates under 64 scan-lines.  Simulator.m_mode() against
the same chain by hand through Context calls, byte for byte, and against the numpy mirror; the labels and the true displacement against
labels() of the still frame; what motion= refuses; what it leaves alone; the C++ shim and the CLI."""
import json
import os
import subprocess
import numpy as np
import pytest

import mmode_mirror as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

f32 = np.float32
E, ROWS, COLS = 64, 200, 250
MOTION = dict(dilation={"KIDNEY": -0.05}, prf_hz=100.0, beats_per_min=60.0, n_pulses=128)


def _scene(mcrt):
    cfg, meshes = mcrt.synth.sphere_scene(3)
    cfg["meshes"][1] = dict(cfg["meshes"][1], material="KIDNEY")                        # the sphere's record: a vessel that pulsates
    return cfg, meshes


@pytest.fixture(scope="module")
def small(mcrt):
    cfg, meshes = _scene(mcrt)
    sd = mcrt.scene_io.build_scene(cfg, meshes)
    tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    return sd, tr, mcrt.host_texture(32)


def make_sim(mcrt, small, **kw):
    sd, tr, tex = small
    return mcrt.Simulator(sd, tr, n_samples=8, texture=tex, tex_n=32, **kw)


def by_hand(mcrt, sim, frame_id, line, motion, noise, hop, height, row_lo, row_hi):
    """m_mode()'s chain through Context calls alone, on sim's context and scene; also the inputs of the two calls, for the mirror"""
    ctx, R = sim.ctx, sim.R
    names = sim.material_names
    T, prf = motion["n_pulses"], motion["prf_hz"]
    dilation = np.zeros(len(names)); dilation[names.index("KIDNEY")] = motion["dilation"]["KIDNEY"]
    dil = mcrt.host_mmode_table(dilation)
    w = mcrt.host_mmode_waveform(prf, motion["beats_per_min"], T)
    b = mcrt.host_mmode_bulk(prf, motion.get("bulk_per_min", 15.0), motion.get("bulk_mm", 0.0) / mcrt.row_pitch_mm(sim.tr.frequency), T)
    cycles = mcrt.host_psf_carrier(sim.tr.frequency)
    n, m, W = E * R, T * R, T // hop
    bufs = [ctx.alloc(size) for size in (4 * n, n, 8 * n, 4 * m, m, 4 * m, height * W, height * W, 4 * height * W)]
    rf, tissue, iq, env, lab, disp, pic, lab_pic, disp_pic = bufs
    try:
        ctx.trace_frame(frame_id, rf)
        ctx.label_frames(tissue_dev=tissue)
        ctx.convolve_frames(rf, 1, E, R, sim.psf.axial_kernel, sim.psf.lateral_kernel)
        if noise is not None:
            ctx.noise_frames(rf, 1, 1, E, R, first_image_id=frame_id, **noise)
        ctx.detect_frames(rf, 1, E, R, iq_dev=iq)
        ctx.mmode_lines_frames(iq, tissue, 1, E, R, [[0, line]], dil, w, b, cycles, first_image_id=frame_id, env_dev=env, truth_disp_dev=disp, truth_label_dev=lab,
                               sigma=motion.get("noise", 0.0), seed=motion.get("seed"))
        ctx.mmode_picture_frames(env, 1, T, R, pic, truth_label_dev=lab, truth_disp_dev=disp, label_out_dev=lab_pic, disp_out_dev=disp_pic, hop=hop, height=height,
                                 row_lo=row_lo, row_hi=row_hi)
        return dict(picture=ctx.d2h(pic, (height, W), np.uint8), labels=ctx.d2h(lab_pic, (height, W), np.uint8), truth_disp=ctx.d2h(disp_pic, (height, W)),
                    env=ctx.d2h(env, (T, R))), dict(iq=ctx.d2h(iq, (1, E, R, 2)), tissue=ctx.d2h(tissue, (1, E, R), np.uint8), dil=dil, w=w, b=b, cycles=cycles)
    finally:
        for p in bufs:
            ctx.free(p)


@pytest.mark.parametrize("noise", [None, dict(snr_db=30.0, seed=7)])
def test_m_mode_equals_the_chain_by_hand_and_the_mirror(mcrt, small, noise):
    motion = dict(MOTION, bulk_mm=0.4, bulk_per_min=30.0, noise=0.0 if noise is None else 1e-4, seed=99)
    sim = make_sim(mcrt, small, motion=motion, noise=noise)
    try:
        pitch = mcrt.row_pitch_mm(sim.tr.frequency)
        got = sim.m_mode(3, line=30, depth_mm=(20.0, 90.0), hop=2, height=150)
        row_lo, row_hi = int(round(20.0 / pitch)), int(round(90.0 / pitch))
        assert (got["lines"]["row_lo"], got["lines"]["row_hi"]) == (row_lo, row_hi)
        want, ins = by_hand(mcrt, sim, 3, 30, motion, noise, 2, 150, row_lo, row_hi)
        for k in sorted(want):
            assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
            assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), k
        assert got["picture"].shape == (150, 64) and got["time_s"].shape == (64,) and got["depth_mm"].shape == (150,)
        assert got["time_s"][1] == 2 / 100.0 and 20.0 - pitch < got["depth_mm"][0] < got["depth_mm"][-1] < 90.0
        lines = mm.lines(ins["iq"], ins["tissue"], [[0, 30]], ins["dil"], ins["w"], ins["b"], ins["cycles"], sigma=motion["noise"], seed=99, first_image_id=3)
        assert np.array_equal(got["env"].view(np.uint32), lines["env"][0].view(np.uint32))
        pic = mm.picture(lines["env"], lines["truth_label"], lines["truth_disp"], hop=2, height=150, row_lo=row_lo, row_hi=row_hi)
        assert np.abs(got["picture"].astype(np.int32) - pic["out"][0].astype(np.int32)).max() <= 1
        assert np.array_equal(got["labels"], pic["label_out"][0]) and np.array_equal(got["truth_disp"].view(np.uint32), pic["disp_out"][0].view(np.uint32))
        assert got["picture"].max() > 128 and (got["truth_disp"] != 0).any() and (got["labels"] == sim.material_names.index("KIDNEY")).any()
    finally:
        sim.close()


def test_truths_are_registered_with_the_still_frame(mcrt, small):
    """where the waveform is 0 (and there is no bulk motion) the column's labels are labels() of the scan-line at the rows the column shows,
    and nothing is displaced; in systole the vessel's far wall moves away from the probe and the tissue above the vessel stays"""
    sim = make_sim(mcrt, small, motion=MOTION)
    try:
        R, line = sim.R, E // 2
        got = sim.m_mode(1, hop=1, height=R)                             # one picture row per line row, one column per pulse
        tissue = sim.labels(picture=False)["tissue"][line]
        names = small[0].material_names
        kidney = np.flatnonzero(tissue == names.index("KIDNEY"))
        assert kidney.size > 20
        w = got["lines"]["w_q16"]
        still = np.flatnonzero(w == 0); beat = int(np.argmax(w))
        assert still.size > 10 and w[beat] > 60000
        for c in still:
            assert np.array_equal(got["labels"][:, c], tissue) and not got["truth_disp"][:, c].any()
        assert not got["truth_disp"][:kidney[0] + 1].any()               # above the vessel nothing moves
        # in systole every row is displaced by the dilations of the labels() above it (the vessel may reach the line's end: nothing is
        # assumed of the anatomy but that the line crosses it): the vessel widens, so what lies below its top is read from further up
        dil = np.where(tissue == names.index("KIDNEY"), int(mm.mmode_table([-0.05])[0]), 0).astype(np.int64)
        D = np.cumsum(dil) - dil
        for c in (beat, beat // 2, beat + 7):
            want = (((D * int(w[c])) >> 16).astype(np.int32).astype(f32) * f32(2.0 ** -24)).astype(f32)
            assert np.array_equal(got["truth_disp"][:, c].view(np.uint32), want.view(np.uint32)), c
        assert (got["truth_disp"][kidney[0] + 1:, beat] < 0).all()
        assert abs(float(got["truth_disp"][kidney[-1], beat]) + 0.05 * (kidney.size - 1) * w[beat] / 65536.0) < 0.01
    finally:
        sim.close()


def test_motion_leaves_frames_alone(mcrt, small):
    """without motion= the simulator never heard of it; with motion= frame() and bmode() give the same bytes, before and after m_mode()"""
    plain = make_sim(mcrt, small, noise=dict(snr_db=35.0))
    moving = make_sim(mcrt, small, noise=dict(snr_db=35.0), motion=MOTION)
    try:
        assert plain.motion is None
        want = plain.bmode(4, out_rows=ROWS, out_cols=COLS), plain.frame(4)
        assert np.array_equal(moving.bmode(4, out_rows=ROWS, out_cols=COLS), want[0])
        moving.m_mode(4)
        assert np.array_equal(moving.bmode(4, out_rows=ROWS, out_cols=COLS), want[0])
        assert np.array_equal(moving.frame(4).view(np.uint32), want[1].view(np.uint32))
        with pytest.raises(RuntimeError, match="motion="):
            plain.m_mode()
    finally:
        plain.close(); moving.close()


def test_what_motion_refuses(mcrt, small):
    sd, tr, tex = small
    with pytest.raises(ValueError, match="no material"):
        make_sim(mcrt, small, motion={"TUMOR": 0.05})
    with pytest.raises(TypeError):
        make_sim(mcrt, small, motion=dict(dilation={"KIDNEY": 0.05}, pulses=8))
    with pytest.raises(mcrt.McrtError):
        make_sim(mcrt, small, motion=dict(dilation={"KIDNEY": 0.3}))                   # above the cap of 25 %
    with pytest.raises(mcrt.McrtError):
        make_sim(mcrt, small, motion=dict(dilation={"KIDNEY": 0.05}, n_pulses=16385))
    with pytest.raises(mcrt.McrtError):
        make_sim(mcrt, small, motion=dict(dilation={"KIDNEY": 0.05}, prf_hz=0.0))
    sim = make_sim(mcrt, small, motion=dict(MOTION, n_pulses=8))
    try:
        with pytest.raises(ValueError, match="scan-line"):
            sim.m_mode(line=E)
        with pytest.raises(ValueError, match="hop"):
            sim.m_mode(hop=9)
        with pytest.raises(ValueError, match="per pulse"):
            sim.m_mode(waveform=np.zeros(7, np.int32))
        with pytest.raises(mcrt.McrtError):
            sim.m_mode(bulk=np.full(8, (32 << 24) + 1, np.int32))
        with pytest.raises(mcrt.McrtError):
            sim.m_mode(height=4097)
    finally:
        sim.close()
    for kw, word in ((dict(sweep=(3, 0.02)), "sweep="), (dict(compound=(-0.1, 0.1)), "compound="), (dict(elevation=True), "elevation="),
                     (dict(psf=mcrt.Psf(freq=tr.frequency, bands=(3.5, 4.5, 5.5))), "bands")):
        sim = make_sim(mcrt, small, motion=MOTION, **kw)
        try:
            with pytest.raises(RuntimeError, match=word):
                sim.m_mode()
        finally:
            sim.close()


# ------------------------------------------------------------------ the C++ shim and the CLI
def _write_scene(mcrt, tmp_path):
    cfg, meshes = _scene(mcrt)
    cfg["workingDirectory"] = str(tmp_path) + "/"
    for f, (V, F) in meshes.items():
        mcrt.scene_io.save_obj(str(tmp_path / f), V, F)
    (tmp_path / "vessel.scene").write_text(json.dumps(cfg))
    return cfg, str(tmp_path / "vessel.scene")


def test_host_shim(mcrt, tmp_path):
    """tests/host/mmode_driver.cpp -- trace, the PSF, rf_image::m_lines, rf_image::m_mode -- writes the Python path's bytes"""
    pkg = os.path.join(ROOT, "mcray-tracing_amd")
    exe = str(tmp_path / "mmode_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(pkg, "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "mmode_driver.cpp"), "-L", pkg, "-lmcrt_hip", "-Wl,-rpath," + pkg])
    cfg, scene = _write_scene(mcrt, tmp_path)
    out = tmp_path / "mmode.bin"
    T, hop, H, R = 96, 3, 120, 465
    r = subprocess.run([exe, scene, str(out), "2", "31", "KIDNEY", "-0.04", str(T), "100", "75", "1.25", "20", str(hop), str(H), "0.0001"],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    blob = out.read_bytes()
    W = T // hop
    assert len(blob) == 2 * H * W + 4 * H * W + 4 * T * R
    sd = mcrt.scene_io.load_scene_file(scene)
    tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    pitch = mcrt.row_pitch_mm(tr.frequency)
    sim = mcrt.Simulator(sd, tr, n_samples=8, motion=dict(dilation={"KIDNEY": -0.04}, prf_hz=100.0, beats_per_min=75.0, n_pulses=T, noise=1e-4))
    try:
        pic = sim.m_mode(2, line=31, hop=hop, height=H, bulk=mcrt.host_mmode_bulk(100.0, 20.0, 1.25, T))
    finally:
        sim.close()
    assert pitch > 0 and (pic["truth_disp"] != 0).any()
    at = 0
    for name in ("picture", "labels", "truth_disp", "env"):
        want = pic[name]
        assert blob[at:at + want.nbytes] == want.tobytes(), name
        at += want.nbytes


def test_cli(mcrt, tmp_path):
    """mattausch_hip --m-mode: the PGM, --m-labels and --m-truth are the Python Simulator's bytes; options that make no sense end the program
    before it touches a device"""
    exe = os.path.join(ROOT, "mcray-tracing_amd", "mattausch_hip")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "mcray-tracing_amd"), "mattausch_hip"])
    cfg, scene = _write_scene(mcrt, tmp_path)
    pgm, labels, truth = tmp_path / "m.pgm", tmp_path / "l.pgm", tmp_path / "t.raw"
    r = subprocess.run([exe, scene, "1", "5", str(tmp_path / "b.pgm"), str(tmp_path / "rf.bin"), "--m-mode", str(pgm), "--m-line", "250", "--motion", "KIDNEY:-0.05,FAT:0.01",
                        "--m-prf", "200", "--m-bpm", "90", "--m-pulses", "160", "--m-hop", "2", "--m-height", "100", "--m-depth-mm", "10,120", "--m-bulk-mm", "0.5,24",
                        "--m-labels", str(labels), "--m-truth", str(truth), "--noise-db", "35"], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    sd = mcrt.scene_io.load_scene_file(scene)
    tr = mcrt.Transducer(512, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    sim = mcrt.Simulator(sd, tr, n_samples=5, noise=dict(snr_db=35.0),
                         motion=dict(dilation={"KIDNEY": -0.05, "FAT": 0.01}, prf_hz=200.0, beats_per_min=90.0, n_pulses=160, bulk_mm=0.5, bulk_per_min=24.0))
    try:
        pic = sim.m_mode(0, line=250, depth_mm=(10.0, 120.0), hop=2, height=100)
    finally:
        sim.close()
    assert (pic["truth_disp"] != 0).any()
    assert pgm.read_bytes() == b"P5\n80 100\n255\n" + pic["picture"].tobytes()
    assert labels.read_bytes() == b"P5\n80 100\n255\n" + pic["labels"].tobytes()
    assert truth.read_bytes() == pic["truth_disp"].tobytes()
    for bad, word in ((["--m-line", "3"], "--m-mode"), (["--m-mode", "x.pgm", "--m-line", "3"], "--motion"), (["--m-mode", "x.pgm", "--motion", "KIDNEY:0.1"], "--m-line"),
                      (["--m-mode", "x.pgm", "--m-line", "3", "--motion", "KIDNEY"], "NAME:e"), (["--m-mode", "x.pgm", "--m-line", "3", "--motion", "TUMOR:0.1"], "TUMOR"),
                      (["--m-mode", "x.pgm", "--m-line", "512", "--motion", "KIDNEY:0.1"], "--m-line"),
                      (["--m-mode", "x.pgm", "--m-line", "3", "--motion", "KIDNEY:0.1", "--m-pulses", "16385"], "--m-pulses"),
                      (["--m-mode", "x.pgm", "--m-line", "3", "--motion", "KIDNEY:0.1", "--m-pulses", "8", "--m-hop", "9"], "--m-hop"),
                      (["--m-mode", "x.pgm", "--m-line", "3", "--motion", "KIDNEY:0.1", "--m-depth-mm", "30,20"], "--m-depth-mm"),
                      (["--m-mode", "x.pgm", "--m-line", "3", "--motion", "KIDNEY:0.1", "--compound", "3"], "--m-mode"),
                      (["--m-mode", "x.pgm", "--m-line", "3", "--motion", "KIDNEY:0.1", "--elevation", "3"], "--m-mode")):
        r = subprocess.run([exe, scene, "1", "5"] + bad, capture_output=True, text=True, timeout=240, cwd=str(tmp_path))
        assert r.returncode == 1 and word in r.stdout, (bad, r.stdout)
