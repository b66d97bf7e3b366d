"""Shear-wave elastography end to end on the MI355X, on the smallest scene the strain chain test uses: a box of LIVER with a sphere of
KIDNEY at twice the shear speed under 64 scan-lines.  Simulator.shear_elastogram() against the same chain by hand through Context calls
and against the mirror's overlay, byte for byte; one trace gives bmode()'s own picture; the truths are registered with labels(); what
shear= leaves alone and what it refuses; the C++ shim and the CLI."""
import json
import os
import subprocess
import numpy as np
import pytest

import shear_mirror as sh
import strain_mirror as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

f32 = np.float32
E, ROWS, COLS = 64, 200, 250
SHEAR = dict(speed_m_s={"KIDNEY": 4.0}, push=(4, 60.0, 120.0), n_pulses=96, prf_hz=8000.0)


def _scene(mcrt):
    cfg, meshes = mcrt.synth.sphere_scene(3)
    cfg["meshes"][1] = dict(cfg["meshes"][1], material="KIDNEY")                        # the sphere's record: a stiff lesion's
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


def by_hand(mcrt, sim, frame_id, shear, noise, out_rows, out_cols, ref_kpa, **display):
    """shear_elastogram()'s chain through Context calls alone, on sim's context and scene"""
    ctx, R = sim.ctx, sim.R
    n, npix = E * R, out_rows * out_cols
    names = sim.material_names
    speeds = np.full(len(names), 2.0); speeds[names.index("KIDNEY")] = shear["speed_m_s"]["KIDNEY"]
    slow, speed_f = mcrt.host_shear_table(speeds, shear["prf_hz"])
    line, depth_mm, length_mm = shear["push"]
    pitch = mcrt.row_pitch_mm(sim.tr.frequency)
    rows = min(max(int(round(length_mm / pitch)), 1), R)
    row0 = min(max(int(round(depth_mm / pitch - rows / 2.0)), 0), R - rows)
    opts = mcrt.shear_opts_struct(sigma=shear.get("noise"), push_line=line, push_row0=row0, push_rows=rows,
                                  **{k: v for k, v in shear.items() if k in ("n_pulses", "window_rows", "prf_hz", "seed", "speed_lines", "avg_rows", "peak_q24")})
    prm = ctx.params
    pitch_q8, pitch_mm = mcrt.host_shear_pitch(E, R, 30.0, np.pi / 3.0, int((prm.depth_cm / float(prm.speed_of_sound)) * 10000.0), int(prm.speed_of_sound))
    cycles = mcrt.host_psf_carrier(sim.tr.frequency)
    bufs = [ctx.alloc(size) for size in (4 * n, n, 8 * n) + (4 * n,) * 7 + (npix, 8 * npix, 3 * npix)]
    rf, tissue, iq, pt, pd, ta, ts, sp, mo, qu, grey, img, rgb = bufs
    try:
        ctx.trace_frame(frame_id, rf)
        ctx.label_frames(tissue_dev=tissue)
        ctx.convolve_frames(rf, 1, E, R, sim.psf.axial_kernel, sim.psf.lateral_kernel)
        if noise is not None:
            ctx.noise_frames(rf, 1, 1, E, R, first_image_id=frame_id, **noise)
        ctx.detect_frames(rf, 1, E, R, iq_dev=iq)
        ctx.shear_wave_frames(iq, tissue, 1, E, R, slow, speed_f, pitch_q8, mcrt.host_shear_shape(12), mcrt.host_shear_decay(E, 8.0), cycles, first_image_id=frame_id,
                              peak_time_dev=pt, peak_disp_dev=pd, truth_arrival_dev=ta, truth_speed_dev=ts, opts=opts)
        ctx.shear_speed_frames(pt, 1, E, R, pitch_mm, speed_dev=sp, modulus_dev=mo, quality_dev=qu, opts=opts)
        ctx.envelope_frames(rf, 1, E, R)
        ctx.bmode_frames(rf, 1, E, R, grey, out_rows=out_rows, out_cols=out_cols)
        ctx.scan_convert_frames(mo, 1, E, R, img, out_rows=out_rows, out_cols=out_cols)
        ctx.scan_convert_frames(qu, 1, E, R, img + 4 * npix, out_rows=out_rows, out_cols=out_cols)
        ctx.elastogram_frames(img, img + 4 * npix, grey, 1, out_rows, out_cols, rgb, lut=mcrt.host_shear_map(), ref_strain=ref_kpa, **display)
        beams = dict(speed=sp, modulus=mo, quality=qu, peak_time=pt, peak_disp=pd, truth_arrival=ta, truth_speed=ts)
        return dict({k: ctx.d2h(p, (E, R)) for k, p in beams.items()}, rgb=ctx.d2h(rgb, (out_rows, out_cols, 3), np.uint8),
                    grey=ctx.d2h(grey, (out_rows, out_cols), np.uint8), modulus_img=ctx.d2h(img, (out_rows, out_cols)),
                    quality_img=ctx.d2h(img + 4 * npix, (out_rows, out_cols)))
    finally:
        for b in bufs:
            ctx.free(b)


@pytest.mark.parametrize("noise", [None, dict(snr_db=30.0, seed=7)])
def test_shear_elastogram_equals_the_chain_by_hand_and_the_mirrors_overlay(mcrt, small, noise):
    shear = dict(SHEAR, window_rows=6, speed_lines=3, avg_rows=1, noise=0.0 if noise is None else 1e-4, seed=99)
    sim = make_sim(mcrt, small, shear=shear, noise=noise)
    try:
        got = sim.shear_elastogram(3, out_rows=ROWS, out_cols=COLS, quality_min=0.8, alpha=200)
        want = by_hand(mcrt, sim, 3, shear, noise, ROWS, COLS, 3.0 * 2.0 * 2.0, rho_min=0.8, alpha=200)
        for k in sorted(want):
            assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
            assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), k
        beams = sim.shear_wave(3)
        for k in sorted(beams):
            assert np.array_equal(beams[k].view(np.uint8), want[k].view(np.uint8)), k
        overlay = sm.elastogram(got["modulus_img"][None], got["quality_img"][None], got["grey"][None], sh.shear_map(), ref_strain=12.0, rho_min=0.8, alpha=200)[0]
        assert np.array_equal(got["rgb"], overlay)
        assert (got["quality"] > 0).any() and np.isfinite(got["speed"]).any() and (got["rgb"] != got["grey"][..., None]).any()       # there is a wave, and it is shown
    finally:
        sim.close()


def test_truths_are_registered_with_the_labels(mcrt, small):
    """the true speed is the table's entry of every sample's label; the true arrival is 0 on the pushed line and grows away from it"""
    sim = make_sim(mcrt, small, shear=SHEAR)
    try:
        w, labels = sim.shear_wave(1), sim.labels(out_rows=ROWS, out_cols=COLS)
        names = small[0].material_names
        tissue = labels["tissue"]
        table = np.zeros(256, f32); table[:len(names)] = 2.0; table[names.index("KIDNEY")] = 4.0
        assert (tissue == names.index("KIDNEY")).any() and (tissue == names.index("LIVER")).any()
        assert np.array_equal(w["truth_speed"], table[tissue])
        ta = w["truth_arrival"]
        passable = (tissue < len(names)).all(axis=0)                         # rows the wave can walk from end to end
        assert not ta[4].any()
        assert (np.diff(ta[4:, passable], axis=0) > 0).all() and (np.diff(ta[:5, passable], axis=0) < 0).all()
    finally:
        sim.close()


def test_shear_leaves_everything_else_alone(mcrt, small):
    plain = make_sim(mcrt, small, noise=dict(snr_db=35.0))
    with_shear = make_sim(mcrt, small, noise=dict(snr_db=35.0), shear=SHEAR)
    try:
        assert plain.shear_opts is None
        want = plain.bmode(4, out_rows=ROWS, out_cols=COLS), plain.frame(4)
        assert np.array_equal(with_shear.bmode(4, out_rows=ROWS, out_cols=COLS), want[0])
        pic = with_shear.shear_elastogram(4, out_rows=ROWS, out_cols=COLS)
        assert np.array_equal(pic["grey"], want[0])                          # the underlay IS bmode()'s picture
        assert np.array_equal(with_shear.bmode(4, out_rows=ROWS, out_cols=COLS), want[0])
        assert np.array_equal(with_shear.frame(4).view(np.uint32), want[1].view(np.uint32))
        with pytest.raises(RuntimeError, match="shear="):
            plain.shear_elastogram()
        with pytest.raises(RuntimeError, match="shear="):
            plain.shear_wave()
    finally:
        plain.close(); with_shear.close()


def test_what_shear_refuses(mcrt, small):
    sd, tr, tex = small
    with pytest.raises(ValueError, match="no material"):
        make_sim(mcrt, small, shear={"TUMOR": 3.0})
    with pytest.raises(TypeError):
        make_sim(mcrt, small, shear=dict(speed_m_s={"KIDNEY": 4.0}, window=8))
    with pytest.raises(mcrt.McrtError):
        make_sim(mcrt, small, shear=dict(speed_m_s={"KIDNEY": 1e-9}))                   # a slowness above 2^38
    for bad in (dict(window_rows=17), dict(push=(E, 60.0, 20.0))):
        sim = make_sim(mcrt, small, shear=dict(dict(speed_m_s={"KIDNEY": 4.0}), **bad))
        try:
            with pytest.raises((mcrt.McrtError, ValueError)):
                sim.shear_wave()
        finally:
            sim.close()
    sim = make_sim(mcrt, small, shear=SHEAR)
    try:
        with pytest.raises(ValueError, match="radius_mm"):                             # the pitch was taken from another sector than the picture's
            sim.shear_elastogram(out_rows=ROWS, out_cols=COLS, radius_mm=40.0)
    finally:
        sim.close()
    for kw, word in ((dict(sweep=(3, 0.02)), "sweep="), (dict(compound=(-0.1, 0.1)), "compound="), (dict(elevation=True), "elevation="),
                     (dict(psf=mcrt.Psf(freq=tr.frequency, bands=(3.5, 4.5, 5.5))), "bands")):
        sim = make_sim(mcrt, small, shear=SHEAR, **kw)
        try:
            for call in (sim.shear_elastogram, sim.shear_wave):
                with pytest.raises(RuntimeError, match=word):
                    call()
        finally:
            sim.close()


# ------------------------------------------------------------------ the C++ shim and the CLI
def _write_scene(mcrt, tmp_path):
    cfg, meshes = _scene(mcrt)
    cfg["workingDirectory"] = str(tmp_path) + "/"
    for f, (V, F) in meshes.items():
        mcrt.scene_io.save_obj(str(tmp_path / f), V, F)
    (tmp_path / "lesion.scene").write_text(json.dumps(cfg))
    return cfg, str(tmp_path / "lesion.scene")


def test_host_shim(mcrt, tmp_path):
    """tests/host/shear_driver.cpp -- trace, the PSF, rf_image::shear_wave, the B-mode chain, rf_image::shear_speed,
    rf_image::shear_elastogram -- writes the Python path's bytes"""
    pkg = os.path.join(ROOT, "mcray-tracing_amd")
    exe = str(tmp_path / "shear_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(pkg, "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "shear_driver.cpp"), "-L", pkg, "-lmcrt_hip", "-Wl,-rpath," + pkg])
    cfg, scene = _write_scene(mcrt, tmp_path)
    out = tmp_path / "shear.bin"
    r = subprocess.run([exe, scene, str(out), "2", "KIDNEY", "4.0", "4", "30", "300", "96", "8000", "0.0001"], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    blob = out.read_bytes()
    npix, R = ROWS * COLS, 465
    assert len(blob) == 3 * npix + npix + 7 * 4 * E * R
    sd = mcrt.scene_io.load_scene_file(scene)
    tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    sim = mcrt.Simulator(sd, tr, n_samples=8, shear=dict(speed_m_s={"KIDNEY": 4.0}, push_line=4, push_row0=30, push_rows=300, n_pulses=96, prf_hz=8000.0, noise=1e-4))
    try:
        pic = sim.shear_elastogram(2, out_rows=ROWS, out_cols=COLS)
    finally:
        sim.close()
    assert (pic["rgb"] != pic["grey"][..., None]).any()
    at = 0
    for name in ("rgb", "grey", "speed", "modulus", "quality", "peak_time", "peak_disp", "truth_arrival", "truth_speed"):
        want = pic[name]
        assert blob[at:at + want.nbytes] == want.tobytes(), name
        at += want.nbytes


def test_cli(mcrt, tmp_path):
    """mattausch_hip --shear-elastogram: the PPM and --shear-truth are the Python Simulator's bytes, the PGM beside it is bmode()'s; options
    that make no sense end the program before it touches a device"""
    exe = os.path.join(ROOT, "mcray-tracing_amd", "mattausch_hip")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "mcray-tracing_amd"), "mattausch_hip"])
    cfg, scene = _write_scene(mcrt, tmp_path)
    ppm, truth, pgm = tmp_path / "s.ppm", tmp_path / "truth.raw", tmp_path / "b.pgm"
    r = subprocess.run([exe, scene, "1", "5", str(pgm), str(tmp_path / "rf.bin"), "--shear-elastogram", str(ppm), "--shear-speed", "KIDNEY:4,FAT:1.2",
                        "--push", "40,60,100", "--shear-pulses", "128", "--shear-prf", "6000", "--shear-truth", str(truth), "--noise-db", "35"],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    sd = mcrt.scene_io.load_scene_file(scene)
    tr = mcrt.Transducer(512, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    sim = mcrt.Simulator(sd, tr, n_samples=5, noise=dict(snr_db=35.0),
                         shear=dict(speed_m_s={"KIDNEY": 4.0, "FAT": 1.2}, push=(40, 60.0, 100.0), n_pulses=128, prf_hz=6000.0))
    try:
        pic = sim.shear_elastogram(0)
    finally:
        sim.close()
    assert (pic["rgb"] != pic["grey"][..., None]).any()
    assert ppm.read_bytes() == b"P6\n500 400\n255\n" + pic["rgb"].tobytes()
    assert truth.read_bytes() == pic["truth_speed"].tobytes()
    assert pgm.read_bytes() == b"P5\n500 400\n255\n" + pic["grey"].tobytes()
    ok = ["--shear-elastogram", "x.ppm", "--shear-speed", "KIDNEY:4", "--push", "40,60,100"]
    for bad, word in ((["--shear-pulses", "64"], "--shear-elastogram"), (["--shear-elastogram", "x.ppm"], "--shear-speed"),
                      (["--shear-elastogram", "x.ppm", "--shear-speed", "KIDNEY:4"], "--push"),
                      (["--shear-elastogram", "x.ppm", "--shear-speed", "KIDNEY", "--push", "40,60,100"], "NAME:c"),
                      (["--shear-elastogram", "x.ppm", "--shear-speed", "TUMOR:3", "--push", "40,60,100"], "TUMOR"),
                      (["--shear-elastogram", "x.ppm", "--shear-speed", "KIDNEY:4", "--push", "40,60"], "--push"),
                      (["--shear-elastogram", "x.ppm", "--shear-speed", "KIDNEY:4", "--push", "512,60,100"], "--push"),
                      (ok + ["--shear-pulses", "3"], "--shear-pulses"), (ok + ["--shear-prf", "0"], "--shear-prf"),
                      (ok + ["--compound", "3"], "--shear-elastogram"), (ok + ["--freq-compound", "3"], "--shear-elastogram"),
                      (ok + ["--elevation", "3"], "--shear-elastogram")):
        r = subprocess.run([exe, scene, "1", "5"] + bad, capture_output=True, text=True, timeout=240, cwd=str(tmp_path))
        assert r.returncode == 1 and word in r.stdout, (bad, r.stdout)
