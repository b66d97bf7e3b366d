"""The image stages of the two front ends over every kind of traced pass: rf_image (tests/host/stages_driver.cpp: trace -> convolve -> add_noise ->
detect | envelope -> despeckle -> autogain, or -> fold_bands alone) writes the bits that Simulator's public stage methods -- freehand() for the
tracked poses -- produce with the same options, for trace(frame), two steered views, a two-plane sweep and two tracked poses, without bands
and with two.  Frame id 3, so that the ids frame_id * n and frame_id * n * B show."""
import os
import subprocess
import numpy as np
import pytest

import image_cases as ic
from test_gpu_compound import _write_scene

pytestmark = pytest.mark.gpu

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, R, S, FRAME, B = 64, 465, 2, 3, 2
MODES = ["plain", "views", "sweep", "tracked"]
CHAINS = [(False, "quadrature"), (True, "quadrature"), (True, "envelope"), (True, "fold")]      # (bands, detector): the driver's order within a mode
MODE_KW = {"plain": {}, "views": dict(compound=(-0.1, 0.1)), "sweep": dict(sweep=(2, 0.02)), "tracked": {}}
GRID = (-140, -20, -4, 2.0, 30, 20, 5)         # x0, y0, z0 [mm, world], pitch, nu, nv, nw: the sphere scene's probe looks along +x from x = -135


@pytest.fixture(scope="module")
def shim(mcrt, tmp_path_factory):
    """one run of the driver -> (the scene file, its config, {(mode, bands, detector): (images [n][E][R], gains [F][R] | None, rows [F] | None,
    voxels | None)})"""
    tmp = tmp_path_factory.mktemp("stages")
    pkg = os.path.join(ROOT, "mcray-tracing_amd")
    exe = str(tmp / "stages_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(pkg, "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "stages_driver.cpp"), "-L", pkg, "-lmcrt_hip", "-Wl,-rpath," + pkg])
    cfg, scene = _write_scene(mcrt, tmp)
    out = tmp / "stages.bin"
    r = subprocess.run([exe, scene, str(out), str(FRAME), str(S), ",".join(str(x) for x in GRID)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    raw, at, got = out.read_bytes(), 0, {}

    def take(dtype, *shape):
        nonlocal at
        a = np.frombuffer(raw, dtype, int(np.prod(shape)), at).reshape(shape)
        at += a.nbytes
        return a

    for mode in MODES:
        n, F = 1 if mode == "plain" else 2, 2 if mode == "tracked" else 1
        for bands, how in CHAINS:
            imgs = take(f32, n, R, E).transpose(0, 2, 1)
            gains, rows = (take(f32, F, R), take(np.uint32, F)) if how != "fold" else (None, None)
            vox = take(f32, GRID[6], GRID[5], GRID[4]) if mode == "tracked" else None
            got[mode, bands, how] = (imgs, gains, rows, vox)
    assert at == len(raw)
    return scene, cfg, got


@pytest.fixture(scope="module")
def texture(mcrt):
    return mcrt.host_texture(256)


@pytest.mark.parametrize("bands", [False, True], ids=["plain_psf", "two_bands"])
@pytest.mark.parametrize("mode", MODES)
def test_shim_and_simulator_agree(mcrt, shim, texture, mode, bands):
    scene, cfg, got = shim
    tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    psf = mcrt.Psf(bands=dict(band_mhz=(4.0, 5.0), weights=(1, 2), var_x=0.05) if bands else None)
    sim = mcrt.Simulator(mcrt.scene_io.load_scene_file(scene), tr, n_samples=S, psf=psf, texture=texture, noise=dict(snr_db=40.0, seed=77),
                         speckle=dict(n_iter=2), autogain=True, detect=dict(n_taps=31), **MODE_KW[mode])
    try:
        assert sim.R == R
        n = 1 if mode == "plain" else 2
        stack = {"plain": sim.rf_dev, "views": sim.views_dev, "sweep": sim.sweep_dev}.get(mode)
        p0 = cfg["transducerPosition"]
        pos, dirs = tr.poses([p0, (p0[0], p0[1], p0[2] + 0.125)], [cfg["transducerAngles"]] * 2)
        grid = mcrt.volume_grid(GRID[:3], (GRID[3], 0, 0), (0, GRID[3], 0), (0, 0, GRID[3]), *GRID[4:])
        for has_bands, how in CHAINS:
            if has_bands != bands:
                continue
            imgs, gains, rows, vox = got[mode, bands, how]
            what = "%s, %s, %s" % (mode, "two bands" if bands else "no bands", how)
            assert np.isfinite(imgs).all() and np.count_nonzero(imgs) > 1000, what
            sim.detect = dict(n_taps=31) if how == "quadrature" else None
            if mode == "tracked":
                ic.assert_same_bits(vox, sim.freehand(FRAME, pos, dirs, grid, envelope=how != "fold"), what + ": the voxels")
                assert np.count_nonzero(vox) > 100, what
            else:
                sim.trace(FRAME)
                sim.convolve()
                sim.add_noise(FRAME)
                if how == "fold":
                    sim.fold_bands()
                else:
                    sim.envelope()
                    sim.despeckle()
                    sim.auto_gain()
                ic.assert_same_bits(imgs, sim.ctx.d2h(stack, (n, E, R)), what + ": the images")
            if how != "fold":
                ic.assert_same_bits(gains, np.atleast_2d(sim.gain_curve()), what + ": the gain curves")
                assert np.array_equal(rows, np.rint(np.atleast_1d(sim.penetration_mm()) / sim.row_mm).astype(np.uint32)), what
    finally:
        sim.close()
