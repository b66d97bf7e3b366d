"""rf_image::autogain of the C++ shim (host/mcrt_host.hpp) on the MI355X: tests/host/autogain_driver.cpp, a stand-alone program built here with
the host compiler, runs it over a traced frame and over the views of a compounded frame; what it writes equals the numpy mirror
(tests/autogain_mirror.py) on what it wrote before the gain."""
import json
import os
import subprocess
import numpy as np
import pytest

import autogain_mirror as am
import image_cases as ic

pytestmark = pytest.mark.gpu

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mcray-tracing_amd")


def test_host_shim(mcrt, tmp_path):
    exe = str(tmp_path / "autogain_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(PKG, "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "autogain_driver.cpp"), "-L", PKG, "-lmcrt_hip", "-Wl,-rpath," + PKG])
    cfg, meshes = mcrt.synth.sphere_scene(3)
    cfg["workingDirectory"] = str(tmp_path) + "/"
    for f, (V, F) in meshes.items():
        mcrt.scene_io.save_obj(str(tmp_path / f), V, F)
    (tmp_path / "sphere.scene").write_text(json.dumps(cfg))
    E, R, sigma, band = 64, 465, 0.01, 24
    out = tmp_path / "blocks.bin"
    r = subprocess.run([exe, str(tmp_path / "sphere.scene"), str(out), "2", "5", repr(sigma), str(band)], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = np.fromfile(str(out), f32)
    n = E * R
    assert raw.size == 2 * n + R + 1 + 4 * n + R + 1
    img = lambda a: np.ascontiguousarray(a.reshape(R, E).T)              # the program's [R][E] as the stack's [E][R]
    before, after, gain, pen = img(raw[:n]), img(raw[n:2 * n]), raw[2 * n:2 * n + R], int(raw[2 * n + R])
    want = am.autogain(before.reshape(1, 1, E, R), dict(band_rows=band), np.array([sigma], f32))
    ic.assert_same_bits(after, want[0][0, 0], "the frame after rf_image::autogain")
    ic.assert_same_bits(gain, want[1][0], "gain_curve()")
    assert pen == want[3][0] and 0 < pen <= R and "penetration %g mm" % (pen * 0.322) in r.stdout
    assert gain.max() > 2.0 * gain.min(), "the curve does nothing"
    rest = raw[2 * n + R + 1:]
    views = np.stack([img(rest[i * n:(i + 1) * n]) for i in range(3)])
    after, gain, pen = img(rest[3 * n:4 * n]), rest[4 * n:4 * n + R], int(rest[4 * n + R])
    want = am.autogain(views.reshape(1, 3, E, R), dict(band_rows=band), np.array([sigma], f32))
    ic.assert_same_bits(after, want[0][0, 1], "the middle view after rf_image::autogain")
    ic.assert_same_bits(gain, want[1][0], "the views' one curve")
    assert pen == want[3][0]
