"""Which call sequences the C++ shim's rf_image accepts and which it refuses (tests/host/state_driver.cpp): what its image stack holds after
each kind of trace -- nothing, steered views, a sweep's planes --, what its label tables hold after labels(), and the limits of the steer list
and the sweep.  The table is the behaviour of the shim as the feature pull requests left it, the two stale-label quirks included."""
import json
import os
import subprocess
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, RANGE = "ok", "invalid_argument", "out_of_range"

TABLE = [
    # a fresh image: no stack, no labels; the host image is zero and goes through every stage
    ("fresh volume", INVALID), ("fresh postprocess(steers3)", INVALID), ("fresh label_picture", INVALID), ("fresh label_volume", INVALID),
    ("fresh view_intensities(0)", RANGE), ("fresh convolve", OK), ("fresh envelope", OK), ("fresh postprocess()", OK), ("fresh intensities", "ok zero"),
    # trace(f)
    ("plain trace", OK), ("plain postprocess()", OK), ("plain postprocess(steers3)", INVALID), ("plain volume", INVALID), ("plain labels", "ok planes=1"),
    ("plain label_picture", OK), ("plain label_volume", INVALID),
    # then trace(f, t, steers3): the stack holds three views, the RF image of trace(f) is left alone, the labels are the unsteered probe's
    ("steered trace", OK), ("steered postprocess(steers3)", OK), ("steered postprocess(steers2)", INVALID), ("steered volume", INVALID),
    ("steered view_intensities(2)", OK), ("steered view_intensities(3)", RANGE), ("steered intensities", "ok same"), ("steered labels", "ok planes=1"),
    ("steered label_picture", OK),
    # then trace(f, t, sweep3): the stack holds a sweep's planes
    ("swept trace", OK), ("swept volume", OK), ("swept postprocess(steers3)", INVALID), ("swept labels", "ok planes=3"), ("swept label_volume", OK),
    ("swept label_picture", INVALID),
    # then trace(f): the swept state ends
    ("plain again trace", OK), ("plain again volume", INVALID), ("plain again labels", "ok planes=1"), ("plain again label_picture", OK),
    ("plain again label_volume", INVALID),
    # the labels of a 3-plane sweep are not those of a 5-plane sweep
    ("resweep trace(sweep3)", OK), ("resweep labels", "ok planes=3"), ("resweep trace(sweep5)", OK), ("resweep label_volume, stale", INVALID),
    ("resweep labels again", "ok planes=5"), ("resweep label_volume", OK),
    # a sweep, then steered views
    ("sweep-steer trace(sweep3)", OK), ("sweep-steer trace(steers3)", OK), ("sweep-steer postprocess(steers3)", OK), ("sweep-steer volume", INVALID),
    # a sweep, then elevation planes folded into the RF image
    ("sweep-elevation trace(sweep3)", OK), ("sweep-elevation trace(psf, 3)", OK), ("sweep-elevation volume", INVALID), ("sweep-elevation convolve", OK),
    ("sweep-elevation postprocess()", OK),
    # argument limits
    ("limits 0 steers", INVALID), ("limits 17 steers", INVALID), ("limits sweep of 0", INVALID), ("limits sweep of 257", INVALID),
]


def test_host_shim_state(mcrt, tmp_path):
    pkg = os.path.join(ROOT, "mcray-tracing_amd")
    exe = str(tmp_path / "state_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(pkg, "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "state_driver.cpp"), "-L", pkg, "-lmcrt_hip", "-Wl,-rpath," + pkg])
    cfg, meshes = mcrt.synth.sphere_scene(3)
    cfg["workingDirectory"] = str(tmp_path) + "/"
    for f, (V, F) in meshes.items():
        mcrt.scene_io.save_obj(str(tmp_path / f), V, F)
    (tmp_path / "sphere.scene").write_text(json.dumps(cfg))
    r = subprocess.run([exe, str(tmp_path / "sphere.scene")], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    got = [tuple(line[2:].split(": ", 1)) for line in r.stdout.splitlines() if line.startswith("> ")]
    print("\n".join("%s: %s" % g for g in got))
    assert got == TABLE
