"""Spectral Doppler end to end on the MI355X, on the vessel scene of tests/test_gpu_flow_chain.py (a box of LIVER with a vascular sphere of
BLOOD under 64 scan-lines): Simulator.spectral_doppler() traces once; its series is the mirror's of the I/Q the chain by hand leaves on
the device; a gate in the lumen reads the truth; a gate in still tissue is black; what it refuses; the C++ shim and the command line
write the same bytes."""
import os
import subprocess
import numpy as np
import pytest

import spectral_mirror as sm
from test_gpu_flow_chain import small, make_sim, _write_scene, E, VEL      # noqa: F401  (the scene's builder, reused as it is)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

f32 = np.float32
T, N, HOP = 1024, 128, 32


def lumen_gate(sim, rows=2, line=E // 2):
    """(gate, rows of the lumen on that line): a gate of `rows` rows on the axis of the BLOOD run of a scan-line through the sphere"""
    tissue = sim.labels(picture=False)["tissue"][line]
    at = np.flatnonzero(tissue == sim.material_names.index("BLOOD"))
    assert at.size > 8 and (np.diff(at) == 1).all()
    pitch = sim.row_mm
    return (line, (at[0] + at[-1] + 1) / 2.0 * pitch, rows * pitch), at


def iq_by_hand(mcrt, sim, frame_id):
    """colour flow's chain up to the detected pairs through Context calls alone -> (iq_static, iq_moving [1][E][R][2], tissue [E][R])"""
    ctx, R = sim.ctx, sim.R
    n = E * R
    vel = np.zeros((len(sim.material_names), 3), f32); vel[sim.material_names.index("BLOOD")] = VEL
    bufs = [ctx.alloc(size) for size in (4 * n, n, 8 * n, 16 * n)]
    rf, tissue, parts, iq = bufs
    try:
        ctx.trace_frame(frame_id, rf)
        ctx.label_frames(tissue_dev=tissue)
        ctx.flow_split_frames(rf, tissue, 1, E, R, (vel != 0).any(axis=1), parts)
        ctx.convolve_frames(parts, 2, E, R, sim.psf.axial_kernel, sim.psf.lateral_kernel)
        ctx.detect_frames(parts, 2, E, R, iq_dev=iq)
        pairs = ctx.d2h(iq, (2, 1, E, R, 2))
        return pairs[0], pairs[1], ctx.d2h(tissue, (E, R), np.uint8)
    finally:
        for b in bufs:
            ctx.free(b)


@pytest.fixture(scope="module")
def sim(mcrt, small):
    s = make_sim(mcrt, small, flow=dict(velocity_mm_s={"BLOOD": VEL}, sigma=2e-4))
    yield s
    s.close()


def test_it_traces_once_and_its_series_is_the_mirrors(mcrt, sim):
    gate, lumen = lumen_gate(sim, rows=6)
    speed = mcrt.host_pulse_waveform(4000.0, 90.0, 250.0, 60.0, T)
    calls = []
    trace = sim.ctx.trace_frame
    sim.ctx.trace_frame = lambda *a, **k: (calls.append(a), trace(*a, **k))[1]
    try:
        out = sim.spectral_doppler(3, gate=gate, waveform=speed, n_fft=N, hop=HOP)
    finally:
        del sim.ctx.trace_frame
    assert len(calls) == 1 and calls[0][0] == 3
    cols = sm.n_cols(T, N, HOP)
    assert out["power"].shape == (cols, N) and out["grey"].shape == (N, cols) and out["mean"].shape == (cols,) and out["truth"].shape == (cols,)
    assert out["series"].shape == (T,) and out["series"].dtype == np.complex64 and out["velocity_axis"].shape == (N,) and out["time_axis"].shape == (cols,)
    g = out["gate"]
    assert g["rows"] == 6 and lumen[0] < g["row0"] and g["row0"] + 6 <= lumen[-1] and (g["frac"] > 0.9).all() and 0.5 < g["axial"] <= 1.0
    st, mv, tissue = iq_by_hand(mcrt, sim, 3)
    moving = np.zeros(len(sim.material_names), np.uint8); moving[sim.material_names.index("BLOOD")] = 1
    assert np.array_equal(g["frac"].view(np.uint32), sm.profile(tissue[g["line"]], g["row0"], 6, moving, 2.0).view(np.uint32))
    assert np.array_equal(g["rate"], sm.rates(g["frac"], g["axial"]))
    v_nyq = sim.flow["v_nyq"]
    z = sm.series(st, mv, [[0, g["line"], g["row0"]]], np.ones(6, f32), g["rate"][None], sm.phase(v_nyq, speed), sigma=2e-4, first_image_id=3)
    assert np.array_equal(out["series"].view(f32).reshape(T, 2).view(np.uint32), z[0].view(np.uint32))
    power, mean = sm.spectrum(z, sm.window(1, N), v_nyq, N=N, hop=HOP)
    assert np.array_equal(out["power"].view(np.uint32), power[0].view(np.uint32)) and np.array_equal(out["mean"].view(np.uint32), mean[0].view(np.uint32))
    grey, _ = sm.sonogram(power)
    assert np.abs(out["grey"].astype(np.int32) - grey[0].astype(np.int32)).max() <= 1
    assert out["velocity_axis"][N // 2] == 0.0 and abs(out["velocity_axis"][-1] - v_nyq * (1 - 2.0 / N)) < 1e-9
    assert abs(out["time_axis"][0] - (N / 2) / 4000.0) < 1e-12


def test_a_gate_in_the_lumen_reads_the_truth(mcrt, sim):
    """a two-row gate on the lumen's axis under a sinusoidal waveform: the mean trace follows the truth to within two bin widths -- the
    bound tests/test_spectral_contract.py derives on the mirror (worst error 1.9 mm/s there) -- plus what the parabola takes of the
    centre-line speed at the gate's rows, (1 - frac) of its largest value"""
    gate, _ = lumen_gate(sim, rows=2)
    speed = (150.0 + 80.0 * np.sin(2 * np.pi * np.arange(2048) / 700.0)).astype(f32)
    out = sim.spectral_doppler(1, gate=gate, waveform=speed, n_fft=N, hop=HOP)
    v_nyq = sim.flow["v_nyq"]
    g = out["gate"]
    want = np.array([(speed[c * HOP:c * HOP + N].astype(np.float64) * g["axial"]).mean() for c in range(out["truth"].size)])
    assert np.allclose(out["truth"], want, rtol=1e-6)
    bound = 2 * (2 * v_nyq / N) + (1.0 - float(g["frac"].min())) * 230.0
    err = np.abs(out["mean"] - out["truth"]).max()
    print("lumen gate: worst |mean - truth| %.3f mm/s, bound %.3f mm/s (a bin is %.3f)" % (err, bound, 2 * v_nyq / N))
    assert err <= bound and out["truth"].max() - out["truth"].min() > 100.0
    peak_rows = out["grey"].argmax(axis=0)                             # row 0 is the highest velocity: the trace lies in the upper half
    assert (peak_rows < N // 2).all()


def test_a_gate_in_still_tissue_is_black(mcrt, small):
    """a gate in the LIVER, thirty rows and more in front of the lumen (the PSF reaches eight)"""
    sim = make_sim(mcrt, small, flow={"BLOOD": VEL})
    try:
        tissue = sim.labels(picture=False)["tissue"][E // 2]
        lumen = np.flatnonzero(tissue == sim.material_names.index("BLOOD"))
        liver = np.flatnonzero(tissue[:lumen[0] - 30] == sim.material_names.index("LIVER"))
        assert liver.size > 20
        gate = (E // 2, float(liver[liver.size // 2]) * sim.row_mm, 3.0)
        out = sim.spectral_doppler(2, gate=gate, n_pulses=512, wall_bins=2)
        assert not out["gate"]["rate"].any()
        assert np.abs(out["series"]).max() > 0 and (out["series"] == out["series"][0]).all()      # the liver echoes, and stands still
        assert not out["power"].view(np.uint32).any() and not out["grey"].any() and not out["mean"].any()
        loud = sim.spectral_doppler(2, gate=gate, n_pulses=512, wall="none", wall_bins=2)
        assert not loud["power"][:, N // 2 - 1:N // 2 + 2].any() and not loud["grey"][N // 2 - 2:N // 2 + 1].any()      # the clutter's bins 63 .. 65 are
        assert loud["power"][:, N // 2 + 2].all() and loud["grey"][N - 1 - (N // 2 + 2)].any()                      # written as zero (rows 64 .. 62), their neighbour not
    finally:
        sim.close()


def test_what_it_refuses(mcrt, small):
    sd, tr, tex = small
    plain = make_sim(mcrt, small)
    try:
        with pytest.raises(RuntimeError, match="flow="):
            plain.spectral_doppler()
    finally:
        plain.close()
    for kw, word in ((dict(sweep=(3, 0.02)), "sweep="), (dict(compound=(-0.1, 0.1)), "compound="), (dict(elevation=True), "elevation="),
                     (dict(psf=mcrt.Psf(freq=tr.frequency, bands=(3.5, 4.5, 5.5))), "bands")):
        s = make_sim(mcrt, small, flow={"BLOOD": VEL}, **kw)
        try:
            with pytest.raises(RuntimeError, match=word):
                s.spectral_doppler(gate=(E // 2, 30.0, 2.0))
        finally:
            s.close()
    s = make_sim(mcrt, small, flow={"BLOOD": VEL})
    try:
        with pytest.raises(ValueError, match="no material"):
            s.spectral_doppler(material="PLASMA")
        with pytest.raises(ValueError, match="no velocity"):
            s.spectral_doppler(material="LIVER")
        with pytest.raises(ValueError, match="scan-line"):
            s.spectral_doppler(gate=(E, 30.0, 2.0))
        with pytest.raises(ValueError, match="fewer"):
            s.spectral_doppler(gate=(1, 30.0, 2.0), n_pulses=64)
        with pytest.raises(mcrt.McrtError):
            s.spectral_doppler(gate=(1, 30.0, 2.0), n_fft=100)
        with pytest.raises(mcrt.McrtError):
            s.spectral_doppler(gate=(1, 30.0, 2.0), waveform=np.full(256, 5000.0, f32))          # more than twice the Nyquist velocity
    finally:
        s.close()


# ------------------------------------------------------------------ the C++ shim and the CLI
def test_host_shim(mcrt, tmp_path):
    """tests/host/spectral_driver.cpp -- trace, rf_image::flow_split, flow, tissue_line, spectral_series, spectrum, sonogram -- writes the
    Python path's bytes"""
    pkg = os.path.join(ROOT, "mcray-tracing_amd")
    exe = str(tmp_path / "spectral_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(pkg, "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "spectral_driver.cpp"), "-L", pkg, "-lmcrt_hip", "-Wl,-rpath," + pkg])
    cfg, scene = _write_scene(mcrt, tmp_path)
    sd = mcrt.scene_io.load_scene_file(scene)
    tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    sim = mcrt.Simulator(sd, tr, n_samples=8, flow=dict(velocity_mm_s={"BLOOD": VEL}, sigma=1e-4))
    try:
        gate, _ = lumen_gate(sim, rows=8)
        want = sim.spectral_doppler(2, gate=gate, n_pulses=T)
    finally:
        sim.close()
    g = want["gate"]
    out = tmp_path / "spectral.bin"
    r = subprocess.run([exe, scene, str(out), "2", "BLOOD"] + [str(v) for v in VEL] + [str(g["line"]), str(g["row0"]), "8", str(T), "1e-4"],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    blob = out.read_bytes()
    at = 0
    for name, arr in (("series", want["series"]), ("power", want["power"]), ("mean", want["mean"]), ("grey", want["grey"])):
        assert blob[at:at + arr.nbytes] == arr.tobytes(), name
        at += arr.nbytes
    assert at == len(blob) and want["grey"].any()


def test_cli(mcrt, tmp_path):
    """mattausch_hip --spectral: the PGM is the Python Simulator's sonogram and --spectral-iq its series; options that make no sense end
    the program before it touches a device"""
    exe = os.path.join(ROOT, "mcray-tracing_amd", "mattausch_hip")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "mcray-tracing_amd"), "mattausch_hip"])
    cfg, scene = _write_scene(mcrt, tmp_path)
    pgm, raw = tmp_path / "sono.pgm", tmp_path / "iq.raw"
    sd = mcrt.scene_io.load_scene_file(scene)
    tr = mcrt.Transducer(512, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    sim = mcrt.Simulator(sd, tr, n_samples=5, flow=dict(velocity_mm_s={"BLOOD": VEL}))
    try:
        gate, _ = lumen_gate(sim, rows=5, line=256)
        gate = (gate[0], round(gate[1], 3), round(gate[2], 3))
        want = sim.spectral_doppler(0, gate=gate, waveform=dict(beats_per_min=100.0, v_peak=200.0, v_min=40.0), n_pulses=768, n_fft=64, hop=16, dynamic_range_db=50.0)
    finally:
        sim.close()
    r = subprocess.run([exe, scene, "1", "5", str(tmp_path / "b.pgm"), str(tmp_path / "rf.bin"), "--flow-velocity", "BLOOD:-150,40,0", "--spectral", str(pgm),
                        "--gate", "%d,%.3f,%.3f" % gate, "--spectral-pulses", "768", "--spectral-fft", "64", "--spectral-hop", "16", "--spectral-db", "50",
                        "--flow-waveform", "100,200,40", "--spectral-iq", str(raw)], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert want["grey"].any()
    assert pgm.read_bytes() == b"P5\n%d %d\n255\n" % (want["grey"].shape[1], want["grey"].shape[0]) + want["grey"].tobytes()
    assert raw.read_bytes() == want["series"].tobytes()
    for bad, word in ((["--gate", "1,2,3"], "--spectral"), (["--spectral", "x.pgm", "--flow-velocity", "BLOOD:1,2,3"], "--gate"),
                      (["--spectral", "x.pgm", "--gate", "1,2,3"], "--flow-velocity"),
                      (["--spectral", "x.pgm", "--gate", "1,2", "--flow-velocity", "BLOOD:1,2,3"], "LINE,DEPTH_MM,LEN_MM"),
                      (["--spectral", "x.pgm", "--gate", "1,2,3", "--flow-velocity", "BLOOD:1,2,3", "--spectral-fft", "100"], "n_fft"),
                      (["--spectral", "x.pgm", "--gate", "1,2,3", "--flow-velocity", "BLOOD:1,2,3", "--flow-waveform", "60,100"], "BPM,PEAK,MIN"),
                      (["--spectral", "x.pgm", "--gate", "1,2,3", "--flow-velocity", "BLOOD:1,2,3", "--compound", "3"], "--spectral")):
        r = subprocess.run([exe, scene, "1", "5"] + bad, capture_output=True, text=True, timeout=240, cwd=str(tmp_path))
        assert r.returncode == 1 and word in r.stdout, (bad, r.stdout)
