"""Strain elastography end to end on the MI355X: a box of LIVER with a sphere of KIDNEY five times as stiff under 64 scan-lines.
Simulator.elastogram() against the same chain by hand through Context calls, byte for byte; the estimated strain inside and outside the
inclusion against the registered truth; where the colour lies against the correlation coefficient; what strain= leaves alone; what it
refuses; the C++ shim and the CLI."""
import json
import os
import subprocess
import numpy as np
import pytest

import strain_mirror as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

f32 = np.float32
E, ROWS, COLS = 64, 200, 250
STRAIN = dict(modulus={"KIDNEY": 5.0}, applied=0.01)


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


def by_hand(mcrt, sim, frame_id, strain, noise, out_rows, out_cols, **display):
    """elastogram()'s chain through Context calls alone, on sim's context and scene"""
    ctx, R = sim.ctx, sim.R
    n, npix = E * R, out_rows * out_cols
    names = sim.material_names
    modulus = np.ones(len(names)); modulus[names.index("KIDNEY")] = strain["modulus"]["KIDNEY"]
    eps = mcrt.host_strain_table(modulus, strain["applied"], 1.0)
    opts = mcrt.strain_opts_struct(sigma=strain.get("noise"), **{k: v for k, v in strain.items() if k in ("window_rows", "search_rows", "lsq_rows", "seed")})
    cycles = mcrt.host_psf_carrier(sim.tr.frequency)
    bufs = [ctx.alloc(size) for size in (4 * n, n, 8 * n, 8 * n, 4 * n, 4 * n, 4 * n, 4 * n, 4 * n, npix, 8 * npix, 3 * npix)]
    rf, tissue, iq, post, td, ts, disp, rho, st, grey, img, rgb = bufs
    try:
        ctx.trace_frame(frame_id, rf)
        ctx.label_frames(tissue_dev=tissue)
        ctx.convolve_frames(rf, 1, E, R, sim.psf.axial_kernel, sim.psf.lateral_kernel)
        if noise is not None:
            ctx.noise_frames(rf, 1, 1, E, R, first_image_id=frame_id, **noise)
        ctx.detect_frames(rf, 1, E, R, iq_dev=iq)
        ctx.strain_compress_frames(iq, tissue, 1, E, R, eps, cycles, first_image_id=frame_id, post_iq_dev=post, truth_disp_dev=td, truth_strain_dev=ts, opts=opts)
        ctx.strain_frames(iq, post, 1, E, R, cycles, disp_dev=disp, rho_dev=rho, strain_dev=st, opts=opts)
        ctx.envelope_frames(rf, 1, E, R)
        ctx.bmode_frames(rf, 1, E, R, grey, out_rows=out_rows, out_cols=out_cols)
        ctx.scan_convert_frames(st, 1, E, R, img, out_rows=out_rows, out_cols=out_cols)
        ctx.scan_convert_frames(rho, 1, E, R, img + 4 * npix, out_rows=out_rows, out_cols=out_cols)
        ctx.elastogram_frames(img, img + 4 * npix, grey, 1, out_rows, out_cols, rgb, ref_strain=strain["applied"], **display)
        beams = dict(strain=st, rho=rho, disp=disp, truth_strain=ts, truth_disp=td)
        return dict({k: ctx.d2h(p, (E, R)) for k, p in beams.items()}, rgb=ctx.d2h(rgb, (out_rows, out_cols, 3), np.uint8),
                    grey=ctx.d2h(grey, (out_rows, out_cols), np.uint8), strain_img=ctx.d2h(img, (out_rows, out_cols)),
                    rho_img=ctx.d2h(img + 4 * npix, (out_rows, out_cols)))
    finally:
        for b in bufs:
            ctx.free(b)


@pytest.mark.parametrize("noise", [None, dict(snr_db=30.0, seed=7)])
def test_elastogram_equals_the_chain_by_hand(mcrt, small, noise):
    strain = dict(STRAIN, window_rows=12, search_rows=6, lsq_rows=9, noise=0.0 if noise is None else 1e-4, seed=99)
    sim = make_sim(mcrt, small, strain=strain, noise=noise)
    try:
        got = sim.elastogram(3, out_rows=ROWS, out_cols=COLS, rho_min=0.8, alpha=200)
        want = by_hand(mcrt, sim, 3, strain, noise, ROWS, COLS, rho_min=0.8, alpha=200)
        for k in sorted(want):
            assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
            assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), k
        beams = sim.strain(3)
        for k in sorted(beams):
            assert np.array_equal(beams[k].view(np.uint8), want[k].view(np.uint8)), k
    finally:
        sim.close()


@pytest.fixture(scope="module")
def lesion(mcrt, small):
    sim = make_sim(mcrt, small, strain=STRAIN)
    try:
        yield sim, sim.elastogram(1, out_rows=ROWS, out_cols=COLS), sim.labels(out_rows=ROWS, out_cols=COLS)
    finally:
        sim.close()


def test_truth_is_registered_with_the_labels(mcrt, small, lesion):
    """the true strain is the table's entry of every sample's label, the true displacement its running sum"""
    sim, pic, labels = lesion
    names = small[0].material_names
    tissue = labels["tissue"]
    eps = np.zeros(256, np.int64); eps[:len(names)] = 167772; eps[names.index("KIDNEY")] = 33554
    want = eps[tissue]
    assert (tissue == names.index("KIDNEY")).any() and (tissue == names.index("LIVER")).any()
    assert np.array_equal(pic["truth_strain"], want.astype(np.int32).astype(f32) * f32(2.0 ** -24))
    assert np.array_equal(pic["truth_disp"], (np.cumsum(want, axis=1) - want).astype(np.int32).astype(f32) * f32(2.0 ** -24))


def test_strain_orders_as_the_truth_does(mcrt, small, lesion):
    """in beam space, over the samples the tracker trusts (rho >= 0.9) a slope window (12 rows) inside their region: the lesion, five
    times as stiff, reads less strain than the liver about it, and each reads its own truth in the mean -- within a factor of two: the
    traced speckle is sparser than fully developed speckle and the lesion holds few independent windows"""
    sim, pic, labels = lesion
    names = small[0].material_names
    tissue = labels["tissue"]

    def interior(label):
        m = tissue == label
        for d in range(1, 13):
            m[:, d:] &= (tissue == label)[:, :-d]; m[:, :-d] &= (tissue == label)[:, d:]; m[:, :d] = False; m[:, -d:] = False
        return m & (pic["rho"] >= 0.9)
    inside, outside = interior(names.index("KIDNEY")), interior(names.index("LIVER"))
    assert inside.sum() > 100 and outside.sum() > 1000, (inside.sum(), outside.sum())
    s_in, s_out = float(pic["strain"][inside].astype(np.float64).mean()), float(pic["strain"][outside].astype(np.float64).mean())
    print("lesion: %d samples, mean strain %.5f (truth 0.002); liver: %d samples, mean strain %.5f (truth 0.01); ratio %.2f"
          % (inside.sum(), s_in, outside.sum(), s_out, s_out / s_in))
    assert pic["truth_strain"][inside].max() < pic["truth_strain"][outside].min()
    assert s_in < s_out
    assert 0.001 <= s_in <= 0.004 and 0.005 <= s_out <= 0.02


def test_colour_lies_where_the_tracker_correlates(mcrt, small, lesion):
    """every shown pixel gathers from at least one sample with rho >= rho_min (the bilinear gather of the samples' indicator is > 0 there),
    the picture is the integer mirror's of the gathered planes, and the lesion's pixels are bluer than the liver's"""
    sim, pic, labels = lesion
    rho_min = 0.7
    lut = mcrt.host_strain_map()
    assert np.array_equal(pic["rgb"], sm.elastogram(pic["strain_img"][None], pic["rho_img"][None], pic["grey"][None], lut, ref_strain=0.01)[0])
    with np.errstate(invalid="ignore"):
        shown = (pic["rho_img"] >= f32(rho_min)) & ~np.isnan(pic["strain_img"])
        ind = (pic["rho"] >= f32(rho_min)).astype(f32)
    assert shown.sum() > 1000 and (pic["rgb"][~shown] == pic["grey"][~shown][:, None]).all()
    p_in = sim.ctx.alloc(ind.nbytes); p_out = sim.ctx.alloc(ROWS * COLS * 4)
    try:
        sim.ctx.h2d(p_in, ind)
        sim.ctx.scan_convert_frames(p_in, 1, E, sim.R, p_out, out_rows=ROWS, out_cols=COLS)
        reach = sim.ctx.d2h(p_out, (ROWS, COLS))
    finally:
        sim.ctx.free(p_in); sim.ctx.free(p_out)
    assert not shown[reach == 0].any(), "%d shown pixels gather from no sample with rho >= rho_min" % int(shown[reach == 0].sum())
    names = small[0].material_names
    kidney, liver = shown & (labels["picture"] == names.index("KIDNEY")), shown & (labels["picture"] == names.index("LIVER"))
    assert kidney.sum() > 50 and liver.sum() > 500
    blue = lambda m: float(pic["rgb"][m][:, 2].astype(np.float64).mean() - pic["rgb"][m][:, 0].astype(np.float64).mean())
    print("blue minus red: lesion %.1f, liver %.1f" % (blue(kidney), blue(liver)))
    assert blue(kidney) > blue(liver)


def test_strain_leaves_bmode_alone(mcrt, small):
    """without strain= the simulator never heard of it; with strain= every other method gives the same bytes, before and after elastogram()"""
    plain = make_sim(mcrt, small, noise=dict(snr_db=35.0))
    with_strain = make_sim(mcrt, small, noise=dict(snr_db=35.0), strain=STRAIN)
    try:
        assert plain.strain_opts is None
        want = plain.bmode(4, out_rows=ROWS, out_cols=COLS), plain.frame(4)
        assert np.array_equal(with_strain.bmode(4, out_rows=ROWS, out_cols=COLS), want[0])
        pic = with_strain.elastogram(4, out_rows=ROWS, out_cols=COLS)
        assert np.array_equal(pic["grey"], want[0])                          # the underlay IS bmode()'s picture
        assert np.array_equal(with_strain.bmode(4, out_rows=ROWS, out_cols=COLS), want[0])
        assert np.array_equal(with_strain.frame(4).view(np.uint32), want[1].view(np.uint32))
        with pytest.raises(RuntimeError, match="strain="):
            plain.elastogram()
        with pytest.raises(RuntimeError, match="strain="):
            plain.strain()
    finally:
        plain.close(); with_strain.close()


def test_what_strain_refuses(mcrt, small):
    sd, tr, tex = small
    with pytest.raises(ValueError, match="no material"):
        make_sim(mcrt, small, strain={"TUMOR": 5.0})
    with pytest.raises(TypeError):
        make_sim(mcrt, small, strain=dict(modulus={"KIDNEY": 5.0}, window=8))
    with pytest.raises(mcrt.McrtError):
        make_sim(mcrt, small, strain=dict(modulus={"KIDNEY": 0.2}, applied=0.01))      # 5 %: above the cap
    sim = make_sim(mcrt, small, strain=dict(modulus={"KIDNEY": 5.0}, window_rows=33))
    try:
        with pytest.raises(mcrt.McrtError):
            sim.strain()
    finally:
        sim.close()
    for kw, word in ((dict(sweep=(3, 0.02)), "sweep="), (dict(compound=(-0.1, 0.1)), "compound="), (dict(elevation=True), "elevation="),
                     (dict(psf=mcrt.Psf(freq=tr.frequency, bands=(3.5, 4.5, 5.5))), "bands")):
        sim = make_sim(mcrt, small, strain=STRAIN, **kw)
        try:
            for call in (sim.elastogram, sim.strain):
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
    """tests/host/strain_driver.cpp -- trace, the PSF, rf_image::compress, the B-mode chain, rf_image::track, rf_image::elastogram -- writes
    the Python path's bytes"""
    pkg = os.path.join(ROOT, "mcray-tracing_amd")
    exe = str(tmp_path / "strain_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(pkg, "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "strain_driver.cpp"), "-L", pkg, "-lmcrt_hip", "-Wl,-rpath," + pkg])
    cfg, scene = _write_scene(mcrt, tmp_path)
    out = tmp_path / "strain.bin"
    r = subprocess.run([exe, scene, str(out), "2", "KIDNEY", "5.0", "0.01", "0.0001"], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    blob = out.read_bytes()
    npix, R = ROWS * COLS, 465
    assert len(blob) == 3 * npix + npix + 5 * 4 * E * R
    sd = mcrt.scene_io.load_scene_file(scene)
    tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    sim = mcrt.Simulator(sd, tr, n_samples=8, strain=dict(STRAIN, noise=1e-4))
    try:
        pic = sim.elastogram(2, out_rows=ROWS, out_cols=COLS)
    finally:
        sim.close()
    assert (pic["rgb"] != pic["grey"][..., None]).any()
    at = 0
    for name in ("rgb", "grey", "strain", "rho", "disp", "truth_strain", "truth_disp"):
        want = pic[name]
        assert blob[at:at + want.nbytes] == want.tobytes(), name
        at += want.nbytes


def test_cli(mcrt, tmp_path):
    """mattausch_hip --elastogram: the PPM and --strain-truth are the Python Simulator's bytes, the PGM beside it is bmode()'s; options that
    make no sense end the program before it touches a device"""
    exe = os.path.join(ROOT, "mcray-tracing_amd", "mattausch_hip")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "mcray-tracing_amd"), "mattausch_hip"])
    cfg, scene = _write_scene(mcrt, tmp_path)
    ppm, truth, pgm = tmp_path / "e.ppm", tmp_path / "truth.raw", tmp_path / "b.pgm"
    r = subprocess.run([exe, scene, "1", "5", str(pgm), str(tmp_path / "rf.bin"), "--elastogram", str(ppm), "--stiffness", "KIDNEY:5,FAT:0.5", "--compress", "0.008",
                        "--strain-window", "12", "--strain-search", "6", "--strain-lsq", "10", "--strain-truth", str(truth), "--noise-db", "35"],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    sd = mcrt.scene_io.load_scene_file(scene)
    tr = mcrt.Transducer(512, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    sim = mcrt.Simulator(sd, tr, n_samples=5, noise=dict(snr_db=35.0),
                         strain=dict(modulus={"KIDNEY": 5.0, "FAT": 0.5}, applied=0.008, window_rows=12, search_rows=6, lsq_rows=10))
    try:
        pic = sim.elastogram(0)
    finally:
        sim.close()
    assert (pic["rgb"] != pic["grey"][..., None]).any()
    assert ppm.read_bytes() == b"P6\n500 400\n255\n" + pic["rgb"].tobytes()
    assert truth.read_bytes() == pic["truth_strain"].tobytes()
    assert pgm.read_bytes() == b"P5\n500 400\n255\n" + pic["grey"].tobytes()
    for bad, word in ((["--strain-window", "8"], "--elastogram"), (["--elastogram", "x.ppm"], "--stiffness"),
                      (["--elastogram", "x.ppm", "--stiffness", "KIDNEY"], "NAME:E"), (["--elastogram", "x.ppm", "--stiffness", "TUMOR:5"], "TUMOR"),
                      (["--elastogram", "x.ppm", "--stiffness", "KIDNEY:5", "--strain-search", "17"], "--strain-search"),
                      (["--elastogram", "x.ppm", "--stiffness", "KIDNEY:5", "--compress", "0.05"], "--compress"),
                      (["--elastogram", "x.ppm", "--stiffness", "KIDNEY:5", "--compound", "3"], "--elastogram"),
                      (["--elastogram", "x.ppm", "--stiffness", "KIDNEY:5", "--freq-compound", "3"], "--elastogram"),
                      (["--elastogram", "x.ppm", "--stiffness", "KIDNEY:5", "--elevation", "3"], "--elastogram")):
        r = subprocess.run([exe, scene, "1", "5"] + bad, capture_output=True, text=True, timeout=240, cwd=str(tmp_path))
        assert r.returncode == 1 and word in r.stdout, (bad, r.stdout)
