"""The oracle under AddressSanitizer + UBSan (CPU build only; GPU sanitizers are not available on the pool): a small frame
through every code path -- brute force, BVH2 and BVH4 walks, thickness draw, vessels, convolution, envelope, scan conversion, the
test entry points into the physics, the counting build and the analysis walks of tools/."""
import os
import subprocess
import sys
import textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_oracle_runs_clean_under_asan_ubsan(mcrt):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "libmcrt_oracle_asan.so"], stdout=subprocess.DEVNULL)
    libasan = subprocess.check_output(["gcc", "-print-file-name=libasan.so"], text=True).strip()
    code = textwrap.dedent("""
        import sys, ctypes, numpy as np
        sys.path.insert(0, %r)
        import mcray_tracing_amd as m
        from oracle import orc
        orc._LIB = None
        orc.build = lambda force=False: %r
        cfg, meshes = m.synth.liver_scene(1)
        sd = m.scene_io.build_scene(cfg, meshes)
        nodes, btri, n4, _ = m.host_build_bvh4(sd.tri, sd.tri_mesh)
        tr = m.Transducer(6, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
        tex = orc.texture(8)
        osc = orc.OracleScene(sd.tri, sd.tri_mesh, sd.meshes, sd.materials, sd.start_mat, sd.spacing, bvh=(nodes, btri)); osc.set_bvh4(n4)
        p = orc.default_params(n_elements=6, n_samples=9, tex_n=8)
        outs = [osc.trace_frame(p, tr.pos, tr.dir, tex, use_bvh=k, want_segs=True) for k in (0, 1, 2)]
        assert all(np.array_equal(outs[0]["hits"], o["hits"]) and np.array_equal(outs[0]["rf_fix"], o["rf_fix"]) for o in outs)
        ax, lat = orc.psf()
        img = orc.envelope(orc.convolve(np.nan_to_num(outs[0]["rf"]), ax, lat))
        sc = orc.scan_convert(img)
        one_row = np.array([[1.0, -2.0, 3.0]], np.float32)
        assert np.array_equal(orc.envelope(one_row), one_row)          # rows == 1: nothing read past the image
        # the test entry points into the physics, the counting walk and the analysis walks (tools/seed_count.py, tools/packet_count.py) as well
        osc.counting(True)
        oc = osc.trace_frame(p, tr.pos, tr.dir, tex, use_bvh=2, want_segs=True); osc.counting(False)
        assert np.array_equal(oc["hits"], outs[0]["hits"]) and orc.counters()["echo_guard_trips"] == 0
        rng = (int(p.seed), 0, 1, 2, 3)
        w, tries = orc.random_unit_vector([0.0, 0.6, 0.8], 0.999, rng); assert tries >= 1 and np.isfinite(w).all()
        assert 0.0 < orc.power_cosine(1000000, 0.5) <= 1.0 and orc.thickness(0.3, rng) >= 0.0
        ray = orc.ray_state([0.0, 0.0, 0.0], [0.0, 0.6, 0.8], media=int(sd.start_mat), intensity=0.25)
        hd = osc.hit_boundary(p, ray, [0.1, 0.2, 0.3], [0.0, -0.6, -0.8], 0, rng); assert hd.ruv_attempts >= 1
        L, f, t = osc.ray_segment(p, ray); assert L > 0 and osc.travel(ray, [0.0, 0.6, 0.8]) > 0
        segs = np.ascontiguousarray(oc["segs"][:, :, 0].reshape(-1))
        rfseg, steps = osc.accumulate_segment(p, tex, segs[0]); assert rfseg.shape == (p.n_rows,)
        L_ = orc.lib(); n = len(segs)
        out = np.zeros((n, 2), np.uint32); tri = np.zeros(n, np.int32)
        L_.orc_seed_count.restype = None
        L_.orc_seed_count.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
        for mode in (0, 1):
            L_.orc_seed_count(ctypes.byref(osc.c), ctypes.byref(p), segs.ctypes.data, n, mode, None, out.ctypes.data, tri.ctypes.data, 2)
            assert np.array_equal(tri, oc["hits"][:, :, 0].reshape(-1))
        pk = np.zeros(((n + 15) // 16, 6), np.uint32)
        L_.orc_packet_count.restype = None
        L_.orc_packet_count.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
        L_.orc_packet_count(ctypes.byref(osc.c), ctypes.byref(p), segs.ctypes.data, n, 16, 1, pk.ctypes.data, tri.ctypes.data, 2)
        assert np.array_equal(tri, oc["hits"][:, :, 0].reshape(-1)) and pk[:, 0].sum() > 0
        print("OK", int((outs[0]["hits"] >= 0).sum()), float(np.abs(sc).sum()) >= 0)
    """) % (ROOT, os.path.join(ROOT, "oracle", "libmcrt_oracle_asan.so"))
    env = dict(os.environ, LD_PRELOAD=libasan, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
