"""The C-ABI library loads without a GPU and exports every symbol include/mcrt.h declares; without a GPU the compute
entry points fail loudly (there is no CPU fallback)."""
import ctypes as C
import os
import re
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "mcrt.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mcrt_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_are_exported(mcrt):
    L = mcrt.load_library()
    names = declared_symbols()
    assert len(names) >= 30
    for n in names:
        assert hasattr(L, n), "libmcrt_hip.so does not export " + n
    from importlib import import_module
    lib_mod = import_module("mcray_tracing_amd._lib")
    assert sorted(lib_mod.SYMBOLS) == names, "python binding list and header disagree"


def test_struct_layouts(mcrt):
    from importlib import import_module
    lib_mod = import_module("mcray_tracing_amd._lib")
    assert C.sizeof(lib_mod.BvhNode) == 64 and lib_mod.SEGMENT_DTYPE.itemsize == 64 and C.sizeof(lib_mod.MeshRec) == 16
    p = mcrt.Params()
    assert mcrt.load_library().mcrt_default_params(C.byref(p)) == 0
    # main.cpp:23-37, ray.h:23-24, scene.h:49
    assert (p.n_elements, p.n_samples, p.max_depth, p.n_rows) == (512, 5, 10, 465)
    assert abs(p.frequency - 4.5) < 1e-7 and p.speed_of_sound == 1500 and p.depth_cm == 15.0
    assert abs(p.intensity_epsilon - 1e-10) < 1e-16 and p.initial_intensity == 1.0 and abs(p.ray_start_offset - 0.1) < 1e-8


def test_no_gpu_means_loud_failure(mcrt):
    L = mcrt.load_library()
    if L.mcrt_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(mcrt.McrtError) as e:
        mcrt.Context(0)
    assert e.value.code == -4 and "no CPU fallback" in str(e.value)
    assert L.mcrt_set_params(None, None) != 0 and b"null context" in L.mcrt_last_error()


def test_debug_beam_records_is_bound_and_checks_its_context(mcrt):
    """mcrt_debug_beam_records (the beam stage's records, lists and group keys; tests/test_gpu_beam_lists.py reads them on the GPU): declared, exported, bound
    with six arguments, and refused without a context before anything is copied"""
    L = mcrt.load_library()
    assert "mcrt_debug_beam_records" in declared_symbols() and len(L.mcrt_debug_beam_records.argtypes) == 6
    info = (C.c_uint32 * 5)(7, 7, 7, 7, 7)
    assert L.mcrt_debug_beam_records(None, 1, info, None, None, None) != 0 and b"null context" in L.mcrt_last_error()
    assert hasattr(mcrt.Context, "debug_beam_records")


def test_product_does_not_touch_the_oracle():
    """the oracle is test infrastructure: nothing in the product package may import, load or link it"""
    pkg = os.path.join(ROOT, "mcray-tracing_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h", ".hpp", "Makefile")):
                txt = open(os.path.join(dp, f), errors="ignore").read()
                assert "oracle" not in txt.lower() or f in ("synth.py",) and "mcrt_oracle" not in txt, (dp, f)


def _build_host_surface_test():
    """tests/host/host_surface_test.cpp against host/mcrt_host.hpp + libmcrt_hip.so -> tests/host/host_surface_test"""
    import os, subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "mcray-tracing_amd")
    exe = os.path.join(root, "tests", "host", "host_surface_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(root, "include"), "-I", os.path.join(pkg, "host"), "-o", exe,
                           os.path.join(root, "tests", "host", "host_surface_test.cpp"), "-L", pkg, "-lmcrt_hip", "-Wl,-rpath," + pkg])
    return exe


def test_host_shim_surface_test_compiles(mcrt):
    """the shim's class surface (transducer<N>, psf<>, volume<>, json, scene::cast_rays<S,E>(transducer&) / distance / step,
    rf_image::clear / add_echo / micros_traveled / get_dt / convolve / envelope / postprocess / save, ray_physics::segment) as used by
    tests/host/host_surface_test.cpp must compile and link against libmcrt_hip.so (it runs on the GPU: tests/test_gpu_parity.py); the
    product's own CLI builds too"""
    import os, subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert os.path.exists(_build_host_surface_test())
    subprocess.check_call(["make", "-C", os.path.join(root, "mcray-tracing_amd"), "mattausch_hip"])


def test_walk_kernel_keeps_its_register_budget():
    """k_trace_lane runs four wavefronts per SIMD with a k_march wavefront (80 registers) beside them: 4 x 104 + 80 <= 512.  One register more
    is allocated as 112 and k_march no longer fits -- the frame gets 9 % slower without a single test failing (it happened in round 4: a
    spilled SCALAR register takes a vector register).  The compiler's own report: at most 104 vector registers, nothing spilled."""
    import re, subprocess
    pkg = os.path.join(ROOT, "mcray-tracing_amd")
    out = subprocess.run(["make", "-C", pkg, "resources"], capture_output=True, text=True).stderr
    blocks = out.split("Function Name: ")
    walk = [b for b in blocks if b.startswith("_ZN4mcrt12k_trace_laneILb0EEE")]
    assert walk, out[-2000:]
    get = lambda key: int(re.search(key + r": (\d+)", walk[0]).group(1))
    assert get("VGPRs") <= 104 and get("VGPRs Spill") == 0 and get("SGPRs Spill") == 0 and get(r"ScratchSize \[bytes/lane\]") == 0, walk[0][:900]
    # the five-wavefront form: 80 registers (5 x 80 + k_march's 80 <= 512), no scalar spills; what it spills of vector registers (a dozen, outside
    # its node and leaf loops) stays under 64 bytes of scratch per lane
    wide = [b for b in blocks if b.startswith("_ZN4mcrt17k_trace_lane_wide")]
    assert wide, out[-2000:]
    getw = lambda key: int(re.search(key + r": (\d+)", wide[0]).group(1))
    assert getw("VGPRs") <= 80 and getw("SGPRs Spill") == 0 and getw(r"ScratchSize \[bytes/lane\]") <= 64, wide[0][:900]
    march = [b for b in blocks if b.startswith("_ZN4mcrt7k_marchILb0ELi2ELb1EEE")]
    assert march and int(re.search(r"VGPRs: (\d+)", march[0]).group(1)) <= 80
    # the other kernels of the frame: nothing spilled to scratch, and at least the wavefronts per SIMD their source budgets registers for
    # (k_march spills scalar registers into vector lanes, which costs no scratch: its SGPR spills are not asserted on)
    src = "".join(open(os.path.join(pkg, "csrc", f)).read() for f in ("mcrt_walk.hip", "mcrt_shade.hip", "mcrt_path.hip", "mcrt_march.hip"))
    waves = lambda knob: int(re.search(r"#define " + knob + r" (\d+)", src).group(1))
    budgets = {"_ZN4mcrt17k_trace_lane_wide": waves("MCRT_LANE_WIDE_WAVES"), "_ZN4mcrt14k_trace_packetE": 1,
               "_ZN4mcrt7k_shadeILb0EEE": waves("MCRT_SHADE_WAVES"), "_ZN4mcrt6k_pathE": waves("MCRT_PATH_WAVES"), "_ZN4mcrt7k_marchI": waves("MCRT_MARCH_WAVES")}
    for prefix, budget in budgets.items():
        found = [b for b in blocks if b.startswith(prefix)]
        assert len(found) == (6 if prefix == "_ZN4mcrt7k_marchI" else 1), (prefix, out[-2000:])
        for b in found:
            val = lambda key: int(re.search(key + r": (\d+)", b).group(1))
            assert val("VGPRs Spill") == 0 and val(r"ScratchSize \[bytes/lane\]") == 0 and val(r"Occupancy \[waves/SIMD\]") >= budget, b[:900]
