"""Volume rendering without a GPU (include/mcrt.h: mcrt_render_view, mcrt_render_opts, mcrt_default_render_opts, mcrt_render_view_for_grid,
mcrt_render_frames): the structs and defaults, the view helper against its formulas in numpy double, its error cases, identities of the numpy
mirror (tests/render_mirror.py) that hold tests/test_gpu_render.py honest, the coverage of the views that test uses, the helper under
AddressSanitizer + UBSan in a program of its own, and k_render's registers."""
import ctypes as C
import math
import os
import re
import subprocess
import numpy as np
import pytest

import render_mirror as rm

f32 = np.float32
INVALID, LIMIT = -1, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mcray-tracing_amd")


# ------------------------------------------------------------------ structs, defaults, header
def test_structs_defaults_and_version(mcrt):
    V, O = mcrt.RenderView, mcrt.RenderOpts
    assert C.sizeof(V) == 64 and [getattr(V, n).offset for n in ("origin", "di", "dj", "ds", "nx", "ny", "n_steps", "_pad")] == [0, 12, 24, 36, 48, 52, 56, 60]
    assert C.sizeof(O) == 32 and [getattr(O, n).offset for n in ("mode", "lo", "hi", "threshold", "ramp", "opacity", "depth_cue", "t_cut")] == [0, 4, 8, 12, 16, 20, 24, 28]
    L = mcrt.load_library()
    for in_u8, hi in ((0, 1.0), (1, 255.0), (7, 255.0)):
        o = O()
        C.memset(C.byref(o), 0xA5, 32)
        assert L.mcrt_default_render_opts(C.byref(o), in_u8) == 0
        assert (o.mode, o.lo, o.hi, o.threshold, o.ramp, o.opacity, o.depth_cue, o.t_cut) == (2, 0.0, hi, 0.25, 0.25, 1.0, 0.5, 0.0)
        assert rm.defaults(bool(in_u8)) == dict(mode=o.mode, lo=o.lo, hi=o.hi, threshold=o.threshold, ramp=o.ramp, opacity=o.opacity, depth_cue=o.depth_cue, t_cut=o.t_cut)
    assert L.mcrt_default_render_opts(None, 0) == INVALID and b"null" in L.mcrt_last_error()
    assert mcrt.RENDER_MODES == {"mip": 0, "mean": 1, "surface": 2}
    assert L.mcrt_version() == 109
    src = open(os.path.join(ROOT, "include", "mcrt.h")).read()
    assert re.search(r"#define MCRT_VERSION 109\b", src)
    block = src[src.index("#define MCRT_VERSION"):src.index("typedef enum")]
    added = block[block.index("mcrt_render_view"):]
    for name in ("mcrt_render_view", "mcrt_render_opts", "mcrt_default_render_opts", "mcrt_render_view_for_grid", "mcrt_render_frames", "additive"):
        assert name in added, name
    assert "enum { MCRT_RENDER_MIP = 0, MCRT_RENDER_MEAN = 1, MCRT_RENDER_SURFACE = 2 };" in src
    # the call without a context is refused before anything else is looked at
    assert L.mcrt_render_frames(None, None, 0, 1, 1, 1, 1, None, None, None, None, None) == INVALID and b"null context" in L.mcrt_last_error()


# ------------------------------------------------------------------ the view helper
def _ulps(got, want):
    """|got - want| in units of want's float32 spacing (want in double).  A component that is zero in exact arithmetic comes out of a double
    evaluation as rounding noise, some 2^-52 of the vector's largest component, or as 0, depending on the order of the operations; an ulp of
    such noise says nothing, so the spacing is taken no finer than that of 2^-24 of the largest component: 2^-47 of it, above the noise and
    2^24 times finer than the largest component's own float spacing"""
    want = np.asarray(want, np.float64)
    scale = np.maximum(np.abs(want), np.abs(want).max() * 2.0 ** -24)
    return np.abs(np.asarray(got, np.float64) - want) / np.spacing(scale.astype(f32)).astype(np.float64)


GRIDS = {"axis": ((-3.0, 41.0, -2.5), (0.5, 0, 0), (0, 0.375, 0), (0, 0, 0.75)),
         "sheared": ((12.0, 55.0, 4.0), (0.5, 0.2, 0.0), (0.0, 0.375, -0.1), (0.3, 0.0, 0.75)),
         "rotated": ((-8.0, 70.0, 1.0), (0.3, 0.4, 0.0), (-0.4, 0.3, 0.0), (0.1, 0.0, 0.6))}


@pytest.mark.parametrize("gname", sorted(GRIDS))
def test_view_helper_matches_its_formulas(mcrt, gname):
    o, du, dv, dw = GRIDS[gname]
    worst = 0.0
    for block in rm.BLOCKS[:3] + [(2, 3, 4)]:
        g = mcrt.volume_grid(o, du, dv, dw, *block)
        for d in rm.DIRECTIONS + [(0.0, 1.0, 0.0)]:
            for up in ((0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.3, -0.2, 0.9)):
                if np.linalg.norm(np.cross(d, up)) < 1e-9:
                    continue
                for (nx, ny), pixel, step in (((33, 35), 0.21, 0.37), ((1, 1), 1.0, 0.5), ((64, 3), 0.0625, 1.25)):
                    v = mcrt.render_view(g, d, up, pixel, step, nx, ny)
                    want = rm.view_model(g, d, up, pixel, step, nx, ny)
                    assert (v.nx, v.ny, v.n_steps, v._pad) == (nx, ny, want[4], 0)
                    assert v.n_steps == int(math.floor(2.0 * rm.half_diagonal(g) / step)) + 1
                    for got, w in zip((v.origin, v.di, v.dj, v.ds), want[:4]):
                        u = _ulps(list(got), w)
                        worst = max(worst, float(u.max()))
                        assert (u <= 1.0).all(), (block, d, up, nx, ny, list(got), w)
    print("worst difference: %.3f float ulps" % worst)


def test_view_helper_is_exact_on_an_axis_aligned_grid(mcrt):
    """power-of-two steps, looking along +dw with up = dv and pixel_mm = |du|: the columns of the picture run along the viewer's right,
    dn x up, which is -du in a right-handed grid and +du in its mirror image; rows run against up"""
    for sign in (1.0, -1.0):
        g = mcrt.volume_grid((-3.0, 41.0, -2.5), (sign * 0.5, 0, 0), (0, 0.25, 0), (0, 0, 0.125), 17, 13, 11)
        v = mcrt.render_view(g, (0, 0, 1), (0, 1, 0), 0.5, 0.0625, 9, 7)
        assert list(v.di) == [-sign, 0.0, 0.0] and list(v.dj) == [0.0, -2.0, 0.0] and list(v.ds) == [0.0, 0.0, 0.5]
        v = mcrt.render_view(g, (0, 0, 1), (0, 1, 0), 0.5, 0.25, 9, 7)
        assert list(v.ds) == [0.0, 0.0, 0.25 / 0.125]
    g = mcrt.volume_grid((0, 0, 0), (-0.5, 0, 0), (0, 0.5, 0), (0, 0, 0.25), 9, 9, 9)       # the mirrored grid with square pixels
    v = mcrt.render_view(g, (0, 0, 3.5), (0, 2, 0), 0.5, 0.5, 9, 9)
    assert list(v.di) == [1.0, 0.0, 0.0] and list(v.dj) == [0.0, -1.0, 0.0] and list(v.ds) == [0.0, 0.0, 0.5 / 0.25]
    # the central ray passes the block's centre: origin + 4 di + 4 dj + t ds = (4, 4, 4) for some t
    o = np.array(list(v.origin), np.float64)
    assert o[0] + 4 == 4.0 and o[1] - 4 == 4.0


def test_view_helper_errors_leave_the_view_untouched(mcrt):
    L = mcrt.load_library()
    good = mcrt.volume_grid((-3.0, 41.0, -2.5), (0.5, 0, 0), (0, 0.375, 0), (0, 0, 0.75), 17, 13, 11)

    def grid(**kw):
        g = mcrt.volume_grid((-3.0, 41.0, -2.5), (0.5, 0, 0), (0, 0.375, 0), (0, 0, 0.75), 17, 13, 11)
        for k, val in kw.items():
            if isinstance(val, tuple):
                getattr(g, k)[val[0]] = val[1]
            else:
                setattr(g, k, val)
        return g

    def call(g=good, d=(0, 0, 1), up=(0, 1, 0), pixel=0.25, step=0.25, nx=4, ny=4, out=True):
        v = mcrt.RenderView()
        C.memset(C.byref(v), 0xA5, 64)
        dd = (C.c_double * 3)(*d) if d is not None else None
        uu = (C.c_double * 3)(*up) if up is not None else None
        rc = L.mcrt_render_view_for_grid(C.byref(g) if g is not None else None, dd, uu, pixel, step, nx, ny, C.byref(v) if out else None)
        assert bytes(v) == b"\xa5" * 64 or rc == 0
        return rc

    nan, inf = math.nan, math.inf
    assert call() == 0
    for kw in (dict(g=None), dict(d=None), dict(up=None), dict(out=False), dict(nx=0), dict(ny=0), dict(d=(0, 0, 0)), dict(d=(0, nan, 1)), dict(d=(inf, 0, 0)),
               dict(up=(0, 0, -2)), dict(up=(0, 0, 0)), dict(up=(nan, 1, 0)), dict(up=(0, inf, 0)), dict(pixel=0.0), dict(pixel=-1.0), dict(pixel=nan), dict(pixel=inf),
               dict(step=0.0), dict(step=-0.5), dict(step=nan), dict(step=inf), dict(g=grid(dw_mm=(2, 0.0))), dict(g=grid(dw_mm=(2, 0.0), du_mm=(2, 0.0))),
               dict(g=grid(nu=0)), dict(g=grid(nv=0)), dict(g=grid(nw=0)), dict(g=grid(origin_mm=(1, nan))),
               dict(g=grid(du_mm=(0, inf))), dict(g=grid(dv_mm=(2, -inf)))):
        assert call(**kw) == INVALID, kw
    coplanar = grid(dw_mm=(2, 0.0)); coplanar.dw_mm[0] = 0.5; coplanar.dw_mm[1] = 0.375      # dw = du + dv
    assert call(g=coplanar) == INVALID and b"span" in L.mcrt_last_error()
    assert call(d=(0, 0, 0)) == INVALID and b"dir_mm" in L.mcrt_last_error()
    assert call(up=(0, 0, 5)) == INVALID and b"up_mm" in L.mcrt_last_error()
    assert call(pixel=0.0) == INVALID and b"pixel_mm" in L.mcrt_last_error()
    assert call(step=0.0) == INVALID and b"step_mm" in L.mcrt_last_error()
    assert call(step=1e-4) == LIMIT and b"n_steps" in L.mcrt_last_error() and call(step=1e-300) == LIMIT
    two_l = 2.0 * rm.half_diagonal(good)
    assert call(step=two_l / 4095.5) == 0 and call(step=two_l / 4096.5) == LIMIT                   # 4096 steps and 4097


# ------------------------------------------------------------------ identities of the mirror
def _identity_view(mcrt, nu, nv, nw):
    v = mcrt.RenderView()
    v.di[0] = 1.0; v.dj[1] = 1.0; v.ds[2] = 1.0
    v.nx, v.ny, v.n_steps = nu, nv, nw
    return v


@pytest.mark.parametrize("shape", [(5, 7, 9), (11, 13, 17), (5, 35, 33)])
def test_mirror_mip_and_mean_under_the_identity_view(mcrt, shape):
    """origin 0, di = e_u, dj = e_v, ds = e_w, one step per layer, one pixel per column: MIP is the block's maximum along w and MEAN the
    float mean summed in layer order -- neither computed with the mirror's sampler"""
    nw, nv, nu = shape
    block = np.random.default_rng(nu).random(shape).astype(f32)
    v = _identity_view(mcrt, nu, nv, nw)
    out, out8, depth = rm.render(block, v, rm.defaults(mode="mip"))
    assert np.array_equal(out, block.max(axis=0)) and np.array_equal(depth, block.argmax(axis=0).astype(f32))
    assert np.array_equal(out8, (out * f32(255.0) + f32(0.5)).astype(np.uint8))
    out, _, depth = rm.render(block, v, rm.defaults(mode="mean"))
    total = np.zeros((nv, nu), f32)
    for k in range(nw):
        total = (total + block[k]).astype(f32)
    assert np.array_equal(out, (total / f32(nw)).astype(f32)) and np.all(depth == -1)
    # bytes: the window 0..255 brings them to the same scale
    b8 = np.random.default_rng(nv).integers(0, 256, shape, dtype=np.uint8)
    out, _, _ = rm.render(b8, v, rm.defaults(True, mode="mip"))
    assert np.array_equal(out, ((b8.max(axis=0).astype(f32) - f32(0)) * f32(1.0 / 255.0)).astype(f32))


def test_mirror_surface_is_the_first_voxel_above_the_threshold(mcrt):
    """opacity 1 with the narrowest ramp is a step at the threshold, and without depth cueing the picture is the first voxel above it"""
    nw, nv, nu = 9, 7, 5
    block = np.random.default_rng(4).random((nw, nv, nu)).astype(f32)
    block[:, 0, 0] = 0.1                                         # a ray that never meets the surface
    thr = 0.6
    ramp = float(np.spacing(f32(thr)))                           # threshold + ramp is the next float: every x above the threshold is opaque
    v = _identity_view(mcrt, nu, nv, nw)
    out, _, depth = rm.render(block, v, rm.defaults(mode="surface", threshold=thr, ramp=1e-6, opacity=1.0, depth_cue=0.0))
    above = block > f32(thr) + f32(1e-6)
    clear = ~((block > f32(thr)) & ~above).any()
    assert clear and ramp < 1e-6
    first = above.argmax(axis=0)
    want = np.where(above.any(axis=0), np.take_along_axis(block, first[None], 0)[0], f32(0))
    assert np.array_equal(out, want)
    assert np.array_equal(depth, np.where(above.any(axis=0), first, -1).astype(f32)) and depth[0, 0] == -1 and out[0, 0] == 0
    # the early stop changes nothing here: behind an opaque voxel nothing is added anyway
    cut = rm.render(block, v, rm.defaults(mode="surface", threshold=thr, ramp=1e-6, opacity=1.0, depth_cue=0.0, t_cut=0.1))
    assert np.array_equal(cut[0], out) and np.array_equal(cut[2], depth)


def test_mirror_ignores_what_is_not_covered(mcrt):
    """a view from outside: rays that miss the block are black with depth -1, in every mode, and NaN voxels are no echo"""
    block = np.full((3, 4, 5), f32(0.8)); block[1, 1, 1] = np.nan
    v = mcrt.RenderView()
    v.origin[0] = -40.0; v.origin[1] = -3.0; v.origin[2] = -2.0
    v.di[0] = 1.0; v.dj[1] = 1.0; v.ds[2] = 0.5
    v.nx, v.ny, v.n_steps = 8, 8, 12
    for mode in ("mip", "mean", "surface"):
        out, out8, depth = rm.render(block, v, rm.defaults(mode=mode))
        assert np.all(out == 0) and np.all(out8 == 0) and np.all(depth == -1)
    assert not rm.coverage(v, block.shape).any()


# ------------------------------------------------------------------ the GPU test's inputs
def test_the_gpu_cases_look_at_their_blocks(mcrt):
    """from the views alone: in every (block, direction, picture) case of tests/test_gpu_render.py at least 80 % of the rays have at least a
    quarter of their steps covered -- a kernel that samples the wrong voxel cannot hide in empty space"""
    worst_rays, worst_steps = 1.0, 1.0
    for block, d, pic in rm.CASES:
        v = rm.case_view(mcrt, block, d, pic)
        cov = rm.coverage(v, block[::-1])
        assert v.n_steps in (36, 37) or (block == (1, 1, 1) and v.n_steps == 1)
        rays = (cov.mean(axis=0) >= 0.25).mean()
        worst_rays = min(worst_rays, rays); worst_steps = min(worst_steps, cov.mean())
        assert rays >= 0.8, (block, d, pic, rays, cov.mean())
    print("worst case: %.1f %% of the rays, %.1f %% of all steps covered" % (100 * worst_rays, 100 * worst_steps))
    # a long thin block under the same recipe is mostly empty space: it is not in the table
    g = mcrt.volume_grid((-3.0, 41.0, -2.5), (0.5, 0, 0), (0, 0.375, 0), (0, 0, 0.75), 257, 3, 2)
    L2 = 2.0 * rm.half_diagonal(g)
    thin = [rm.coverage(mcrt.render_view(g, d, rm.UP, 0.6 * L2 / 35, L2 / 36, 33, 35), (2, 3, 257)).mean() for d in rm.DIRECTIONS]
    assert min(thin) < 0.25 and (257, 3, 2) not in rm.BLOCKS


# ------------------------------------------------------------------ sanitizers, registers
def test_host_functions_run_clean_under_asan_ubsan(mcrt, tmp_path):
    """tests/host/render_sanitize_driver.cpp + csrc/mcrt_host.cpp under AddressSanitizer and UBSan, a program of its own: the helper's error
    cases leave a guarded view untouched, its good cases give what the shipped library gives"""
    exe = str(tmp_path / "render_sanitize_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "host", "render_sanitize_driver.cpp"),
                           os.path.join(PKG, "csrc", "mcrt_host.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("DONE"), r.stdout[-3000:] + r.stderr[-6000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-6000:]
    out = dict(line.split(": ", 1) for line in r.stdout.splitlines()[:-1])
    assert len(out) == 31
    good = {"view.along_w": "ok 33 x 35, 48 steps, finite", "view.oblique": "ok 64 x 3, 238 steps, finite", "view.one_pixel": "ok 1 x 1, 12 steps, finite",
            "view.one_voxel": "ok 5 x 4, 1 steps, finite", "view.sheared_grid": None, "view.many_steps": "ok 2 x 2, 3884 steps, finite"}
    for k, val in out.items():
        if k in good:
            assert val.startswith("ok ") and val.endswith(", finite") and (good[k] is None or val == good[k]), (k, val)
        elif k == "opts.defaults":
            assert val == "0 -1 mode 2 window 0 1"
        else:
            assert val == "error %d untouched" % (LIMIT if k in ("view.too_many_steps", "view.steps_overflow") else INVALID), (k, val)
    g = mcrt.volume_grid((-3.0, 41.0, -2.5), (0.5, 0, 0), (0, 0.375, 0), (0, 0, 0.75), 17, 13, 11)
    assert mcrt.render_view(g, (0, 0, 1), (0, 1, 0), 0.25, 0.25, 33, 35).n_steps == 48


def test_render_kernels_keep_their_registers():
    """the compiler's own report: neither k_render spills or uses scratch or LDS, both fit 64 registers and run 8 wavefronts per SIMD;
    k_volume and the plain k_compound, which live in other translation units, keep the parent commit's figures: k_volume<false> / <true>
    93 / 96 registers at 5 wavefronts per SIMD, k_compound's plain instantiations 75 / 89 / 81 registers; no vector register of either is spilled, no scratch"""
    out = subprocess.run(["make", "-C", PKG, "resources"], capture_output=True, text=True).stderr
    blocks = out.split("Function Name: ")
    val = lambda b, key: int(re.search(key + r": (\d+)", b).group(1))
    one = lambda prefix: [b for b in blocks if b.startswith(prefix)]
    render = one("_ZN4mcrt8k_renderILb")
    assert len(render) == 2, out[-2000:]
    for b in render:
        assert val(b, "VGPRs Spill") == 0 and val(b, "SGPRs Spill") == 0 and val(b, r"ScratchSize \[bytes/lane\]") == 0 and val(b, r"LDS Size \[bytes/block\]") == 0, b[:900]
        assert val(b, "VGPRs") <= 64 and val(b, r"Occupancy \[waves/SIMD\]") == 8, b[:900]
    for prefix, vgprs, waves in (("_ZN4mcrt8k_volumeILb0EEE", 93, 5), ("_ZN4mcrt8k_volumeILb1EEE", 96, 5), ("_ZN4mcrt10k_compoundILb0ELb0ELi0ELi0EEE", 75, None),
                                 ("_ZN4mcrt10k_compoundILb1ELb1ELi0ELi0EEE", 89, None), ("_ZN4mcrt10k_compoundILb1ELb0ELi0ELi0EEE", 81, None)):
        found = one(prefix)
        assert len(found) == 1, (prefix, out[-2000:])
        b = found[0]
        assert val(b, "VGPRs") == vgprs and val(b, "VGPRs Spill") == 0 and val(b, r"ScratchSize \[bytes/lane\]") == 0, b[:900]
        assert waves is None or (val(b, r"Occupancy \[waves/SIMD\]") == waves and val(b, "SGPRs Spill") == 0), b[:900]
