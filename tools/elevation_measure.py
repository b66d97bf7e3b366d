"""Measurements for DESIGN 5.6: the fold kernel beside k_conv_lateral over the same images and a device-to-device copy of the input's bytes
(HIP events here; the same run under rocprofv3 gives the kernel trace), and a K = 7 frame end to end against 7 frames of a plain pass."""
import ctypes as C
import json
import os
import sys
import time
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mcray_tracing_amd as m

hip = C.CDLL("libamdhip64.so")
vp = C.c_void_p
hip.hipMemcpyAsync.argtypes = [vp, vp, C.c_size_t, C.c_int, vp]
hip.hipEventRecord.argtypes = [vp, vp]
hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), vp, vp]
hip.hipEventSynchronize.argtypes = [vp]


def chk(rc):
    assert rc == 0, rc


def main():
    out = {}
    ctx = m.Context(0)
    st = vp(); chk(hip.hipStreamCreate(C.byref(st)))
    ctx.set_stream(st.value)
    e0, e1 = vp(), vp(); chk(hip.hipEventCreate(C.byref(e0))); chk(hip.hipEventCreate(C.byref(e1)))

    def timed(fn, n=30, warm=3):
        ts = []
        for i in range(warm + n):
            chk(hip.hipEventRecord(e0, st)); fn(); chk(hip.hipEventRecord(e1, st)); chk(hip.hipEventSynchronize(e1))
            ms = C.c_float(); chk(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
            if i >= warm:
                ts.append(ms.value * 1000.0)
        return float(np.median(ts))

    K, E, R = 7, 128, 465
    psf = m.Psf()
    w = m.host_psf_elevation(0.1, 145, R, 0.322, (), 20.0, K, True)
    rng = np.random.default_rng(1)
    for F in (20, 128):
        n_in = F * K * E * R
        src = ctx.alloc(n_in * 4); dst = ctx.alloc(n_in * 4); rf = ctx.alloc(F * E * R * 4)
        ctx.h2d(src, rng.standard_normal(n_in).astype(np.float32))
        ctx.synchronize()
        r = {}
        r["fold_us"] = timed(lambda: ctx.elevation_frames(src, F, K, E, R, w, rf))
        r["convolve_frames_us (axial + lateral)"] = timed(lambda: ctx.convolve_frames(src, F * K, E, R, psf.axial_kernel, psf.lateral_kernel))
        r["d2d_copy_us"] = timed(lambda: chk(hip.hipMemcpyAsync(vp(dst), vp(src), n_in * 4, 3, st)))
        r["bytes_in"] = n_in * 4; r["bytes_out"] = F * E * R * 4
        out["F=%d" % F] = r
        for d in (src, dst, rf):
            ctx.free(d)
    ctx.close()

    # end to end: a frame with K = 7 planes against 7 frames of a plain pass (sphere scene, 128 scan-lines)
    cfg, meshes = m.synth.sphere_scene(5)
    sd = m.scene_io.build_scene(cfg, meshes)
    tr = m.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    for S in (5, 64):
        sim = m.Simulator(sd, tr, n_samples=S, elevation=True)
        c = sim.ctx
        buf = c.alloc(K * E * sim.R * 4)

        def plain():
            c.trace_frames(0, K, buf); c.synchronize()

        def slab():
            sim.trace(0); c.synchronize()

        tp, ts = [], []
        for i in range(25):
            t = time.perf_counter(); plain(); tp.append(time.perf_counter() - t)
            t = time.perf_counter(); slab(); ts.append(time.perf_counter() - t)
        out["end_to_end S=%d" % S] = {"7 frames of a pass ms": float(np.median(tp[5:]) * 1e3), "one frame, 7 planes + fold ms": float(np.median(ts[5:]) * 1e3)}
        c.free(buf); sim.close()
    print(json.dumps(out, indent=1))
    os.makedirs("out", exist_ok=True)
    with open("out/elevation_measure_%s.json" % (sys.argv[1] if len(sys.argv) > 1 else "events"), "w") as f:
        json.dump(out, f, indent=1)


main()
