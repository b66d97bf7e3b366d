"""Measurements for DESIGN 5.20 (HIP events on a stream of the tool's own, warmed up, the forms alternating inside one loop, medians and the
spread): mcrt_flow_frames (k_flow<N, WALL> + k_flow_avg) at F = 1, E = 512, R = 465 and at F = 20, E = 128, R = 465, for N = 8 and 16, at
sigma 0 and > 0, with every output and with corr_dev alone, beside a device-to-device copy of the bytes the call moves at least once (17
in and 24 out per sample with every output: the two I/Q stacks and the labels in, corr, vel, var and truth out); mcrt_flow_split_frames
beside its own 13 bytes per sample; and mcrt_colour_frames at 400 x 500 beside its 13 + 7.  Appends rows
`tag,what,median_us,min_us,p90_us,n` to the csv given as the second argument (default out/flow_measure.csv); the tag names the build."""
import ctypes as C
import os
import sys
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
    tag = sys.argv[1] if len(sys.argv) > 1 else "default"
    path = sys.argv[2] if len(sys.argv) > 2 else "out/flow_measure.csv"
    ctx = m.Context(0)
    st = vp(); chk(hip.hipStreamCreate(C.byref(st)))
    ctx.set_stream(st.value)
    e0, e1 = vp(), vp(); chk(hip.hipEventCreate(C.byref(e0))); chk(hip.hipEventCreate(C.byref(e1)))

    def once(fn):
        chk(hip.hipEventRecord(e0, st)); fn(); chk(hip.hipEventRecord(e1, st)); chk(hip.hipEventSynchronize(e1))
        ms = C.c_float(); chk(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
        return ms.value * 1000.0

    def alternate(forms, n=200, warm=10):
        ts = {k: [] for k in forms}
        for i in range(warm + n):
            for k, fn in forms.items():
                t = once(fn)
                if i >= warm:
                    ts[k].append(t)
        return {k: (float(np.median(v)), float(np.min(v)), float(np.percentile(v, 90)), len(v)) for k, v in ts.items()}

    rows = {}
    rng = np.random.default_rng(1)
    v_nyq = m.host_flow_nyquist(4.5)
    for F, E, R in ((1, 512, 465), (20, 128, 465)):
        n = F * E * R
        iq, tissue, out, sink = ctx.alloc(16 * n), ctx.alloc(n), ctx.alloc(24 * n), ctx.alloc(41 * n)
        rf, parts = ctx.alloc(4 * n), ctx.alloc(8 * n)
        ctx.h2d(iq, rng.standard_normal(4 * n).astype(np.float32))
        ctx.h2d(rf, rng.standard_normal(n).astype(np.float32))
        labels = np.zeros((F, E, R), np.uint8); labels[:, :, R // 3:R // 2] = 1               # a vessel across every scan-line
        ctx.h2d(tissue, labels)
        d = rng.standard_normal((E, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
        ph, tr = m.host_flow_phasors(v_nyq, [[0, 0, 0], [100.0, -50.0, 20.0]], d.astype(np.float32))
        corr, vel, var, truth = out, out + 12 * n, out + 16 * n, out + 20 * n
        shape = "%dx%dx%d " % (F, E, R)
        forms = {"d2d copy of 41 B per sample": lambda: chk(hip.hipMemcpyAsync(vp(sink), vp(iq), 16 * n, 3, st)) or chk(hip.hipMemcpyAsync(vp(sink + 16 * n), vp(out), 24 * n, 3, st))
                 or chk(hip.hipMemcpyAsync(vp(sink + 40 * n), vp(tissue), n, 3, st)),
                 "d2d copy of 13 B per sample": lambda: chk(hip.hipMemcpyAsync(vp(sink), vp(iq), 13 * n, 3, st)),
                 "flow_split_frames": lambda: ctx.flow_split_frames(rf, tissue, F, E, R, [0, 1], parts)}
        for N in (8, 16):
            for sigma in (0.0, 0.05):
                o = m.flow_opts_struct(n_packets=N, sigma=sigma)
                name = "flow_frames N=%d sigma=%g" % (N, sigma)
                forms[name + " all outputs"] = lambda o=o: ctx.flow_frames(iq, iq + 8 * n, tissue, F, E, R, v_nyq, ph, tr, corr_dev=corr, vel_dev=vel, var_dev=var, truth_dev=truth, opts=o)
                forms[name + " corr alone"] = lambda o=o: ctx.flow_frames(iq, iq + 8 * n, tissue, F, E, R, v_nyq, ph, tr, corr_dev=corr, opts=o)
        o = m.flow_opts_struct(n_packets=8, sigma=0.05, avg_rows=8, avg_lines=4)
        forms["flow_frames N=8 sigma=0.05 window (8, 4) all outputs"] = lambda o=o: ctx.flow_frames(iq, iq + 8 * n, tissue, F, E, R, v_nyq, ph, tr, corr_dev=corr, vel_dev=vel,
                                                                                                   var_dev=var, truth_dev=truth, opts=o)
        rows.update({shape + k: v for k, v in alternate(forms).items()})
        for p in (iq, tissue, out, sink, rf, parts):
            ctx.free(p)
    H, W = 400, 500
    n = H * W
    img, grey, rgb, vel, sink = ctx.alloc(12 * n), ctx.alloc(n), ctx.alloc(3 * n), ctx.alloc(4 * n), ctx.alloc(20 * n)
    x = rng.standard_normal((3, H, W)).astype(np.float32); x[0] = np.abs(x[0])
    ctx.h2d(img, x); ctx.h2d(grey, rng.integers(0, 256, n).astype(np.uint8))
    lut = m.host_colour_map()
    rows.update({"400x500 " + k: v for k, v in alternate({
        "d2d copy of 20 B per pixel": lambda: chk(hip.hipMemcpyAsync(vp(sink), vp(img), 12 * n, 3, st)) or chk(hip.hipMemcpyAsync(vp(sink + 12 * n), vp(vel), 4 * n, 3, st))
        or chk(hip.hipMemcpyAsync(vp(sink + 16 * n), vp(rgb), 3 * n, 3, st)) or chk(hip.hipMemcpyAsync(vp(sink + 19 * n), vp(grey), n, 3, st)),
        "colour_frames rgb + vel": lambda: ctx.colour_frames(img, grey, 1, H, W, v_nyq, rgb, vel_img_dev=vel, lut=lut, power_thr=0.3, vel_thr_mm_s=10.0),
        "colour_frames rgb alone": lambda: ctx.colour_frames(img, grey, 1, H, W, v_nyq, rgb, lut=lut, power_thr=0.3, vel_thr_mm_s=10.0),
    }).items()})
    for p in (img, grey, rgb, vel, sink):
        ctx.free(p)
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    new = not os.path.exists(path)
    with open(path, "a") as f:
        if new:
            f.write("tag,what,median_us,min_us,p90_us,n\n")
        for k, (med, lo, p90, cnt) in rows.items():
            line = "%s,%s,%.2f,%.2f,%.2f,%d" % (tag, k, med, lo, p90, cnt)
            print(line)
            f.write(line + "\n")
    ctx.close()


main()
