"""Measurements for DESIGN 5.22 (HIP events on a stream of the tool's own, warmed up, the forms alternating inside one loop, medians and the
spread): mcrt_strain_compress_frames (k_strain_warp) at sigma 0 and > 0, mcrt_strain_frames (k_strain_track + k_strain_slope) with every
output at the default windows (16, 8, 12) and at the largest (32, 16, 32), and without the slope, at F x E x R = 1 x 512 x 465,
20 x 128 x 465 and 1 x 512 x 2048, beside a device-to-device copy of the 28 bytes per sample the tracker moves at least once (the two
stacks of pairs in, three maps out); and mcrt_elastogram_frames at 400 x 500 beside a copy of its 12 bytes per pixel.  The tracker's rows
carry its complex multiply-adds per second: samples x (2 L + 1)(2 a + 1) over the median (the clipped windows at a line's ends count
as whole).  Appends rows `tag,what,median_us,min_us,p90_us,n,cmadd_per_s` to the csv given as the second argument (default
out/strain_measure.csv); the tag names the build."""
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
CARRIER = 0.3475


def chk(rc):
    assert rc == 0, rc


def main():
    tag = sys.argv[1] if len(sys.argv) > 1 else "default"
    path = sys.argv[2] if len(sys.argv) > 2 else "out/strain_measure.csv"
    ctx = m.Context(0)
    st = vp(); chk(hip.hipStreamCreate(C.byref(st)))
    ctx.set_stream(st.value)
    e0, e1 = vp(), vp(); chk(hip.hipEventCreate(C.byref(e0))); chk(hip.hipEventCreate(C.byref(e1)))

    def once(fn):
        chk(hip.hipEventRecord(e0, st)); fn(); chk(hip.hipEventRecord(e1, st)); chk(hip.hipEventSynchronize(e1))
        ms = C.c_float(); chk(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
        return ms.value * 1000.0

    def alternate(forms, n=100, warm=10):
        ts = {k: [] for k in forms}
        for i in range(warm + n):
            for k, fn in forms.items():
                t = once(fn)
                if i >= warm:
                    ts[k].append(t)
        return {k: (float(np.median(v)), float(np.min(v)), float(np.percentile(v, 90)), len(v)) for k, v in ts.items()}

    rows, work = {}, {}
    rng = np.random.default_rng(1)
    eps = m.host_strain_table([1.0, 5.0], 0.01, 1.0)
    for F, E, R in ((1, 512, 465), (20, 128, 465), (1, 512, 2048)):
        n = F * E * R
        iq, post, tissue, maps, sink = ctx.alloc(8 * n), ctx.alloc(8 * n), ctx.alloc(n), ctx.alloc(12 * n), ctx.alloc(28 * n)
        b = rng.standard_normal((F * E, R + 6, 2)); b = sum(b[:, i:i + R] for i in range(7)) / 7.0
        z = (b[..., 0] + 1j * b[..., 1]) * np.exp(2j * np.pi * CARRIER * np.arange(R))
        ctx.h2d(iq, np.stack([z.real, z.imag], axis=-1).astype(np.float32))
        labels = np.zeros((F, E, R), np.uint8); labels[:, :, R // 3:R // 2] = 1               # a stiff band across every scan-line
        ctx.h2d(tissue, labels)
        disp, rho, strain = maps, maps + 4 * n, maps + 8 * n
        ctx.strain_compress_frames(iq, tissue, F, E, R, eps, CARRIER, post_iq_dev=post)
        shape = "%dx%dx%d " % (F, E, R)
        forms = {"d2d copy of 28 B per sample": lambda: chk(hip.hipMemcpyAsync(vp(sink), vp(iq), 8 * n, 3, st)) or chk(hip.hipMemcpyAsync(vp(sink + 8 * n), vp(post), 8 * n, 3, st))
                 or chk(hip.hipMemcpyAsync(vp(sink + 16 * n), vp(maps), 12 * n, 3, st))}
        for sigma in (0.0, 0.05):
            o = m.strain_opts_struct(sigma=sigma)
            forms["strain_compress_frames sigma=%g all outputs" % sigma] = lambda o=o: ctx.strain_compress_frames(
                iq, tissue, F, E, R, eps, CARRIER, post_iq_dev=sink, truth_disp_dev=sink + 8 * n, truth_strain_dev=sink + 12 * n, opts=o)
        for a, L, g in ((16, 8, 12), (32, 16, 32)):
            o = m.strain_opts_struct(window_rows=a, search_rows=L, lsq_rows=g)
            name = "strain_frames (%d, %d, %d)" % (a, L, g)
            forms[name + " all outputs"] = lambda o=o: ctx.strain_frames(iq, post, F, E, R, CARRIER, disp_dev=disp, rho_dev=rho, strain_dev=strain, opts=o)
            forms[name + " disp and rho"] = lambda o=o: ctx.strain_frames(iq, post, F, E, R, CARRIER, disp_dev=disp, rho_dev=rho, opts=o)
            work[shape + name + " all outputs"] = work[shape + name + " disp and rho"] = n * (2 * L + 1) * (2 * a + 1)
        rows.update({shape + k: v for k, v in alternate(forms).items()})
        for p in (iq, post, tissue, maps, sink):
            ctx.free(p)
    H, W = 400, 500
    n = H * W
    img, grey, rgb, sink = ctx.alloc(8 * n), ctx.alloc(n), ctx.alloc(3 * n), ctx.alloc(12 * n)
    x = np.stack([rng.uniform(-0.002, 0.022, (H, W)), rng.uniform(0.5, 1.0, (H, W))]).astype(np.float32)
    ctx.h2d(img, x); ctx.h2d(grey, rng.integers(0, 256, n).astype(np.uint8))
    lut = m.host_strain_map()
    rows.update({"400x500 " + k: v for k, v in alternate({
        "d2d copy of 12 B per pixel": lambda: chk(hip.hipMemcpyAsync(vp(sink), vp(img), 8 * n, 3, st)) or chk(hip.hipMemcpyAsync(vp(sink + 8 * n), vp(rgb), 3 * n, 3, st))
        or chk(hip.hipMemcpyAsync(vp(sink + 11 * n), vp(grey), n, 3, st)),
        "elastogram_frames": lambda: ctx.elastogram_frames(img, img + 4 * n, grey, 1, H, W, rgb, lut=lut),
    }).items()})
    for p in (img, grey, rgb, sink):
        ctx.free(p)
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    new = not os.path.exists(path)
    with open(path, "a") as f:
        if new:
            f.write("tag,what,median_us,min_us,p90_us,n,cmadd_per_s\n")
        for k, (med, lo, p90, cnt) in rows.items():
            line = "%s,%s,%.2f,%.2f,%.2f,%d,%s" % (tag, k, med, lo, p90, cnt, "%.3e" % (work[k] / (med * 1e-6)) if k in work else "")
            print(line)
            f.write(line + "\n")
    ctx.close()


main()
