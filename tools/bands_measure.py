"""Measurements for DESIGN 5.18 (HIP events on a stream of the tool's own, warmed up, the forms alternating inside one loop, medians and the
spread): mcrt_convolve_bands_frames at F = 20, E = 128, R = 465, B = 3, n_ax 7, n_lat 13 beside three calls of mcrt_convolve_frames on three
copies of the stack (alone, and with the three device-to-device copies that make them), and mcrt_band_fold_frames beside mcrt_elevation_frames
at K = 3.  Appends rows `tag,what,median_us,min_us,p90_us,n` to the csv given as the second argument (default out/bands_measure.csv); the tag
names the build (MCRT_LIB picks a variant library: make variant NAME=strip8 DEFS=-DMCRT_BANDS_STRIP=8)."""
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
    path = sys.argv[2] if len(sys.argv) > 2 else "out/bands_measure.csv"
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

    F, E, R, B, n_ax, n_lat = 20, 128, 465, 3, 7, 13
    n = F * E * R
    psf = m.Psf(bands=(3.5, 4.5, 5.5))
    ax_rows, w_rows = psf.axial_rows(R, 0.322), psf.band_weights(R, 0.322)
    axs = [np.ascontiguousarray(ax_rows[b, 0]) for b in range(B)]
    rf = ctx.alloc(n * 4); bands = ctx.alloc(B * n * 4); copies = ctx.alloc(B * n * 4); folded = ctx.alloc(n * 4)
    ctx.h2d(rf, np.random.default_rng(1).standard_normal(n).astype(np.float32))
    ctx.synchronize()

    def three_copies():
        for b in range(B):
            chk(hip.hipMemcpyAsync(vp(copies + 4 * n * b), vp(rf), n * 4, 3, st))

    def three_plain():
        for b in range(B):
            ctx.convolve_frames(copies + 4 * n * b, F, E, R, axs[b], psf.lateral_kernel)

    def copies_and_plain():
        three_copies(); three_plain()

    rows = alternate({"convolve_bands_frames B=3": lambda: ctx.convolve_bands_frames(rf, F, E, R, ax_rows, bands, lateral=psf.lateral_kernel),
                      "3 x convolve_frames": three_plain,
                      "3 x d2d copy + 3 x convolve_frames": copies_and_plain})
    rows.update(alternate({"band_fold_frames B=3": lambda: ctx.band_fold_frames(bands, F, B, E, R, w_rows, folded),
                           "elevation_frames K=3": lambda: ctx.elevation_frames(bands, F, B, E, R, w_rows, folded)}))
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    new = not os.path.exists(path)
    with open(path, "a") as f:
        if new:
            f.write("tag,what,median_us,min_us,p90_us,n\n")
        for k, (med, lo, p90, cnt) in rows.items():
            line = "%s,%s,%.2f,%.2f,%.2f,%d" % (tag, k, med, lo, p90, cnt)
            print(line)
            f.write(line + "\n")
    for d in (rf, bands, copies, folded):
        ctx.free(d)
    ctx.close()


main()
