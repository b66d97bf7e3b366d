"""Measurements for DESIGN 5.19 (HIP events on a stream of the tool's own, warmed up, the forms alternating inside one loop, medians and the
spread): mcrt_detect_frames at 31 taps -- in place, out of place, with the I/Q output, and at 3 and 63 taps -- beside mcrt_envelope_frames at
F = 20, E = 128, R = 465 and at F = 1, E = 512, R = 465, on Gaussian RF convolved with the pulse (every form restores its input first:
a device-to-device copy that is timed on its own and is part of every row).  Appends rows `tag,what,median_us,min_us,p90_us,n` to the csv
given as the second argument (default out/detect_measure.csv); the tag names the build (MCRT_LIB picks a variant library: make variant
NAME=waves1 DEFS=-DMCRT_DETECT_WAVES=1u).  Then the aliasing table: a tone cos(2 pi f r + 0.3) of constant amplitude 1, R = 465, 4 scan-lines, under both
detectors on the device -- the largest deviation from 1 of mcrt_envelope_frames over the rows 20 .. 445 and of mcrt_detect_frames over the
interior rows -- printed, and appended to the third argument (default out/detect_tone.csv)."""
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
    path = sys.argv[2] if len(sys.argv) > 2 else "out/detect_measure.csv"
    tone_path = sys.argv[3] if len(sys.argv) > 3 else "out/detect_tone.csv"
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
    ax, lat = m.host_psf()
    for F, E, R in ((20, 128, 465), (1, 512, 465)):
        n = F * E * R
        src, work, env, iq = ctx.alloc(n * 4), ctx.alloc(n * 4), ctx.alloc(n * 4), ctx.alloc(n * 8)
        ctx.h2d(src, np.random.default_rng(1).standard_normal(n).astype(np.float32))
        ctx.convolve_frames(src, F, E, R, ax, lat)
        ctx.synchronize()
        restore = lambda: chk(hip.hipMemcpyAsync(vp(work), vp(src), n * 4, 3, st))
        shape = "%dx%dx%d " % (F, E, R)

        def form(fn):
            return lambda: (restore(), fn())

        rows.update({shape + k: v for k, v in alternate({
            "d2d copy alone": restore,
            "copy + envelope_frames": form(lambda: ctx.envelope_frames(work, F, E, R)),
            "copy + detect_frames 31 in place": form(lambda: ctx.detect_frames(work, F, E, R, env_dev=work, n_taps=31)),
            "copy + detect_frames 31 out of place": form(lambda: ctx.detect_frames(work, F, E, R, env_dev=env, n_taps=31)),
            "copy + detect_frames 31 iq alone": form(lambda: ctx.detect_frames(work, F, E, R, iq_dev=iq, n_taps=31)),
            "copy + detect_frames 31 env + iq": form(lambda: ctx.detect_frames(work, F, E, R, env_dev=env, iq_dev=iq, n_taps=31)),
            "copy + detect_frames 3 in place": form(lambda: ctx.detect_frames(work, F, E, R, env_dev=work, n_taps=3)),
            "copy + detect_frames 63 in place": form(lambda: ctx.detect_frames(work, F, E, R, env_dev=work, n_taps=63)),
        }).items()})
        for d in (src, work, env, iq):
            ctx.free(d)
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    new = not os.path.exists(path)
    with open(path, "a") as f:
        if new:
            f.write("tag,what,median_us,min_us,p90_us,n\n")
        for k, (med, lo, p90, cnt) in rows.items():
            line = "%s,%s,%.2f,%.2f,%.2f,%d" % (tag, k, med, lo, p90, cnt)
            print(line)
            f.write(line + "\n")

    # the aliasing table
    R, lines = 465, 4
    a, b = ctx.alloc(lines * R * 4), ctx.alloc(lines * R * 4)
    os.makedirs(os.path.dirname(tone_path) or ".", exist_ok=True)
    new = not os.path.exists(tone_path)
    with open(tone_path, "a") as f:
        if new:
            f.write("tag,cycles_per_row,envelope_frames_max_dev,detect_31_max_dev,detect_31_gain,detect_15_max_dev,detect_15_gain\n")
        for cyc in (0.3475, 0.2025, 0.10, 0.45, 0.4925):
            x = np.tile(np.cos(2.0 * np.pi * cyc * np.arange(R) + 0.3).astype(np.float32), (lines, 1))
            ctx.h2d(a, x)
            ctx.envelope_frames(a, 1, lines, R)
            ref = np.abs(ctx.d2h(a, (lines, R)).astype(np.float64)[:, 20:R - 20] - 1.0).max()
            out = [ref]
            for n_taps in (31, 15):
                M = (n_taps - 1) // 2
                ctx.h2d(b, x)
                ctx.detect_frames(b, 1, lines, R, env_dev=b, n_taps=n_taps)
                out += [np.abs(ctx.d2h(b, (lines, R)).astype(np.float64)[:, M:R - M] - 1.0).max(), m.host_detect_gain(m.host_detect_taps(n_taps), cyc)]
            line = "%s,%.4f,%.4f,%.5f,%.5f,%.5f,%.5f" % ((tag, cyc) + tuple(out))
            print(line)
            f.write(line + "\n")
    ctx.free(a); ctx.free(b)
    ctx.close()


main()
