"""Measurements for DESIGN 5.23 (HIP events on a stream of the tool's own, warmed up, the forms alternating inside one loop, medians and the
spread): mcrt_shear_wave_frames (k_shear_arrival + k_shear_track) with the peak and the truths at T = 64 and T = 256 pulses, at sigma 0
and > 0 and with the truths alone (the arrival kernel on its own), and mcrt_shear_speed_frames (k_shear_speed) with every output at
the default fit (4 lines, +- 2 rows) and at the largest (16, 16), at F x E x R = 1 x 512 x 465, beside device-to-device copies of the
bytes the calls move at least once (the wave: the pairs and the labels in, four maps out, 25 bytes per sample; the speed: one map in,
three out, 16 bytes).  The tracker's rows carry its complex multiply-adds per second: samples x T x (2 a + 1) over the median (the
clipped windows at a line's ends count as whole, the arrival kernel's time is inside).  Appends rows
`tag,what,median_us,min_us,p90_us,n,cmadd_per_s` to the csv given as the second argument (default out/shear_measure.csv); the tag names
the build."""
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
    path = sys.argv[2] if len(sys.argv) > 2 else "out/shear_measure.csv"
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
    F, E, R, a = 1, 512, 465, 8
    n = F * E * R
    iq, tissue, maps, sink, times = ctx.alloc(8 * n), ctx.alloc(n), ctx.alloc(16 * n), ctx.alloc(25 * n), ctx.alloc(4 * n)
    b = rng.standard_normal((F * E, R + 6, 2)); b = sum(b[:, i:i + R] for i in range(7)) / 7.0
    z = (b[..., 0] + 1j * b[..., 1]) * np.exp(2j * np.pi * CARRIER * np.arange(R))
    ctx.h2d(iq, np.stack([z.real, z.imag], axis=-1).astype(np.float32))
    labels = np.zeros((F, E, R), np.uint8); labels[:, 300:340, R // 3:R // 2] = 1              # an inclusion at twice the speed
    ctx.h2d(tissue, labels)
    slow, spf = m.host_shear_table([2.0, 4.0], 10000.0)
    pitch_q8, pitch_mm = m.host_shear_pitch(E, R, 30.0, 1.0471975511965976)
    tab = dict(slow_q16=slow, speed_f=spf, pitch_q8=pitch_q8, shape_q16=m.host_shear_shape(12), amp_q16=m.host_shear_decay(E, 8.0))
    pt, pd, ta, ts = maps, maps + 4 * n, maps + 8 * n, maps + 12 * n
    shape = "%dx%dx%d " % (F, E, R)
    forms = {"d2d copy of 25 B per sample": lambda: chk(hip.hipMemcpyAsync(vp(sink), vp(iq), 8 * n, 3, st)) or chk(hip.hipMemcpyAsync(vp(sink + 8 * n), vp(tissue), n, 3, st))
             or chk(hip.hipMemcpyAsync(vp(sink + 9 * n), vp(maps), 16 * n, 3, st)),
             "d2d copy of 16 B per sample": lambda: chk(hip.hipMemcpyAsync(vp(sink), vp(maps), 4 * n, 3, st)) or chk(hip.hipMemcpyAsync(vp(sink + 4 * n), vp(maps + 4 * n), 12 * n, 3, st))}
    for T in (64, 256):
        for sigma in (0.0, 0.05):
            o = m.shear_opts_struct(n_pulses=T, window_rows=a, push_line=E // 2, sigma=sigma)
            name = "shear_wave_frames T=%d a=%d sigma=%g peak and truths" % (T, a, sigma)
            forms[name] = lambda o=o: ctx.shear_wave_frames(iq, tissue, F, E, R, cycles_per_row=CARRIER, peak_time_dev=pt, peak_disp_dev=pd, truth_arrival_dev=ta,
                                                            truth_speed_dev=ts, opts=o, **tab)
            work[shape + name] = n * T * (2 * a + 1)
    o = m.shear_opts_struct(n_pulses=64, push_line=E // 2)
    forms["shear_wave_frames the truths alone"] = lambda o=o: ctx.shear_wave_frames(iq, tissue, F, E, R, cycles_per_row=CARRIER, truth_arrival_dev=ta, truth_speed_dev=ts, opts=o, **tab)
    # the speed call reads the peak times of a real wave, written once here
    ctx.shear_wave_frames(iq, tissue, F, E, R, cycles_per_row=CARRIER, peak_time_dev=times, opts=o, **tab)
    ctx.synchronize()
    for lines, avg in ((4, 2), (16, 16)):
        o2 = m.shear_opts_struct(push_line=E // 2, speed_lines=lines, avg_rows=avg)
        forms["shear_speed_frames (%d, %d) all outputs" % (lines, avg)] = lambda o2=o2: ctx.shear_speed_frames(times, F, E, R, pitch_mm, speed_dev=maps, modulus_dev=maps + 4 * n,
                                                                                                       quality_dev=maps + 8 * n, opts=o2)
    rows.update({shape + k: v for k, v in alternate(forms).items()})
    for p in (iq, tissue, maps, sink, times):
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
