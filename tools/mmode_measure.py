"""Measurements for DESIGN 5.24 (HIP events on a stream of the tool's own, warmed up, the forms alternating inside one loop, medians and the
spread): mcrt_mmode_lines_frames (k_mmode_lines) with every output (17 bytes written per pulse sample: the envelope, the pair, the
displacement and the label), with the envelope alone (4 bytes) and with noise, and mcrt_mmode_picture_frames (k_mmode_peak +
k_mmode_picture; hop 4, 400 rows, the line's own peak, the two truths registered) at 1 line x 1024 pulses x 465 rows and at 8 lines x
4096 x 465 of a 1 x 64 x 465 stack, beside device-to-device copies of the bytes each call writes (the lines) or reads (the picture: the
envelopes once).  The last column is the bytes a call writes (the picture: reads) over its median.  Appends rows
`tag,what,median_us,min_us,p90_us,n,bytes,bytes_per_s` to the csv given as the second argument (default out/mmode_measure.csv); the tag
names the build."""
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
    path = sys.argv[2] if len(sys.argv) > 2 else "out/mmode_measure.csv"
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

    rows, moved = {}, {}
    rng = np.random.default_rng(1)
    F, E, R = 1, 64, 465
    n = F * E * R
    iq, tissue = ctx.alloc(8 * n), ctx.alloc(n)
    b = rng.standard_normal((F * E, R + 6, 2)); b = sum(b[:, i:i + R] for i in range(7)) / 7.0
    z = (b[..., 0] + 1j * b[..., 1]) * np.exp(2j * np.pi * CARRIER * np.arange(R))
    ctx.h2d(iq, np.stack([z.real, z.imag], axis=-1).astype(np.float32))
    labels = np.zeros((F, E, R), np.uint8); labels[:, :, 200:260] = 1                          # a lumen of 60 rows under every scan-line
    ctx.h2d(tissue, labels)
    dil = m.host_mmode_table([0.0, -0.03])
    for n_lines, T in ((1, 1024), (8, 4096)):
        which = [[0, 4 + 7 * j] for j in range(n_lines)]
        w, bulk = m.host_mmode_waveform(1000.0, 72.0, T), m.host_mmode_bulk(1000.0, 15.0, 1.5, T)
        s = n_lines * T * R
        hop, H = 4, 400
        px = n_lines * H * (T // hop)
        env, pair, disp, lab, sink = ctx.alloc(4 * s), ctx.alloc(8 * s), ctx.alloc(4 * s), ctx.alloc(s), ctx.alloc(17 * s)
        pic, lab_pic, disp_pic = ctx.alloc(px), ctx.alloc(px), ctx.alloc(4 * px)
        shape = "%dx%dx%d " % (n_lines, T, R)
        call = lambda sigma=0.0, **outs: ctx.mmode_lines_frames(iq, tissue, F, E, R, which, dil, w, bulk, CARRIER, sigma=sigma, **outs)
        forms = {"d2d copy of 17 B per sample": lambda: chk(hip.hipMemcpyAsync(vp(sink), vp(pair), 8 * s, 3, st)) or chk(hip.hipMemcpyAsync(vp(sink + 8 * s), vp(env), 4 * s, 3, st))
                 or chk(hip.hipMemcpyAsync(vp(sink + 12 * s), vp(disp), 4 * s, 3, st)) or chk(hip.hipMemcpyAsync(vp(sink + 16 * s), vp(lab), s, 3, st)),
                 "d2d copy of 4 B per sample": lambda: chk(hip.hipMemcpyAsync(vp(sink), vp(env), 4 * s, 3, st)),
                 "mmode_lines_frames every output": lambda: call(env_dev=env, iq_out_dev=pair, truth_disp_dev=disp, truth_label_dev=lab),
                 "mmode_lines_frames every output sigma=0.05": lambda: call(0.05, env_dev=env, iq_out_dev=pair, truth_disp_dev=disp, truth_label_dev=lab),
                 "mmode_lines_frames env alone": lambda: call(env_dev=env),
                 "mmode_lines_frames the truths alone": lambda: call(truth_disp_dev=disp, truth_label_dev=lab)}
        forms["mmode_lines_frames every output"]()                       # the display reads a real sweep
        forms["mmode_picture_frames hop=4 H=400 with the truths"] = lambda: ctx.mmode_picture_frames(env, n_lines, T, R, pic, truth_label_dev=lab, truth_disp_dev=disp,
                                                                                                      label_out_dev=lab_pic, disp_out_dev=disp_pic, hop=hop, height=H)
        forms["mmode_picture_frames hop=4 H=400 ref=1"] = lambda: ctx.mmode_picture_frames(env, n_lines, T, R, pic, hop=hop, height=H, ref=1.0)
        for k, bytes_ in (("d2d copy of 17 B per sample", 17 * s), ("d2d copy of 4 B per sample", 4 * s), ("mmode_lines_frames every output", 17 * s),
                          ("mmode_lines_frames every output sigma=0.05", 17 * s), ("mmode_lines_frames env alone", 4 * s), ("mmode_lines_frames the truths alone", 5 * s),
                          ("mmode_picture_frames hop=4 H=400 with the truths", 8 * s), ("mmode_picture_frames hop=4 H=400 ref=1", 4 * s)):
            moved[shape + k] = bytes_                                    # (the picture with its own peak reads the envelopes twice)
        rows.update({shape + k: v for k, v in alternate(forms, n=100 if n_lines == 1 else 30).items()})
        for p in (env, pair, disp, lab, sink, pic, lab_pic, disp_pic):
            ctx.free(p)
    ctx.free(iq); ctx.free(tissue)
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    new = not os.path.exists(path)
    with open(path, "a") as f:
        if new:
            f.write("tag,what,median_us,min_us,p90_us,n,bytes,bytes_per_s\n")
        for k, (med, lo, p90, cnt) in rows.items():
            line = "%s,%s,%.2f,%.2f,%.2f,%d,%d,%.3e" % (tag, k, med, lo, p90, cnt, moved[k], moved[k] / (med * 1e-6))
            print(line)
            f.write(line + "\n")
    ctx.close()


main()
