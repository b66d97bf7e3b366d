"""Measurements for DESIGN 5.21 (HIP events on a stream of the tool's own, warmed up, the forms alternating inside one loop, medians and the
spread): mcrt_spectral_series_frames (k_gate_series) at sigma 0 and > 0, mcrt_spectral_frames (k_spectrum<N>) with both outputs and
mcrt_sonogram_frames (k_sonogram_peak + k_sonogram) with the automatic reference, at 1 gate x 2048 pulses x N = 128, 64 gates x 4096 pulses
x N = 256 and 512 gates x 2048 pulses x N = 128, hop 32 and gates of 8 rows throughout, beside a device-to-device copy of the spectra the
call writes (and reads).  Appends rows `tag,what,median_us,min_us,p90_us,n` to the csv given as the second argument (default
out/spectral_measure.csv); the tag names the build."""
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
    path = sys.argv[2] if len(sys.argv) > 2 else "out/spectral_measure.csv"
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

    rows = {}
    rng = np.random.default_rng(1)
    v_nyq = m.host_flow_nyquist(4.5)
    F, E, R, G = 1, 128, 465, 8
    n = F * E * R
    iq = ctx.alloc(16 * n)
    ctx.h2d(iq, rng.standard_normal(4 * n).astype(np.float32))
    for n_gates, T, N in ((1, 2048, 128), (64, 4096, 256), (512, 2048, 128)):
        hop = 32
        cols = (T - N) // hop + 1
        gates = np.stack([np.zeros(n_gates), rng.integers(0, E, n_gates), rng.integers(0, R - G + 1, n_gates)], axis=1).astype(np.uint32)
        frac = m.host_spectral_profile(np.ones(R, np.uint8), R // 2 - G // 2, G, [0, 1], 2.0)
        rate = np.tile(m.host_spectral_rates(frac, 0.8), (n_gates, 1))
        phase = m.host_spectral_phase(v_nyq, m.host_pulse_waveform(4000.0, 72.0, 250.0, 40.0, T))
        weight = np.ones(G, np.float32)
        series, power, mean, grey, sink = ctx.alloc(8 * n_gates * T), ctx.alloc(4 * n_gates * cols * N), ctx.alloc(4 * n_gates * cols), ctx.alloc(n_gates * cols * N), \
            ctx.alloc(8 * n_gates * cols * N)
        quiet = m.spectral_opts_struct(n_pulses=T, gate_rows=G, n_fft=N, hop=hop)
        noisy = m.spectral_opts_struct(n_pulses=T, gate_rows=G, n_fft=N, hop=hop, sigma=0.05)
        h = m.host_spectral_window("hann", N)
        shape = "%dx%dxN%d " % (n_gates, T, N)
        forms = {
            "d2d copy of the spectra": lambda: chk(hip.hipMemcpyAsync(vp(sink), vp(power), 4 * n_gates * cols * N, 3, st)),
            "spectral_series_frames sigma=0": lambda: ctx.spectral_series_frames(iq, iq + 8 * n, F, E, R, gates, weight, rate, phase, series, opts=quiet),
            "spectral_series_frames sigma=0.05": lambda: ctx.spectral_series_frames(iq, iq + 8 * n, F, E, R, gates, weight, rate, phase, series, opts=noisy),
            "spectral_frames power + mean": lambda: ctx.spectral_frames(series, n_gates, v_nyq, power_dev=power, mean_dev=mean, window=h, opts=quiet),
            "sonogram_frames": lambda: ctx.sonogram_frames(power, n_gates, cols, N, grey),
        }
        rows.update({shape + k: v for k, v in alternate(forms).items()})
        for p in (series, power, mean, grey, sink):
            ctx.free(p)
    ctx.free(iq)
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
