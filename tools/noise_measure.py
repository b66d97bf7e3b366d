"""Measurements for DESIGN 5.14: mcrt_noise_frames -- MCRT_NOISE_SNR_DB (a clear, k_bmode_peak, k_noise), MCRT_NOISE_ABS (k_noise alone) and
MCRT_NOISE_ABS with a gain table -- on an RF stack of F = 20 frames of 128 x 465 and of one frame of 512 x 465, beside two yardsticks in the
same process: a device-to-device copy of the same stack (the stage's traffic: 8 bytes per sample) and mcrt_convolve_frames on it (7 axial
and 13 lateral taps: the stage before it):

    python tools/noise_measure.py profiles/noise/measure.csv

Device events on the stream the context enqueues on; 2 warm-up calls, then 7 timed rounds in which the legs alternate.  A timed sample is
a batch of 16 back-to-back calls between two events; the figures are per call: the median, the smallest and the largest, the time per
sample and the ratio to the copy."""
import os
import sys
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STACKS = [(20, 128, 465), (1, 512, 465)]
WARM, ROUNDS, BATCH = 2, 7, 16


def timed(torch, stream, calls):
    """calls: name -> function; WARM calls of each, then ROUNDS rounds in which they alternate, BATCH calls per sample -> name -> ms per call"""
    with torch.cuda.stream(stream):
        for _ in range(WARM):
            for fn in calls.values():
                fn()
        stream.synchronize()
        ms = {name: [] for name in calls}
        for _ in range(ROUNDS):
            for name, fn in calls.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                for _ in range(BATCH):
                    fn()
                b.record(stream)
                b.synchronize()
                ms[name].append(a.elapsed_time(b) / BATCH)
    return ms


def main(out_csv):
    import torch
    import mcray_tracing_amd as m
    ctx = m.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    psf = m.Psf()
    rng = np.random.default_rng(1)
    rows = []
    for F, E, R in STACKS:
        n = F * E * R
        x = (rng.rayleigh(1.0, n) * np.where(rng.random(n) < 0.5, -1.0, 1.0)).astype(np.float32)
        src = torch.from_numpy(x).cuda(); dst = torch.empty_like(src); work = src.clone(); conv = src.clone()
        gain = np.ones(E, np.float32); gain[E // 2] = 0.0
        calls = {"copy (device to device)": lambda: dst.copy_(src),
                 "mcrt_convolve_frames 7 x 13": lambda: ctx.convolve_frames(conv.data_ptr(), F, E, R, psf.axial_kernel, psf.lateral_kernel),
                 "mcrt_noise_frames SNR_DB": lambda: ctx.noise_frames(work.data_ptr(), F, 1, E, R, snr_db=50.0),
                 "mcrt_noise_frames ABS": lambda: ctx.noise_frames(work.data_ptr(), F, 1, E, R, sigma=0.01),
                 "mcrt_noise_frames ABS + gain": lambda: ctx.noise_frames(work.data_ptr(), F, 1, E, R, sigma=0.01, element_gain=gain)}
        ms = timed(torch, stream, calls)
        copy = float(np.median(ms["copy (device to device)"]))
        for name, t in ms.items():
            med = float(np.median(t))
            rows.append(("%d x %d x %d" % (F, E, R), name, med, min(t), max(t), med * 1e6 / n, med / copy))
            print("%-14s %-30s %9.4f ms (%.4f .. %.4f)  %8.4f ns/sample  %6.2f x copy" % rows[-1])
        del src, dst, work, conv
    os.makedirs(os.path.dirname(os.path.abspath(out_csv)), exist_ok=True)
    with open(out_csv, "w") as f:
        f.write("stack,leg,median_ms,min_ms,max_ms,ns_per_sample,ratio_to_copy\n")
        for r in rows:
            f.write("%s,%s,%.5f,%.5f,%.5f,%.5f,%.3f\n" % r)
    ctx.synchronize()
    ctx.close()


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "profiles/noise/measure.csv")
