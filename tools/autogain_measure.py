"""Measurements for DESIGN 5.17: mcrt_autogain_frames -- estimate only (a clear, k_autogain_hist, k_autogain_curve) and the whole call (with
k_autogain_apply), with one LDS histogram per workgroup of k_autogain_hist (the default) and with four interleaved ones
(MCRT_AUTOGAIN_COPIES=4, a context each) -- on enveloped stacks of F = 20 and F = 128 frames of 512 x 465 with bands of 16 rows, beside yardsticks in the same process:
a device-to-device copy of the same stack, and mcrt_noise_frames in its two modes, whose difference is a clear and k_bmode_peak, the kernel
that reads the bytes k_autogain_hist reads:

    python tools/autogain_measure.py profiles/autogain/measure.csv

Device events on the stream the contexts enqueue on; 2 warm-up calls, then 7 timed rounds in which the legs alternate.  A timed sample is
a batch of 16 back-to-back calls between two events; the figures are per call: the median, the smallest and the largest, the time per
sample and the ratios to the copy and to the peak.  A second argument (20 or 128) keeps that stack alone: the kernels' own times come
from such runs under rocprofv3 --kernel-trace --stats."""
import os
import sys
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STACKS = [(20, 512, 465), (128, 512, 465)]
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


def main(out_csv, only_frames=None):
    import torch
    import mcray_tracing_amd as m
    os.environ["MCRT_TUNING"] = "1"
    stream = torch.cuda.Stream()
    ctxs = {}
    for copies in (1, 4):
        os.environ["MCRT_AUTOGAIN_COPIES"] = str(copies)
        ctxs[copies] = m.Context(0)
        ctxs[copies].set_stream(stream.cuda_stream)
    os.environ.pop("MCRT_AUTOGAIN_COPIES")
    rng = np.random.default_rng(1)
    rows = []
    for F, E, R in STACKS:
        if only_frames is not None and F != only_frames:
            continue
        n = F * E * R
        decay = np.exp(-np.arange(R) / 60.0).astype(np.float32)
        x = (rng.rayleigh(1.0, (F * E, R)).astype(np.float32) * decay + rng.rayleigh(0.002, (F * E, R)).astype(np.float32)).reshape(-1)
        src = torch.from_numpy(x).cuda(); dst = torch.empty_like(src); work = src.clone(); noisy = src.clone()
        floor = torch.full((F,), 0.002, dtype=torch.float32).cuda()
        gain = torch.empty(F * R, dtype=torch.float32).cuda()
        calls = {"copy (device to device)": lambda: dst.copy_(src),
                 "mcrt_noise_frames SNR_DB": lambda: ctxs[1].noise_frames(noisy.data_ptr(), F, 1, E, R, snr_db=50.0),
                 "mcrt_noise_frames ABS": lambda: ctxs[1].noise_frames(noisy.data_ptr(), F, 1, E, R, sigma=0.01)}
        for copies in (1, 4):
            c = ctxs[copies]
            calls["mcrt_autogain_frames estimate only (%d LDS histograms)" % copies] = \
                lambda c=c: c.autogain_frames(src.data_ptr(), F, 1, E, R, floor_dev=floor.data_ptr(), gain_dev=gain.data_ptr(), apply=False)
            calls["mcrt_autogain_frames (%d LDS histograms)" % copies] = \
                lambda c=c: c.autogain_frames(work.data_ptr(), F, 1, E, R, floor_dev=floor.data_ptr(), gain_dev=gain.data_ptr())
        ms = timed(torch, stream, calls)
        copy = float(np.median(ms["copy (device to device)"]))
        peak = float(np.median(ms["mcrt_noise_frames SNR_DB"])) - float(np.median(ms["mcrt_noise_frames ABS"]))
        for name, t in ms.items():
            med = float(np.median(t))
            rows.append(("%d x %d x %d" % (F, E, R), name, med, min(t), max(t), med * 1e6 / n, med / copy, med / peak))
            print("%-16s %-58s %9.4f ms (%.4f .. %.4f)  %8.4f ns/sample  %6.2f x copy  %6.2f x peak" % rows[-1])
        rows.append(("%d x %d x %d" % (F, E, R), "a clear and k_bmode_peak (SNR_DB minus ABS)", peak, float("nan"), float("nan"), peak * 1e6 / n, peak / copy, 1.0))
        print("%-16s %-58s %9.4f ms" % rows[-1][:3])
        del src, dst, work, noisy
    os.makedirs(os.path.dirname(os.path.abspath(out_csv)), exist_ok=True)
    with open(out_csv, "w") as f:
        f.write("stack,leg,median_ms,min_ms,max_ms,ns_per_sample,ratio_to_copy,ratio_to_peak\n")
        for r in rows:
            f.write("%s,%s,%.5f,%.5f,%.5f,%.5f,%.3f,%.3f\n" % r)
    for c in ctxs.values():
        c.synchronize()
        c.close()


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "profiles/autogain/measure.csv", int(sys.argv[2]) if len(sys.argv) > 2 else None)
