"""Measurements for DESIGN 5.11: mcrt_speckle_frames with k_srad fusing 2 and 4 iterations per launch (a context each, MCRT_SPECKLE_FUSE
under MCRT_TUNING=1, read when a context is made; SPECKLE_FORMS=1,2,4 adds the un-fused form of tools/variants/srad_unfused.patch, which
the archived run was made with) -- at n_iter = 20 on 128 x 1024 and 512 x 465 frames, F = 1 and F = 20,
out of place and in place, beside two yardsticks in the same process: a device-to-device copy of the same stack (the traffic floor of ONE
un-fused iteration: 8 bytes per pixel) and mcrt_convolve_frames on it (7 axial and 13 lateral taps, the two-pass stencil users already pay for):

    python tools/speckle_measure.py profiles/speckle/measure.csv

Device events on the stream every context enqueues on; 2 warm-up calls, then 7 timed rounds in which the forms and the yardsticks
alternate.  A timed sample is a BATCH of back-to-back calls between two events (16 at F = 1, 4 at F = 20); the figures are per call.  Per
leg: the median, the smallest and the largest time per call, the time per iteration and frame, and the ratio of that to the copy's
time per frame."""
import os
import sys
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(128, 1024), (512, 465)]
FRAMES = (1, 20)
N_ITER = 20
FUSE = tuple(int(t) for t in os.environ.get("SPECKLE_FORMS", "2,4").split(","))
WARM, ROUNDS = 2, 7


def timed(torch, stream, calls, batch):
    """calls: name -> function; WARM calls of each, then ROUNDS rounds in which they alternate, `batch` calls per sample -> name -> ms per
    call of every round"""
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
                for _ in range(batch):
                    fn()
                b.record(stream)
                b.synchronize()
                ms[name].append(a.elapsed_time(b) / batch)
    return ms


def main(out_csv):
    import torch
    import mcray_tracing_amd as m
    os.environ["MCRT_TUNING"] = "1"
    ctxs = {}
    for t in FUSE:
        os.environ["MCRT_SPECKLE_FUSE"] = str(t)
        ctxs["k_srad<%d>" % t] = m.Context(0)
    stream = torch.cuda.Stream()
    for c in ctxs.values():
        c.set_stream(stream.cuda_stream)
    any_ctx = next(iter(ctxs.values()))
    psf = m.Psf()
    rng = np.random.default_rng(1)
    rows = []
    for H, W in SHAPES:
        for F in FRAMES:
            n = F * H * W
            x = rng.rayleigh(1.0, n).astype(np.float32)
            src = torch.from_numpy(x).cuda(); dst = torch.empty_like(src); work = src.clone(); conv = src.clone()
            calls = {"copy (device to device)": lambda: dst.copy_(src),
                     "mcrt_convolve_frames 7 x 13": lambda: any_ctx.convolve_frames(conv.data_ptr(), F, H, W, psf.axial_kernel, psf.lateral_kernel)}
            for name, c in ctxs.items():
                calls[name + " out of place"] = lambda c=c: c.speckle_frames(src.data_ptr(), F, H, W, dst.data_ptr(), n_iter=N_ITER)
                calls[name + " in place"] = lambda c=c: c.speckle_frames(work.data_ptr(), F, H, W, n_iter=N_ITER)
            ms = timed(torch, stream, calls, 16 if F == 1 else 4)
            copy_per_frame = float(np.median(ms["copy (device to device)"])) / F
            for name, t in ms.items():
                med = float(np.median(t))
                iters = N_ITER if name.startswith("k_srad") else 1
                per = med / iters / F
                rows.append(("%d x %d" % (H, W), name, F, med, min(t), max(t), per, per / copy_per_frame))
                print("%-10s F=%-3d %-34s %9.4f ms (%.4f .. %.4f)  %9.5f ms/iteration/frame  %6.2f x copy" % (rows[-1][0], F, name, med, min(t), max(t), per, per / copy_per_frame))
            del src, dst, work, conv
    os.makedirs(os.path.dirname(os.path.abspath(out_csv)), exist_ok=True)
    with open(out_csv, "w") as f:
        f.write("frame,leg,frames,median_ms,min_ms,max_ms,ms_per_iteration_per_frame,ratio_to_copy\n")
        for r in rows:
            f.write("%s,%s,%d,%.5f,%.5f,%.5f,%.6f,%.3f\n" % r)
    for c in ctxs.values():
        c.synchronize()
        c.close()


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "profiles/speckle/measure.csv")
