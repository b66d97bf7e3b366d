"""Measurements for DESIGN 5.16: mcrt_speckle_volume_frames (k_srad3, one iteration per launch) at n_iter = 20 on voxel blocks of 64^3, 160^3
and 256 x 256 x 128 (nu x nv x nw), out of place, beside two yardsticks in the same process: a device-to-device copy of the block (the
traffic floor of one iteration: 8 bytes per voxel) and mcrt_speckle_frames over the block as nw frames of [nv][nu] -- the slice-wise 2-D
filter, which is all a user could run over a block before:

    python tools/speckle3d_measure.py profiles/speckle3d/measure.csv

Legs: the copy; the 2-D call; the new call at weights (1, 1, 1); the new call at (1, 1, 0), which computes the 2-D call's bits.  Device
events on the stream the context enqueues on; 2 warm-up calls of every leg, then 7 timed rounds in which the legs alternate.  A timed sample
is a batch of back-to-back calls between two events (8 for the small block, 2 for the others); the figures are per call.  Per leg: the
median, the smallest and the largest time per call, the time per iteration and voxel, and the ratio of that to the copy's.  MCRT_LIB
selects a tuning build (make variant DEFS=-DSRAD3_CW=...), whose name then goes into the `build` column."""
import os
import sys
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BLOCKS = [(64, 64, 64), (160, 160, 160), (256, 256, 128)]       # (nu, nv, nw)
N_ITER = 20
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
    build = os.path.basename(os.environ.get("MCRT_LIB") or "libmcrt_hip.so")
    ctx = m.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    rng = np.random.default_rng(1)
    rows = []
    for nu, nv, nw in BLOCKS:
        n = nu * nv * nw
        shape = (nw, nv, nu)
        x = rng.rayleigh(1.0, n).astype(np.float32)
        src = torch.from_numpy(x).cuda(); dst = torch.empty_like(src)
        calls = {"copy (device to device)": lambda: dst.copy_(src),
                 "mcrt_speckle_frames, nw frames": lambda: ctx.speckle_frames(src.data_ptr(), nw, nv, nu, dst.data_ptr(), n_iter=N_ITER),
                 "mcrt_speckle_volume_frames (1, 1, 1)": lambda: ctx.speckle_volume_frames(src.data_ptr(), 1, shape, dst.data_ptr(), n_iter=N_ITER),
                 "mcrt_speckle_volume_frames (1, 1, 0)": lambda: ctx.speckle_volume_frames(src.data_ptr(), 1, shape, dst.data_ptr(), n_iter=N_ITER, weights=(1, 1, 0))}
        ms = timed(torch, stream, calls, 8 if n <= 64 ** 3 else 2)
        copy_ns = float(np.median(ms["copy (device to device)"])) * 1e6 / n
        for name, t in ms.items():
            med = float(np.median(t))
            iters = 1 if name.startswith("copy") else N_ITER
            per = med * 1e6 / iters / n                 # ns per iteration and voxel
            rows.append((build, "%d x %d x %d" % (nu, nv, nw), name, med, min(t), max(t), per, per / copy_ns))
            print("%-12s %-34s %9.4f ms (%.4f .. %.4f)  %8.5f ns/iteration/voxel  %6.2f x copy" % (rows[-1][1], name, med, min(t), max(t), per, per / copy_ns))
        del src, dst
    os.makedirs(os.path.dirname(os.path.abspath(out_csv)), exist_ok=True)
    with open(out_csv, "w") as f:
        f.write("build,block,leg,median_ms,min_ms,max_ms,ns_per_iteration_per_voxel,ratio_to_copy\n")
        for r in rows:
            f.write("%s,%s,\"%s\",%.5f,%.5f,%.5f,%.6f,%.3f\n" % r)
    ctx.synchronize()
    ctx.close()


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "profiles/speckle3d/measure.csv")
