"""Measurements for DESIGN 5.10: k_render in both tile shapes -- a wavefront owning an 8 x 8 tile of the picture, or 64 pixels of one row --
beside k_volume writing a 400 x 500 C-plane at F = 20 in the same process.  A 160 x 200 x 96 block (random voxels; floats and bytes) rendered
to a 500 x 400 picture in the three modes, along w, along u and obliquely, at F = 1 and F = 20:

    python tools/render_measure.py profiles/render/measure.csv

Device events on the stream both contexts enqueue on; 2 warm-up calls, then 7 timed rounds in which the two tile shapes alternate (the
shape is a context's knob, MCRT_RENDER_ROW_TILE under MCRT_TUNING=1, read when the context is made).  A timed sample is a BATCH of
back-to-back calls between two events, long enough (milliseconds) that the events and the launches are a small part of it: 64 calls of the
yardstick, 16 of a one-picture render, 2 of a 20-picture render; the figures are per call.  Per leg: the median, the smallest and
the largest time per call, the time per picture, and taps per second -- 8 taps per covered step, the covered steps counted on the host
from the view alone (steps outside the block read nothing).  The yardstick issues 8 taps per point of its C-plane."""
import os
import sys
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NU, NV, NW = 160, 200, 96
NX, NY = 500, 400
E, R, K, STEP, PIVOT = 128, 465, 32, 0.02, 10.0          # the yardstick's stack: tools/volume_measure.py's
WARM, ROUNDS = 2, 7
DIRECTIONS = [("along w", (0.0, 0.0, 1.0)), ("along u", (1.0, 0.0, 0.0)), ("oblique", (0.5, 0.3, 0.8))]
UP = (0.0, 1.0, 0.0)


def covered_steps(view):
    """the covered (pixel, step) pairs of a view on the block, from the contract's float expressions"""
    f32 = np.float32
    o, di, dj, ds = (np.array(list(v), f32) for v in (view.origin, view.di, view.dj, view.ds))
    i = np.arange(view.nx, dtype=f32)[None, :]; j = np.arange(view.ny, dtype=f32)[:, None]
    base = [((o[c] + i * di[c]).astype(f32) + j * dj[c]).astype(f32) for c in range(3)]
    total = 0
    for s in range(view.n_steps):
        ok = np.ones((view.ny, view.nx), bool)
        for c, n in enumerate((NU, NV, NW)):
            f = np.floor((base[c] + f32(f32(s) * ds[c])).astype(f32))
            ok &= (f >= -1) & (f < n)
        total += int(ok.sum())
    return total


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
    for name, knob in (("tile 8x8", "0"), ("row 64x1", "1")):
        os.environ["MCRT_RENDER_ROW_TILE"] = knob
        ctxs[name] = m.Context(0)
    stream = torch.cuda.Stream()
    for c in ctxs.values():
        c.set_stream(stream.cuda_stream)
    any_ctx = ctxs["tile 8x8"]
    rng = np.random.default_rng(1)
    g = m.volume_grid((-23.85, 60.0, -14.25), (0.3, 0, 0), (0, 0.4, 0), (0, 0, 0.3), NU, NV, NW)
    nvox, npix = NU * NV * NW, NX * NY
    F_MAX = 20
    vol_f = any_ctx.alloc(F_MAX * nvox * 4); vol_b = any_ctx.alloc(F_MAX * nvox)
    for f in range(F_MAX):
        any_ctx.h2d(vol_f + f * nvox * 4, rng.random(nvox, dtype=np.float32)); any_ctx.h2d(vol_b + f * nvox, rng.integers(0, 256, nvox, dtype=np.uint8))
    out = any_ctx.alloc(F_MAX * npix * 4); out8 = any_ctx.alloc(F_MAX * npix)
    rows = []

    def record(leg, name, F, taps, ms):
        med = float(np.median(ms))
        rows.append((leg, name, F, med, min(ms), max(ms), med / F, taps / (med * 1e-3)))
        print("%-44s %-9s F=%-3d %9.3f ms (%.3f .. %.3f)  %8.3f ms/picture  %8.1f G taps/s" % (leg, name, F, med, min(ms), max(ms), med / F, taps / (med * 1e-3) / 1e9))

    # the yardstick: a 400 x 500 C-plane at F = 20 from a stack of K planes
    cut = m.cplane_grid(90.0, 500, 400, 0.1)
    src = any_ctx.alloc(20 * K * E * R * 4)
    any_ctx.h2d(src, np.abs(rng.standard_normal(20 * K * E * R)).astype(np.float32))
    sweep = (K, STEP, PIVOT)
    ms = timed(torch, stream, {"k_volume<false>": lambda: any_ctx.volume_frames(src, 20, E, R, sweep, cut, out),
                               "k_bmode_grey + k_volume<true>": lambda: any_ctx.bmode_volume_frames(src, 20, E, R, sweep, cut, out8, ref=1.0)}, 64)
    for name, t in ms.items():
        record("C-plane 400 x 500 (yardstick)", name, 20, 20 * npix * 8, t)
    any_ctx.free(src)

    import math
    diag = math.sqrt((0.3 * (NU - 1)) ** 2 + (0.4 * (NV - 1)) ** 2 + (0.3 * (NW - 1)) ** 2)
    for dname, d in DIRECTIONS:
        view = m.render_view(g, d, UP, diag / NX, 0.3, NX, NY)
        pairs = covered_steps(view)
        print("%s: %d steps, %.3f of the (pixel, step) pairs covered" % (dname, view.n_steps, pairs / (npix * view.n_steps)))
        for in_u8, vol in ((False, vol_f), (True, vol_b)):
            for mode in ("mip", "mean", "surface"):
                for F in (1, 20):
                    calls = {name: (lambda c=c: c.render_frames(vol, F, (NW, NV, NU), view, out_dev=None if in_u8 else out, out8_dev=out8 if in_u8 else None,
                                                                in_u8=in_u8, mode=mode)) for name, c in ctxs.items()}
                    for name, t in timed(torch, stream, calls, 16 if F == 1 else 2).items():
                        record("render %s %s %s" % (dname, "uint8" if in_u8 else "float", mode), name, F, F * pairs * 8, t)
    os.makedirs(os.path.dirname(os.path.abspath(out_csv)), exist_ok=True)
    with open(out_csv, "w") as f:
        f.write("leg,variant,frames,median_ms,min_ms,max_ms,ms_per_picture,taps_per_s\n")
        for r in rows:
            f.write("%s,%s,%d,%.4f,%.4f,%.4f,%.4f,%.4g\n" % r)
    for c in ctxs.values():
        c.synchronize()
    for p in (vol_f, vol_b, out, out8):
        any_ctx.free(p)
    for c in ctxs.values():
        c.close()


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "profiles/render/measure.csv")
