#!/usr/bin/env python3
"""DESIGN 5.13's figures: mcrt_recon_label_frames beside mcrt_recon_frames on the same poses and grid -- 100 frames of 128 x 465 into 128^3
voxels of 1 mm, a probe swept along its elevation with a fan (tools/recon_measure.py's first case), 8 labels in layers a few millimetres
thick whose boundaries move from line to line, fill radius 1 -- and, with RECON_LABEL_VARIANT naming a library built with
tools/variants/recon_label_by_label.patch applied (a path below the repository's root), the vote table in its other layout,
[label][voxel], from that second copy of the library in the same process.  Per leg CALLS calls between two HIP events on a stream of its
own; a warm-up, then ROUNDS rounds with the legs in alternating order; median and extremes per call.  The layouts' outputs are compared in
the first round.

    python tools/recon_label_measure.py [FILE.csv]        (default profiles/recon_label/measure.csv)
"""
import csv
import ctypes as C
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["MCRT_TUNING"] = "1"
import torch  # noqa: E402
import mcray_tracing_amd as mcrt  # noqa: E402
from tools.recon_measure import poses  # noqa: E402

ROUNDS, WARM, CALLS = 7, 3, 5
CASE = dict(name="128x465_into_128^3_1mm_8_labels", F=100, E=128, R=465, n=128, pitch=1.0, step_mm=1.0, fan_deg=0.1, n_labels=8, H=1)


def tissue(c, seed=2):
    """[F][E][R] uint8: layers 10..40 rows (3..13 mm) thick, their boundaries jittered by a few rows from line to line"""
    rng = np.random.default_rng(seed)
    n_layers = c["R"] // 10 + 1
    edges = np.cumsum(rng.integers(10, 41, n_layers))[None, None, :] + rng.integers(-3, 4, (c["F"], c["E"], n_layers))
    layer = (np.arange(c["R"])[None, None, :, None] >= np.sort(edges, -1)[:, :, None, :]).sum(-1)
    return ((layer * 3) % c["n_labels"]).astype(np.uint8)


class Variant:
    """a second copy of the library, by its C ABI: a context on the same stream and the one call"""
    def __init__(self, path, stream):
        self.L = C.CDLL(path)
        vp, u32 = C.c_void_p, C.c_uint32
        self.L.mcrt_create.argtypes = [C.c_int, C.POINTER(vp)]
        self.L.mcrt_set_stream.argtypes = [vp, vp]
        self.L.mcrt_destroy.argtypes = [vp]
        self.L.mcrt_recon_label_frames.argtypes = [vp, vp, u32, u32, u32, vp, vp, C.c_double, C.c_double, C.POINTER(mcrt.VolumeGrid), C.POINTER(mcrt.ReconLabelOpts), vp, vp, vp, vp]
        self.h = vp()
        assert self.L.mcrt_create(0, C.byref(self.h)) == 0 and self.L.mcrt_set_stream(self.h, vp(stream)) == 0

    def recon_label_frames(self, *a):
        assert self.L.mcrt_recon_label_frames(self.h, *a) == 0

    def close(self):
        self.L.mcrt_destroy(self.h)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "recon_label", "measure.csv")
    c = CASE
    pos, dirs = poses(c)
    n, p = c["n"], c["pitch"]
    row_mm = 150.0 / c["R"]
    g = mcrt.volume_grid((-(n - 1) * p / 2.0, 35.0, -(n - 1) * p / 2.0), (p, 0, 0), (0, p, 0), (0, 0, p), n, n, n)
    labels = torch.from_numpy(tissue(c)).cuda()
    stack = torch.from_numpy(np.random.default_rng(1).rayleigh(1.0, (c["F"], c["E"], c["R"])).astype(np.float32)).cuda()
    dpos, ddir = torch.from_numpy(pos).cuda(), torch.from_numpy(dirs).cuda()
    out8 = torch.empty((n, n, n), dtype=torch.uint8, device="cuda")
    out = torch.empty((n, n, n), dtype=torch.float32, device="cuda")
    cnt = torch.empty((n, n, n), dtype=torch.int32, device="cuda"); win = torch.empty_like(cnt)
    st = torch.zeros(2, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    ctx = mcrt.Context(0)
    ctx.set_stream(stream.cuda_stream)
    variant = Variant(os.path.join(ROOT, os.environ["RECON_LABEL_VARIANT"]), stream.cuda_stream) if os.environ.get("RECON_LABEL_VARIANT") else None
    opts = mcrt.recon_label_opts_struct(c["n_labels"], fill_radius=c["H"])
    vp = C.c_void_p

    def label():
        ctx.recon_label_frames(labels.data_ptr(), dpos, ddir, c["F"], c["E"], c["R"], g, c["n_labels"], out8.data_ptr(), count_dev=cnt.data_ptr(), votes_dev=win.data_ptr(),
                               stats_dev=st.data_ptr(), row_mm=row_mm, fill_radius=c["H"])

    def label_by_label():
        variant.recon_label_frames(vp(labels.data_ptr()), c["F"], c["E"], c["R"], vp(dpos.data_ptr()), vp(ddir.data_ptr()), row_mm, 10.0, C.byref(g), C.byref(opts),
                                   vp(out8.data_ptr()), vp(cnt.data_ptr()), vp(win.data_ptr()), vp(st.data_ptr()))

    def floats():
        ctx.recon_frames(stack.data_ptr(), dpos, ddir, c["F"], c["E"], c["R"], g, out.data_ptr(), count_dev=cnt.data_ptr(), stats_dev=st.data_ptr(), row_mm=row_mm, mode="mean",
                         fill_radius=c["H"])

    legs = {"labels [voxel][label]": label, "float mean": floats}
    if variant:
        legs["labels [label][voxel]"] = label_by_label
    times = {k: [] for k in legs}
    ref = None
    for r in range(WARM + ROUNDS):
        for name in (list(legs) if r % 2 == 0 else list(legs)[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(CALLS):
                legs[name]()
            e1.record(stream)
            e1.synchronize()
            stream.synchronize()
            if r >= WARM:
                times[name].append(e0.elapsed_time(e1) / CALLS)
            if r == 0 and name.startswith("labels"):
                got = [t.cpu().numpy().copy() for t in (out8, cnt, win, st)]
                ref = ref or got
                assert all(np.array_equal(a, b) for a, b in zip(ref, got)), "the layouts differ"
    samples = c["F"] * c["E"] * c["R"]
    rows = []
    for name, t in times.items():
        t = np.array(t)
        rows.append(dict(case=c["name"], leg=name, fill_radius=c["H"], median_ms=round(float(np.median(t)), 4), min_ms=round(float(t.min()), 4), max_ms=round(float(t.max()), 4),
                         samples=samples, voted=int(ref[1].astype(np.int64).sum()), voxels=n ** 3, sampled_voxels=int((ref[1] > 0).sum()),
                         ns_per_sample=round(float(np.median(t)) * 1e6 / samples, 4)))
        print(rows[-1], flush=True)
    ctx.close()
    if variant:
        variant.close()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(rows[0]))
        w.writeheader()
        w.writerows(rows)


if __name__ == "__main__":
    main()
