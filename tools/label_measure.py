#!/usr/bin/env python3
"""What the label pass costs beside the traced pass it explains (profiles/labels/README.md).

The benchmark's workload -- the 1 M-triangle scene, 128 scan-lines x 1024 sample paths, 465 rows -- with a table of 20 probe poses (bench.py's
moving probe: 30 degrees about the probe's axis over the pass): mcrt_label_frames (both rules; all three outputs, and the tissue map alone)
and mcrt_trace_frames_poses of the same 20 frames, each call between two HIP events on the context's stream, the legs ALTERNATING within
one process so that they share the machine's mood.  Prints one JSON document: per leg the median, the smallest and the largest of the
timed calls in milliseconds, and each label leg's share of the traced pass.

    python tools/label_measure.py [--repeats 15] [--warmup 3] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import mcray_tracing_amd as m
    E, S, R, F = 128, 1024, 465, args.frames
    cfg, meshes = m.synth.random_scene(1_000_000, 8, 12345)
    sd = m.scene_io.build_scene(cfg, meshes)
    tr = m.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    ctx = m.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    ctx.set_params(n_elements=E, n_samples=S, n_rows=R, frequency=tr.frequency)
    ctx.upload_scene(sd); ctx.upload_texture(None, 256); ctx.set_transducer(tr.pos, tr.dir)
    sweep = [m.Transducer(E, position=cfg["transducerPosition"], angles_deg=np.asarray(cfg["transducerAngles"], np.float64) + np.array([30.0 * f / F - 15.0, 0.0, 0.0]))
             for f in range(F)]
    pos = torch.from_numpy(np.stack([t.pos for t in sweep])).cuda(); dirs = torch.from_numpy(np.stack([t.dir for t in sweep])).cuda()
    rf = torch.empty((F, E, R), dtype=torch.float32, device="cuda")
    tissue = torch.empty((F, E, R), dtype=torch.uint8, device="cuda")
    interface = torch.empty((F, E, R), dtype=torch.int32, device="cuda")
    crossings = torch.empty((F, E), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    frame = [0]

    def traced():
        ctx.trace_frames_poses(frame[0], pos, dirs, rf, n_frames=F); frame[0] += F

    def lab(rule, offs, full):
        return lambda: ctx.label_frames(pos, dirs, rule=rule, start_offset=offs, n_frames=F, tissue_dev=tissue, interface_dev=interface if full else None,
                                        crossings_dev=crossings if full else None)

    legs = {"traced_pass": traced, "label_traced": lab("traced", None, True), "label_geometric": lab("geometric", 1e-3, True),
            "label_traced_tissue_only": lab("traced", None, False)}
    ms = {k: [] for k in legs}
    for rep in range(args.warmup + args.repeats):
        for name, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream); fn(); b.record(stream)
            ctx.synchronize()
            if rep >= args.warmup:
                ms[name].append(a.elapsed_time(b))
    cr = crossings.cpu().numpy().astype(np.uint32)
    out = {"workload": "random1m: 1 M triangles, %d scan-lines x %d sample paths, %d rows, a table of %d poses" % (E, S, R, F), "repeats": args.repeats,
           "warmup": args.warmup, "crossings_per_beam": {"mean": float((cr & 0x7fffffff).mean()), "max": int((cr & 0x7fffffff).max()), "capped_beams": int((cr >> 31).sum())},
           "legs_ms": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in ms.items()}}
    base = out["legs_ms"]["traced_pass"]["median"]
    out["share_of_traced_pass"] = {k: v["median"] / base for k, v in out["legs_ms"].items() if k != "traced_pass"}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
