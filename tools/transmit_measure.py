#!/usr/bin/env python3
"""What the transmission pass costs beside the label pass whose walk it shares (profiles/transmit/measure.csv).

The reference's liver scene, 512 scan-lines, 465 rows: mcrt_transmit_frames (both modes, all three outputs) and mcrt_label_frames (all three
outputs) on the same poses -- one frame, and a table of 20 poses (bench.py's moving probe: 30 degrees about the probe's axis over the pass).
A timed window is `calls` calls of one leg between two HIP events on the context's stream; the legs ALTERNATE within one process so that
they share the machine's mood; the first windows of every shape are warm-up.  Writes one CSV row per (frames, leg): the median, the smallest
and the largest window in milliseconds PER CALL.

    python tools/transmit_measure.py [--repeats 15] [--warmup 3] [--calls 20] [--out profiles/transmit/measure.csv]
"""
import argparse
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
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--subdiv", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transmit", "measure.csv"))
    args = ap.parse_args()
    import torch
    import mcray_tracing_amd as m
    E, R = 512, 465
    cfg, meshes = m.synth.liver_scene(args.subdiv)
    sd = m.scene_io.build_scene(cfg, meshes)
    ctx = m.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    ctx.set_params(n_elements=E, n_rows=R)
    ctx.upload_scene(sd)
    rows = []
    for F in (1, 20):
        sweep = [m.Transducer(E, position=cfg["transducerPosition"], angles_deg=np.asarray(cfg["transducerAngles"], np.float64) + np.array([30.0 * f / F - (15.0 if F > 1 else 0.0), 0.0, 0.0]))
                 for f in range(F)]
        pos = torch.from_numpy(np.stack([t.pos for t in sweep])).cuda(); dirs = torch.from_numpy(np.stack([t.dir for t in sweep])).cuda()
        transmit = torch.empty((F, E, R), dtype=torch.float32, device="cuda")
        reflect = torch.empty((F, E, R), dtype=torch.float32, device="cuda")
        tissue = torch.empty((F, E, R), dtype=torch.uint8, device="cuda")
        interface = torch.empty((F, E, R), dtype=torch.int32, device="cuda")
        crossings = torch.empty((F, E), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        legs = {"label_frames": lambda: ctx.label_frames(pos, dirs, n_frames=F, tissue_dev=tissue, interface_dev=interface, crossings_dev=crossings),
                "transmit_frames_total": lambda: ctx.transmit_frames(pos, dirs, mode="total", n_frames=F, transmit_dev=transmit, reflect_dev=reflect, crossings_dev=crossings),
                "transmit_frames_boundaries": lambda: ctx.transmit_frames(pos, dirs, mode="boundaries", n_frames=F, transmit_dev=transmit, reflect_dev=reflect,
                                                                          crossings_dev=crossings)}
        ms = {k: [] for k in legs}
        for rep in range(args.warmup + args.repeats):
            for name, fn in legs.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                for _ in range(args.calls):
                    fn()
                b.record(stream)
                ctx.synchronize()
                if rep >= args.warmup:
                    ms[name].append(a.elapsed_time(b) / args.calls)
        cr = crossings.cpu().numpy().astype(np.uint32) & 0x7fffffff
        for name, v in ms.items():
            rows.append((F, E, R, name, statistics.median(v), min(v), max(v), args.repeats, args.calls, float(cr.mean()), int(cr.max())))
    text = "frames,scan_lines,rows,leg,median_ms_per_call,min_ms_per_call,max_ms_per_call,windows,calls_per_window,mean_crossings,max_crossings\n"
    text += "".join("%d,%d,%d,%s,%.5f,%.5f,%.5f,%d,%d,%.2f,%d\n" % r for r in rows)
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
