#!/usr/bin/env python3
"""Paths that have left the image, COUNTED on the CPU oracle before anything is built for them.

The accumulation loop takes a step only while t < max_travel and adds an echo only into a row < n_rows; path time never decreases.  A segment
whose start time t_start = distance_traveled * 1000 / sos is past both limits adds nothing, and neither does anything after it on its path:
its closest-hit query, its interface physics, its march record and its slot in k_march are work the image does not need.  Per bounce this
script counts, on one frame of a workload: live segments, segments that start past the image ("late"), the RF steps a segment nominally has
and the steps the loop really takes (min(steps, ceil((max_travel - t_start) / time_step)), 0 in a silent medium or past max_travel; a segment that
misses every triangle runs to the ray's end, so the nominal counts are astronomic -- `iterations_8_sort_class` caps a segment at the 63 iterations
k_march's tile sort distinguishes); and over
the frame the share of closest-hit queries that belong to late segments.  With `sample=N` it also replays the queries of the first N scan-lines
one by one through the oracle's BVH4 walk, each over its own segment (from -> to: the hit point plus the thickness draw, or the ray's end on a miss --
a CLIPPED ray, so the visits are a lower bound of the walk's, for late and other queries alike) and reports the late share of node visits.

    python tools/late_count.py [workload=random1m|liver|sphere] [rays=1024] [scan-lines=128] [sample=8]   -> JSON (profiles/retire_fold/late_count_*.json)
"""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mcray_tracing_amd as m
from oracle import orc

workload = sys.argv[1] if len(sys.argv) > 1 else "random1m"
S = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
E = int(sys.argv[3]) if len(sys.argv) > 3 else 128
sample = int(sys.argv[4]) if len(sys.argv) > 4 else 8
cfg, meshes = {"random1m": lambda: m.synth.random_scene(1_000_000, 8, 12345), "liver": lambda: m.synth.liver_scene(5), "sphere": lambda: m.synth.sphere_scene(5)}[workload]()
sd = m.scene_io.build_scene(cfg, meshes)
tr = m.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
nodes, btri, n4, _ = m.host_build_bvh4(sd.tri, sd.tri_mesh)
osc = orc.OracleScene(sd.tri, sd.tri_mesh, sd.meshes, sd.materials, sd.start_mat, sd.spacing, bvh=(nodes, btri)); osc.set_bvh4(n4)
tex = orc.texture(256)
p = orc.default_params(n_elements=E, n_samples=S)
k = orc.constants(p.frequency, p.sos, p.depth_cm)
t0 = time.time()
o = osc.trace_frame(p, tr.pos, tr.dir, tex, frame_id=0, use_bvh=2, n_threads=os.cpu_count(), want_segs=True, want_ref=False, want_fix=False)
segs, cnt = o["segs"], o["seg_count"]
mats = np.asarray(sd.materials, np.float32).reshape(-1, 8)
axial_mm, time_step, max_travel = float(k.axial_res_mm), float(k.time_step_us), float(k.max_travel_us)
image_end = float(m.host_row_thresholds(float(k.row_dt_us), p.n_rows)[-1])          # the first time past the image
limit = max(max_travel, image_end)

rows, late_all = [], np.zeros(segs.shape, bool)
for b in range(p.max_depth):
    live = cnt > b
    if not live.any(): break
    sg = segs[:, :, b]
    t_start = sg["distance_traveled"] * 1000.0 / float(p.sos)
    late = live & (t_start >= limit)
    late_all[:, :, b] = late
    d = (sg["to"] - sg["from"]).astype(np.float32)
    dist_f = (np.sqrt((d ** 2).sum(-1, dtype=np.float32)) * np.float32(10.0)).astype(np.float64)
    steps = np.where(live, np.floor(dist_f / axial_mm), 0).astype(np.int64)
    silent = (mats[sg["media"], 2] == 0) & (mats[sg["media"], 4] == 0)
    room = np.ceil(np.maximum(max_travel - t_start, 0.0) / time_step).astype(np.int64)
    taken = np.where(silent, 0, np.minimum(steps, room))
    nz = sg["reflected_intensity"] != 0
    rows.append({"bounce": b, "live": int(live.sum()), "late_start": int(late.sum()), "steps_nominal": int(steps.sum()), "steps_taken": int(taken.sum()),
                 "iterations_8_nominal": int(((steps + 7) // 8).sum()), "iterations_8_sort_class": int(np.minimum(np.where(silent, 0, (steps + 7) // 8), 63).sum()),
                 "iterations_8_taken": int(((taken + 7) // 8).sum()),
                 "silent_segments": int((live & silent).sum()), "boundary_echo_nonzero": int((live & nz).sum())})
queries, late_q = int(sum(r["live"] for r in rows)), int(late_all.sum())
out = {"workload": workload, "scan_lines": E, "rays": S, "max_travel_us": max_travel, "image_end_us": image_end, "queries": queries, "late_queries": late_q,
       "late_query_share": late_q / queries, "per_bounce": rows}
if sample > 0:
    # bounce 0 is ONE query per scan-line on the GPU (every sample path starts as the same ray): counted once here too
    vis = {False: 0, True: 0}; n_q = {False: 0, True: 0}
    for e in range(min(sample, E)):
        for s in range(S):
            for b in range(int(cnt[e, s])):
                if b == 0 and s != 0: continue
                g = segs[e, s, b]
                st = osc.closest_hit(g["from"], g["to"], use_bvh=2)[4]
                is_late = bool(late_all[e, s, b])
                vis[is_late] += st["nodes_visited"]; n_q[is_late] += 1
    out["sampled"] = {"scan_lines": min(sample, E), "queries": n_q[False] + n_q[True], "late_queries": n_q[True], "late_query_share": n_q[True] / max(1, n_q[False] + n_q[True]),
                      "node_visits": vis[False] + vis[True], "late_node_visits": vis[True], "late_node_visit_share": vis[True] / max(1, vis[False] + vis[True]),
                      "note": "each query replayed over its own clipped segment: a lower bound of the walk's visits"}
out["seconds"] = round(time.time() - t0, 1)
print(json.dumps(out, indent=1))
