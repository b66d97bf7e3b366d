#!/usr/bin/env python3
"""A bounce as BEAMS, COUNTED on the CPU oracle: what csrc/mcrt_beam.hip shares per scan-line (bounce 1) and per group (bounce b >= 2).

Every bounce-1 ray of a scan-line starts at bounce 0's hit point.  On frame 0 of a workload this script groups the bounce-1 segments of the
oracle into beams as the kernels do -- scan-line x history (the medium after bounce 0 is the start medium: reflected) x dominant axis x its
sign --, and per beam takes the bounds of the two slopes d_other / |d_dom| and, with the kernels' volume (cross-section at both ends of a
box's depth range, the margin of 2^-18 x the largest coordinate), the CANDIDATES: triangles whose padded bounds touch the volume.  Counted:
whether the origin is one point per scan-line; the spread of the slopes; candidates up to the scene's exit and up to the depth by which
90 % of the beam's hitting rays have hit ("near"); how many hit triangles are missing from their beam's candidates (must be 0); the share
of rays that hit nothing.

With a bounce b >= 2 the group is the kernels' widened key -- scan-line, the triangle the previous segment ended on, medium -- and a beam is a group's rays
of one dominant axis and sign.  Also counted then, per bounce: the list entries a ray tests before it is final (its hit's depth plus 2 m lies before the next
entry's begin; a miss tests the whole list), ray-weighted; the same for the slowest ray of every beam among 64 QUEUE NEIGHBOURS, summed over the wavefront's
beams (what k_beam_test's loop runs through); and the beams per 64 queue neighbours -- in k_shade's queue order: per 256 rays of the previous queue the
reflected survivors first, then the refracted ones; and the same two figures for the BEAM ORDER (one beam per wavefront by construction; a beam's rays cut into
wavefronts, the slowest ray of each), to set against mcrt_debug_beam_order's counter.  `lines` counts only that many scan-lines, spread evenly (the trace covers all of them).  A sixth argument `beams` adds the list of every beam (`per_beam`:
thousands of lines at the deeper bounces) to the totals.

    python tools/beam_count.py [workload=random1m|liver|sphere] [rays=1024] [scan-lines=128] [bounce=1] [lines=all] [beams]   -> JSON (profiles/beam/beam_count_*.json,
                                                                                                                          profiles/beam_deep/beam_count_*_b*.json)
"""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mcray_tracing_amd as m
from oracle import orc

workload = sys.argv[1] if len(sys.argv) > 1 else "random1m"
S = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
E = int(sys.argv[3]) if len(sys.argv) > 3 else 128
BN = int(sys.argv[4]) if len(sys.argv) > 4 else 1
NL = int(sys.argv[5]) if len(sys.argv) > 5 else E
PER_BEAM = len(sys.argv) > 6 and sys.argv[6] == "beams"
counted = sorted(set(int(round(x)) for x in np.linspace(0, E - 1, min(NL, E))))
cfg, meshes = {"random1m": lambda: m.synth.random_scene(1_000_000, 8, 12345), "liver": lambda: m.synth.liver_scene(5), "sphere": lambda: m.synth.sphere_scene(5)}[workload]()
sd = m.scene_io.build_scene(cfg, meshes)
tr = m.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
nodes, btri, n4, _ = m.host_build_bvh4(sd.tri, sd.tri_mesh)
osc = orc.OracleScene(sd.tri, sd.tri_mesh, sd.meshes, sd.materials, sd.start_mat, sd.spacing, bvh=(nodes, btri)); osc.set_bvh4(n4)
tex = orc.texture(256)
p = orc.default_params(n_elements=E, n_samples=S)
t0 = time.time()
o = osc.trace_frame(p, tr.pos, tr.dir, tex, frame_id=0, use_bvh=2, n_threads=os.cpu_count(), want_segs=True, want_ref=False, want_fix=False)
segs, cnt = o["segs"], o["seg_count"]
t_trace = time.time() - t0

# the triangles' padded bounds (contract: pad = 2e-4 * largest extent + pad_abs), as tri_padded_bounds
V = np.asarray(sd.tri, np.float32).reshape(-1, 3, 3)
lo, hi = V.min(1), V.max(1)
ext = np.maximum(0.0, (hi - lo).max(1)).astype(np.float32)
pad = (np.float32(2e-4) * ext + np.float32(osc.c.pad_abs)).astype(np.float32)
plo, phi = (lo - pad[:, None]).astype(np.float64), (hi + pad[:, None]).astype(np.float64)
scene_abs = float(max(np.abs(plo).max(), np.abs(phi).max()))
spacing = np.asarray(sd.spacing, np.float64)
offs = float(p.ray_start_offset)

sg = segs[:, :, BN]
live = cnt > BN
# k_shade's queue order of bounce BN: position of every live (scan-line, sample) in the queue
order = np.arange(E * S)
for b in range(BN):
    alive = (cnt.reshape(-1)[order] > b + 1)
    refl = segs[:, :, min(b + 1, segs.shape[2] - 1)]["media"].reshape(-1)[order] == segs[:, :, b]["media"].reshape(-1)[order]
    nxt = []
    for c0 in range(0, len(order), 256):
        o, a_, r_ = order[c0:c0 + 256], alive[c0:c0 + 256], refl[c0:c0 + 256]
        nxt.append(o[a_ & r_]); nxt.append(o[a_ & ~r_])
    order = np.concatenate(nxt) if nxt else order[:0]
qpos = np.full(E * S, -1, np.int64); qpos[order] = np.arange(len(order))
ray_beam = np.full(E * S, -1, np.int64); ray_tested = np.zeros(E * S, np.int64)
same_origin, beams = 0, []
missing = hitting = rays = small = 0
for e in counted:
    L = live[e]
    if not L.any(): continue
    flat = e * S + np.flatnonzero(L)
    fr = sg["from"][e][L].astype(np.float64)
    same_origin += int((sg["from"][e][L].view(np.uint32) == sg["from"][e][L][0].view(np.uint32)).all())
    d = sg["dir"][e][L].astype(np.float64)
    D = d * spacing                                              # the tested segment's direction (the start offset along dir moves f2, not the slopes, by 1e-7)
    f2 = fr + offs * d
    tri = sg["tri"][e][L]
    to = sg["to"][e][L].astype(np.float64)
    hist = (sg["media"][e][L] != sd.start_mat) if BN == 1 else (segs[:, :, BN - 1]["tri"][e][L].astype(np.int64) * 4096 + sg["media"][e][L])
    dom = np.abs(D).argmax(1)
    neg = D[np.arange(len(D)), dom] < 0
    ok = np.isfinite(D).all(1)
    for key in np.unique(np.stack([hist, dom, neg], 1)[ok], axis=0):
        sel = ok & (hist == key[0]) & (dom == key[1]) & (neg == bool(key[2]))
        if sel.sum() < 16: small += int(sel.sum())
        k, ka, kb = int(key[1]), (int(key[1]) + 1) % 3, (int(key[1]) + 2) % 3
        sgn = -1.0 if key[2] else 1.0
        ad = np.abs(D[sel, k])
        u, v = D[sel, ka] / ad, D[sel, kb] / ad
        flo, fhi = f2[sel].min(0), f2[sel].max(0)
        cmax = max(np.abs(f2[sel]).max(), scene_abs)
        mg = cmax * 2.0 ** -18
        xref = fhi[k] if key[2] else flo[k]
        w = fhi[k] - flo[k]
        sb0 = (xref - phi[:, k]) if key[2] else (plo[:, k] - xref)
        sb1 = (xref - plo[:, k]) if key[2] else (phi[:, k] - xref)
        s0, s1 = np.maximum(sb0 - mg, -mg), sb1 + mg
        cand = s0 <= s1
        sa = s0 - w
        for (smin, smax, axis) in ((u.min(), u.max(), ka), (v.min(), v.max(), kb)):
            prod = np.stack([sa * smin, sa * smax, s1 * smin, s1 * smax])
            cand &= (flo[axis] + prod.min(0) - mg <= phi[:, axis]) & (fhi[axis] + prod.max(0) + mg >= plo[:, axis])
        begin = sb0[cand] - mg
        ids = np.flatnonzero(cand)
        hit = tri[sel] >= 0
        missing += int((~np.isin(tri[sel][hit], ids)).sum()); hitting += int(hit.sum()); rays += int(sel.sum())
        depth = sgn * (to[sel, k] - xref)
        d90 = float(np.quantile(depth[hit], 0.9)) if hit.any() else 0.0
        srt = np.sort(begin)
        ray_tested[flat[sel]] = np.where(hit, np.searchsorted(srt, depth + 2 * mg, side="right"), len(srt))
        ray_beam[flat[sel]] = len(beams)
        beams.append({"scan_line": e, "reflected": bool(not key[0]) if BN == 1 else None, "axis": k, "negative": bool(key[2]), "rays": int(sel.sum()), "hitting": int(hit.sum()),
                      "spread_mrad": [float(1e3 * (u.max() - u.min())), float(1e3 * (v.max() - v.min()))],
                      "candidates": int(cand.sum()), "candidates_near": int((begin <= d90 + 2 * mg).sum()) if hit.any() else 0, "depth_90": d90})

with_hits = [b for b in beams if b["hitting"]]
# per 64 queue neighbours (wavefronts that lie wholly inside the counted scan-lines' rays count; others are skipped)
in_beam = ray_beam >= 0
wave_beams, wave_entries = [], []
for w0 in range(0, len(order), 64):
    ids = order[w0:w0 + 64]
    if not in_beam[ids].all(): continue
    bs = ray_beam[ids]
    wave_beams.append(len(np.unique(bs)))
    wave_entries.append(int(sum(ray_tested[ids][bs == u].max() for u in np.unique(bs))))
# ... and per 64 words of the BEAM ORDER (k_beam_rank / k_beam_scan / k_beam_place): a beam's rays in queue order, its segment cut into wavefronts -- one beam each by
# construction, the last of a segment padded.  (Which run of a segment a wavefront's members take depends on atomic timing on the GPU: queue order stands in for it.)
ordered_entries, ordered_lanes = [], 0
counted_ids = order[in_beam[order]]
for u in np.unique(ray_beam[counted_ids]):
    ids = counted_ids[ray_beam[counted_ids] == u]
    for w0 in range(0, len(ids), 64):
        ordered_entries.append(int(ray_tested[ids[w0:w0 + 64]].max())); ordered_lanes += 64
spread = [max(b["spread_mrad"]) for b in beams]
out = {"workload": workload, "scan_lines": E, "rays_per_line": S, "frame": 0, "bounce": BN, "scan_lines_counted": len(counted),
       "beams_per_counted_scan_line": len(beams) / max(len(counted), 1), "rays_per_beam_mean": rays / max(len(beams), 1), "share_of_rays_in_beams_of_fewer_than_16": small / max(rays, 1),
       "entries_tested_per_ray_mean": float(ray_tested[in_beam].mean()) if in_beam.any() else None,
       "wavefronts_counted": len(wave_beams), "beams_per_64_queue_neighbours_mean_max": [float(np.mean(wave_beams)), int(np.max(wave_beams))] if wave_beams else None,
       "entries_per_64_queue_neighbours_summed_over_their_beams_mean": float(np.mean(wave_entries)) if wave_entries else None, "oracle_trace_seconds": round(t_trace, 1),
       "beam_order_wavefronts": len(ordered_entries), "beam_order_beams_per_wavefront": 1.0 if ordered_entries else None,
       "beam_order_entries_per_wavefront_mean": float(np.mean(ordered_entries)) if ordered_entries else None, "beam_order_pad_lane_share": 1.0 - int(in_beam.sum()) / max(ordered_lanes, 1),
       "lines_reaching_the_bounce": int(live.any(1).sum()), "lines_with_one_origin": same_origin,
       "rays_of_the_bounce": int(live.sum()), "rays_in_beams": rays, "rays_hitting": hitting, "miss_share": 1.0 - hitting / max(rays, 1),
       "hit_triangles_missing_from_candidates": missing,
       "beams": len(beams), "beams_with_hits": len(with_hits),
       "spread_mrad_min_median_max": [float(np.min(spread)), float(np.median(spread)), float(np.max(spread))],
       "candidates_to_exit_mean_max": [float(np.mean([b["candidates"] for b in beams])), int(np.max([b["candidates"] for b in beams]))],
       "candidates_near_mean_max": [float(np.mean([b["candidates_near"] for b in with_hits])), int(np.max([b["candidates_near"] for b in with_hits]))] if with_hits else None,
       }
if PER_BEAM: out["per_beam"] = beams
print(json.dumps(out, indent=1))
