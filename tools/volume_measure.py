"""Measurements for DESIGN 5.8: k_volume in both forms beside k_remap producing the same number of output pixels in the same session (per
point k_remap has half the taps and two-thirds of the map reads), and the existing display kernels k_remap and k_compound, to be run on
this library and on the parent commit's (MCRT_LIB) to show that they did not move.  A stack of K = 32 planes of 128 x 465, random data,
33 calls of each kernel per leg, every leg in a run of its own:

    rocprofv3 --kernel-trace --stats -d DIR -o volume -- python tools/volume_measure.py run LEG
    python tools/volume_measure.py summarise LEG DIR/.../volume_kernel_trace.csv profiles/volume/LEG.csv

LEG: volume_f1, volume_f4 (a 160 x 200 x 96 volume), cplane_f20, cplane_f128 (a 400 x 500 C-plane), label_f20, label_f128 (k_label_gather:
the same C-plane gathered from a byte stack of the same shape), existing (k_remap and k_compound as tools/compound_measure.py runs them at
F = 20 and 128, N = 3).  The summary takes the kernels of the trace in launch order and the median
over the last 30 of each family's 33."""
import csv
import os
import sys
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

E, R, K = 128, 465, 32
STEP, PIVOT = 0.02, 10.0                      # 32 planes over 0.62 rad about a pivot 20 mm behind the apex
CALLS, WARM = 33, 3
LEGS = {"volume_f1": ("volume", 1), "volume_f4": ("volume", 4), "cplane_f20": ("cplane", 20), "cplane_f128": ("cplane", 128), "label_f20": ("label", 20), "label_f128": ("label", 128),
        "existing": ("existing", 0)}
FAMILIES = {"volume": [("k_volume float", lambda k: "k_volume<false" in k), ("k_volume 8-bit", lambda k: "k_volume<true" in k), ("k_remap, same pixels", lambda k: "k_remap(" in k)],
            "existing": [("k_remap F=20x3", None), ("k_compound float F=20 N=3", None), ("k_remap F=128x3", None), ("k_compound float F=128 N=3", None)]}
FAMILIES["cplane"] = FAMILIES["volume"]
FAMILIES["label"] = [("k_label_gather", lambda k: "k_label_gather(" in k)]


def grid_of(m, what):
    if what == "cplane":                      # 400 x 500 points 0.1 mm apart at y = 90 mm, inside the sweep
        return m.cplane_grid(90.0, 500, 400, 0.1)
    return m.volume_grid((-23.85, 60.0, -14.25), (0.3, 0, 0), (0, 0.4, 0), (0, 0, 0.3), 160, 200, 96)      # 48 x 80 x 28.5 mm inside the sweep


def run(leg):
    import mcray_tracing_amd as m
    what, F = LEGS[leg]
    ctx = m.Context(0)
    rng = np.random.default_rng(1)
    if what == "existing":
        for F in (20, 128):
            src = ctx.alloc(F * 3 * E * R * 4)
            ctx.h2d(src, np.abs(rng.standard_normal(F * 3 * E * R)).astype(np.float32))
            pic = ctx.alloc(F * 3 * 400 * 500 * 4)
            steers = tuple(np.deg2rad(5.0) * (n - 1) for n in range(3))
            for _ in range(CALLS):
                ctx.scan_convert_frames(src, F * 3, E, R, pic)
            for _ in range(CALLS):
                ctx.compound_frames(src, F, E, R, steers, pic)
            ctx.synchronize()
            ctx.free(src); ctx.free(pic)
        ctx.close()
        return
    g = grid_of(m, "cplane" if what == "label" else what)
    n = g.nu * g.nv * g.nw
    if what == "label":
        src = ctx.alloc(F * K * E * R)
        ctx.h2d(src, rng.integers(0, 200, F * K * E * R).astype(np.uint8))
        out = ctx.alloc(F * n)
        ctx.synchronize()
        for _ in range(CALLS):
            ctx.label_volume_frames(src, F, E, R, (K, STEP, PIVOT), g, out)
        ctx.synchronize()
        ctx.free(src); ctx.free(out)
        ctx.close()
        return
    maps = m.host_volume_maps(E, R, (K, STEP, PIVOT), g)
    inside = np.mean((maps[0] >= 0) & (maps[0] < K - 1) & (maps[1] >= 0) & (maps[1] < R - 1) & (maps[2] >= 0) & (maps[2] < E - 1))
    print("%s: %d points, %.3f of them with all eight taps inside" % (leg, n, inside))
    images = F * g.nw                          # k_remap over this many nv x nu pictures writes the same number of pixels
    src = ctx.alloc(max(F * K, images) * E * R * 4)
    ctx.h2d(src, np.abs(rng.standard_normal(max(F * K, images) * E * R)).astype(np.float32))
    out = ctx.alloc(F * n * 4)
    ctx.synchronize()
    for _ in range(CALLS):
        ctx.volume_frames(src, F, E, R, (K, STEP, PIVOT), g, out)
    for _ in range(CALLS):
        ctx.bmode_volume_frames(src, F, E, R, (K, STEP, PIVOT), g, out)
    for _ in range(CALLS):
        ctx.scan_convert_frames(src, images, E, R, out, out_rows=g.nv, out_cols=g.nu)
    ctx.synchronize()
    ctx.free(src); ctx.free(out)
    ctx.close()


def summarise(leg, trace_csv, out_csv):
    what, F = LEGS[leg]
    rows = list(csv.DictReader(open(trace_csv)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    us = lambda rs: [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0 for r in rs]
    table = []
    if what == "existing":                     # launch order: remap x 33, compound x 33 at F = 20, then at F = 128
        d = [r for r in rows if "k_remap(" in r["Kernel_Name"] or "k_compound<" in r["Kernel_Name"]]
        assert len(d) == 4 * CALLS, len(d)
        for i, (name, _) in enumerate(FAMILIES["existing"]):
            part = d[i * CALLS:(i + 1) * CALLS]
            assert len({r["Kernel_Name"] for r in part}) == 1
            table.append((name, float(np.median(us(part)[WARM:]))))
    else:
        for name, match in FAMILIES[what]:
            d = us([r for r in rows if match(r["Kernel_Name"])])
            assert len(d) == CALLS, (name, len(d))
            table.append((name, float(np.median(d[WARM:]))))
    with open(out_csv, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["leg", "kernel", "median_us"])
        for name, t in table:
            w.writerow([leg, name, "%.2f" % t])
    for name, t in table:
        print("%-12s %-28s %10.2f us" % (leg, name, t))


if sys.argv[1:2] == ["summarise"]:
    summarise(sys.argv[2], sys.argv[3], sys.argv[4])
else:
    run(sys.argv[2])
