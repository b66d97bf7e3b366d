"""Measurements for DESIGN 5.7, the compounding modes: k_compound alone, float and 8-bit, 128 x 465 views -> 400 x 500 pictures, F = 20 and
128, N = 3, 5 and 9, 33 calls per leg, shape and form; the median over the last 30.

    rocprofv3 --kernel-trace --stats -d DIR -o modes -- python tools/compound_modes_measure.py trace default weighted max median
    python tools/compound_modes_measure.py summarise DIR/.../modes_kernel_trace.csv profiles/compound_modes/NAME.csv default weighted max median

Legs: default (the calls without options: the plain mean), weighted (weights 1, 0.5, 2, ... and a ramp of 8 scan-lines), max, median (both with
weights 1 and no ramp).  The same `trace default` run with MCRT_TUNING=1 MCRT_LIB=<another build> measures that build: the parent commit's
library for the default leg, a -DMCRT_MEDIAN_PIX=2 / 1 variant for the median.  The summary takes the k_compound launches of the trace in
launch order: leg after leg, shape after shape, the float form's 33 calls and then the 8-bit form's."""
import csv
import os
import sys
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

E, R, ROWS, COLS = 128, 465, 400, 500
SHAPES = [(F, N) for F in (20, 128) for N in (3, 5, 9)]
CALLS, WARM = 33, 3
WEIGHTS = (1.0, 0.5, 2.0, 1.5, 0.75, 1.25, 1.0, 0.5, 2.0)


def steers(N):
    """N views 5 degrees apart, centred on the unsteered one"""
    return tuple(np.deg2rad(5.0) * (n - (N - 1) // 2) for n in range(N))


def options(leg, N):
    if leg == "default":
        return {}, {}
    if leg == "weighted":
        return dict(mode="mean", view_weights=WEIGHTS[:N], feather_lines=8.0), dict(compound_mode="mean", view_weights=WEIGHTS[:N], feather_lines=8.0)
    return dict(mode=leg), dict(compound_mode=leg)


def trace(legs):
    import mcray_tracing_amd as m
    ctx = m.Context(0)
    rng = np.random.default_rng(1)
    for leg in legs:
        for F, N in SHAPES:
            n_in = F * N * E * R
            src = ctx.alloc(n_in * 4)
            ctx.h2d(src, np.abs(rng.standard_normal(n_in)).astype(np.float32))
            pic = ctx.alloc(F * ROWS * COLS * 4)
            ctx.synchronize()
            s = steers(N)
            kf, kb = options(leg, N)
            for _ in range(CALLS):
                ctx.compound_frames(src, F, E, R, s, pic, **kf)
            ctx.synchronize()
            for _ in range(CALLS):
                ctx.bmode_compound_frames(src, F, E, R, s, pic, **kb)
            ctx.synchronize()
            ctx.free(src); ctx.free(pic)
    ctx.close()


def summarise(trace_csv, out_csv, legs):
    rows = [r for r in csv.DictReader(open(trace_csv)) if "k_compound" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0 for r in rows]
    assert len(d) == CALLS * 2 * len(SHAPES) * len(legs), (len(d), legs)
    table, i = [], 0
    for leg in legs:
        for F, N in SHAPES:
            for form in ("float", "8-bit"):
                names = {rows[j]["Kernel_Name"] for j in range(i, i + CALLS)}
                assert len(names) == 1 and (("k_compound<false" in min(names)) == (form == "float")), names
                table.append((leg, form, F, N, float(np.median(d[i + WARM:i + CALLS])), min(names).split("(")[0]))
                i += CALLS
    os.makedirs(os.path.dirname(os.path.abspath(out_csv)), exist_ok=True)
    with open(out_csv, "w") as f:
        f.write("leg,form,F,N,median_us,kernel\n")
        for t in table:
            f.write("%s,%s,%d,%d,%.2f,\"%s\"\n" % t)
    for t in table:
        print("%-9s %-6s F=%-4d N=%d  %9.2f us  %s" % t)


if sys.argv[1:2] == ["summarise"]:
    summarise(sys.argv[2], sys.argv[3], sys.argv[4:])
elif sys.argv[1:2] == ["trace"]:
    trace(sys.argv[2:] or ["default"])
else:
    sys.exit(__doc__)
