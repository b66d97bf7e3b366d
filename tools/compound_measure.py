"""Measurements for DESIGN 5.7: k_compound in both forms beside what converting the F * N views one by one would cost at the least --
k_remap and k_bmode over the same F * N images, before any averaging pass.  128 x 465 views -> 400 x 500 pictures, F = 20 and 128,
N = 3, 5 and 9, 33 calls of each per shape.

    python tools/compound_measure.py events                 HIP events around each call (launch included) -> out/compound_measure_events.json
    rocprofv3 --kernel-trace --stats -d DIR -o compound -- python tools/compound_measure.py trace
    python tools/compound_measure.py summarise DIR/.../compound_kernel_trace.csv profiles/compound/kernel_medians.csv
    rocprofv3 --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_WAIT_INST_ANY SQ_INSTS_VMEM_RD SQ_INSTS_VALU SQ_BUSY_CU_CYCLES --output-format csv -d DIR -o compound \
        -- python tools/compound_measure.py counters      a counter run of its own: F = 20, N = 3 alone, 5 calls of each

The summary takes the kernels of the trace in launch order: every family (k_compound float, k_compound 8-bit, k_remap, k_bmode) is launched
33 times per shape, shape after shape, and the median is taken over the last 30 of each 33."""
import csv
import ctypes as C
import json
import os
import sys
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

E, R, ROWS, COLS = 128, 465, 400, 500
SHAPES = [(F, N) for F in (20, 128) for N in (3, 5, 9)]
CALLS, WARM = 33, 3
FAMILIES = [("k_compound float", lambda k: "k_compound<false" in k), ("k_compound 8-bit", lambda k: "k_compound<true" in k),
            ("k_remap", lambda k: "k_remap(" in k), ("k_bmode", lambda k: "k_bmode<" in k)]


def steers(N):
    """N views 5 degrees apart, centred on the unsteered one"""
    return tuple(np.deg2rad(5.0) * (n - (N - 1) // 2) for n in range(N))


def measure(mode):
    import mcray_tracing_amd as m
    hip = C.CDLL("libamdhip64.so")
    vp = C.c_void_p
    hip.hipEventRecord.argtypes = [vp, vp]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), vp, vp]
    hip.hipEventSynchronize.argtypes = [vp]

    def chk(rc):
        assert rc == 0, rc

    ctx = m.Context(0)
    st = vp(); chk(hip.hipStreamCreate(C.byref(st)))
    ctx.set_stream(st.value)
    e0, e1 = vp(), vp(); chk(hip.hipEventCreate(C.byref(e0))); chk(hip.hipEventCreate(C.byref(e1)))

    def timed(fn):
        ts = []
        for i in range(WARM + 2 if mode == "counters" else CALLS):
            chk(hip.hipEventRecord(e0, st)); fn(); chk(hip.hipEventRecord(e1, st)); chk(hip.hipEventSynchronize(e1))
            ms = C.c_float(); chk(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
            if i >= WARM:
                ts.append(ms.value * 1000.0)
        return float(np.median(ts))

    out = {}
    rng = np.random.default_rng(1)
    for F, N in (SHAPES[:1] if mode == "counters" else SHAPES):
        n_in = F * N * E * R
        src = ctx.alloc(n_in * 4)
        ctx.h2d(src, np.abs(rng.standard_normal(n_in)).astype(np.float32))
        pic = ctx.alloc(F * N * ROWS * COLS * 4)            # room for the F * N separate conversions
        ctx.synchronize()
        s = steers(N)
        r = {}
        r["compound_frames_us"] = timed(lambda: ctx.compound_frames(src, F, E, R, s, pic))
        r["bmode_compound_frames_us (peak + grey + k_compound)"] = timed(lambda: ctx.bmode_compound_frames(src, F, E, R, s, pic))
        r["scan_convert_frames over F*N images_us"] = timed(lambda: ctx.scan_convert_frames(src, F * N, E, R, pic))
        r["bmode_frames over F*N images_us (peak + grey + k_bmode)"] = timed(lambda: ctx.bmode_frames(src, F * N, E, R, pic))
        out["F=%d N=%d" % (F, N)] = r
        ctx.free(src); ctx.free(pic)
    ctx.close()
    print(json.dumps(out, indent=1))
    os.makedirs("out", exist_ok=True)
    with open("out/compound_measure_%s.json" % mode, "w") as f:
        json.dump(out, f, indent=1)


def summarise(trace_csv, out_csv):
    rows = list(csv.DictReader(open(trace_csv)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    table = []
    for name, match in FAMILIES:
        d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0 for r in rows if match(r["Kernel_Name"])]
        assert len(d) == CALLS * len(SHAPES), (name, len(d))
        for i, (F, N) in enumerate(SHAPES):
            table.append((name, F, N, float(np.median(d[i * CALLS + WARM:(i + 1) * CALLS]))))
    with open(out_csv, "w") as f:
        f.write("kernel,F,N,median_us\n")
        for t in table:
            f.write("%s,%d,%d,%.2f\n" % t)
    for t in table:
        print("%-18s F=%-4d N=%d  %9.2f us" % t)


if sys.argv[1:2] == ["summarise"]:
    summarise(sys.argv[2], sys.argv[3])
else:
    measure(sys.argv[1] if len(sys.argv) > 1 else "events")
