#!/usr/bin/env python3
"""DESIGN 5.12's figures: mcrt_recon_frames with k_recon_splat in its two forms -- one atomic pair per run of equal voxels inside a wavefront
(the default) and, with RECON_FORMS=combined,plain on a library built with tools/variants/recon_splat_plain.patch, one per lane
(MCRT_RECON_PLAIN=1) -- at a user's sizes: 100 frames of 128 x 465 into 128^3 voxels of 1 mm and of 512 x 465 into 256^3 voxels of 0.5 mm, a probe
swept along its elevation with a fan, MEAN and MAX, fill radius 1 and 0 (no hole filling: the resolve pass at its cheapest).  Two contexts
in one process; per leg CALLS calls between two HIP events; a warm-up, then ROUNDS rounds with the legs in alternating order; median and
extremes per call.  The forms' outputs are compared bit for bit in the first round.  A device-to-device copy of the stack in the same
process is the yardstick.

    python tools/recon_measure.py [FILE.csv]        (default profiles/recon/measure.csv)
"""
import csv
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["MCRT_TUNING"] = "1"
import torch  # noqa: E402
import mcray_tracing_amd as mcrt  # noqa: E402

ROUNDS, WARM, CALLS = 7, 3, 5
CASES = [dict(name="128x465_into_128^3_1mm", F=100, E=128, R=465, n=128, pitch=1.0, step_mm=1.0, fan_deg=0.1),
         dict(name="512x465_into_256^3_0.5mm", F=100, E=512, R=465, n=256, pitch=0.5, step_mm=1.0, fan_deg=0.1)]


def context(plain):
    saved = os.environ.get("MCRT_RECON_PLAIN")
    os.environ["MCRT_RECON_PLAIN"] = "1" if plain else "0"
    try:
        return mcrt.Context(0)
    finally:
        if saved is None:
            os.environ.pop("MCRT_RECON_PLAIN", None)
        else:
            os.environ["MCRT_RECON_PLAIN"] = saved


def poses(c):
    """the probe at the origin looking along +y, moved along z in F steps with a fan: (pos, dir) [F][E][3] in cm"""
    tr = mcrt.Transducer(c["E"])
    k = np.arange(c["F"]) - (c["F"] - 1) / 2.0
    tabs = [mcrt.host_transducer_swept(c["E"], tr.radius_cm, tr.separation_mm, (0.0, 0.0, kk * c["step_mm"] / 10.0), (0, 0, 0), float(np.deg2rad(kk * c["fan_deg"])), 30.0) for kk in k]
    return np.stack([t[0] for t in tabs]), np.stack([t[1] for t in tabs])


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "recon", "measure.csv")
    names = os.environ.get("RECON_FORMS", "combined").split(",")
    if not set(names) <= {"combined", "plain"}:
        sys.exit("RECON_FORMS takes combined and plain, got %s" % ",".join(names))
    # only a library built with the variant patch reads MCRT_RECON_PLAIN (the knob's name is in it); any other would time the combined form twice
    if "plain" in names and b"MCRT_RECON_PLAIN" not in open(mcrt._lib._SO, "rb").read():
        sys.exit("%s does not know MCRT_RECON_PLAIN: build it with tools/variants/recon_splat_plain.patch applied (MCRT_LIB names the library)" % mcrt._lib._SO)
    forms = {name: context(name == "plain") for name in names}
    rows = []
    for c in CASES:
        pos, dirs = poses(c)
        n, p = c["n"], c["pitch"]
        row_mm = 150.0 / c["R"]
        g = mcrt.volume_grid((-(n - 1) * p / 2.0, 35.0, -(n - 1) * p / 2.0), (p, 0, 0), (0, p, 0), (0, 0, p), n, n, n)
        rng = np.random.default_rng(1)
        stack = torch.from_numpy(rng.rayleigh(1.0, (c["F"], c["E"], c["R"])).astype(np.float32)).cuda()
        copy = torch.empty_like(stack)
        dpos, ddir = torch.from_numpy(pos).cuda(), torch.from_numpy(dirs).cuda()
        out = torch.empty((n, n, n), dtype=torch.float32, device="cuda")
        cnt = torch.empty((n, n, n), dtype=torch.int32, device="cuda")
        st = torch.zeros(2, dtype=torch.int32, device="cuda")
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        for ctx in forms.values():
            ctx.set_stream(stream.cuda_stream)
        legs = [(form, mode, H) for mode in ("mean", "max") for H in (1, 0) for form in forms]
        times = {leg: [] for leg in legs}
        times[("copy", "-", 0)] = []
        ref = {}

        def call(form, mode, H):
            forms[form].recon_frames(stack.data_ptr(), dpos, ddir, c["F"], c["E"], c["R"], g, out.data_ptr(), count_dev=cnt.data_ptr(), stats_dev=st.data_ptr(), row_mm=row_mm,
                                     mode=mode, fill_radius=H)

        for r in range(WARM + ROUNDS):
            order = legs if r % 2 == 0 else legs[::-1]
            for leg in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(CALLS):
                    call(*leg)
                e1.record(stream)
                e1.synchronize()
                stream.synchronize()
                if r >= WARM:
                    times[leg].append(e0.elapsed_time(e1) / CALLS)
                if r == 0:
                    key = (leg[1], leg[2])
                    got = (out.cpu().numpy().view(np.uint32).copy(), cnt.cpu().numpy().copy(), st.cpu().numpy().copy())
                    ref.setdefault(key, got)
                    assert all(np.array_equal(a, b) for a, b in zip(ref[key], got)), ("the forms differ", leg)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            with torch.cuda.stream(stream):
                for _ in range(CALLS):
                    copy.copy_(stack)
            e1.record(stream)
            e1.synchronize()
            if r >= WARM:
                times[("copy", "-", 0)].append(e0.elapsed_time(e1) / CALLS)
        sampled = int((ref[("mean", 1)][1] > 0).sum())
        samples = c["F"] * c["E"] * c["R"]
        binned = int(ref[("mean", 1)][1].astype(np.int64).sum())
        for leg, t in times.items():
            t = np.array(t)
            rows.append(dict(case=c["name"], form=leg[0], mode=leg[1], fill_radius=leg[2], median_ms=round(float(np.median(t)), 4), min_ms=round(float(t.min()), 4),
                             max_ms=round(float(t.max()), 4), samples=samples, binned=binned, voxels=n ** 3, sampled_voxels=sampled,
                             ns_per_sample=round(float(np.median(t)) * 1e6 / samples, 4)))
            print(rows[-1], flush=True)
    for ctx in forms.values():
        ctx.close()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(rows[0]))
        w.writeheader()
        w.writerows(rows)


if __name__ == "__main__":
    main()
