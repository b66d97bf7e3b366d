"""What k_beam_bounds and k_beam_collect (csrc/mcrt_beam.hip) PRODUCE -- every beam's record and candidate list, and the group table, read back with
mcrt_debug_beam_records -- against tests/beam_mirror.py: brute force per ray and per triangle, no tree.  DESIGN.md A.10 "Exact" rests the beams' exactness on
three statements; the bit-identical comparisons of tests/test_gpu_beam*.py see a broken one only where a ray's true hit happens to be the triangle that was
dropped.  Here they are checked as stated:

  bounds        every ray of a beam is inside the record's slope, start-point and size bounds (or within the band of 8 float32 ulps: at most 2 % of a case's
                rays); the record's bounds are the rays' own minima and maxima with the kernel's padding; m = 2^-18 x the record's largest coordinate, which
                is at least 1.0625 x the largest coordinate of the rays and the scene; xref is the near end of the start points; an empty beam has the
                empty-interval record
  refusal       a record is refused exactly when the spread of its rays' slopes exceeds MCRT_BEAM_SPREAD (beams within the band of the cap are skipped and
                counted); a refused record has 0 entries
  completeness  for every certain member, EVERY triangle whose padded bounds its segment crosses (float64 slab rule, no margin) and which begins before
                s_end is in the list
  no garbage    every entry is a triangle the volume test accepts at margin 2 m, carries the scene's vertices of that id bit for bit, and a begin word
                within m / 8 of the recomputation (the kernel's m is 16 x its own rounding); no id twice
  order, cut    begins do not decrease; entries = min(N, capacity) with N counted by the mirror at margins 0.7 m and 1.3 m; s_end is +inf for a complete list, the
                begin of entry `capacity` for a cut one, -inf with 0 entries where N passes 1024 by more than the band
  counters      mcrt_debug_beam_bounce's used / cut / refused are the counts of such records; decided + walked is the bounce's ray count; the rays of
                refused, overflowed and slot-less beams are among the walked, and no more are walked than those, the cut beams' and the band's
  bounces >= 2  every key of the group table is (scan-line, medium, triangle left) of some ray; `claimed` is the number of keys; `lost` the rays without a slot

Method and environment are tests/test_gpu_beam_deep.py's (MCRT_PATH_MAX=0 MCRT_BEAM_B1=2), E = 8, S = 256, ONE debug call of frame 3 -- a single frame, so
k_beam_bounds samples the whole queue --, the bounce under test made the last beamed one with MCRT_BEAM_LAST.  Each case names the record classes it must
contain and fails without them.  mcrt_debug_beam_records refuses every other bounce.

Record classes met and band shares (GPU, this file's print): DESIGN.md A.10, "The argument itself, checked"."""
import numpy as np
import pytest

import beam_mirror as bm
from test_gpu_beam_deep import _context, STAGED

pytestmark = pytest.mark.gpu

# scene, extra knobs, the record classes the case must contain at the named bounces
CASES = {
    "liver": ("liver", {}, {1: {"complete"}, 2: {"complete"}, 3: {"complete"}}),
    "sphere": ("sphere", {}, {1: {"complete"}, 2: {"complete"}, 3: {"complete"}}),
    "sphere_shiny50": ("sphere_shiny50", {}, {1: {"refused", "complete", "codes5"}, 2: {"refused", "complete"}, 3: {"refused", "complete"}}),
    "soup_shiny1000": ("soup_shiny1000", {}, {1: {"refused", "cut", "overflowed", "complete"}, 2: {"refused", "complete"}, 3: {"complete"}}),
    "liver_cap4": ("liver", {"MCRT_BEAM_CAP": 4}, {1: {"cut"}, 2: {"cut"}, 3: {"cut"}}),
}
PLAIN = ("liver", "sphere")      # nothing refused, nothing overflowed
# beam_box in float32 against the mirror's float64: a bound l = lo + min(products) - m takes three roundings, a product's factor s two more, each of at most
# 2^-24 of a magnitude below 3 x the largest coordinate: 6 x 3 x 2^-24 cmax = 0.28 m.  A triangle inside at 0.7 m is a candidate for certain, one outside at 1.3 m is not
N_LO, N_HI = 0.7, 1.3


def _trace(mcrt, name, b):
    scene, extra, _ = CASES[name]
    cfg, sd = bm.scene(mcrt, scene)
    tr = mcrt.Transducer(bm.E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    ctx = _context(mcrt, dict(STAGED, MCRT_BEAM_B1=2, MCRT_BEAM_LAST=b, **extra))
    try:
        ctx.set_params(n_elements=bm.E, n_samples=bm.S, frequency=tr.frequency)
        ctx.upload_scene(sd); ctx.upload_texture(None, 256); ctx.set_transducer(tr.pos, tr.dir)
        with ctx.temp(bm.E * ctx.params.n_rows * 4) as dev:
            hits, segs, cnt = ctx.trace_frame_debug(bm.FRAME, dev, want_segs=True)
            R = ctx.debug_beam_records(b)
            dbg = [ctx.debug_beam_bounce(k) for k in range(b + 2)]
            for other in (b - 1, b + 1):      # the buffers hold the last beamed bounce's: no other is answered
                with pytest.raises(mcrt.McrtError) as refused:
                    ctx.debug_beam_records(other)
                assert refused.value.code == -1 and "bounce %d" % other in str(refused.value)      # MCRT_ERR_INVALID, with a message
        return sd, ctx.params, segs, cnt, R, dbg
    finally:
        ctx.close()


@pytest.mark.parametrize("b", bm.BOUNCES)
@pytest.mark.parametrize("name", list(CASES))
def test_records_and_lists_against_brute_force(mcrt, orc, name, b):
    _check(orc, name, b, *_trace(mcrt, name, b))


def _check(orc, name, b, sd, p, segs, cnt, R, dbg):
    T = sd.n_tri
    pad_abs = orc.OracleScene(sd.tri, sd.tri_mesh, sd.meshes, sd.materials, sd.start_mat, sd.spacing).c.pad_abs
    plo, phi = bm.padded_bounds(sd.tri, pad_abs)
    slo, shi = plo.min(0), phi.max(0)
    index = bm.BoxIndex(plo, phi)
    scene_abs = float(max(np.abs(slo).max(), np.abs(shi).max()))
    tri_words = np.ascontiguousarray(sd.tri, np.float32).reshape(-1, 9).view(np.uint32)
    r = bm.rays_of_bounce(segs, cnt, b, sd.spacing, p.ray_start_offset, p.intensity_epsilon, p.frequency, sd.start_mat, orc.lib().orc_logf)
    ran, decided, walked, n_cut, n_refused, n_used, lost, claimed = dbg[b]
    assert ran and all(dbg[k][0] for k in range(1, b + 1)) and not dbg[b + 1][0]
    assert decided + walked == r.n == int((cnt > b).sum())
    n_beams, cap, near, groups, n_lists = (R[k] for k in ("n_beams", "cap", "near", "groups", "n_lists"))
    recs, lists, keys = R["records"], R["lists"], R["keys"]
    assert recs.shape == (n_beams, bm.REC) and lists.shape == (n_lists, cap, 16) and near == min(512, cap)
    if b == 1:
        assert groups == 0 and n_beams == n_lists == 12 * bm.E
    else:
        assert groups > 0 and groups & (groups - 1) == 0 and n_beams == 6 * groups and keys.shape == (groups,)
        have = set(r.key[r.ok].tolist())
        nz = keys[keys != 0]
        assert set(nz.tolist()) <= have, "a key of the group table belongs to no ray: %r" % [bm.decode_key(k) for k in set(nz.tolist()) - have][:4]
        assert len(set(nz.tolist())) == len(nz) == claimed
    ids = bm.beam_ids(r, keys)
    slotless = int((ids < 0).sum())
    if b >= 2: assert lost == int((r.ok & (ids < 0)).sum())
    cls = np.array([bm.classify(rec) for rec in recs])
    assert not (cls == "bad").any()
    with_rays = np.unique(ids[ids >= 0])
    # a beam without rays: the empty-interval record
    no_rays = np.setdiff1d(np.arange(n_beams), with_rays)
    assert (recs[no_rays] == bm.EMPTY_RECORD).all(), "a beam without rays has a record"
    assert n_used == len(with_rays)

    tol1 = bm.BAND_ULPS * bm.ULP
    met = {"refused": 0, "complete": 0, "cut": 0, "overflowed": 0}
    band_rays = band_beams = missing = 0
    must_walk, may_walk = slotless, slotless
    lists_used = set()
    n_accept = 0
    for bid in with_rays:
        sel = np.flatnonzero(ids == bid)
        code, rec = int(bid % 6), recs[bid]
        raw = bm.raw_bounds(r, sel)
        du, dv = raw[1] - raw[0], raw[3] - raw[2]
        wide = du > bm.SPREAD_CAP + tol1 or dv > bm.SPREAD_CAP + tol1
        narrow = du < bm.SPREAD_CAP - tol1 and dv < bm.SPREAD_CAP - tol1
        if not (wide or narrow):
            band_beams += 1; may_walk += len(sel)
            continue
        # ---- refusal
        if wide:
            assert cls[bid] == "none" and (rec == bm.EMPTY_RECORD).all(), "beam %d of spread %g, %g is not refused" % (bid, du, dv)
            met["refused"] += 1; must_walk += len(sel); may_walk += len(sel)
            continue
        n_accept += 1
        assert cls[bid] != "none", "beam %d of spread %g, %g is refused (lists in use: %d of %d)" % (bid, du, dv, n_accept, n_lists)
        met[cls[bid]] += 1
        # ---- bounds
        G = bm.Geometry.from_record(rec, code)
        G0 = bm.Geometry.from_raw(raw, code, scene_abs)
        inside, outside = G.membership(r, sel)
        assert not outside.any(), "beam %d: %d of its rays lie outside the record's bounds" % (bid, int(outside.sum()))
        band_rays += int((~inside).sum())
        f = rec.view(np.float32)
        assert f[11] == np.float32(f[10]) * np.float32(2.0 ** -18) and G.cmax >= G0.cmax * (1.0 - 4 * bm.ULP), "beam %d: margin %g, largest coordinate %g against %g" % (bid, G.m, G.cmax, G0.cmax)
        assert G.cmax <= G0.cmax * (1.0 + 2.0 ** -10)      # (the scene's part is the tree's root box, which may be a little wider than the triangles' bounds)
        assert G.xref_rec == G.xref and G.list < n_lists and G.entries <= cap and G.list not in lists_used
        lists_used.add(G.list)
        if b == 1: assert G.list == bid
        for got, want in ((G.umin, G0.umin), (G.umax, G0.umax), (G.vmin, G0.vmin), (G.vmax, G0.vmax)):
            assert abs(got - want) <= tol1, "beam %d: a slope bound %r against the rays' padded %r" % (bid, got, want)
        assert np.abs(G.flo - G0.flo).max() <= tol1 * G.cmax and np.abs(G.fhi - G0.fhi).max() <= tol1 * G.cmax
        members = sel[inside]
        if cls[bid] == "overflowed":
            assert G.entries == 0
            must_walk += len(sel); may_walk += len(sel)
        # ---- the candidates the mirror counts: inside the volume at margin N_LO m for certain, at N_HI m at most
        box = bm.volume_box(G, slo, shi, 2.0)
        near_tris = index.query(*box) if box is not None else np.zeros(0, np.int64)
        vol = {mg: near_tris[G.volume(plo[near_tris], phi[near_tris], margin=mg)] for mg in (N_LO, 1.0, N_HI, 2.0)}
        n_lo, n_hi = len(vol[N_LO]), len(vol[N_HI])
        if n_lo > bm.BEAM_EN:
            assert cls[bid] == "overflowed", "beam %d holds %d candidates and is %s" % (bid, n_lo, cls[bid])
        if cls[bid] == "overflowed":
            assert name not in PLAIN
            continue
        # ---- order and cut
        ent = lists[G.list, :G.entries]
        e_ids, e_begin = ent[:, 3].astype(np.int64), ent[:, 7].view(np.float32).astype(np.float64)
        assert min(n_lo, cap) <= G.entries <= min(n_hi, cap), "beam %d: %d entries, the mirror counts %d .. %d candidates" % (bid, G.entries, n_lo, n_hi)
        assert (np.diff(e_begin) >= 0).all(), "beam %d: begins decrease" % bid
        if n_hi <= cap: assert cls[bid] == "complete"
        if n_lo > cap: assert cls[bid] == "cut"
        if cls[bid] == "cut":
            srt = np.sort(G.begin(plo[vol[1.0]], phi[vol[1.0]]))
            lo_k, hi_k = cap - (len(vol[1.0]) - n_lo), min(cap + (n_hi - len(vol[1.0])), len(srt) - 1)      # (the band's candidates may shift the place by as many)
            assert srt[max(lo_k, 0)] - G.m / 8 <= G.s_end <= srt[hi_k] + G.m / 8, "beam %d: s_end %r, the mirror's entry %d begins at %r" % (bid, G.s_end, cap, srt[min(cap, len(srt) - 1)])
            assert G.entries == cap and G.s_end >= e_begin[-1]
            may_walk += len(sel)
        else:
            may_walk += int((~inside).sum())
        # ---- no garbage
        assert (e_ids >= 0).all() and (e_ids < T).all() and len(np.unique(e_ids)) == len(e_ids)
        assert (ent[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]] == tri_words[e_ids]).all(), "beam %d: an entry's vertices are not its triangle's" % bid
        assert (ent[:, 12:16] == 0).all()
        assert G.volume(plo[e_ids], phi[e_ids], margin=2.0).all(), "beam %d: an entry lies outside the volume at 2 m" % bid
        if len(e_ids): assert np.abs(e_begin - G.begin(plo[e_ids], phi[e_ids])).max() <= G.m / 8
        # ---- completeness, per member and per triangle
        if len(members):
            reach = bm.reach_box(r.f2[members], r.D[members], slo, shi)
            cand = index.query(*reach) if reach is not None else np.zeros(0, np.int64)
            cand = cand[G.begin(plo[cand], phi[cand]) < G.s_end - G.m / 8]
            listed = np.isin(cand, e_ids)
            for j in members:
                missing += int((bm.crossed(r.f2[j], r.D[j], plo[cand], phi[cand]) & ~listed).sum())
    share = band_rays / max(r.n, 1)
    print("%s bounce %d: %d rays (%d without a beam), %d beams with rays -- refused %d, complete %d, cut %d, overflowed %d, in the spread band %d; codes %s; "
          "band rays %d (%.2f %%); decided %d, walked %d (at least %d, at most %d); missing (ray, triangle) pairs %d"
          % (name, b, r.n, slotless, len(with_rays), met["refused"], met["complete"], met["cut"], met["overflowed"], band_beams, sorted(set((with_rays % 6).tolist())),
             band_rays, 100.0 * share, decided, walked, must_walk, may_walk, missing))
    assert missing == 0, "%d (ray, triangle) pairs: a triangle a member crosses before s_end is not in its beam's list" % missing
    assert share <= 0.02
    # ---- counters
    assert n_refused == met["refused"] or band_beams, (n_refused, met)
    assert n_cut == met["cut"] + met["overflowed"] or band_beams, (n_cut, met)
    assert met["refused"] <= n_refused <= met["refused"] + band_beams and met["cut"] + met["overflowed"] <= n_cut <= met["cut"] + met["overflowed"] + band_beams
    assert must_walk <= walked <= may_walk, (must_walk, walked, may_walk)
    if name in PLAIN: assert met["refused"] == 0 and n_refused == 0
    # ---- not vacuous
    need = CASES[name][2][b]
    for k in need - {"codes5"}:
        assert met[k] > 0, "the case holds no %s beam at bounce %d" % (k, b)
    if "codes5" in need: assert len(set((with_rays % 6).tolist())) >= 5
