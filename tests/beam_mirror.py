"""numpy reading of the BEAM STAGE (csrc/mcrt_beam.hip; DESIGN.md A.10 "Exact", A.11): what a bounce's rays are, which beam each belongs to,
what a beam's volume is and which triangles a single ray can meet -- written plainly, so that the kernels' records and lists (mcrt_debug_beam_records)
can be checked against brute force per ray and per triangle.  Nothing here walks a tree.

What is mirrored, and where it stands in the kernels:
  rays_of_bounce   csrc/mcrt_device.h:184-195 (ray_len, ray_of: to = from + Ls * spacing * dir, f2 = from + offset * dir), :202-211 (beam_dir, beam_code:
                   D = to - f2, dominant axis, sign, code = 2 axis + sign), csrc/mcrt_beam.hip:72-105 (beam_ray: u, v = D_other / |D_dom|, cmax, the
                   refusal of a ray that is no number, the beam of bounce 1 = (scan-line x 2 + history) x 6 + code, the key of a bounce >= 2 =
                   bit 63 | scan-line << 40 | (medium & 0xff) << 32 | the triangle the ray left).  The rays come from the segments of a debug call: bounce b's
                   from, dir, media, initial_intensity and attenuation (csrc/mcrt_shade.h:153-162 stores them), bounce b - 1's tri.
  padded_bounds    csrc/mcrt_device.h:87-95 (tri_padded_bounds) in float32, as tools/beam_count.py:48-53 has them
  crossed          the contract's slab rule on the padded bounds, in float64 with NO margin: the triangles a ray's segment can be accepted on
  raw_bounds       csrc/mcrt_beam.hip:122-152 (k_beam_bounds: minima and maxima of u, v, f2, cmax over the beam's rays)
  Geometry         csrc/mcrt_beam.hip:310-325 (beam_collect: the padding by a sixteenth of the extent plus 1e-6 on the slopes and m on f2, cmax x 1.0625,
                   m = cmax 2^-18, xref, w, smax) from raw bounds, or read back from a record (:402-404, the layout at :282)
  volume           csrc/mcrt_beam.hip:260-280 (beam_box) in float64, the margin a multiple of m; the begin depth sb0 - m
  membership       csrc/mcrt_beam.hip:436-440 (k_beam_test: a ray is a member where comparisons prove it inside the record's bounds), with the BAND: a ray
                   is `in` only if it is inside by 8 float32 ulps of the compared magnitude, `out` only if outside by as much, `undecided` between.
                   (The ray is rebuilt in float32, operation by operation, so its numbers are the kernel's own up to the device logarithm's last bit;
                   a float64 chain would differ from the kernel's by roundings of |to|, |from| relative to |D|: far more than the 1e-6 by which a beam of
                   parallel rays is padded)
  classify         a record: empty or refused (the slope interval is empty), overflowed (s_end = -inf, 0 entries), cut (s_end finite), complete (+inf)"""
import numpy as np

ULP = 2.0 ** -23
BAND_ULPS = 8.0
REC = 16                     # words of a record (MCRT_DEBUG_BEAM_REC)
SPREAD_CAP = 0.25            # MCRT_BEAM_SPREAD
BEAM_EN = 1024               # candidates a collection holds before it gives up (csrc/mcrt_beam.hip:40)


def padded_bounds(tri, pad_abs):
    """the contract's padded bounds of every triangle, float32 arithmetic, as float64 arrays [T][3] lo, hi"""
    V = np.asarray(tri, np.float32).reshape(-1, 3, 3)
    lo, hi = V.min(1), V.max(1)
    ext = np.maximum(np.float32(0.0), (hi - lo).max(1)).astype(np.float32)
    pad = (np.float32(2e-4) * ext + np.float32(pad_abs)).astype(np.float32)
    return (lo - pad[:, None]).astype(np.float32).astype(np.float64), (hi + pad[:, None]).astype(np.float32).astype(np.float64)


class Rays:
    """the rays of one bounce, one row per live path (arrays of equal length n)"""
    pass


def rays_of_bounce(segs, cnt, b, spacing, offset, eps, freq, start_mat, logf):
    """segs [E][S][B] and cnt [E][S] of a debug call -> the rays of bounce b >= 1.  logf: the contract's float logarithm (orc.lib().orc_logf).
    The ray itself -- Ls, to, f2, D, the slopes -- is rebuilt in float32, one rounding per operation as the kernels are compiled (no contraction):
    the same bits as beam_ray's wherever logf is the device's.  Everything derived from it is float64."""
    f32 = np.float32
    E, S = cnt.shape
    live = cnt > b
    e, s = np.nonzero(live)
    sg = segs[:, :, b][live]
    r = Rays()
    r.n, r.E, r.S, r.b = len(e), E, S, b
    r.scan, r.sample, r.flat = e.astype(np.int64), s.astype(np.int64), (e * S + s).astype(np.int64)
    frm, d = sg["from"].astype(f32), sg["dir"].astype(f32)
    inten, att = sg["initial_intensity"].astype(f32), sg["attenuation"].astype(f32)
    sp = np.asarray(spacing, f32)
    idx = np.arange(r.n)
    with np.errstate(all="ignore"):
        q = (f32(eps) / inten).astype(f32)
        lg = np.array([logf(float(x)) for x in q.tolist()], f32).reshape(q.shape)
        Ls = ((((f32(10.0) * lg).astype(f32) / -att).astype(f32) * f32(freq)).astype(f32) / f32(100.0)).astype(f32)      # ray_len
        to = (frm + (Ls[:, None] * (sp * d).astype(f32)).astype(f32)).astype(f32)                                    # ray_of
        f2 = (frm + (f32(offset) * d).astype(f32)).astype(f32)
        D = (to - f2).astype(f32)                                                                                    # beam_dir
        aD = np.abs(D)
        r.dom = np.where((aD[:, 0] >= aD[:, 1]) & (aD[:, 0] >= aD[:, 2]), 0, np.where(aD[:, 1] >= aD[:, 2], 1, 2))
        dd = D[idx, r.dom]
        r.neg = dd < 0.0
        r.code = (2 * r.dom + r.neg).astype(np.int64)
        ad = np.abs(dd)
        u, v = (D[idx, (r.dom + 1) % 3] / ad).astype(f32), (D[idx, (r.dom + 2) % 3] / ad).astype(f32)                  # beam_ray
        total = np.abs(f2).astype(np.float64).sum(1) + np.abs(to).astype(np.float64).sum(1)
        r.ok = (total < 1e30) & (ad > 0.0) & (np.abs(u) <= 1.0) & (np.abs(v) <= 1.0)
        # a ray whose dominant axis or sign a last-bit difference of logf could change has no certain beam
        srt = np.sort(aD.astype(np.float64), 1)
        r.code_shaky = ~r.ok | (srt[:, 2] - srt[:, 1] <= BAND_ULPS * ULP * srt[:, 2])
    r.Ls, r.to, r.f2, r.D, r.u, r.v = (x.astype(np.float64) for x in (Ls, to, f2, D, u, v))
    r.cmax = np.abs(r.f2).max(1)
    r.mag_u, r.mag_v, r.mag_f2 = np.abs(r.u), np.abs(r.v), np.abs(r.f2)                                             # the compared magnitudes
    r.media = sg["media"].astype(np.int64)
    r.tri = sg["tri"].astype(np.int64)                                   # the triangle bounce b hits (-1: none)
    r.hit_to = sg["to"].astype(np.float64)
    r.left = segs[:, :, b - 1][live]["tri"].astype(np.int64)             # the triangle the ray left
    r.hist = (r.media != int(start_mat)).astype(np.int64)
    r.key = ((1 << 63) | (r.scan.astype(np.uint64) << np.uint64(40)) | ((r.media.astype(np.uint64) & np.uint64(0xff)) << np.uint64(32))
             | (r.left.astype(np.uint64) & np.uint64(0xffffffff))).astype(np.uint64)
    return r


def beam_ids(r, keys=None):
    """the beam of every ray (-1: none): bounce 1 addressed directly, a bounce >= 2 through the group table `keys` (mcrt_debug_beam_records)"""
    if r.b == 1:
        return np.where(r.ok, (r.scan * 2 + r.hist) * 6 + r.code, -1)
    keys = np.asarray(keys, np.uint64)
    slot_of = {int(k): i for i, k in enumerate(keys.tolist()) if k != 0}
    slot = np.array([slot_of.get(int(k), -1) for k in r.key.tolist()], np.int64)
    return np.where(r.ok & (slot >= 0), slot * 6 + r.code, -1)


def group_ids(r):
    """bounces >= 2 without a table: a number per distinct key, then x 6 + code (the kernels' grouping, whatever slots the groups get)"""
    if r.b == 1:
        return beam_ids(r)
    _, g = np.unique(r.key, return_inverse=True)
    return np.where(r.ok, g.astype(np.int64) * 6 + r.code, -1)


def decode_key(key):
    """a non-zero group key -> (scan-line, medium & 0xff, triangle left)"""
    key = int(key)
    return (key >> 40) & 0x7fffff, (key >> 32) & 0xff, key & 0xffffffff


def raw_bounds(r, sel):
    """k_beam_bounds over the rays `sel`: (umin, umax, vmin, vmax, f2 lo [3], f2 hi [3], cmax)"""
    return (r.u[sel].min(), r.u[sel].max(), r.v[sel].min(), r.v[sel].max(), r.f2[sel].min(0), r.f2[sel].max(0), r.cmax[sel].max())


def spread(raw):
    return max(raw[1] - raw[0], raw[3] - raw[2])


class Geometry:
    """a beam's bounds and volume as beam_collect makes them"""

    @staticmethod
    def from_raw(raw, code, scene_abs):
        g = Geometry()
        umin, umax, vmin, vmax, lo, hi, cmax = raw
        g.cmax = max(float(cmax), float(scene_abs)) * 1.0625
        g.m = g.cmax * 2.0 ** -18
        pu, pv = 0.0625 * (umax - umin) + 1e-6, 0.0625 * (vmax - vmin) + 1e-6
        g.umin, g.umax, g.vmin, g.vmax = umin - pu, umax + pu, vmin - pv, vmax + pv
        p = 0.0625 * (hi - lo) + g.m
        g.flo, g.fhi = lo - p, hi + p
        g._finish(code)
        return g

    @staticmethod
    def from_record(rec, code):
        f = np.asarray(rec, np.uint32).view(np.float32).astype(np.float64)
        g = Geometry()
        g.umin, g.umax, g.vmin, g.vmax = f[0], f[1], f[2], f[3]
        g.flo, g.fhi, g.cmax, g.m = f[4:7].copy(), f[7:10].copy(), f[10], f[11]
        g._finish(code)
        g.xref_rec, g.s_end = f[12], f[13]
        g.entries, g.list = int(np.asarray(rec, np.uint32)[14]), int(np.asarray(rec, np.uint32)[15])
        return g

    def _finish(self, code):
        self.dom, self.neg = int(code) >> 1, bool(int(code) & 1)
        self.xref = self.fhi[self.dom] if self.neg else self.flo[self.dom]
        self.w = self.fhi[self.dom] - self.flo[self.dom]
        self.smax = 2.0 * self.cmax + self.m

    def begin(self, plo, phi):
        """the depth at which padded bounds begin, less m (what a list entry carries)"""
        sb0 = (self.xref - phi[:, self.dom]) if self.neg else (plo[:, self.dom] - self.xref)
        return sb0 - self.m

    def volume(self, plo, phi, margin=1.0):
        """beam_box over boxes [n][3]: which come within margin x m of the volume"""
        k, ka, kb, m = self.dom, (self.dom + 1) % 3, (self.dom + 2) % 3, margin * self.m
        sb0 = (self.xref - phi[:, k]) if self.neg else (plo[:, k] - self.xref)
        sb1 = (self.xref - plo[:, k]) if self.neg else (phi[:, k] - self.xref)
        s0, s1 = np.maximum(sb0 - m, -m), np.minimum(sb1 + m, self.smax)
        ok = s0 <= s1
        sa = s0 - self.w
        for smin, smax, lo, hi, ax in ((self.umin, self.umax, self.flo[ka], self.fhi[ka], ka), (self.vmin, self.vmax, self.flo[kb], self.fhi[kb], kb)):
            prod = np.stack([sa * smin, sa * smax, s1 * smin, s1 * smax])
            ok &= (lo + prod.min(0) - m <= phi[:, ax]) & (hi + prod.max(0) + m >= plo[:, ax])
        return ok

    def membership(self, r, sel):
        """rays `sel` against these bounds -> (inside for certain, outside for certain); neither: within the band"""
        band = BAND_ULPS * ULP
        tu, tv, tf = band * r.mag_u[sel], band * r.mag_v[sel], band * r.mag_f2[sel]
        u, v, f2, c = r.u[sel], r.v[sel], r.f2[sel], r.cmax[sel]
        tc = band * np.maximum(c, self.cmax)
        inside = ((u - tu > self.umin) & (u + tu < self.umax) & (v - tv > self.vmin) & (v + tv < self.vmax)
                  & (f2 - tf > self.flo).all(1) & (f2 + tf < self.fhi).all(1) & (c + tc < self.cmax))
        outside = ((u + tu < self.umin) | (u - tu > self.umax) | (v + tv < self.vmin) | (v - tv > self.vmax)
                   | (f2 + tf < self.flo).any(1) | (f2 - tf > self.fhi).any(1) | (c - tc > self.cmax))
        shaky = r.code_shaky[sel]
        return inside & ~shaky, outside & ~shaky


def crossed(f2, D, plo, phi):
    """one ray's segment f2 + t D, 0 <= t <= 1, against boxes [n][3]: the slab rule in float64, no margin -> mask [n]"""
    with np.errstate(all="ignore"):
        t0 = (plo - f2) / D
        t1 = (phi - f2) / D
    par = D == 0.0
    lo_t = np.where(par, -np.inf, np.minimum(t0, t1))
    hi_t = np.where(par, np.inf, np.maximum(t0, t1))
    ok = ~(par & ((f2 < plo) | (f2 > phi))).any(1)
    return ok & (np.maximum(lo_t.max(1), 0.0) <= np.minimum(hi_t.min(1), 1.0))


def reach_box(f2, D, slo, shi):
    """the bounds of the parts of the segments f2 + t D [n][3] that lie inside the box slo .. shi (None: none does).  Every triangle a ray crosses lies inside the
    scene's bounds, so it meets this box: a cheap cut of the triangles before `crossed` is asked per ray, independent of any beam"""
    with np.errstate(all="ignore"):
        t0, t1 = (slo - f2) / D, (shi - f2) / D
    par = D == 0.0
    tin = np.maximum(np.where(par, -np.inf, np.minimum(t0, t1)).max(1), 0.0)
    tout = np.minimum(np.where(par, np.inf, np.maximum(t0, t1)).min(1), 1.0)
    ok = (tin <= tout) & ~(par & ((f2 < slo) | (f2 > shi))).any(1)
    if not ok.any():
        return None
    a, b = f2[ok] + tin[ok, None] * D[ok], f2[ok] + tout[ok, None] * D[ok]
    pad = 1e-9 * np.maximum(np.abs(slo), np.abs(shi)).max()
    return np.minimum(a, b).min(0) - pad, np.maximum(a, b).max(0) + pad


def classify(rec):
    """a record -> 'none' (empty or refused: the slope interval is empty), 'overflowed', 'cut' or 'complete'"""
    f = np.asarray(rec, np.uint32).view(np.float32)
    entries = int(np.asarray(rec, np.uint32)[14])
    if not (f[0] <= f[1] and f[2] <= f[3]):
        return "none"
    if f[13] == -np.inf:
        return "overflowed" if entries == 0 else "bad"
    return "complete" if f[13] == np.inf else "cut" if np.isfinite(f[13]) else "bad"


EMPTY_RECORD = np.array([0x7f800000, 0xff800000, 0x7f800000, 0xff800000] + [0] * 9 + [0xff800000, 0, 0], np.uint32)      # csrc/mcrt_beam.hip:306


# ---- the scenes of tests/test_beam_contract.py and tests/test_gpu_beam_lists.py, built once per process (the 400 000-triangle soup's build dominates its cases)
E, S, FRAME = 8, 256, 3
SCENE_NAMES = ("liver", "sphere", "sphere_shiny50", "soup_shiny1000")
BOUNCES = (1, 2, 3)
_scenes = {}


def scene(mcrt, name):
    """-> (config, SceneData): liver(3), sphere(3), sphere(3) with shininess 50 on every material (wide bundles: beams on five of the six axis / sign codes at
    bounce 1, spreads either side of MCRT_BEAM_SPREAD), the 400 000-triangle soup with shininess 1000 (beams refused, cut at the capacity, and one whose
    collection outgrows its 1024 candidates)"""
    if name not in _scenes:
        s = mcrt.synth
        shiny = lambda v: s.materials({row[0]: {"shininess": v} for row in s._MATERIALS})
        if name == "liver": cfg, meshes = s.liver_scene(3)
        elif name == "sphere": cfg, meshes = s.sphere_scene(3)
        elif name == "sphere_shiny50": cfg, meshes = s.sphere_scene(3); cfg["materials"] = shiny(50)
        elif name == "soup_shiny1000": cfg, meshes = s.random_scene(400000, 8, seed=99); cfg["materials"] = shiny(1000)
        else: raise KeyError(name)
        _scenes[name] = (cfg, mcrt.scene_io.build_scene(cfg, meshes))
    return _scenes[name]


def volume_box(G, slo, shi, margin):
    """bounds that hold every box inside slo .. shi which G.volume accepts at `margin` or less: the volume's own extremes over the depths the scene spans
    (depth range and cross-section are monotone in the range, so a box's test passes only inside them) -- a cheap cut before G.volume is asked"""
    k, ka, kb, m = G.dom, (G.dom + 1) % 3, (G.dom + 2) % 3, margin * G.m
    sb0 = (G.xref - shi[k]) if G.neg else (slo[k] - G.xref)
    sb1 = (G.xref - slo[k]) if G.neg else (shi[k] - G.xref)
    s0, s1 = max(sb0 - m, -m), min(sb1 + m, G.smax)
    if not s0 <= s1:
        return None
    sa = s0 - G.w
    lo, hi = np.empty(3), np.empty(3)
    lo[k], hi[k] = (G.xref - s1 - m, G.xref - s0 + m) if G.neg else (G.xref + s0 - m, G.xref + s1 + m)
    for smin, smax, l, h, ax in ((G.umin, G.umax, G.flo[ka], G.fhi[ka], ka), (G.vmin, G.vmax, G.flo[kb], G.fhi[kb], kb)):
        prod = (sa * smin, sa * smax, s1 * smin, s1 * smax)
        lo[ax], hi[ax] = l + min(prod) - m, h + max(prod) + m
    return lo, hi


def overlapping(plo, phi, lo, hi):
    """indices of the boxes that touch lo .. hi"""
    return np.flatnonzero((plo[:, 0] <= hi[0]) & (plo[:, 1] <= hi[1]) & (plo[:, 2] <= hi[2]) & (phi[:, 0] >= lo[0]) & (phi[:, 1] >= lo[1]) & (phi[:, 2] >= lo[2]))


class BoxIndex:
    """`overlapping` for many queries over many boxes: the boxes sorted by the grid cell of their centre, a query widened by the largest half extent and
    answered from the runs of cells it meets, then by the exact comparison -- the same answer as overlapping(plo, phi, lo, hi), sorted"""

    def __init__(self, plo, phi, cells=32):
        self.plo, self.phi, self.n = plo, phi, cells
        self.cols_lo, self.cols_hi = np.ascontiguousarray(plo.T), np.ascontiguousarray(phi.T)      # (a column at a time: six passes over contiguous memory)
        self.lo = plo.min(0)
        self.size = np.maximum((phi.max(0) - self.lo) / cells, 1e-30)
        self.half = ((phi - plo) * 0.5).max(0)
        c = np.clip(((0.5 * (plo + phi) - self.lo) / self.size).astype(np.int64), 0, cells - 1)
        key = (c[:, 0] * cells + c[:, 1]) * cells + c[:, 2]
        self.order = np.argsort(key, kind="stable")
        self.start = np.searchsorted(key[self.order], np.arange(cells ** 3 + 1))

    def query(self, lo, hi):
        n = self.n
        c0 = np.clip(np.floor((lo - self.half - self.lo) / self.size).astype(np.int64), 0, n - 1)
        c1 = np.clip(np.floor((hi + self.half - self.lo) / self.size).astype(np.int64), 0, n - 1)
        if (c1[0] - c0[0] + 1) * (c1[1] - c0[1] + 1) > 256 or len(self.plo) < 50000:
            return overlapping(self.cols_lo.T, self.cols_hi.T, lo, hi)
        runs = [self.order[self.start[(x * n + y) * n + c0[2]]:self.start[(x * n + y) * n + c1[2] + 1]] for x in range(c0[0], c1[0] + 1) for y in range(c0[1], c1[1] + 1)]
        idx = np.sort(np.concatenate(runs)) if runs else np.zeros(0, np.int64)
        return idx[(self.plo[idx] <= hi).all(1) & (self.phi[idx] >= lo).all(1)]
