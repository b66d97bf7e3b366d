"""Structural checks of the BVH4 the walk reads (numpy only; a helper module, not a conftest).

The closest-hit contract makes every image independent of the hierarchy under ONE property: each child box
contains the padded bounds of every triangle below it, and every triangle is reachable exactly once.  check_tree() asserts
that property in its exact form -- a slot's box EQUALS the union of its triangles' padded bounds (rounded outwards to
halves for a tree as walked) -- so a box one ulp short (a wrong image for a grazing ray) and a box one ulp wide (a silent
slowdown) both fail, on the node that has it, without a ray having to find it.

half_out() is the specification of the walk's half-float rounding, written from its description: the result is the
nearest member, on the outward side, of the set the walk may store -- zero, the NORMAL halves and +-infinity."""
import copy

import numpy as np

EMPTY = -2 ** 31                      # MCRT_BVH4_EMPTY
CHILD = np.dtype([("lo", "<f4", 3), ("hi", "<f4", 3), ("ref", "<i4"), ("pad", "<u4")])      # mcrt_bvh4_child, four per 128-byte node
VERT_COLS = [0, 1, 2, 4, 5, 6, 8, 9, 10]                                                     # v0 | id, v1 | mesh, v2 | 0


class TreeError(AssertionError):
    pass


def _allowed_halves():
    """every value a walked box may hold, ascending: -inf, the normal halves, 0, +inf (no subnormal, no NaN)"""
    h = np.arange(1 << 16, dtype=np.uint16).view(np.float16)
    keep = ~np.isnan(h) & ((h == 0) | np.isinf(h) | (np.abs(h.astype(np.float32)) >= np.float32(2.0 ** -14)))
    return np.unique(h[keep].astype(np.float32))          # (+-0 collapse to one zero)


_HALVES = _allowed_halves()


def half_out(x, up):
    """float32 -> the walk's half, as float32.  up=False: the largest storable value <= x; up=True: the smallest >= x.
    Storable: 0, +-[2^-14, 65504] in half steps, +-inf.  So a value inside (0, 2^-14) goes down to 0 and up to 2^-14 (the
    subnormal halves snapped outwards), 7e4 goes up to +inf and down to 65504, -2e5 goes down to -inf and up to -65504.
    A zero result is +0 (callers compare zeros as values)."""
    x = np.asarray(x, np.float32)
    if np.isnan(x).any():
        raise ValueError("half_out: NaN")
    if up:
        return _HALVES[np.searchsorted(_HALVES, x, side="left")]
    return _HALVES[np.searchsorted(_HALVES, x, side="right") - 1]


def pad_abs_of(tri):
    """4e-6f * max(largest finite |coordinate|, 1e-3f), in float32 (mcrt_build_bvh / k_pad)"""
    a = np.abs(np.asarray(tri, np.float32)).ravel()
    a = a[np.isfinite(a)]
    scale = a.max() if a.size else np.float32(0)
    return np.float32(4e-6) * np.maximum(np.float32(scale), np.float32(1e-3))


def padded_bounds(tri):
    """[T,9] float32 -> (lo [T,3], hi [T,3]): the contract's padded bounds of every triangle, one float32 rounding per operation:
    pad = 2e-4f * (largest extent) + pad_abs;  lo = min - pad;  hi = max + pad"""
    v = np.asarray(tri, np.float32).reshape(-1, 3, 3)
    l, h = v.min(axis=1), v.max(axis=1)
    ext = np.maximum(np.float32(0), (h - l).max(axis=1))
    pad = (np.float32(2e-4) * ext).astype(np.float32) + pad_abs_of(tri)
    return (l - pad[:, None]).astype(np.float32), (h + pad[:, None]).astype(np.float32)


def _bits(a):
    """float32 -> uint32 bit patterns with -0 folded onto +0 (the two zeros are the same plane)"""
    return (np.ascontiguousarray(a, np.float32) + np.float32(0)).view(np.uint32)


def _first(mask):
    return tuple(int(i) for i in np.argwhere(mask)[0])


def slots(nodes4):
    """the 128-byte nodes as a [N,4] record array of children"""
    return np.ascontiguousarray(nodes4).view(np.uint8).reshape(-1, 128).view(CHILD).reshape(-1, 4)


def check_tree(tri, nodes4, btri, max_stack, walked, leaf_max, tri_mesh):
    """tri [T,9]: the uploaded vertices; nodes4: the 128-byte nodes of get_bvh4() / host_build_bvh4(); btri [T,12]: the leaf-order
    records of get_bvh(); max_stack: the reported stack bound; walked: the boxes are the walk's halves (a context's tree) rather than
    the builder's floats; leaf_max: the largest leaf the builder may make; tri_mesh [T]: the uploaded mesh words.
    Raises TreeError naming the first offending node / slot / axis.  Returns what it counted."""
    tri = np.ascontiguousarray(tri, np.float32).reshape(-1, 9)
    btri = np.ascontiguousarray(btri, np.float32).reshape(-1, 12)
    T = tri.shape[0]
    rec = slots(nodes4)
    N = rec.shape[0]
    ref = rec["ref"]
    if N == 0:
        raise TreeError("topology: no nodes")
    empty, inner = ref == EMPTY, ref >= 0
    leaf = ~empty & ~inner
    used = (~empty).sum(axis=1)

    # ---- 1. topology
    if (used == 0).any():
        raise TreeError("topology: node %d has no used slot" % _first(used == 0))
    if (inner & (ref >= N)).any():
        n, k = _first(inner & (ref >= N))
        raise TreeError("topology: node %d slot %d refers to node %d of %d" % (n, k, ref[n, k], N))
    times = np.bincount(ref[inner], minlength=N)
    if times[0]:
        n, k = _first(inner & (ref == 0))
        raise TreeError("topology: the root is referenced by node %d slot %d" % (n, k))
    if (times[1:] != 1).any():
        n = 1 + _first(times[1:] != 1)[0]
        raise TreeError("topology: node %d is referenced %d times" % (n, times[n]))
    depth = np.full(N, -1, np.int64)
    depth[0] = 0
    front, d = np.zeros(1, np.int64), 0
    while front.size:                            # one pass per LEVEL: with one parent per node nothing is met twice
        d += 1
        r = ref[front]
        front = r[r >= 0].astype(np.int64)
        depth[front] = d
    if (depth < 0).any():
        raise TreeError("topology: node %d is not reached from the root" % _first(depth < 0))
    inf = np.float32(np.inf)
    bad = empty[..., None] & ((rec["lo"] != inf) | (rec["hi"] != -inf))
    if bad.any():
        n, k, a = _first(bad)
        raise TreeError("topology: unused slot %d of node %d does not hold the +inf/-inf box (axis %d: %r, %r)" % (k, n, a, rec["lo"][n, k, a], rec["hi"][n, k, a]))

    # ---- 2. leaves and records
    ln, lk = np.nonzero(leaf)
    v = (~ref[ln, lk]).astype(np.int64) & 0xFFFFFFFF
    first, count = v >> 3, (v & 7) + 1
    if (count > leaf_max).any():
        i = _first(count > leaf_max)[0]
        raise TreeError("leaf: node %d slot %d holds %d triangles, the builder's limit is %d" % (ln[i], lk[i], count[i], leaf_max))
    if (first + count > T).any():
        i = _first(first + count > T)[0]
        raise TreeError("leaf: node %d slot %d covers records %d..%d of %d" % (ln[i], lk[i], first[i], first[i] + count[i] - 1, T))
    order = np.argsort(first, kind="stable")
    ln, lk, first, count = ln[order], lk[order], first[order], count[order]
    start = np.concatenate([[0], (first + count)[:-1]])
    if (first != start).any():
        i = _first(first != start)[0]
        raise TreeError("leaf: node %d slot %d starts at record %d where the ranges before it end at %d (a gap or an overlap)" % (ln[i], lk[i], first[i], start[i]))
    if first.size == 0 or first[-1] + count[-1] != T:
        raise TreeError("leaf: the ranges end at record %d of %d" % (0 if first.size == 0 else first[-1] + count[-1], T))
    if btri.shape[0] != T:
        raise TreeError("record: %d records for %d triangles" % (btri.shape[0], T))
    ids = btri[:, 3].copy().view(np.uint32).astype(np.int64)
    if (ids >= T).any():
        raise TreeError("record: record %d carries id %d of %d" % (_first(ids >= T)[0], ids[_first(ids >= T)[0]], T))
    seen = np.bincount(ids, minlength=T)
    if (seen != 1).any():
        raise TreeError("record: triangle %d appears in %d records" % (_first(seen != 1)[0], seen[_first(seen != 1)[0]]))
    bad = btri[:, VERT_COLS].view(np.uint32) != tri[ids].view(np.uint32)
    if bad.any():
        r, c = _first(bad)
        raise TreeError("record: record %d (triangle %d) vertex word %d is %r, uploaded %r" % (r, ids[r], c, btri[r, VERT_COLS[c]], tri[ids[r], c]))
    words = btri.view(np.uint32)
    tm = np.ascontiguousarray(tri_mesh, np.uint32)
    if tm.shape != (T,):
        raise TreeError("record: %d mesh words for %d triangles" % (tm.size, T))
    if (words[:, 7] != tm[ids]).any():
        r = _first(words[:, 7] != tm[ids])[0]
        raise TreeError("record: record %d (triangle %d) mesh word is %d, uploaded %d" % (r, ids[r], words[r, 7], tm[ids[r]]))
    if (words[:, 11] != 0).any():
        raise TreeError("record: record %d last word is 0x%x, not 0" % (_first(words[:, 11] != 0)[0], words[_first(words[:, 11] != 0)[0], 11]))

    # ---- 3. boxes (exact) and 4. the stack bound, level by level from the deepest
    plo, phi = padded_bounds(tri)
    plo, phi = plo[ids], phi[ids]                                   # in record order
    owner = np.repeat(np.arange(first.size), count)                 # record -> its leaf (the ranges are a partition in order)
    leaf_lo = np.full((first.size, 3), inf, np.float32); leaf_hi = np.full((first.size, 3), -inf, np.float32)
    np.minimum.at(leaf_lo, owner, plo)
    np.maximum.at(leaf_hi, owner, phi)
    want_lo = np.full((N, 4, 3), inf, np.float32); want_hi = np.full((N, 4, 3), -inf, np.float32)
    want_lo[ln, lk], want_hi[ln, lk] = leaf_lo, leaf_hi
    node_lo = np.empty((N, 3), np.float32); node_hi = np.empty((N, 3), np.float32)
    need = np.zeros(N, np.int64)
    by_depth = np.argsort(depth, kind="stable")
    cut = np.searchsorted(depth[by_depth], np.arange(depth.max() + 2))
    for d in range(int(depth.max()), -1, -1):
        nd = by_depth[cut[d]:cut[d + 1]]
        r = ref[nd]
        rows, cols = np.nonzero(r >= 0)
        kids = r[rows, cols]
        want_lo[nd[rows], cols], want_hi[nd[rows], cols] = node_lo[kids], node_hi[kids]
        below = np.zeros(r.shape, np.int64)
        below[rows, cols] = need[kids]
        node_lo[nd], node_hi[nd] = want_lo[nd].min(axis=1), want_hi[nd].max(axis=1)      # (unused slots are the neutral +inf/-inf)
        need[nd] = used[nd] - 1 + below.max(axis=1)
    if walked:
        want_lo, want_hi = half_out(want_lo, False), half_out(want_hi, True)
    live = ~empty[..., None]
    for name, got in (("lo", rec["lo"]), ("hi", rec["hi"])):
        if np.isnan(got).any():
            n, k, a = _first(np.isnan(got))
            raise TreeError("box: node %d slot %d axis %d %s is NaN" % (n, k, a, name))
    bad = np.stack([live & (_bits(rec["lo"]) != _bits(want_lo)), live & (_bits(rec["hi"]) != _bits(want_hi))], axis=-1)      # [N,4,3,lo|hi]
    if bad.any():
        # the first offender in the order the boxes were derived, from the deepest level: a fault low in the tree also shows in every
        # ancestor's union, and the slot to look at is the one it starts in
        at = np.nonzero(bad.reshape(N, -1).any(axis=1))[0]
        n = int(at[np.argmax(depth[at])])
        k, a, h = _first(bad[n])
        name, got, want = ("lo", rec["lo"], want_lo) if h == 0 else ("hi", rec["hi"], want_hi)
        raise TreeError("box: node %d slot %d axis %d %s is %r, the %sunion of the padded bounds below it is %r (%s)" % (
            n, k, a, name, got[n, k, a], "outward half of the " if walked else "", want[n, k, a],
            "too small" if (got[n, k, a] > want[n, k, a]) == (name == "lo") else "too large"))
    if int(need[0]) != int(max_stack):
        raise TreeError("stack: the tree needs %d entries (used slots - 1 per node down the hungriest path), max_stack reports %d" % (need[0], max_stack))
    return {"n_nodes": int(N), "n_tri": int(T), "depth": int(depth.max()) + 1, "max_leaf": int(count.max()), "leaves": int(first.size),
            "leaf_hist": np.bincount(count, minlength=9)[1:].tolist(), "need": int(need[0])}


# ------------------------------------------------------------------ the scenes both test files build trees of
def with_triangles(sd, tri, tri_mesh=None):
    """a copy of scene `sd` over other triangles (same tables)"""
    out = copy.copy(sd)
    out.tri = np.ascontiguousarray(tri, np.float32).reshape(-1, 9)
    out.tri_mesh = np.ascontiguousarray(sd.tri_mesh[:out.tri.shape[0]] if tri_mesh is None else tri_mesh, np.uint32)
    assert out.tri_mesh.shape[0] == out.tri.shape[0]
    return out


def shifted(tri, dx):
    t = np.asarray(tri, np.float32).reshape(-1, 3, 3).copy()
    t[:, :, 0] += np.float32(dx)
    return t.reshape(-1, 9)


def scaled(tri, s):
    return (np.asarray(tri, np.float32) * np.float32(s)).astype(np.float32)


def flattened(tri, axis=0):
    t = np.asarray(tri, np.float32).reshape(-1, 3, 3).copy()
    t[:, :, axis] = 0.0
    return t.reshape(-1, 9)


def smooth(tri):
    """a smooth deformation that keeps the spatial order roughly intact"""
    t = np.asarray(tri, np.float32).reshape(-1, 3, 3).copy()
    t[:, :, 2] += (0.25 * np.cos(0.7 * t[:, :, 0]) + 0.1 * t[:, :, 1]).astype(np.float32)
    return t.reshape(-1, 9).astype(np.float32)


HALF_BIG_UP, HALF_BIG_DOWN, HALF_TINY = 7.0e4, -2.0e5, 1.0e-5      # across the half range: beyond +-65504, and inside +-2^-14


def all_scenes(mcrt):
    """name -> scene: sphere (sphere_scene(3): T = 1292, not a multiple of 64), liver (liver_scene(3), the level the GPU parity tests use:
    T = 14080), the 100 k soup, and the edge scenes"""
    out = {}
    for name, (cfg, meshes) in (("sphere", mcrt.synth.sphere_scene(3)), ("liver", mcrt.synth.liver_scene(3)),
                                ("soup", mcrt.synth.random_scene(100000, 8, seed=99))):
        out[name] = mcrt.scene_io.build_scene(cfg, meshes)
    out.update(edge_scenes(out["sphere"]))
    return out


def edge_scenes(sphere_sd):
    """name -> scene: the shapes where a bottom-up fit or the half rounding can go wrong, all made of the sphere scene's triangles"""
    s = sphere_sd
    one = s.tri[s.n_tri // 2:s.n_tri // 2 + 1]
    m1 = s.tri_mesh[s.n_tri // 2:s.n_tri // 2 + 1]
    return {
        "twice": with_triangles(s, np.concatenate([s.tri, s.tri]), np.concatenate([s.tri_mesh, s.tri_mesh])),     # every Morton code ties
        "copies64": with_triangles(s, np.repeat(one, 64, 0), np.repeat(m1, 64)),                                   # centroid extent 0 on every axis
        "copies257": with_triangles(s, np.repeat(one, 257, 0), np.repeat(m1, 257)),
        "flat": with_triangles(s, flattened(s.tri, 0), s.tri_mesh),
        "t8": with_triangles(s, s.tri[-8:], s.tri_mesh[-8:]),                                                      # the device builder's minimum
        "t9": with_triangles(s, s.tri[-9:], s.tri_mesh[-9:]),
        "up7e4": with_triangles(s, shifted(s.tri, HALF_BIG_UP), s.tri_mesh),                                       # halves overflow to +inf / stop at 65504
        "down2e5": with_triangles(s, shifted(s.tri, HALF_BIG_DOWN), s.tri_mesh),
        "tiny": with_triangles(s, scaled(s.tri, HALF_TINY), s.tri_mesh),                                           # boxes inside +-2^-14
    }
