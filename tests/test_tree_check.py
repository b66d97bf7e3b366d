"""tests/tree_check.py on the CPU: half_out() against the properties that define it, check_tree() against trees with one planted
fault each (a checker that cannot fail checks nothing), and then over the HOST builder's trees -- the padded-bounds contract in
its exact form, at leaves of 1, 4 and 8 triangles, on the scenes tests/test_gpu_tree_structure.py puts through the device code."""
import numpy as np
import pytest

import tree_check as tc

TINY = np.float32(2.0 ** -14)          # the smallest normal half


@pytest.fixture(scope="module")
def scenes(mcrt):
    return tc.all_scenes(mcrt)


# ------------------------------------------------------------------ half_out
def _step(r, up):
    """the storable value next to storable r (float32 holding 0, a normal half or +-inf) on the `up` side: float16's own successor,
    with the subnormals skipped"""
    if not up:
        return -_step(-r, True)
    n = np.nextafter(r.astype(np.float16), np.float16(np.inf)).astype(np.float32)
    n = np.where(r == 0, TINY, n)
    return np.where(r == -TINY, np.float32(0), n).astype(np.float32)


def _half_inputs():
    h = np.arange(1 << 16, dtype=np.uint16).view(np.float16)
    h = h[np.isfinite(h)].astype(np.float32)                      # every finite half, the subnormal ones included
    big = np.float32(3.4e38)
    x = np.concatenate([h, np.nextafter(h, big), np.nextafter(h, -big),
                        np.array([7e4, -7e4, 1e5, -1e5, 65519.9, 65520.0, 1e-8, -1e-8, 3e38, -3e38], np.float32)])
    return np.unique(x[np.isfinite(x)])


@pytest.mark.parametrize("up", [False, True])
def test_half_out_is_the_nearest_storable_value_on_the_outward_side(up):
    x = _half_inputs()
    assert x.size > 180000 and x.dtype == np.float32
    with np.errstate(over="ignore"):
        r = tc.half_out(x, up)
        assert r.dtype == np.float32 and r.shape == x.shape and not np.isnan(r).any()
        assert np.all(r >= x) if up else np.all(r <= x)                                   # the correct side
        assert np.array_equal(r.astype(np.float16).astype(np.float32), r)                 # a half ...
        assert np.all((r == 0) | (np.abs(r) >= TINY))                                     # ... never a subnormal one
        nxt = _step(r, not up)                                                            # one storable step back towards the input
        assert np.all(nxt < x) if up else np.all(nxt > x)                                 # nothing storable strictly between input and result
    for v, dn, u in [(7e4, 65504.0, np.inf), (-2e5, -np.inf, -65504.0), (65519.9, 65504.0, np.inf), (65520.0, 65504.0, np.inf),
                     (65504.0, 65504.0, 65504.0), (1e-8, 0.0, 2.0 ** -14), (-1e-8, -2.0 ** -14, 0.0), (3e-5, 0.0, 2.0 ** -14),
                     (2.0 ** -14, 2.0 ** -14, 2.0 ** -14), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (1.0 + 2.0 ** -20, 1.0, 1.0 + 2.0 ** -10)]:
        assert tc.half_out(np.float32(v), up) == np.float32(u if up else dn), v
    with pytest.raises(ValueError):
        tc.half_out(np.float32(np.nan), up)


# ------------------------------------------------------------------ the checker must be able to fail
def _host_tree(mcrt, sd):
    _, btri, n4, ms = mcrt.host_build_bvh4(sd.tri, sd.tri_mesh)
    return btri, n4, ms


def _parents(rec):
    ref = rec["ref"]
    parent = np.full(len(rec), -1)
    n, k = np.nonzero(ref >= 0)
    parent[ref[n, k]] = n
    return parent


def _as_walked(n4):
    """a host tree as a context would hand it out: every used box rounded outwards to halves"""
    w = n4.copy()
    rec = tc.slots(w)
    live = rec["ref"] != tc.EMPTY
    rec["lo"][live] = tc.half_out(rec["lo"][live], False)
    rec["hi"][live] = tc.half_out(rec["hi"][live], True)
    return w


def test_check_tree_catches_each_planted_fault(mcrt, scenes):
    sd = scenes["sphere"]
    btri, n4, ms = _host_tree(mcrt, sd)
    args = lambda nodes=n4, recs=btri, stack=ms, walked=False: (sd.tri, nodes, recs, stack, walked, 4, sd.tri_mesh)
    st = tc.check_tree(*args())
    assert st["n_tri"] == sd.n_tri and st["need"] == ms and 1 < st["max_leaf"] <= 4
    base = tc.slots(n4)
    ln, lk = np.nonzero((base["ref"] < 0) & (base["ref"] != tc.EMPTY))
    big = np.float32(3e38)

    def planted(match, edit, **kw):
        m = n4.copy()
        edit(tc.slots(m))
        with pytest.raises(tc.TreeError, match=match):
            tc.check_tree(*args(nodes=m, **kw))

    n, k = int(ln[-1]), int(lk[-1])
    def lo_up(rec): rec["lo"][n, k, 1] = np.nextafter(rec["lo"][n, k, 1], big)
    planted(r"box: node %d slot %d axis 1 lo .*too small" % (n, k), lo_up)                         # one lo one ulp up: a box that loses grazing rays
    def hi_up(rec): rec["hi"][n, k, 2] = np.nextafter(rec["hi"][n, k, 2], big)
    planted(r"box: node %d slot %d axis 2 hi .*too large" % (n, k), hi_up)                         # one hi one ulp up: a box that only costs time
    # ... the same two faults in an INNER slot near the root
    i, j = (int(a[0]) for a in np.nonzero(base["ref"][:1] >= 0))
    def in_lo(rec): rec["lo"][i, j, 0] = np.nextafter(rec["lo"][i, j, 0], big)
    planted(r"box: node %d slot %d axis 0 lo .*too small" % (i, j), in_lo)

    cnt = ((~base["ref"][ln, lk]) & 7) + 1
    first = (~base["ref"][ln, lk]) >> 3
    pick = int(np.nonzero((cnt < 4) & (first + cnt < sd.n_tri))[0][0])
    def one_more(rec): rec["ref"][ln[pick], lk[pick]] = ~((~rec["ref"][ln[pick], lk[pick]]) + 1)
    planted(r"leaf: node \d+ slot \d starts at record %d .*overlap" % (first[pick] + cnt[pick]), one_more)    # a leaf count increased by one
    def too_many(rec): rec["ref"][ln[pick], lk[pick]] = ~((~rec["ref"][ln[pick], lk[pick]]) | 7)
    planted(r"leaf: node %d slot %d holds 8 triangles" % (ln[pick], lk[pick]), too_many)

    a, b = 0, len(ln) - 1                                                                           # two leaves far apart: different boxes
    def swapped(rec):
        ra, rb = int(rec["ref"][ln[a], lk[a]]), int(rec["ref"][ln[b], lk[b]])
        rec["ref"][ln[a], lk[a]], rec["ref"][ln[b], lk[b]] = rb, ra
    planted(r"box: node (%d slot %d|%d slot %d) axis \d" % (ln[a], lk[a], ln[b], lk[b]), swapped)                                             # two leaf refs swapped, boxes left in place

    parent = _parents(base)
    deep = int(np.nonzero((parent > 0) & (base["ref"] >= 0).any(axis=1))[0][0])                     # an inner node whose parent is not the root
    kk = int(np.nonzero(base["ref"][deep] >= 0)[0][0])
    def to_ancestor(rec): rec["ref"][deep, kk] = parent[deep]
    planted(r"topology: node %d is referenced 2 times" % parent[deep], to_ancestor)                # an inner ref pointing at an ancestor
    def to_root(rec): rec["ref"][deep, kk] = 0
    planted(r"topology: the root is referenced by node %d slot %d" % (deep, kk), to_root)
    def out_of_range(rec): rec["ref"][deep, kk] = len(rec)
    planted(r"topology: node %d slot %d refers to node %d of %d" % (deep, kk, len(base), len(base)), out_of_range)
    def dirty_empty(rec):
        e = tuple(int(x[0]) for x in np.nonzero(rec["ref"] == tc.EMPTY))
        rec["lo"][e[0], e[1], 0] = 0.0
    if (base["ref"] == tc.EMPTY).any():
        planted(r"topology: unused slot \d of node \d+ does not hold", dirty_empty)

    moved = btri.copy()
    moved[5, 4] = np.nextafter(moved[5, 4], big)
    with pytest.raises(tc.TreeError, match=r"record: record 5 \(triangle \d+\) vertex word 3"):    # one record's vertex changed
        tc.check_tree(*args(recs=moved))
    twice = btri.copy()
    twice[7, 3] = twice[8, 3]
    with pytest.raises(tc.TreeError, match=r"record: triangle \d+ appears in"):
        tc.check_tree(*args(recs=twice))
    mesh = btri.copy()
    mesh.view(np.uint32)[9, 7] ^= 1
    with pytest.raises(tc.TreeError, match=r"record: record 9 \(triangle \d+\) mesh word"):
        tc.check_tree(*args(recs=mesh))

    with pytest.raises(tc.TreeError, match=r"stack: the tree needs %d entries.* reports %d" % (ms, ms - 1)):  # max_stack - 1
        tc.check_tree(*args(stack=ms - 1))

    # as walked: the float boxes themselves are NOT what a context may hand out; their outward halves are; one half step inwards is not
    with pytest.raises(tc.TreeError, match=r"box: "):
        tc.check_tree(*args(walked=True))
    w = _as_walked(n4)
    assert tc.check_tree(*args(nodes=w, walked=True)) == st
    with pytest.raises(tc.TreeError, match=r"box: "):
        tc.check_tree(*args(nodes=w))
    for name, up, why in (("lo", True, "too small"), ("hi", False, "too small"), ("lo", False, "too large"), ("hi", True, "too large")):
        m = w.copy()
        rec = tc.slots(m)
        rec[name][n, k, 0] = _step(rec[name][n, k, 0:1], up)[0]
        with pytest.raises(tc.TreeError, match=r"box: node %d slot %d axis 0 %s .*outward half.*%s" % (n, k, name, why)):
            tc.check_tree(*args(nodes=m, walked=True))


def test_walked_boxes_across_the_half_range_on_the_cpu(mcrt, scenes):
    """the three scenes that leave the half range, rounded as the walk would: the rounded trees pass, and really hold what the GPU test expects
    of them -- +-inf beside +-65504, and 0 / +-2^-14 with nothing in between"""
    for name, want in (("up7e4", (np.inf, 65504.0)), ("down2e5", (-np.inf, -65504.0))):
        sd = scenes[name]
        btri, n4, ms = _host_tree(mcrt, sd)
        w = _as_walked(n4)
        tc.check_tree(sd.tri, w, btri, ms, True, 4, sd.tri_mesh)
        rec = tc.slots(w); live = rec["ref"] != tc.EMPTY
        x = np.concatenate([rec["lo"][live][:, 0], rec["hi"][live][:, 0]])
        assert set(np.unique(x).tolist()) == set(want)
    sd = scenes["tiny"]
    btri, n4, ms = _host_tree(mcrt, sd)
    w = _as_walked(n4)
    tc.check_tree(sd.tri, w, btri, ms, True, 4, sd.tri_mesh)
    rec = tc.slots(w); live = rec["ref"] != tc.EMPTY
    x = np.concatenate([rec["lo"][live].ravel(), rec["hi"][live].ravel()])
    assert (x == 0).any() and (x == TINY).any() and (x == -TINY).any() and not ((x != 0) & (np.abs(x) < TINY)).any()


# ------------------------------------------------------------------ the host builder, in the contract's exact form
@pytest.mark.parametrize("leaf", [1, 4, 8])
def test_host_builder_boxes_equal_the_padded_unions(mcrt, scenes, leaf, monkeypatch):
    monkeypatch.setenv("MCRT_TUNING", "1")
    monkeypatch.setenv("MCRT_SAH_LEAF_MAX", str(leaf))
    if leaf == 8:
        monkeypatch.setenv("MCRT_SAH_COST_TRI", "0.001")
    else:
        monkeypatch.delenv("MCRT_SAH_COST_TRI", raising=False)
    for name, sd in scenes.items():
        btri, n4, ms = _host_tree(mcrt, sd)
        st = tc.check_tree(sd.tri, n4, btri, ms, False, leaf, sd.tri_mesh)
        assert st["max_leaf"] <= leaf and st["n_tri"] == sd.n_tri, name
        assert 0 <= ms <= 64, name
        if leaf == 1:
            assert st["leaves"] == sd.n_tri, name
        if leaf == 8:
            assert st["max_leaf"] >= 5, name                      # leaves of 5..8 triangles really occur, on every scene
