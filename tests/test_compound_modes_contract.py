"""The compounding modes without a GPU (include/mcrt.h: mcrt_compound_opts, mcrt_compound_weights): the struct, the host weight map against
tests/compound_modes_mirror.py bit for bit, its errors, identities of the mirror, the seam a feathered mean removes as a fact of the
contract, and k_compound's resource lines."""
import ctypes as C
import math
import os
import re
import subprocess
import numpy as np
import pytest

import compound_mirror as cm
import compound_modes_mirror as mm
import image_cases as ic

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRIES = ic.SCAN_GEOMETRIES + [(30.0, math.pi / 3, 33, 35)]
STEERS = (0.0, 0.3, -0.3, 0.5)


def maps_of(mcrt, E, R, steers, geom):
    radius, angle, rows, cols = geom
    return [mcrt.host_compound_maps(E, R, s, radius, angle, out_rows=rows, out_cols=cols) for s in steers]


# ------------------------------------------------------------------ the struct
def test_struct_layout_and_defaults(mcrt):
    O = mcrt.CompoundOpts
    assert C.sizeof(O) == 72 and O.mode.offset == 0 and O.feather_lines.offset == 4 and O.view_weight.offset == 8 and O.view_weight.size == 64
    assert C.sizeof(mcrt.Compound) == 68                                   # mcrt_compound is as it was
    o = O(); o.mode = 7; o.feather_lines = 3.0
    L = mcrt.load_library()
    assert L.mcrt_default_compound_opts(C.byref(o)) == 0
    assert o.mode == 0 and o.feather_lines == 0.0 and list(o.view_weight) == [1.0] * 16
    assert L.mcrt_default_compound_opts(None) == -1
    assert L.mcrt_version() == 109
    o = mcrt.compound_opts_struct("median", (0.5, 0.0, 2.0), 2.5)
    assert (o.mode, o.feather_lines) == (2, 2.5) and list(o.view_weight) == [0.5, 0.0, 2.0] + [1.0] * 13
    assert mcrt.compound_opts_struct("max").mode == 1 and mcrt.compound_opts_struct().mode == 0
    with pytest.raises(ValueError):
        mcrt.compound_opts_struct(view_weights=[1.0] * 17)


# ------------------------------------------------------------------ mcrt_compound_weights
@pytest.mark.parametrize("gi", range(len(GEOMETRIES)))
def test_weights_equal_the_mirror(mcrt, gi):
    """divide, min, max and multiply only: bit for bit.  0 exactly where the view does not contribute (the NaN holes of (20 mm, 3.6 rad) at
    steer 0.5 included), view_weight where feather_lines <= mx <= E-1-feather_lines on a covered pixel"""
    geom = GEOMETRIES[gi]
    radius, angle, rows, cols = geom
    holes = 0
    for E, R in ic.SCAN_SHAPES:
        for steer in STEERS:
            mr, mc = mcrt.host_compound_maps(E, R, steer, radius, angle, out_rows=rows, out_cols=cols)
            cov = cm.covered(cm.remap_point(mc, mr), E, R)
            for vw, fl in ((1.0, 0.0), (0.75, 2.5), (3.0, 16.0), (0.0, 2.5)):
                got = mcrt.host_compound_weights(E, R, steer, vw, fl, radius, angle, out_rows=rows, out_cols=cols)
                ic.assert_same_bits(got, mm.weight_map(mr, mc, E, R, vw, fl), "geometry %s shape %s steer %g weight %g feather %g" % (geom, (E, R), steer, vw, fl))
                assert np.all(got[~cov] == 0) and not np.signbit(got).any()
                assert np.all(got[np.isnan(mc)] == 0)
                with np.errstate(invalid="ignore"):
                    flat = cov & (mc >= f32(fl)) & (mc <= f32(f32(E - 1) - f32(fl)))
                assert np.all(got[flat] == f32(vw))
                if fl > 0:
                    with np.errstate(invalid="ignore"):
                        assert np.all(got[(mc <= 0) | (mc >= f32(E - 1))] == 0)                     # the half-covered rim is gone
                    if E == 1:
                        assert not got.any()                                                         # one scan-line, feathered: black
                else:
                    assert np.array_equal(got != 0, cov & (vw > 0))
            holes += int(np.isnan(mc).sum())
    if geom[:2] == (20.0, 3.6):
        assert holes > 0


def test_weights_errors(mcrt):
    L = mcrt.load_library()
    w = np.full((20, 24), -7.25, f32)
    p = w.ctypes.data_as(C.c_void_p)

    def call(E=16, R=40, radius=30.0, angle=1.0, rows=20, cols=24, steer=0.1, vw=1.0, fl=2.0, out=p):
        return L.mcrt_compound_weights(E, R, radius, angle, 100, 1500, rows, cols, steer, vw, fl, out)

    for kw, word in ((dict(out=None), b"null"), (dict(E=0), b""), (dict(R=0), b""), (dict(rows=0), b""), (dict(cols=0), b""), (dict(angle=0.0), b""),
                     (dict(steer=math.nan), b"steer"), (dict(steer=1.6), b"steer"), (dict(vw=-0.5), b"view_weight"), (dict(vw=math.nan), b"view_weight"),
                     (dict(vw=math.inf), b"view_weight"), (dict(fl=-1.0), b"feather_lines"), (dict(fl=math.nan), b"feather_lines"), (dict(fl=math.inf), b"feather_lines")):
        assert call(**kw) == -1, kw
        assert word in L.mcrt_last_error(), (kw, L.mcrt_last_error())
        assert np.all(w == f32(-7.25)), kw
    assert call() == 0 and w.max() == 1.0 and w.min() == 0.0


# ------------------------------------------------------------------ identities of the mirror
def test_mirror_identities(mcrt):
    E, R = 37, 211
    geom = ic.SCAN_GEOMETRIES[3]                        # (20 mm, 3.6 rad): pixels with 0, 1, 2 and 3 contributing views
    steers = (0.5, 0.0, -0.4)
    maps = maps_of(mcrt, E, R, steers, geom)
    st = np.stack([ic.scan_image(E, R, seed=n) for n in range(3)])
    st.reshape(-1)[::61] = -0.0
    for weights, fl in ((None, 0.0), ((2.0, 2.0, 2.0), 0.0)):
        mean, cnt = mm.compound(st, maps, "mean", weights, fl)
        med, c2 = mm.compound(st, maps, "median", weights, fl)
        mx, c3 = mm.compound(st, maps, "max", weights, fl)
        assert np.array_equal(cnt, c2) and np.array_equal(cnt, c3)
        assert all((cnt == k).sum() > 20 for k in (0, 1, 2, 3))
        if weights is None:
            ic.assert_same_bits(mean, cm.compound(st, maps)[0], "defaults are the plain mean")
            ic.assert_same_bits(med[cnt <= 2], mean[cnt <= 2], "median == mean up to two views")
        else:                                           # equal weights w: (w a + w b) / (2 w) against (a + b) * 0.5 -- equal where nothing overflows or goes subnormal
            ok = (cnt <= 2) & np.isfinite(mean) & (np.abs(mean) > 1e-30)
            ic.assert_same_bits(med[ok], mean[ok], "median == weighted mean up to two views")
        ic.assert_same_bits(mx[cnt == 1], mean[cnt == 1] if weights is None else med[cnt == 1], "max == mean with one view")
    perm = (2, 0, 1)
    for mode in ("median", "max"):
        a = mm.compound(st, maps, mode, (1.0, 0.5, 2.0), 2.5)[0]
        b = mm.compound(st[list(perm)], [maps[i] for i in perm], mode, [(1.0, 0.5, 2.0)[i] for i in perm], 2.5)[0]
        ic.assert_same_bits(a, b, mode + " under a permutation of the views")
    # a NaN look makes max and median NaN; no contributing view gives +0.0
    med = mm.compound(st, maps, "median")[0]
    assert np.isnan(med).any() and np.all(med[cnt == 0] == 0) and not np.signbit(med[cnt == 0]).any()


# ------------------------------------------------------------------ the seam
def test_the_seam_and_its_removal(mcrt):
    """Constant views 1, 2, 3 at steers (0, 0.3, -0.3), 128 x 465 -> 400 x 500.  Over horizontally neighbouring pixel pairs on which the unsteered
    view has weight 1 at feather_lines = 16 and 0 <= my <= R-1-16: the plain mean steps by more than 0.5 where a steered view's lateral edge
    crosses; feathered with 16 lines the largest step is at most (cmax - cmin) * max over the pairs of sum_n |dw_n| (wsum >= 1 there: the
    compound is a convex combination whose coefficients move by at most sum |dw| / wsum), which the test computes from the weight maps and
    which must be below 0.25."""
    E, R, FL = 128, 465, 16.0
    steers = (0.0, 0.3, -0.3)
    consts = (1.0, 2.0, 3.0)
    geom = ic.SCAN_GEOMETRIES[0]
    maps = maps_of(mcrt, E, R, steers, geom)
    st = np.stack([np.full((E, R), c, f32) for c in consts])
    w = [mcrt.host_compound_weights(E, R, s, 1.0, FL) for s in steers]
    my0 = maps[0][0]
    inside = (w[0] == 1) & (my0 >= 0) & (my0 <= f32(R - 1 - 16))
    pair = inside[:, :-1] & inside[:, 1:]
    assert pair.sum() > 50000
    plain = mm.compound(st, maps, "mean")[0]
    soft = mm.compound(st, maps, "mean", None, FL)[0]
    step = lambda img: np.abs(np.diff(img.astype(np.float64), axis=1))[pair].max()
    dw = sum(np.abs(np.diff(x.astype(np.float64), axis=1)) for x in w)[pair].max()
    bound = (max(consts) - min(consts)) * dw
    print("seam: plain step %.4f, feathered step %.4f, bound %.4f" % (step(plain), step(soft), bound))
    assert step(plain) > 0.5
    assert bound < 0.25
    assert step(soft) <= bound


# ------------------------------------------------------------------ the kernel's resources
def test_k_compound_resources():
    """Every k_compound instantiation: no scratch, no spilled vector register.  The three instantiations of the plain mean (MODE 0) are
    there with no more vector registers than before the modes were added: 75 (float), 89 (8-bit, word stores), 81 (8-bit, byte stores)."""
    pkg = os.path.join(ROOT, "mcray-tracing_amd")
    out = subprocess.run(["make", "-C", pkg, "resources"], capture_output=True, text=True).stderr
    blocks = [b for b in out.split("Function Name: ") if b.startswith("_ZN4mcrt10k_compoundI")]
    val = lambda b, key: int(re.search(key + r": (\d+)", b).group(1))
    names = [b.split()[0] for b in blocks]
    assert len(blocks) == 18 and len(set(names)) == 18, names                 # {float, word, byte} x {plain, weighted, max, median x 3 buckets}
    for b in blocks:
        assert val(b, r"ScratchSize \[bytes/lane\]") == 0 and val(b, "VGPRs Spill") == 0, b[:900]
    for args, vgprs in (("ILb0ELb0ELi0ELi0EEE", 75), ("ILb1ELb1ELi0ELi0EEE", 89), ("ILb1ELb0ELi0ELi0EEE", 81)):
        found = [b for b in blocks if b.startswith("_ZN4mcrt10k_compound" + args)]
        assert len(found) == 1, (args, names)
        assert val(found[0], "VGPRs") <= vgprs, found[0][:900]
