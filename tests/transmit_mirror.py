"""numpy mirror of the acoustic ground truth (include/mcrt.h: mcrt_transmit_frames, mcrt_transmit_boundary): the header's specification restated
in np.float32 / float64.  The walk is tests/label_mirror.py's -- the closest hit is OracleScene.closest_hit (the contract's own, brute force
over the triangles), the constants orc.constants, the TRACED medium update label_mirror.update_traced --; on top of it the beam carries the
tracer's intensity: the attenuation of every segment through the contract's expf (orc.lib().orc_expf), the impedance rule at every boundary
(boundary(), written out here).  The scenes are label_mirror's."""
import math
import numpy as np

import label_mirror as lm

f32 = np.float32
TOTAL, BOUNDARIES = 0, 1
M_IMP, M_ATT = 0, 1           # columns of a material row: impedance, attenuation


def boundary(z1, z2, inc, ia):
    """mcrt_transmit_boundary in float32, every operation rounded on its own -> (i_refl, i_refr)"""
    z1, z2, inc, ia = f32(z1), f32(z2), f32(inc), f32(ia)
    with np.errstate(all="ignore"):
        rr = f32(z1 / z2)
        refa = f32(f32(1) - f32(f32(rr * rr) * f32(f32(1) - f32(inc * inc))))
        if refa < 0:
            return ia, f32(0)
        refa = f32(np.sqrt(refa))
        num = f32(f32(z1 * inc) - f32(z2 * refa))
        den = f32(f32(z1 * inc) + f32(z2 * refa))
        qq = f32(num / den)
        i_refl = f32(np.float64(ia) * (np.float64(qq) * np.float64(qq)))
        return i_refl, f32(ia - i_refl)


def dot(a, b):
    return f32(f32(f32(a[0] * b[0]) + f32(a[1] * b[1])) + f32(a[2] * b[2]))


def attenuated(expf, intensity, att, mm, freq):
    """intensity * expf(-att * ((float)mm * 0.01f) * freq): the tracer's attenuation over mm millimetres (a double)"""
    with np.errstate(all="ignore"):
        x = f32(f32(-att * f32(f32(mm) * f32(0.01))) * freq)
        return f32(intensity * f32(expf(float(x))))


def walk(osc, orc, pos, direction, n_rows, mode=TOTAL, rule=lm.TRACED, offs=0.1, frequency=4.5, sos=1500, depth_cm=15.0, cap=lm.MAX_CROSSINGS,
         detail=None):
    """one scan-line -> (transmit float32 [R], reflect float32 [R], crossings); detail: a list that receives (row, Ia, i_refl, I behind) per boundary"""
    c = orc.constants(frequency, sos, depth_cm)
    expf = orc.lib().orc_expf
    meshes = [(int(m.mat_inside), int(m.mat_outside), int(m.vascular)) for m in osc.mesh]
    mats = osc.mat
    att_of = (lambda m: f32(mats[m, M_ATT])) if mode == TOTAL else (lambda m: f32(0.0))
    sp = [f32(x) for x in osc.c.spacing]
    start = int(osc.c.start_mat)
    frm = [f32(x) for x in pos]; d = [f32(x) for x in direction]
    offs = f32(offs); freq = f32(frequency)
    Ls = f32(2.0 * depth_cm)
    dist, b_prev, k, flag = 0.0, 0, 0, 0
    media, outside, stack = start, lm.OUT_NONE, []
    I, t_prev = f32(1.0), 0.0
    transmit = np.empty(n_rows, f32); reflect = np.zeros(n_rows, f32); written = np.zeros(n_rows, bool)

    def fill(lo, hi):
        """rows [lo, hi) of the segment that runs in `media` from t_prev on (attenuated(), a row per element: numpy rounds every operation on its own)"""
        if hi <= lo:
            return
        att = att_of(media)
        dt = np.arange(lo, hi, dtype=np.float64) * c.row_dt_us - t_prev
        dt = np.where(dt > 0.0, dt, 0.0)
        mm = (dt * float(sos)) / 1000.0
        x = ((-att * (mm.astype(f32) * f32(0.01))).astype(f32) * freq).astype(f32)
        transmit[lo:hi] = I * np.array([expf(v) for v in x.tolist()], f32)

    while True:
        if k == cap:
            flag = lm.CAPPED
            break
        to = [f32(frm[i] + f32(Ls * f32(sp[i] * d[i]))) for i in range(3)]
        f2 = [f32(frm[i] + f32(offs * d[i])) for i in range(3)]
        tri, frac, n, p, _ = osc.closest_hit(f2, to)
        if tri < 0:
            break
        xd, yd, zd = (float(f32(abs(f32(frm[i] - p[i])) * sp[i])) for i in range(3))
        mm = math.sqrt(xd * xd + yd * yd + zd * zd) * 10
        dist = dist + mm
        t = ((dist * 1000.0) / 1.0) / float(sos)
        if not t < c.max_travel_us:
            break
        q = t / c.row_dt_us
        if not q < float(n_rows):
            break
        b = int(q)
        mesh = int(osc.tri_mesh[tri])
        fill(b_prev, b)
        ia = attenuated(expf, I, att_of(media), mm, freq)
        z1 = f32(mats[media, M_IMP])
        if rule == lm.TRACED:
            media, outside = lm.update_traced(media, outside, meshes[mesh])
        else:
            if mesh in stack:
                stack.remove(mesh)
            elif len(stack) < lm.STACK:
                stack.append(mesh)
            else:
                flag = lm.CAPPED
            media = meshes[stack[-1]][0] if stack else start
        z2 = f32(mats[media, M_IMP])
        # the closest hit's normal is the triangle's normalised plane normal, negated when it faces away from the origin: inc's two candidates
        # are each other's negation, so either orientation gives the same inc
        nn = [f32(x) for x in n]
        inc = dot(d, [f32(-x) for x in nn])
        if inc < 0:
            inc = dot(d, nn)
        i_refl, i_refr = boundary(z1, z2, inc, ia)
        if not written[b]:
            reflect[b] = i_refl; written[b] = True
        I = i_refr if i_refr > 0 else f32(0.0)
        if detail is not None:
            detail.append((b, ia, i_refl, I))
        t_prev, b_prev, frm, k = t, b, [f32(x) for x in p], k + 1
    fill(b_prev, n_rows)
    return transmit, reflect, k | flag


def transmit_frames(osc, orc, pos, dirs, n_rows, **kw):
    """pos / dirs [..., 3] -> (transmit float32 [..., R], reflect float32 [..., R], crossings uint32 [...])"""
    pos = np.asarray(pos, f32); dirs = np.asarray(dirs, f32)
    lead = pos.shape[:-1]
    rows = [walk(osc, orc, p, d, n_rows, **kw) for p, d in zip(pos.reshape(-1, 3), dirs.reshape(-1, 3))]
    return (np.stack([r[0] for r in rows]).reshape(lead + (n_rows,)), np.stack([r[1] for r in rows]).reshape(lead + (n_rows,)),
            np.array([r[2] for r in rows], np.uint32).reshape(lead))


def same_bits(got, want, what):
    """float arrays equal bit for bit (a NaN equals itself, -0 differs from 0)"""
    g = np.ascontiguousarray(got, f32).view(np.uint32); w = np.ascontiguousarray(want, f32).reshape(np.shape(got)).view(np.uint32)
    if not np.array_equal(g, w):
        at = tuple(np.argwhere(g != w)[0])
        raise AssertionError("%s: %d of %d floats differ, first at %s: got %r, want %r" % (what, int((g != w).sum()), g.size, at,
                                                                                         np.asarray(got, f32)[at], np.asarray(want, f32).reshape(np.shape(got))[at]))
