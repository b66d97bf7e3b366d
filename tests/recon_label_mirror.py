"""The contracts of mcrt_recon_label_frames and mcrt_render_label_frames (include/mcrt.h) in numpy.  The positions are recon_mirror's, the nearest
rule is label_mirror's and the ray points are render_mirror's, by import: the label calls restate the float calls' contracts and so do these.
Like recon_mirror it takes the product's own host floats (A, b from mcrt_recon_transform; row_u = float32(row_mm / unit_mm)).  Everything
after the positions is integers."""
import numpy as np

import label_mirror as lm
import recon_mirror as rm
import render_mirror as vm

f32 = np.float32
NONE = lm.NONE
DEFAULTS = dict(fill_radius=1, fill_min=1)


def vote(stack, pos, dirs, A, b, row_u, shape, n_labels):
    """-> (votes int64 [n][n_labels], stats uint32 [2], voxel int64 [F][E][R] (-1: no vote)); shape = (nw, nv, nu)"""
    stack = np.ascontiguousarray(stack, np.uint8)
    F, E, R = stack.shape
    nw, nv, nu = shape
    idx = rm.indices(rm.positions(np.asarray(pos, f32).reshape(F, E, 3), np.asarray(dirs, f32).reshape(F, E, 3), R, row_u), A, b)
    with np.errstate(invalid="ignore"):
        inside = np.ones(stack.shape, bool)
        for c, nc in enumerate((nu, nv, nw)):
            inside &= (idx[..., c] >= f32(0.0)) & (idx[..., c] < f32(nc))
    valid = stack < n_labels
    take = inside & valid
    stats = np.array([(~inside).sum(), (inside & ~valid).sum()], np.uint32)
    ii = np.where(take[..., None], idx, 0).astype(np.int64)
    vox = (ii[..., 2] * nv + ii[..., 1]) * nu + ii[..., 0]
    votes = np.zeros((nw * nv * nu, n_labels), np.int64)
    np.add.at(votes, (vox[take], stack[take].astype(np.int64)), 1)
    return votes, stats, np.where(take, vox, -1)


def winners(votes, shape):
    """-> (winner uint8 [nw][nv][nu] (NONE: no vote), count uint32, the winner's votes uint32, tie bool: the winner has an equal)"""
    count = votes.sum(1)
    best = votes.max(1)
    win = np.where(count > 0, votes.argmax(1), NONE).astype(np.uint8)             # (argmax: the first of the largest, the smallest label)
    tie = (count > 0) & ((votes == best[:, None]).sum(1) > 1)
    return win.reshape(shape), count.astype(np.uint32).reshape(shape), best.astype(np.uint32).reshape(shape), tie.reshape(shape)


def fill(win, n_labels, fill_radius=1, fill_min=1):
    """winner [nw][nv][nu] -> (labels uint8 the same: the holes filled from SAMPLED voxels only, filled bool, tie bool: a hole decided by a tie)"""
    shape = win.shape
    H = int(fill_radius)
    out = win.copy()
    todo = win == NONE
    filled = np.zeros(shape, bool); tie = np.zeros(shape, bool)
    pw = np.pad(win, H, constant_values=NONE) if H else win
    for h in range(1, H + 1):
        tally = np.zeros((n_labels,) + shape, np.int32)
        for dw in range(-h, h + 1):
            for dv in range(-h, h + 1):
                for du in range(-h, h + 1):
                    w = pw[H + dw:H + dw + shape[0], H + dv:H + dv + shape[1], H + du:H + du + shape[2]]
                    at = np.nonzero(w != NONE)
                    tally[(w[at].astype(np.int64),) + at] += 1                   # (one neighbour per voxel and offset: no index repeats)
        n = tally.sum(0)
        ok = todo & (n >= int(fill_min))
        best = tally.max(0)
        out = np.where(ok, tally.argmax(0), out).astype(np.uint8)
        tie |= ok & ((tally == best[None]).sum(0) > 1)
        filled |= ok
        todo &= ~ok
    return out, filled, tie


def recon_labels(stack, pos, dirs, A, b, row_u, shape, n_labels, fill_radius=1, fill_min=1):
    """mcrt_recon_label_frames -> (labels uint8 [nw][nv][nu], count uint32, votes uint32, stats uint32 [2])"""
    votes, stats, _ = vote(stack, pos, dirs, A, b, row_u, shape, n_labels)
    win, count, best, _ = winners(votes, shape)
    return fill(win, n_labels, fill_radius, fill_min)[0], count, best, stats


def nearest_float(p):
    """k = f + (a >= 0.5f ? 1 : 0) as a float: label_mirror.nearest's rule before its clip (the render call compares in float)"""
    p = np.asarray(p, f32)
    with np.errstate(invalid="ignore"):
        f = np.floor(p)
        return (f + ((p - f).astype(f32) >= f32(0.5)).astype(f32)).astype(f32)


def render_labels(labels, view, depth):
    """mcrt_render_label_frames: labels uint8 [F][nw][nv][nu], depth float32 [F][ny][nx] -> uint8 [F][ny][nx]"""
    labels = np.asarray(labels, np.uint8); depth = np.asarray(depth, f32)
    F, nw, nv, nu = labels.shape
    n_steps = int(view.n_steps)
    out = np.empty(depth.shape, np.uint8)
    for f in range(F):
        s = depth[f]
        with np.errstate(invalid="ignore"):
            seen = (s >= f32(0.0)) & (s < f32(n_steps))
            p = vm.ray_points(view, np.where(seen, s, f32(0.0)).astype(f32))
            ok = seen.copy()
            k = []
            for x, n in zip(p, (nu, nv, nw)):
                kf = nearest_float(x)
                i, inside = lm.nearest(x, n)
                assert np.array_equal(inside, (kf >= f32(0.0)) & (kf < f32(n))), "the two forms of the nearest rule"
                ok &= inside
                k.append(i)
        out[f] = np.where(ok, labels[f][k[2], k[1], k[0]], np.uint8(NONE))
    return out
