"""numpy mirror of volume rendering (include/mcrt.h: mcrt_render_frames), in np.float32 with one rounding per operation: the ray of every
pixel, the trilinear sample of every step, and the three folds (MIP, mean, surface).  The view floats are an INPUT -- the product's own
(mcrt_render_view_for_grid), or any twelve finite floats -- so that no libm difference can enter the kernel comparisons;
tests/test_render_contract.py checks the helper itself against the formulas in double.
Also here: the double-precision model of the helper, the coverage of a view (which steps of which rays can see the block), and the table of
blocks, directions and pictures both test files use."""
import math
import numpy as np

f32 = np.float32
MIP, MEAN, SURFACE = 0, 1, 2
MODES = {"mip": MIP, "mean": MEAN, "surface": SURFACE}


def defaults(in_u8=False, **kw):
    """mcrt_default_render_opts as a dict, with overrides"""
    o = dict(mode=SURFACE, lo=0.0, hi=255.0 if in_u8 else 1.0, threshold=0.25, ramp=0.25, opacity=1.0, depth_cue=0.5, t_cut=0.0)
    o.update(kw)
    if isinstance(o["mode"], str):
        o["mode"] = MODES[o["mode"]]
    return o


def view_floats(view):
    """(origin, di, dj, ds) float32 [3] each, and (nx, ny, n_steps), of an mcrt_render_view"""
    return tuple(np.array(list(v), f32) for v in (view.origin, view.di, view.dj, view.ds)), (int(view.nx), int(view.ny), int(view.n_steps))


def ray_points(view, s):
    """p_c = ((origin_c + (float)i * di_c) + (float)j * dj_c) + (float)s * ds_c for every pixel: three float32 [ny][nx]"""
    (o, di, dj, ds), (nx, ny, _) = view_floats(view)
    i = np.arange(nx, dtype=f32)[None, :]; j = np.arange(ny, dtype=f32)[:, None]
    with np.errstate(all="ignore"):
        return [(((o[c] + (i * di[c]).astype(f32)).astype(f32) + (j * dj[c]).astype(f32)).astype(f32) + f32(f32(s) * ds[c])).astype(f32) for c in range(3)]


def split(p, shape):
    """floor, fraction and `covered` of the contract for the points p = (pu, pv, pw); shape = (nw, nv, nu)"""
    nw, nv, nu = shape
    with np.errstate(all="ignore"):
        f = [np.floor(x) for x in p]
        a = [(x - fx).astype(f32) for x, fx in zip(p, f)]
        covered = np.ones(p[0].shape, bool)
        for x, fx, n in zip(p, f, (nu, nv, nw)):
            covered &= ~np.isnan(x) & (fx >= f32(-1.0)) & (fx < f32(n))
    return f, a, covered


def sample(block, p):
    """block float32 [nw][nv][nu], p = (pu, pv, pw) -> (v, covered): the trilinear blend, a NaN sample 0; v is meaningless where not covered"""
    nw, nv, nu = block.shape
    f, a, covered = split(p, block.shape)
    iu, iv, iw = (np.where(covered, fx, 0).astype(np.int64) for fx in f)
    t = {}
    for dw in (0, 1):
        for dv in (0, 1):
            for du in (0, 1):
                u, v, w = iu + du, iv + dv, iw + dw
                inside = covered & (u >= 0) & (u < nu) & (v >= 0) & (v < nv) & (w >= 0) & (w < nw)
                t[dw, dv, du] = np.where(inside, block[np.clip(w, 0, nw - 1), np.clip(v, 0, nv - 1), np.clip(u, 0, nu - 1)], f32(0)).astype(f32)
    one = f32(1.0)
    with np.errstate(all="ignore"):
        def mix(x0, x1, al):
            return ((x0 * (one - al).astype(f32)).astype(f32) + (x1 * al).astype(f32)).astype(f32)
        c = {(dw, dv): mix(t[dw, dv, 0], t[dw, dv, 1], a[0]) for dw in (0, 1) for dv in (0, 1)}
        e = [mix(c[dw, 0], c[dw, 1], a[1]) for dw in (0, 1)]
        v = mix(e[0], e[1], a[2])
    return np.where(np.isnan(v), f32(0), v).astype(f32), covered


def clamp01(x):
    """fminf(fmaxf(x, 0), 1): a NaN becomes 0"""
    return np.fmin(np.fmax(x, f32(0)), f32(1)).astype(f32)


def render(block, view, opts):
    """block [nw][nv][nu] (float32, or uint8: a voxel b is (float)b) -> (out float32, out8 uint8, depth float32), each [ny][nx]"""
    block = np.asarray(block)
    block = block.astype(f32) if block.dtype == np.uint8 else np.asarray(block, f32)
    _, (nx, ny, n_steps) = view_floats(view)
    mode = opts["mode"]
    lo = f32(opts["lo"]); inv_range = f32(1.0 / (float(f32(opts["hi"])) - float(lo)))
    thr = f32(opts["threshold"]); inv_ramp = f32(1.0 / float(f32(opts["ramp"]))); opacity = f32(opts["opacity"]); cue = f32(opts["depth_cue"]); t_cut = f32(opts["t_cut"])
    inv_steps = f32(1.0 / (n_steps - 1)) if n_steps > 1 else f32(0)
    m = np.zeros((ny, nx), f32); depth = np.full((ny, nx), -1, f32); total = np.zeros((ny, nx), f32); cnt = np.zeros((ny, nx), np.int64)
    C = np.zeros((ny, nx), f32); T = np.ones((ny, nx), f32); alive = np.ones((ny, nx), bool)
    one = f32(1.0)
    for s in range(n_steps):
        v, covered = sample(block, ray_points(view, s))
        act = covered & alive
        with np.errstate(all="ignore"):
            x = clamp01(((v - lo).astype(f32) * inv_range).astype(f32))
            if mode == MIP:
                up = act & (x > m)
                m = np.where(up, x, m); depth = np.where(up, f32(s), depth)
            elif mode == MEAN:
                total = np.where(act, (total + x).astype(f32), total); cnt = cnt + act
            else:
                al = (clamp01(((x - thr).astype(f32) * inv_ramp).astype(f32)) * opacity).astype(f32)
                shade = (one - (cue * f32(f32(s) * inv_steps)).astype(f32)).astype(f32)
                C = np.where(act, (C + ((T * al).astype(f32) * (x * shade).astype(f32)).astype(f32)).astype(f32), C)
                T = np.where(act, (T * (one - al).astype(f32)).astype(f32), T)
                depth = np.where(act & (depth < 0) & (T <= f32(0.5)), f32(s), depth)
                alive = alive & ~(act & (T < t_cut))
    if mode == MIP:
        out = m
    elif mode == MEAN:
        with np.errstate(all="ignore"):
            out = np.where(cnt > 0, (total / np.maximum(cnt, 1).astype(f32)).astype(f32), f32(0)).astype(f32)
        depth = np.full((ny, nx), -1, f32)
    else:
        out = C
    out = out.astype(f32)
    out8 = ((clamp01(out) * f32(255.0)).astype(f32) + f32(0.5)).astype(f32).astype(np.uint8)
    return out, out8, depth.astype(f32)


def render_frames(blocks, view, opts):
    """blocks [F][nw][nv][nu] -> (out, out8, depth), each [F][ny][nx]"""
    r = [render(b, view, opts) for b in blocks]
    return tuple(np.stack([x[k] for x in r]) for k in range(3))


def coverage(view, shape):
    """bool [n_steps][ny][nx]: the steps of every ray at which at least one tap can lie inside a block of shape (nw, nv, nu)"""
    _, (nx, ny, n_steps) = view_floats(view)
    return np.stack([split(ray_points(view, s), shape)[2] for s in range(n_steps)])


# ------------------------------------------------------------------ the helper, in double
def grid_arrays(g):
    return tuple(np.array(list(v), np.float64) for v in (g.origin_mm, g.du_mm, g.dv_mm, g.dw_mm)) + ((g.nu, g.nv, g.nw),)


def half_diagonal(g):
    """L: half the longest of the block's four space diagonals"""
    _, du, dv, dw, (nu, nv, nw) = grid_arrays(g)
    return max(np.linalg.norm((nu - 1) * du + sv * (nv - 1) * dv + sw * (nw - 1) * dw) for sv in (-1, 1) for sw in (-1, 1)) / 2.0


def view_model(g, direction, up, pixel_mm, step_mm, nx, ny):
    """include/mcrt.h's formulas of mcrt_render_view_for_grid in numpy double -> (origin, di, dj, ds as float64 [3], n_steps)"""
    o, du, dv, dw, (nu, nv, nw) = grid_arrays(g)
    d = np.asarray(direction, np.float64); upv = np.asarray(up, np.float64)
    dn = d / np.linalg.norm(d)
    right = np.cross(dn, upv); right = right / np.linalg.norm(right)
    down = -np.cross(right, dn)
    Cc = o + (nu - 1) / 2.0 * du + (nv - 1) / 2.0 * dv + (nw - 1) / 2.0 * dw
    L = half_diagonal(g)
    P0 = Cc - L * dn - (nx - 1) / 2.0 * pixel_mm * right - (ny - 1) / 2.0 * pixel_mm * down
    Minv = np.linalg.inv(np.stack([du, dv, dw], axis=1))
    return Minv @ (P0 - o), Minv @ (pixel_mm * right), Minv @ (pixel_mm * down), Minv @ (step_mm * dn), int(math.floor(2.0 * L / step_mm)) + 1


# ------------------------------------------------------------------ the cases of the tests
BLOCKS = [(17, 13, 11), (33, 35, 5), (40, 48, 24), (1, 1, 1)]                    # (nu, nv, nw)
DIRECTIONS = [(0.0, 0.0, 1.0), (-1.0, 0.0, 0.0), (0.5, 0.3, 0.8), (-0.7, 0.6, -0.2)]
PICTURES = [(33, 35), (1, 1), (64, 3)]                                          # (nx, ny)
CASES = [(b, d, p) for b in BLOCKS for d in DIRECTIONS for p in PICTURES]
UP = (0.0, 1.0, 0.0)        # no direction of the table is parallel to it


def case_grid(mcrt, block):
    """a grid for a block of the table: the block fills a cube of 16 mm whatever its voxel counts (a thin block seen along its thin axis
    would otherwise be a few steps of a long ray), so the voxels are not cubic and the rays cross them at another pitch along every axis;
    origin off zero.  The renderer never sees the millimetres, only what the helper makes of them"""
    nu, nv, nw = block
    pitch = [16.0 / (n - 1) if n > 1 else 0.5 for n in block]
    return mcrt.volume_grid((-3.0, 41.0, -2.5), (pitch[0], 0, 0), (0, pitch[1], 0), (0, 0, pitch[2]), nu, nv, nw)


def case_view(mcrt, block, direction, picture, n=36):
    """pixel_mm = 0.6 * 2L / max(nx, ny), step_mm = 2L / n: the picture is 0.6 diagonals wide and the rays take n + 1 steps (n when the
    quotient rounds below n).  A block of one voxel has L = 0: its picture is 0.6 voxel diagonals wide and its rays take one step."""
    g = case_grid(mcrt, block)
    nx, ny = picture
    L2 = 2.0 * half_diagonal(g)
    if L2 == 0.0:
        L2 = float(np.linalg.norm(grid_arrays(g)[1] + grid_arrays(g)[2] + grid_arrays(g)[3]))
    return mcrt.render_view(g, direction, UP, 0.6 * L2 / max(nx, ny), L2 / n, nx, ny)


def float_block(shape, seed=0):
    """[nw][nv][nu] float32: noise around the window [0, 1] with NaN, +-inf (image_cases.scan_image) and -0.0 voxels"""
    import image_cases as ic
    nw, nv, nu = shape
    b = (ic.scan_image(nw * nv, nu, seed=seed) * f32(0.5) + f32(0.4)).astype(f32).reshape(shape)
    flat = b.reshape(-1)
    if flat.size >= 8:
        flat[np.random.default_rng(seed + nu).integers(0, flat.size, max(1, flat.size // 61))] = -0.0
    else:
        flat[:] = f32(0.9375)                                    # a block of a few voxels is bright: its picture must not be blank
    return b


def byte_block(shape, seed=0):
    b = np.random.default_rng(700 + seed).integers(0, 256, shape, dtype=np.uint8)
    if b.size < 8:
        b[...] = 230
    return b
