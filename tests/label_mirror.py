"""numpy mirror of the ground-truth label maps (include/mcrt.h: mcrt_label_frames, mcrt_label_scan_convert_frames, mcrt_label_volume_frames).
The walk is the header's specification restated in np.float32 / float64 on top of the CPU oracle's existing entry points: the closest hit is
OracleScene.closest_hit (the contract's own, brute force over the triangles), the constants orc.constants; the segment arithmetic, the
distance, the row rule and the two medium updates are written out here.  The gathers take the maps as an INPUT -- the product's own
(mcrt_scan_maps, mcrt_volume_maps) -- as the other image mirrors do."""
import math
import numpy as np

f32 = np.float32
TRACED, GEOMETRIC = 0, 1
NONE = 255
MAX_CROSSINGS = 64
CAPPED = 1 << 31
OUT_NONE, OUT_SELF = -1, -2
STACK = 16


def update_traced(media, outside, mesh):
    """the four branches of hit_boundary that make the refracted ray's medium and vascular memory (ray.cpp:13-47) -> (media, outside)"""
    inside, out, vascular = mesh
    if outside != OUT_NONE:
        if vascular:
            return (media if outside == OUT_SELF else outside), OUT_NONE
        return media, (out if outside == inside else inside)
    if vascular:
        return inside, OUT_SELF
    return inside, OUT_NONE          # quirk 1: leaving a non-vascular mesh keeps its mat_inside


def walk(osc, orc, pos, direction, n_rows, rule=TRACED, offs=0.1, frequency=4.5, sos=1500, depth_cm=15.0, cap=MAX_CROSSINGS):
    """one scan-line -> (tissue uint8 [R], interface int32 [R], crossings)"""
    c = orc.constants(frequency, sos, depth_cm)
    meshes = [(int(m.mat_inside), int(m.mat_outside), int(m.vascular)) for m in osc.mesh]
    sp = [f32(x) for x in osc.c.spacing]
    start = int(osc.c.start_mat)
    frm = [f32(x) for x in pos]; d = [f32(x) for x in direction]
    offs = f32(offs)
    Ls = f32(2.0 * depth_cm)
    dist, b_prev, k, flag = 0.0, 0, 0, 0
    media, outside, stack = start, OUT_NONE, []
    tissue = np.empty(n_rows, np.uint8); interface = np.full(n_rows, -1, np.int32)
    while True:
        if k == cap:
            flag = CAPPED
            break
        to = [f32(frm[i] + f32(Ls * f32(sp[i] * d[i]))) for i in range(3)]
        f2 = [f32(frm[i] + f32(offs * d[i])) for i in range(3)]
        tri, frac, _, p, _ = osc.closest_hit(f2, to)
        if tri < 0:
            break
        xd, yd, zd = (float(f32(abs(f32(frm[i] - p[i])) * sp[i])) for i in range(3))
        dist = dist + math.sqrt(xd * xd + yd * yd + zd * zd) * 10
        t = ((dist * 1000.0) / 1.0) / float(sos)
        if not t < c.max_travel_us:
            break
        q = t / c.row_dt_us
        if not q < float(n_rows):
            break
        b = int(q)
        mesh = int(osc.tri_mesh[tri])
        tissue[b_prev:b] = media
        if interface[b] == -1:
            interface[b] = mesh
        if rule == TRACED:
            media, outside = update_traced(media, outside, meshes[mesh])
        else:
            if mesh in stack:
                stack.remove(mesh)
            elif len(stack) < STACK:
                stack.append(mesh)
            else:
                flag = CAPPED
            media = meshes[stack[-1]][0] if stack else start
        b_prev, frm, k = b, [f32(x) for x in p], k + 1
    tissue[b_prev:] = media
    return tissue, interface, k | flag


def label_frames(osc, orc, pos, dirs, n_rows, **kw):
    """pos / dirs [..., 3] -> (tissue uint8 [..., R], interface int32 [..., R], crossings uint32 [...])"""
    pos = np.asarray(pos, f32); dirs = np.asarray(dirs, f32)
    lead = pos.shape[:-1]
    rows = [walk(osc, orc, p, d, n_rows, **kw) for p, d in zip(pos.reshape(-1, 3), dirs.reshape(-1, 3))]
    return (np.stack([r[0] for r in rows]).reshape(lead + (n_rows,)), np.stack([r[1] for r in rows]).reshape(lead + (n_rows,)),
            np.array([r[2] for r in rows], np.uint32).reshape(lead))


# ------------------------------------------------------------------ the nearest-neighbour gathers
def nearest(m, extent):
    """map coordinate -> (index int64, clipped into the extent; inside?): f = floorf(m), a = m - f, i = f + (a >= 0.5f), inside 0 <= i < extent"""
    m = np.asarray(m, f32)
    with np.errstate(invalid="ignore"):
        f = np.floor(m)
        a = (m - f).astype(f32)
        ok = np.isfinite(f)
        i = np.where(ok, np.clip(f, -4.0, float(extent) + 4.0), -4.0).astype(np.int64) + (a >= f32(0.5))
    inside = ok & (i >= 0) & (i < extent)
    return np.clip(i, 0, extent - 1), inside


def scan_convert(tissue, map_row, map_col):
    """tissue [E][R] -> uint8 of the maps' shape"""
    tissue = np.asarray(tissue, np.uint8)
    E, R = tissue.shape
    x, okx = nearest(map_col, E); y, oky = nearest(map_row, R)
    return np.where(okx & oky, tissue[x, y], np.uint8(NONE)).astype(np.uint8)


def volume(tissue, maps):
    """tissue [K][E][R], maps (map_plane, map_row, map_col) -> uint8 of the maps' shape"""
    tissue = np.asarray(tissue, np.uint8)
    K, E, R = tissue.shape
    z, okz = nearest(maps[0], K); y, oky = nearest(maps[1], R); x, okx = nearest(maps[2], E)
    return np.where(okx & oky & okz, tissue[z, x, y], np.uint8(NONE)).astype(np.uint8)


# ------------------------------------------------------------------ scenes of the label tests
def _scene(mcrt, parts, start="GEL"):
    """parts: [(name, (V, F), material, outside, vascular)] -> SceneData in the reference's schema, unit scaling"""
    cfg = {"transducerPosition": [0.0, 0.0, 0.0], "transducerAngles": [0.0, 0.0, 0.0], "materials": mcrt.synth.materials(), "meshes": [],
           "origin": [0.0, 0.0, 0.0], "spacing": [1.0, 1.0, 1.0], "scaling": 1.0, "startingMaterial": start}
    meshes = {}
    for name, vf, mat, out, vasc in parts:
        meshes[name] = vf
        cfg["meshes"].append({"file": name, "rigid": True, "vascular": vasc, "deltas": [0.0, 0.0, 0.0], "material": mat, "outsideMaterial": out,
                              "outsideNormals": True})
    return mcrt.scene_io.build_scene(cfg, meshes)


SPHERES_CENTRE, SPHERES_OUTER, SPHERES_INNER = (7.5, 0.0, 0.0), 3.0, 1.5


def spheres_scene(mcrt, subdiv=4):
    """two concentric spheres: LIVER (in GEL) around BONE (in LIVER); the probe's beams start at the origin"""
    ico = mcrt.synth.icosphere
    return _scene(mcrt, [("outer.obj", ico(subdiv, SPHERES_OUTER, SPHERES_CENTRE), "LIVER", "GEL", False),
                         ("inner.obj", ico(subdiv, SPHERES_INNER, SPHERES_CENTRE), "BONE", "LIVER", False)])


def fan(n, half_angle, dz=0.0):
    """n beams from the origin, spread over +-half_angle about +x in the x-y plane and lifted by dz out of it (a beam in the plane z = 0 runs
    along the shared diagonal of a box's face) -> (pos, dir) float32 [n][3], unit directions"""
    th = np.linspace(-half_angle, half_angle, n) if n > 1 else np.zeros(1)
    d = np.stack([np.cos(th), np.sin(th), np.full(n, dz)], 1)
    return np.zeros((n, 3), f32), (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)


def sheets_scene(mcrt, xs, materials=("LIVER", "FAT"), half=4.0):
    """parallel two-triangle sheets normal to x at the positions xs [cm], dealt in turn to as many meshes as there are materials -- so that
    GEOMETRIC, which reads a second meeting with a mesh as leaving it, never holds more than that many (lopsided in y: the x axis does not
    run through the two triangles' shared diagonal)"""
    n = len(materials)
    parts = []
    for m in range(n):
        mine = list(xs)[m::n]
        if not mine:
            continue
        V = np.array([[[x, -half, -half], [x, half + 1.0, -half], [x, half + 1.0, half], [x, -half, half]] for x in mine], f32).reshape(-1, 3)
        F = np.array([[4 * k, 4 * k + 1, 4 * k + 2, 4 * k, 4 * k + 2, 4 * k + 3] for k in range(len(mine))], np.int32).reshape(-1, 3)
        parts.append(("sheets_%d.obj" % m, (V, F), materials[m], "GEL", False))
    return _scene(mcrt, parts)


def boxes_scene(mcrt, n, centre=(6.0, 0.0, 0.0), outer=4.0, step=0.2):
    """n nested boxes, the outermost first, half-sizes outer - i * step"""
    mats = ("LIVER", "FAT", "KIDNEY")
    return _scene(mcrt, [("box_%d.obj" % i, mcrt.synth.box((outer - i * step,) * 3, centre), mats[i % 3], "GEL", False) for i in range(n)])


def oracle_scene(orc, sd):
    return orc.OracleScene(sd.tri, sd.tri_mesh, sd.meshes, sd.materials, sd.start_mat, sd.spacing)
