// mcrt_label.hip -- ground-truth label maps (mcrt_label_frames, mcrt_label_scan_convert_frames, mcrt_label_volume_frames; contracts in
// include/mcrt.h): k_label walks the central beam of every scan-line through the scene and names the tissue of every RF row and the
// interface met in it; k_label_gather gathers a tissue map through the scan-conversion and volume maps, nearest neighbour.
// The reference draws pictures only (ray.cpp:13-47 decides the medium behind a boundary, rfimage.h:33-40 the row of a time,
// rfimage.h:183-215 the sector's maps); it keeps no map of what it drew.
#include "mcrt_pixels.h"
#include "mcrt_walk.h"

#ifndef MCRT_LABEL_STACK
#define MCRT_LABEL_STACK 16          // traversal-stack entries of a lane in LDS (the walk's steps index it with a stride of 256 lanes whatever the workgroup's size: 16 KB)
#endif

namespace mcrt {

// =============================================================================================================
// k_label -- one lane walks one (frame, scan-line): closest hit (the lane walk's own node and leaf steps, so the tracer's answers bit for
// bit), the row of the hit's time, the medium behind the boundary, from the hit point on -- at most MCRT_LABEL_MAX_CROSSINGS times.  A
// workgroup is ONE wavefront: the pass has E x F beams where the tracer has E x S x F x B rays, it cannot fill the GPU and is as long as
// its longest beam, so nothing is gained by packing wavefronts, and the boundary lists of 64 beams (64 x 64 x 8 B) are 32 KB of LDS.
// Phase 1 leaves every beam's boundaries {row, medium behind, mesh} in LDS; after a barrier phase 2 turns the lists into rows, the lanes
// ALONG the rows: the workgroup's 64 scan-lines are 64 R consecutive bytes of the tissue map, written as aligned 32-bit words (four rows
// each, single bytes at the two ragged ends) whatever R and the pointer are, and 64 R consecutive words of the interface map.
// No scratch: the GEOMETRIC rule's stack of open meshes lives in LDS as well.
// =============================================================================================================
struct LabelList { const uint2 *e; uint32_t n, start; };      // the boundaries of one beam: entry i at e[64 i], x = row | medium behind << 16, y = mesh
// the medium of a row: that behind the deepest boundary at or above it (the rows ascend along the list)
MCRT_DEV uint32_t label_tissue(const LabelList &l, uint32_t row)
{
    uint32_t m = l.start;
    for (uint32_t i = 0; i < l.n; i++) { const uint32_t w = l.e[64u * i].x; if ((w & 0xffffu) <= row) m = w >> 16; }
    return m;
}
// the interface of a row: the shallowest boundary that falls into it
MCRT_DEV int label_interface(const LabelList &l, uint32_t row)
{
    for (uint32_t i = 0; i < l.n; i++) { const uint2 w = l.e[64u * i]; if ((w.x & 0xffffu) == row) return (int)w.y; }
    return -1;
}

__global__ void __launch_bounds__(64) k_label(FrameArgs a, LabelArgs l)
{
    __shared__ int stack[MCRT_LABEL_STACK * 256];
    __shared__ uint2 list[MCRT_LABEL_MAX_CROSSINGS * 64];     // [crossing][lane]
    __shared__ int open_mesh[16 * 64];                        // [depth][lane]  GEOMETRIC: the meshes the beam is inside of, innermost last
    __shared__ uint32_t count[64];
    const int tid = threadIdx.x;
    const uint32_t line0 = blockIdx.x * 64u, line = line0 + (uint32_t)tid;      // line = frame * ne_frame + scan-line: the outputs' own order
    const LaneStackT<MCRT_LABEL_STACK> S = { stack, a.stack_ovf + ((size_t)blockIdx.x * 64 + tid), (size_t)gridDim.x * 64, tid };
    bool active = line < a.ne;
    f3 from = mk(0, 0, 0), dir = mk(0, 0, 1);
    if (active) {
        const uint32_t fr = line / a.ne_frame, scan = line - fr * a.ne_frame;
        const size_t pe = (size_t)fr * a.pose_stride + a.e_begin + scan;
        from = mk(a.el_pos[3 * pe], a.el_pos[3 * pe + 1], a.el_pos[3 * pe + 2]);
        dir = mk(a.el_dir[3 * pe], a.el_dir[3 * pe + 1], a.el_dir[3 * pe + 2]);
    }
    double dist = 0.0;
    uint32_t k = 0, capped = 0, depth = 0;
    int media = (int)a.start_mat, outside = OUT_NONE;
    MCRT_WATCHDOG_DECL()
    bool abandoned = false;
    while (__any(active) && !abandoned) {
        // ---- the closest hit of the segment from the last boundary on (ray_of: the tracer's segment with the beam's full length) ----
        const Ray ry = ray_of(from, dir, l.Ls, a);
        const f3 f2 = ry.f2, to = ry.to, d = to - f2;
        const f3 inv = mk(rcp_dir(d.x), rcp_dir(d.y), rcp_dir(d.z)), rc = ray_c(f2, inv);
        const LaneRay lr = { rc.x, rc.y, rc.z, inv.x, inv.y, inv.z, inv.x < 0.0f, inv.y < 0.0f, inv.z < 0.0f };
        Best best; best.frac = 1.0f; best.tri = -1;
        int sp = 0, sb = 0, cur = (active && a.n_nodes != 0u) ? 0 : CUR_IDLE;
        while (MCRT_WALKING(cur) != 0ull) {
            if ((++wd_iter & 4095u) == 0u && wall_clock64() - wd_start > (unsigned long long)MCRT_WATCHDOG_SECONDS * 100000000ull) { if (tid == 0) atomicOr(a.error_flag, 2u); abandoned = true; break; }
            const float tcap = fminf(1.0f, best.frac);
            while (MCRT_ON_INNER(cur) != 0ull && popc_mask(MCRT_ON_LEAF(cur)) < (uint32_t)MCRT_LANE_LEAF_BATCH)
                if (cur >= 0) lane_node_step(a, S, lr, 0.0f, tcap, cur, sp, sb);
            if ((uint32_t)cur > 0x80000000u) lane_leaf_test(a, S, f2, to, inv, rc, 0.0f, false, best, cur, sp, sb);
        }
        if (abandoned) break;
        // ---- the boundary: its row, the medium behind it ----
        if (active) {
            active = false;
            if (best.tri >= 0) {
                const float s = 1.0f - best.frac;
                const f3 p = mk(s * f2.x + best.frac * to.x, s * f2.y + best.frac * to.y, s * f2.z + best.frac * to.z);      // the contract's own hit point
                const float xd = fabsf(from.x - p.x) * a.sx, yd = fabsf(from.y - p.y) * a.sy, zd = fabsf(from.z - p.z) * a.sz;      // travel (ray.cpp:99-103, scene.cpp:281-290)
                const double mm = sqrt((double)xd * (double)xd + (double)yd * (double)yd + (double)zd * (double)zd) * 10;
                dist = dist + mm;
                const double t = ((dist * 1000.0) / 1.0) / a.sos_d;
                const int row = t < a.max_travel ? row_of_thr(t, a.row_thr, a.R, a.inv_row_dt, a.thr_end) : -1;
                if (row >= 0) {
                    const int mesh = __float_as_int(a.tris_id[MCRT_TRI_PIECES * (size_t)best.tri + 1].w);
                    const uint4 organ = a.meshes[mesh];      // mat_inside, mat_outside, vascular
                    if (l.rule == MCRT_LABEL_TRACED) {
                        // hit_boundary's material transition (ray.cpp:14-47; shade_path's four branches), the beam always going THROUGH the boundary
                        int after_vasc, mat_after;
                        if (outside != OUT_NONE) {
                            if (organ.z) { after_vasc = OUT_NONE; mat_after = (outside == OUT_SELF) ? media : outside; }
                            else { after_vasc = (outside == (int)organ.x) ? (int)organ.y : (int)organ.x; mat_after = media; }
                        } else {
                            if (organ.z) { after_vasc = OUT_SELF; mat_after = (int)organ.x; }
                            else { after_vasc = OUT_NONE; mat_after = (int)organ.x; }
                        }
                        media = mat_after; outside = after_vasc;
                    } else {
                        // the anatomy of closed, nested meshes: a mesh the beam is inside of is left, any other is entered
                        uint32_t at = depth;
                        for (uint32_t i = 0; i < depth; i++) if (open_mesh[64u * i + tid] == mesh) at = i;
                        if (at < depth) {
                            for (uint32_t i = at; i + 1u < depth; i++) open_mesh[64u * i + tid] = open_mesh[64u * (i + 1u) + tid];
                            depth--;
                        } else if (depth < 16u) open_mesh[64u * depth++ + tid] = mesh;
                        else capped = 0x80000000u;
                        media = depth ? (int)a.meshes[open_mesh[64u * (depth - 1u) + tid]].x : (int)a.start_mat;
                    }
                    list[64u * k + tid] = make_uint2((uint32_t)row | ((uint32_t)media << 16), (uint32_t)mesh);
                    from = p; k++;
                    if (k < MCRT_LABEL_MAX_CROSSINGS) active = true; else capped = 0x80000000u;
                }
            }
        }
    }
    count[tid] = k;
    if (l.crossings && line < a.ne) l.crossings[line] = k | capped;
    __syncthreads();
    if (abandoned) return;      // (the error word is set: the next synchronising call reports it, the maps are not to be read)
    // ---- the lists as rows: the workgroup's scan-lines are one contiguous span of each map ----
    const uint32_t lines = min(64u, a.ne - line0), R = a.R, span = lines * R;
    if (l.tissue) {
        uint8_t *o = l.tissue + (size_t)line0 * R;
        const uint32_t head = min(span, (uint32_t)((4u - ((uintptr_t)o & 3u)) & 3u)), words = (span - head) >> 2;
        for (uint32_t w = (uint32_t)tid; w < words; w += 64u) {
            const uint32_t g = head + 4u * w;
            uint32_t v = 0u;
#pragma unroll
            for (uint32_t j = 0; j < 4u; j++) {      // (a word may begin in one scan-line and end in another)
                const uint32_t sj = (g + j) / R, rj = g + j - sj * R;
                const LabelList ll = { list + sj, count[sj], a.start_mat };
                v |= (label_tissue(ll, rj) & 0xffu) << (8u * j);
            }
            *(uint32_t *)(o + g) = v;
        }
        // the ragged ends, byte by byte: [0, head) and [head + 4 words, span)
        const uint32_t tail0 = head + 4u * words, ragged = head + (span - tail0);
        if ((uint32_t)tid < ragged) {
            const uint32_t g = (uint32_t)tid < head ? (uint32_t)tid : tail0 + ((uint32_t)tid - head), s = g / R, row = g - s * R;
            const LabelList ll = { list + s, count[s], a.start_mat };
            o[g] = (uint8_t)label_tissue(ll, row);
        }
    }
    if (l.interface) {
        int32_t *o = l.interface + (size_t)line0 * R;
        for (uint32_t g = (uint32_t)tid; g < span; g += 64u) {
            const uint32_t s = g / R, row = g - s * R;
            const LabelList ll = { list + s, count[s], a.start_mat };
            o[g] = label_interface(ll, row);
        }
    }
}

uint32_t label_blocks(size_t lines) { return (uint32_t)((lines + 63u) / 64u); }
uint32_t label_stack_entries() { return MCRT_LABEL_STACK; }
hipError_t launch_label(const FrameArgs &a, const LabelArgs &l, hipStream_t st)
{
    hipLaunchKernelGGL(k_label, dim3(label_blocks(a.ne)), dim3(64), 0, st, a, l);
    return hipGetLastError();
}

// =============================================================================================================
// the nearest-neighbour gathers: labels cannot be interpolated.  Per coordinate m of an output point: f = floorf(m), i = (long long)f +
// (m - f >= 0.5f), inside when 0 <= i < extent; a NaN coordinate or one outside gives MCRT_LABEL_NONE.  The maps are the float calls' own
// buffers (k_remap's two maps, k_volume's three, padded to a multiple of 256 points); the layout, the frame chunks and the byte store are
// the pixel tile's (mcrt_pixels.h).
// =============================================================================================================
MCRT_DEV bool label_nearest(float m, uint32_t extent, uint32_t &i_o)
{
    const float f = floorf(m), al = m - f;
    const long long i = (long long)f + (al >= 0.5f ? 1 : 0);
    i_o = (uint32_t)i;
    return m == m && f >= -1.0f && f < 4294967296.0f && i >= 0 && i < (long long)extent;      // (f outside the range of the conversion: outside the map)
}

__global__ void __launch_bounds__(256) k_label_gather(LabelGatherArgs a)
{
    PixelTile tile;
    if (!pixel_tile(a.pass, tile)) return;
    const uint32_t p0 = tile.p0, n = a.pass.n;
    const size_t plane = (size_t)a.E * a.R, frame = plane * a.K;
    size_t at[4]; bool in[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        uint32_t z = 0u, x, y;
        in[j] = label_nearest(a.map_col[p0 + 64 * j], a.E, x);
        in[j] = label_nearest(a.map_row[p0 + 64 * j], a.R, y) && in[j];
        if (a.map_plane) in[j] = label_nearest(a.map_plane[p0 + 64 * j], a.K, z) && in[j];
        at[j] = in[j] ? (size_t)z * plane + (size_t)x * a.R + y : 0;
    }
    for (uint32_t f = tile.f0; f < tile.f1; f++) {
        const uint8_t *src = a.src + (size_t)f * frame;
        uint32_t bytes = 0u;                                // byte j: point p0 + 64 j
#pragma unroll
        for (int j = 0; j < 4; j++) bytes |= (in[j] ? (uint32_t)src[at[j]] : MCRT_LABEL_NONE) << (8 * j);
        tile_store_u8(a.out + (size_t)f * n, tile, n, bytes, a.pass.vec != 0u);
    }
}

hipError_t launch_label_gather(const LabelGatherArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(k_label_gather, pixel_grid(a.pass), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace mcrt
