// mcrt_transmit.hip -- acoustic ground truth (mcrt_transmit_frames; the contract is in include/mcrt.h): k_transmit walks the central beam of
// every scan-line through the scene as k_label does and carries the tracer's intensity along it -- the attenuation of every segment
// (mcrt_shade.h: intensity * det_expf(...)), the impedance rule at every boundary (mcrt_transmit.h) -- into two float maps: the fraction of the
// emitted intensity that arrives at every RF row, the fraction every boundary turns back.
// The reference computes the quantity on every sample path (scene.cpp:122-165, ray.cpp:11-97) and keeps none of it.
#include "mcrt_walk.h"
#include "mcrt_transmit.h"

#ifndef MCRT_TRANSMIT_STACK
#define MCRT_TRANSMIT_STACK 16       // traversal-stack entries of a lane in LDS (the walk's steps index it with a stride of 256 lanes whatever the workgroup's size: 16 KB)
#endif

namespace mcrt {

// =============================================================================================================
// k_transmit -- k_label's shape: a workgroup is ONE wavefront, in phase 1 one lane walks one (frame, scan-line) with the lane walk's own node
// and leaf steps (the tracer's closest hits bit for bit), the label walk's row and medium rules, and at every boundary the intensity that
// arrives (Ia), what the boundary turns back (i_refl) and what goes on (I).  Every beam leaves its boundaries in LDS -- row, I behind, the
// attenuation behind, i_refl, the boundary's time (a double): 24 B x MCRT_LABEL_MAX_CROSSINGS x 64 lanes = 96 KB, with the traversal stack
// (16 KB) and the GEOMETRIC rule's open meshes (4 KB) 116 KB of the CU's 160: one workgroup per CU, which a pass of E x F beams does not
// fill anyway.  After the barrier phase 2 runs the lanes ALONG the rows: the workgroup's 64 scan-lines are 64 R consecutive floats of each
// map; a row finds its segment in its beam's list and evaluates ONE det_expf (the pass's only real arithmetic: F E R double-precision
// polynomials; mode is wave-uniform, MCRT_TRANSMIT_BOUNDARIES evaluates none).  16-byte stores where the address allows, single floats at
// the two ragged ends, chosen by the address: any float pointer is right.  No scratch.
// =============================================================================================================
struct TransmitLists { const uint32_t *row; const float *I, *att, *refl; const double *t; const uint32_t *count; float att0; };   // entry i of beam s at [64 i + s]

// transmit of row r of beam s: the segment behind the deepest boundary at or above the row (the rows ascend along a list)
template <bool TOTAL>
MCRT_DEV float transmit_row(const FrameArgs &a, const TransmitLists &l, uint32_t s, uint32_t r)
{
    const uint32_t n = l.count[s];
    int j = -1;
    for (uint32_t i = 0; i < n && l.row[64u * i + s] <= r; i++) j = (int)i;
    const float I = j < 0 ? 1.0f : l.I[64 * j + s];
    if (!TOTAL) return I;
    const float att = j < 0 ? l.att0 : l.att[64 * j + s];
    const double t_prev = j < 0 ? 0.0 : l.t[64 * j + s];
    double dt = (double)r * a.row_dt - t_prev;
    if (!(dt > 0.0)) dt = 0.0;
    const double mm = (dt * a.sos_d) / 1000.0;
    return I * det_expf(-att * ((float)mm * 0.01f) * a.freq);
}
// reflect of row r of beam s: the shallowest boundary that falls into it
MCRT_DEV float reflect_row(const TransmitLists &l, uint32_t s, uint32_t r)
{
    const uint32_t n = l.count[s];
    for (uint32_t i = 0; i < n; i++) { const uint32_t b = l.row[64u * i + s]; if (b == r) return l.refl[64u * i + s]; if (b > r) break; }
    return 0.0f;
}

// the workgroup's span of one map, o[0 .. span): WHAT 0 transmit in TOTAL mode, 1 transmit in BOUNDARIES mode, 2 reflect
template <int WHAT>
MCRT_DEV void transmit_store(const FrameArgs &a, const TransmitLists &l, float *o, uint32_t span, int tid)
{
    const uint32_t R = a.R;
    auto value = [&](uint32_t g) {
        const uint32_t s = g / R, r = g - s * R;
        return WHAT == 2 ? reflect_row(l, s, r) : transmit_row<WHAT == 0>(a, l, s, r);
    };
    const uint32_t head = min(span, (uint32_t)(((16u - ((uintptr_t)o & 15u)) & 15u) >> 2)), quads = (span - head) >> 2;
    for (uint32_t w = (uint32_t)tid; w < quads; w += 64u) {
        const uint32_t g = head + 4u * w;      // (a quad may begin in one scan-line and end in another)
        float4 v;
        v.x = value(g); v.y = value(g + 1u); v.z = value(g + 2u); v.w = value(g + 3u);
        *(float4 *)(o + g) = v;
    }
    // the ragged ends, float by float: [0, head) and [head + 4 quads, span)
    const uint32_t tail0 = head + 4u * quads, ragged = head + (span - tail0);
    if ((uint32_t)tid < ragged) {
        const uint32_t g = (uint32_t)tid < head ? (uint32_t)tid : tail0 + ((uint32_t)tid - head);
        o[g] = value(g);
    }
}

__global__ void __launch_bounds__(64) k_transmit(FrameArgs a, TransmitArgs l)
{
    __shared__ int stack[MCRT_TRANSMIT_STACK * 256];
    __shared__ double b_t[MCRT_LABEL_MAX_CROSSINGS * 64];       // [crossing][lane] the boundary's time
    __shared__ uint32_t b_row[MCRT_LABEL_MAX_CROSSINGS * 64];   // its row
    __shared__ float b_I[MCRT_LABEL_MAX_CROSSINGS * 64];        // the intensity that goes on behind it
    __shared__ float b_att[MCRT_LABEL_MAX_CROSSINGS * 64];      // the attenuation of the medium behind it (0 in BOUNDARIES mode)
    __shared__ float b_refl[MCRT_LABEL_MAX_CROSSINGS * 64];     // what it turns back
    __shared__ int open_mesh[16 * 64];                          // [depth][lane]  GEOMETRIC: the meshes the beam is inside of, innermost last
    __shared__ uint32_t count[64];
    const int tid = threadIdx.x;
    const uint32_t line0 = blockIdx.x * 64u, line = line0 + (uint32_t)tid;      // line = frame * ne_frame + scan-line: the outputs' own order
    const LaneStackT<MCRT_TRANSMIT_STACK> S = { stack, a.stack_ovf + ((size_t)blockIdx.x * 64 + tid), (size_t)gridDim.x * 64, tid };
    const bool total = l.mode == MCRT_TRANSMIT_TOTAL;
    bool active = line < a.ne;
    f3 from = mk(0, 0, 0), dir = mk(0, 0, 1);
    if (active) {
        const uint32_t fr = line / a.ne_frame, scan = line - fr * a.ne_frame;
        const size_t pe = (size_t)fr * a.pose_stride + a.e_begin + scan;
        from = mk(a.el_pos[3 * pe], a.el_pos[3 * pe + 1], a.el_pos[3 * pe + 2]);
        dir = mk(a.el_dir[3 * pe], a.el_dir[3 * pe + 1], a.el_dir[3 * pe + 2]);
    }
    double dist = 0.0;
    float I = 1.0f;
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
        // ---- the boundary: its row, what arrives, what it turns back, the medium behind it ----
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
                    const float4 *T = a.tris_id + MCRT_TRI_PIECES * (size_t)best.tri;
                    const float4 t1 = T[1];                                      // (v1, mesh)
                    const int mesh = __float_as_int(t1.w);
                    const uint4 organ = a.meshes[mesh];      // mat_inside, mat_outside, vascular
                    const float4 m0 = a.mats[2 * media];      // imp, att, .. of the medium the segment ran in
                    const float Ia = total ? I * det_expf(-m0.y * ((float)mm * 0.01f) * a.freq) : I;      // (shade_path's attenuation; att = 0.0f: I * 1)
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
                    // the impedance rule on the triangle's own plane normal: no random perturbation (the two candidates of inc are each other's negation, so
                    // the tracer's flip of the normal towards the origin changes nothing)
                    const float4 m2 = a.mats[2 * media];
                    const f3 nn = normalized(xyz(tri_plane(xyz(T[0]), xyz(t1), xyz(T[2]))));
                    float inc = dot(dir, neg(nn));
                    if (inc < 0) inc = dot(dir, nn);
                    float i_refl, i_refr;
                    transmit_boundary(m0.x, m2.x, inc, Ia, i_refl, i_refr);
                    I = i_refr > 0 ? i_refr : 0.0f;      // (a NaN or a negative remainder ends the energy, not the walk)
                    b_row[64u * k + tid] = (uint32_t)row; b_I[64u * k + tid] = I; b_att[64u * k + tid] = total ? m2.y : 0.0f;
                    b_refl[64u * k + tid] = i_refl; b_t[64u * k + tid] = t;
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
    const uint32_t lines = min(64u, a.ne - line0), span = lines * a.R;
    const TransmitLists tl = { b_row, b_I, b_att, b_refl, b_t, count, a.mats[2 * a.start_mat].y };
    if (l.transmit) {
        float *o = l.transmit + (size_t)line0 * a.R;
        if (total) transmit_store<0>(a, tl, o, span, tid); else transmit_store<1>(a, tl, o, span, tid);
    }
    if (l.reflect) transmit_store<2>(a, tl, l.reflect + (size_t)line0 * a.R, span, tid);
}

uint32_t transmit_blocks(size_t lines) { return (uint32_t)((lines + 63u) / 64u); }
uint32_t transmit_stack_entries() { return MCRT_TRANSMIT_STACK; }
hipError_t launch_transmit(const FrameArgs &a, const TransmitArgs &l, hipStream_t st)
{
    hipLaunchKernelGGL(k_transmit, dim3(transmit_blocks(a.ne)), dim3(64), 0, st, a, l);
    return hipGetLastError();
}

}  // namespace mcrt
