// mcrt_walk.h -- the lane-per-ray walk's node and leaf steps, shared by the walk kernels (mcrt_walk.hip) and k_path (mcrt_path.hip)
#pragma once
#include "mcrt_device.h"

namespace mcrt {

// the four children's plane distances from a packed pair of half-float words: the contract's t = fl(plane * inv + c), c = -(o * inv),
// ONE mixed-precision fma per plane (v_fma_mix_f32 reads the half operand directly; op_sel picks the half of the word)
struct Planes4 { float a0, a1, b0, b1; };
MCRT_DEV Planes4 planes4(uint32_t w01, uint32_t w23, float c, float inv)
{
    Planes4 r;
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel_hi:[1,0,0]" : "=v"(r.a0) : "v"(w01), "v"(inv), "v"(c));
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r.a1) : "v"(w01), "v"(inv), "v"(c));
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel_hi:[1,0,0]" : "=v"(r.b0) : "v"(w23), "v"(inv), "v"(c));
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r.b1) : "v"(w23), "v"(inv), "v"(c));
    return r;
}

// ---- the lane-per-ray walk's two steps ---------------------------------------------------------------------------------
// A lane's traversal stack: entries [sb, sp), entry e of thread t at lds[e * 256 + t] while e < MCRT_LANE_STACK, beyond that in the
// global overflow array (only reachable on degenerate paths of deep trees).
template <int STACK> struct LaneStackT { int *lds; int *ovf; size_t ovf_stride; int tid; static constexpr int depth = STACK; };     // depth: entries in LDS
constexpr int CUR_IDLE = (int)0x80000000;      // walk state: cur >= 0 inner node, cur < 0 ~(leaf descriptor), CUR_IDLE = no walk in progress
template <class LS> MCRT_DEV void lane_pop(const LS &S, int &cur, int &sp, int sb)
{
    if (sp > sb) {
        sp--;
        // (the overflow part is asked for the whole wavefront first: the general form alone computes the 64-bit overflow address in every popping lane and reads through a flat load)
        if (__builtin_expect(__any(sp >= LS::depth), 0)) cur = (sp < LS::depth) ? S.lds[sp * 256 + S.tid] : S.ovf[(size_t)(sp - LS::depth) * S.ovf_stride];
        else cur = S.lds[sp * 256 + S.tid];
    }
    else cur = CUR_IDLE;
}
template <class LS> MCRT_DEV void lane_push(const LS &S, int &sp, int v)
{
    if (sp < LS::depth) S.lds[sp * 256 + S.tid] = v; else S.ovf[(size_t)(sp - LS::depth) * S.ovf_stride] = v;
    sp++;
}
struct LaneRay { float cx, cy, cz, ix, iy, iz; bool nx, ny, nz; };     // c = -(origin * reciprocal direction) and the reciprocal direction; reciprocal negative?
// wave masks of the lanes on an inner node, parked on a leaf, walking at all (cur as above; one scalar compare each)
#define MCRT_ON_INNER(c) __builtin_amdgcn_sicmp((c), -1, 38)
#define MCRT_ON_LEAF(c) __builtin_amdgcn_uicmp((uint32_t)(c), 0x80000000u, 34)
#define MCRT_WALKING(c) __builtin_amdgcn_sicmp((c), CUR_IDLE, 33)

// slab interval of one child from the distances of its three NEAR and three FAR planes
MCRT_DEV bool slab_near_far(float nx, float ny, float nz, float fx, float fy, float fz, float tlow, float tcap, float &tmin_o)
{
    float tmin, tmax;
    asm("v_max_f32 %0, %1, %2" : "=v"(nz) : "v"(nz), "v"(tlow));
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(tmin) : "v"(nx), "v"(ny), "v"(nz));
    asm("v_min_f32 %0, %1, %2" : "=v"(fz) : "v"(fz), "v"(tcap));
    asm("v_min3_f32 %0, %1, %2, %3" : "=v"(tmax) : "v"(fx), "v"(fy), "v"(fz));
    tmin_o = tmin;
    return tmin <= tmax;
}

// one inner node: the four children's slab tests, the nearest hit child next, the other hit children stacked in slot order
template <class LS> MCRT_DEV void lane_node_compute(const LS &S, const LaneRay &r, float t_lo, float tcap, const uint4 Q0, const uint4 Q1, const uint4 Q2, const uint4 RF, int &cur, int &sp, int sb);
template <class LS> MCRT_DEV void lane_node_step(const FrameArgs &a, const LS &S, const LaneRay &r, float t_lo, float tcap, int &cur, int &sp, int sb)
{
    const uint4 *N = (const uint4 *)((const char *)a.nodes_walk + ((uint32_t)cur << 6));
    const uint4 Q0 = N[0], Q1 = N[1], Q2 = N[2], RF = N[3];            // (as eight 8-byte pieces instead: 0.492 vs 0.427 ms per frame, round 3)
    lane_node_compute(S, r, t_lo, tcap, Q0, Q1, Q2, RF, cur, sp, sb);
}

template <class LS> MCRT_DEV void lane_node_compute(const LS &S, const LaneRay &r, float t_lo, float tcap, const uint4 Q0, const uint4 Q1, const uint4 Q2, const uint4 RF, int &cur, int &sp, int sb)
{
    // six plane distances of the four children
    // Which plane of a slab the ray meets first follows from the SIGN of the reciprocal direction (low plane for a positive one):
    // the packed words of the near and far planes are picked per axis (12 selects) instead of ordering the 24 distances afterwards
    // (24 min / max).  With low <= high and a monotone distance function the picked distances ARE the minimum and maximum whenever
    // both are numbers; where one is not (rays parallel to an axis) the interval comes out wider, never narrower -- a node may be
    // entered that min/max would have skipped, the triangle tests decide as before.
    const Planes4 XN = planes4(r.nx ? Q1.z : Q0.x, r.nx ? Q1.w : Q0.y, r.cx, r.ix), XF = planes4(r.nx ? Q0.x : Q1.z, r.nx ? Q0.y : Q1.w, r.cx, r.ix);
    const Planes4 YN = planes4(r.ny ? Q2.x : Q0.z, r.ny ? Q2.y : Q0.w, r.cy, r.iy), YF = planes4(r.ny ? Q0.z : Q2.x, r.ny ? Q0.w : Q2.y, r.cy, r.iy);
    const Planes4 ZN = planes4(r.nz ? Q2.z : Q1.x, r.nz ? Q2.w : Q1.y, r.cz, r.iz), ZF = planes4(r.nz ? Q1.x : Q2.z, r.nz ? Q1.y : Q2.w, r.cz, r.iz);
    float tn0, tn1, tn2, tn3;
    const bool h0 = slab_near_far(XN.a0, YN.a0, ZN.a0, XF.a0, YF.a0, ZF.a0, t_lo, tcap, tn0);
    const bool h1 = slab_near_far(XN.a1, YN.a1, ZN.a1, XF.a1, YF.a1, ZF.a1, t_lo, tcap, tn1);
    const bool h2 = slab_near_far(XN.b0, YN.b0, ZN.b0, XF.b0, YF.b0, ZF.b0, t_lo, tcap, tn2);
    const bool h3 = slab_near_far(XN.b1, YN.b1, ZN.b1, XF.b1, YF.b1, ZF.b1, t_lo, tcap, tn3);
    // nearest hit child first (key unique per node: t_near bits with the slot number in the two low bits), the others are
    // stacked in slot order -- exactly the quad walk's order
    const uint32_t k0 = h0 ? ((__float_as_uint(tn0) & ~3u) | 0u) : 0xffffffffu, k1 = h1 ? ((__float_as_uint(tn1) & ~3u) | 1u) : 0xffffffffu;
    const uint32_t k2 = h2 ? ((__float_as_uint(tn2) & ~3u) | 2u) : 0xffffffffu, k3 = h3 ? ((__float_as_uint(tn3) & ~3u) | 3u) : 0xffffffffu;
    const uint32_t kmin = min(min(k0, k1), min(k2, k3));
    typedef int vi4 __attribute__((ext_vector_type(4)));
    vi4 RV = { (int)RF.x, (int)RF.y, (int)RF.z, (int)RF.w };
    asm volatile("" : "+v"(RV));                                     // (the child references are fetched WITH the boxes, not after the tests in a second round trip:
                                                                     //  with the references only for nodes that have a hit child 0.440 vs 0.429 ms per frame, round 3)
    const int r0 = RV.x, r1 = RV.y, r2 = RV.z, r3 = RV.w;
    if (kmin == 0xffffffffu) { lane_pop(S, cur, sp, sb); return; }
    const bool e0 = k0 == kmin, e1 = k1 == kmin, e2 = k2 == kmin, e3 = k3 == kmin;
    const bool p0 = h0 && !e0, p1 = h1 && !e1, p2 = h2 && !e2, p3 = h3 && !e3;
    if (__builtin_expect(__any(sp + 4 > LS::depth), 0)) {       // (some lane may leave the LDS part: the general form)
        if (p0) lane_push(S, sp, r0);
        if (p1) lane_push(S, sp, r1);
        if (p2) lane_push(S, sp, r2);
        if (p3) lane_push(S, sp, r3);
    } else {
        // four UNCONDITIONAL stores instead of four branches: a reference that is not kept is overwritten by the next one (its
        // offset does not advance), and the last lands above the new top of the stack (inside the lane's column: sp + 3 < 32)
        // (offsets as 0 / 1 counts shifted into the address -- v_lshl_add_u32 with inline constants --: with 0 / 256 the step also paid for the literal and for a shift of the sum)
        char *top = (char *)&S.lds[sp * 256 + S.tid];
        int c0 = p0 ? 1 : 0, c1 = p1 ? 1 : 0, c2 = p2 ? 1 : 0, c3 = p3 ? 1 : 0;
        asm("" : "+v"(c0), "+v"(c1), "+v"(c2));      // (opaque: seen through, every shifted count becomes a second select on a literal)
        char *t1 = top + (c0 << 10), *t2 = t1 + (c1 << 10), *t3 = t2 + (c2 << 10);
        *(int *)top = r0;
        *(int *)t1 = r1;
        *(int *)t2 = r2;
        *(int *)t3 = r3;
        sp += c0 + c1 + c2 + c3;
    }
    cur = e0 ? r0 : e1 ? r1 : e2 ? r2 : r3;      // (on the comparisons the pushes made already)
}

// one leaf: the contract's triangle test (btTriangleRaycastCallback::processTriangle behind the padded-bounds rule) on each of its
// triangles, then the next stack entry.  helper: the lane walks an adopted subtree (see k_trace_lane): a triangle at exactly the
// owner's closest fraction is a candidate.  Returns the number of triangles of the leaf.
template <class LS> MCRT_DEV uint32_t lane_leaf_test(const FrameArgs &a, const LS &S, f3 f2, f3 to, f3 inv, f3 rc, float t_lo, bool helper, Best &best, int &cur, int &sp, int sb)
{
    const uint32_t v = (uint32_t)~cur;
    const uint32_t first = v >> 3, cnt = (v & 7u) + 1u;
    for (uint32_t k = 0; k < cnt; k++) {
        const float4 *T = (const float4 *)((const char *)a.tris + (first + k) * (uint32_t)(16 * MCRT_TRI_PIECES));
        // the record's pieces are fetched TOGETHER, not stage by stage behind the early exits: a leaf phase then costs one
        // memory round trip (the pieces of a rejected triangle are wasted loads; staged: 0.349 against 0.343 ms per frame, round 4)
        typedef float vf4 __attribute__((ext_vector_type(4)));
        vf4 W0 = ((const vf4 *)T)[0], W1 = ((const vf4 *)T)[1], W2 = ((const vf4 *)T)[2];
        asm volatile("" : "+v"(W0), "+v"(W1), "+v"(W2));      // (pinned as three register tuples: pinned word by word the compiler copied seven of them out of the tuples first)
        const float4 V0 = make_float4(W0.x, W0.y, W0.z, W0.w), V1 = make_float4(W1.x, W1.y, W1.z, W1.w), V2 = make_float4(W2.x, W2.y, W2.z, W2.w);
        const float4 P = tri_plane(xyz(V0), xyz(V1), xyz(V2));
        const f3 nrm = xyz(P);
        const float da = dot(nrm, f2) - P.w;
        const float db = dot(nrm, to) - P.w;
        if (da * db >= 0.0f) continue;
        const int id = __float_as_int(V0.w);
        const float proj = da - db;
        const float frac = da / proj;
        if (!(frac < best.frac || (frac == best.frac && (id < best.tri || (helper && best.tri < 0)))) || !(frac >= t_lo)) continue;
        float tmin, tmax;
        f3 plo, phi;
        tri_padded_bounds(xyz(V0), xyz(V1), xyz(V2), a.pad_abs, plo, phi);
        if (!(slab_c(plo, phi, rc, inv, 0.0f, 1.0f, tmin, tmax) && frac >= tmin && frac <= tmax)) continue;
        const float edge_tol = V2.w;
        const float s = 1.0f - frac;
        const f3 p = mk(s * f2.x + frac * to.x, s * f2.y + frac * to.y, s * f2.z + frac * to.z);
        const f3 p0 = xyz(V0) - p, p1 = xyz(V1) - p, p2 = xyz(V2) - p;
        if (!(dot(cross(p0, p1), nrm) >= edge_tol)) continue;
        if (!(dot(cross(p1, p2), nrm) >= edge_tol)) continue;
        if (!(dot(cross(p2, p0), nrm) >= edge_tol)) continue;
        best.frac = frac; best.tri = id;
    }
    lane_pop(S, cur, sp, sb);
    return cnt;
}

// ---- triangles through the SCALAR cache (k_trace_packet's leaves, k_beam_test's candidates): the record is wave-uniform, every lane tests it against ITS ray ----
typedef uint32_t u32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
MCRT_DEV u32x16 sload16(const void *p) { u32x16 r; asm volatile("s_load_dwordx16 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(r) : "s"(p) : "memory"); return r; }
MCRT_DEV u32x8 sload8(const void *p) { u32x8 r; asm volatile("s_load_dwordx8 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(r) : "s"(p) : "memory"); return r; }
MCRT_DEV u32x4 sload4(const void *p) { u32x4 r; asm volatile("s_load_dwordx4 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(r) : "s"(p) : "memory"); return r; }

// the contract's triangle test of one wave-uniform record (A: v0 | id, v1 | -; C2: v2 | edge tolerance) by every lane `on`, with the early exits of a
// wavefront: lane_leaf_test's expressions, so a lane's closest hit is the lane walk's bit for bit
MCRT_DEV void packet_tri_test(const u32x8 A, const u32x4 C2, const f3 f2, const f3 to, const f3 inv, const f3 rc, const float pad_abs, const bool on, Best &best)
{
    const f3 v0 = mk(__uint_as_float(A[0]), __uint_as_float(A[1]), __uint_as_float(A[2])), v1 = mk(__uint_as_float(A[4]), __uint_as_float(A[5]), __uint_as_float(A[6]));
    const f3 v2 = mk(__uint_as_float(C2[0]), __uint_as_float(C2[1]), __uint_as_float(C2[2]));
    const int id = (int)A[3];
    const float edge_tol = __uint_as_float(C2[3]);
    const float4 P = tri_plane(v0, v1, v2);
    const f3 nrm = xyz(P);
    const float da = dot(nrm, f2) - P.w;
    const float db = dot(nrm, to) - P.w;
    bool ok = on && da * db < 0.0f;
    if (!__any(ok)) return;
    const float proj = da - db;
    const float frac = da / proj;
    ok = ok && (frac < best.frac || (frac == best.frac && id < best.tri)) && frac >= 0.0f;
    if (!__any(ok)) return;
    float tmin, tmax;
    f3 plo, phi;
    tri_padded_bounds(v0, v1, v2, pad_abs, plo, phi);
    ok = ok && slab_c(plo, phi, rc, inv, 0.0f, 1.0f, tmin, tmax) && frac >= tmin && frac <= tmax;
    if (!__any(ok)) return;
    const float s = 1.0f - frac;
    const f3 p = mk(s * f2.x + frac * to.x, s * f2.y + frac * to.y, s * f2.z + frac * to.z);
    const f3 p0 = v0 - p, p1 = v1 - p, p2 = v2 - p;
    ok = ok && dot(cross(p0, p1), nrm) >= edge_tol && dot(cross(p1, p2), nrm) >= edge_tol && dot(cross(p2, p0), nrm) >= edge_tol;
    if (ok) { best.frac = frac; best.tri = id; }
}

}  // namespace mcrt
