// mcrt_walk.hip -- the closest-hit walk of the staged pipeline (Bullet's rayTest, scene.cpp:115-126): k_trace_lane / k_trace_lane_wide,
// one lane per ray, and k_trace_packet, one wavefront per ray packet; k_nodes_walk / k_nodes_walk_decode, the walk's 64-byte nodes.
#include <hip/hip_fp16.h>
#include "mcrt_device.h"
#include "mcrt_walk.h"

#ifndef MCRT_LANE_VGPRS
#define MCRT_LANE_VGPRS 104          // register budget of k_trace_lane: four of its wavefronts per SIMD (1024 persistent workgroups, 4 per CU) take 416 of the
#endif                               // SIMD's 512 registers and leave 96 for a k_march wavefront (80) beside them; at 96 (five wavefronts' worth, rounds 2-3)
                                     // the refill that rebuilds the ray from the path state spilled four registers
#ifndef MCRT_LANE_REFILL
#define MCRT_LANE_REFILL 16          // fetch and set up new rays once this many of a wavefront's 64 lanes are without one
#endif
#ifndef MCRT_LANE_ADOPT_STEPS
#define MCRT_LANE_ADOPT_STEPS 4      // while idle lanes wait for a subtree, the inner-node phase returns to the hand-over after this many steps
#endif
#ifndef MCRT_LANE_FETCH
#define MCRT_LANE_FETCH 128          // queue positions a wavefront claims per atomic in a LARGE launch (>= MCRT_LANE_FETCH_FROM items), 64 below: measured
#endif                               // 0.434 / 0.426 / 0.426 ms per frame with 64 / 128 / 256 at 128 frames in flight (16.7 M items), 0.523 / 0.531 with 64 / 128 on
#ifndef MCRT_LANE_FETCH_SMALL
#define MCRT_LANE_FETCH_SMALL 64
#endif
#ifndef MCRT_LANE_FETCH_FROM         // a 20-frame pass (2.6 M items: what a wavefront holds back at the end of the queue weighs more there)
#define MCRT_LANE_FETCH_FROM 4194304
#endif

namespace mcrt {

// ray parameter interval [tmin,tmax] (clamped to [tlow,tcap]) in which o + t*d lies inside the box
MCRT_DEV bool slab(f3 lo, f3 hi, f3 o, f3 inv, float tlow, float tcap, float &tmin_o, float &tmax_o)
{
    float t0x = (lo.x - o.x) * inv.x, t1x = (hi.x - o.x) * inv.x;
    float t0y = (lo.y - o.y) * inv.y, t1y = (hi.y - o.y) * inv.y;
    float t0z = (lo.z - o.z) * inv.z, t1z = (hi.z - o.z) * inv.z;
    float tmin = fmaxf(fmaxf(fminf(t0x, t1x), fminf(t0y, t1y)), fmaxf(fminf(t0z, t1z), tlow));
    float tmax = fminf(fminf(fmaxf(t0x, t1x), fmaxf(t0y, t1y)), fminf(fmaxf(t0z, t1z), tcap));
    tmin_o = tmin; tmax_o = tmax;
    return tmin <= tmax;
}

// pieces per ray for a bounce with n rays: the largest power of two <= limit / n, at most 16 (1 when the bounce is large)
MCRT_DEV uint32_t ksplit(uint32_t n, uint32_t limit)
{
    uint32_t k = 1u;
    while (k < 16u && n * (k * 2u) <= limit) k *= 2u;
    return k;
}

// =============================================================================================================
// k_trace_lane -- the closest-hit walk (Bullet's rayTest, scene.cpp:115-126), ONE LANE per ray, 64 rays per wavefront.
//
// (Round 1 walked a ray with a quad of four lanes, one child of the BVH4 node each: 16 rays in flight per wavefront, with the
// counters showing its wavefronts parked on memory for more than half of their life -- latency-bound.  One lane per ray puts
// four times as many rays behind every wavefront and spends fewer instructions per ray: no quad ranking exchanges, and the
// slab planes of two children at a time go through the packed-f32 pipe.)
//
// Nodes are read from a COMPACT copy of the BVH4 (k_nodes_walk): 64 bytes per node instead of 128 -- the walk is bound by the
// vector memory pipe (tools/fetch_roof.hip: a scattered 16-byte-per-lane load costs the compute unit's TCP ~0.75 lanes per
// clock, whatever the cache level), so what counts is the number of 16-byte pieces a lane fetches per node: four
//     lo.x[4] lo.y[4] | lo.z[4] hi.x[4] | hi.y[4] hi.z[4] | ref[4]          (boxes as IEEE half floats, child-transposed)
// instead of seven.  The halves are rounded OUTWARDS (lo down, hi up), so every stored box contains the builder's box: node
// boxes only ever cull, and the contract's closest hit does not depend on them as long as they contain their triangles'
// padded bounds -- hits stay bit-identical, the walk visits ~2.5 % more nodes (measured on the 1 M-triangle
// scene).  Unused slots are stored as the point box at +infinity, which no slab test hits (so the walk needs no EMPTY test).
// mcrt_get_bvh4 hands out the tree AS WALKED (the decoded boxes), so a CPU walk of it counts exactly this walk's visits.
// Per ray the arithmetic is the contract's slab test, (plane - origin) * reciprocal with the min / max combination of slab();
// the next node is the nearest hit child (key: t_near bits with the slot number in the two low bits), the other hit children
// are stacked in slot order -- the order, and therefore the visit counts, of a sequential walk.
// Traversal stacks: MCRT_LANE_STACK entries per lane in LDS ([entry][thread], conflict-free); deeper entries (only reachable on
// degenerate paths of deep trees) go to a global overflow array.
// =============================================================================================================
// float -> half, rounded towards -infinity / +infinity (integer steps on the half's bit pattern from the nearest-even conversion)
MCRT_DEV uint32_t half_towards(float x, bool up)
{
    __half h = __float2half_rn(x);
    uint32_t b = (uint32_t)__half_as_ushort(h);
    const float back = __half2float(h);
    if (x != x) return 0x7e00u;                                  // NaN stays NaN (never produced by the builders)
    if (up ? (back < x) : (back > x)) {                          // the nearest half lies on the wrong side: one step towards the target
        const bool neg = (b & 0x8000u) != 0u;
        if ((b & 0x7fffu) == 0u) b = up ? 0x0001u : 0x8001u;     // +-0 -> the smallest subnormal of the right sign
        else if (neg == up) b -= 1u;                             // magnitude shrinks: negative going up, positive going down
        else b += 1u;                                            // magnitude grows (0x7bff + 1 = 0x7c00 = infinity: still an outward bound)
    }
    b &= 0xffffu;
    // no subnormal halves (the walk's arithmetic then never depends on a denormal mode): snap outwards to 0 or +-2^-14
    if ((b & 0x7c00u) == 0u && (b & 0x03ffu) != 0u) {
        const bool neg = (b & 0x8000u) != 0u;
        b = up ? (neg ? 0x8000u : 0x0400u) : (neg ? 0x8400u : 0x0000u);
    }
    return b;
}
MCRT_DEV float half_bits_to_float(uint32_t b) { return __half2float(__ushort_as_half((unsigned short)b)); }

// the walk's 64-byte nodes from the builders' 128-byte ones
__global__ void k_nodes_walk(const float4 *in, uint32_t n_nodes, uint4 *out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes) return;
    uint32_t lo[3][4], hi[3][4]; int ref[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const float4 A = in[8 * (size_t)i + 2 * c], B = in[8 * (size_t)i + 2 * c + 1];
        ref[c] = __float_as_int(B.z);
        const bool empty = ref[c] == MCRT_BVH4_EMPTY;
        const float l[3] = { A.x, A.y, A.z }, h[3] = { A.w, B.x, B.y };
#pragma unroll
        for (int k = 0; k < 3; k++) { lo[k][c] = empty ? 0x7c00u : half_towards(l[k], false); hi[k][c] = empty ? 0x7c00u : half_towards(h[k], true); }
    }
    uint4 *o = out + 4 * (size_t)i;
#define MCRT_PACK4(v) (v)[0] | ((v)[1] << 16), (v)[2] | ((v)[3] << 16)
    o[0] = make_uint4(MCRT_PACK4(lo[0]), MCRT_PACK4(lo[1]));
    o[1] = make_uint4(MCRT_PACK4(lo[2]), MCRT_PACK4(hi[0]));
    o[2] = make_uint4(MCRT_PACK4(hi[1]), MCRT_PACK4(hi[2]));
    o[3] = make_uint4((uint32_t)ref[0], (uint32_t)ref[1], (uint32_t)ref[2], (uint32_t)ref[3]);
#undef MCRT_PACK4
}
// ... and back: the tree as the walk sees it, in the builders' layout (for mcrt_get_bvh4)
__global__ void k_nodes_walk_decode(const uint4 *in, uint32_t n_nodes, float4 *out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes) return;
    const uint4 q0 = in[4 * (size_t)i], q1 = in[4 * (size_t)i + 1], q2 = in[4 * (size_t)i + 2], q3 = in[4 * (size_t)i + 3];
    const uint32_t w[12] = { q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w };      // lo.x lo.y lo.z hi.x hi.y hi.z, two words each
    uint32_t ref[4] = { q3.x, q3.y, q3.z, q3.w };
#pragma unroll
    for (int c = 0; c < 4; c++) {
        float v[6];
#pragma unroll
        for (int k = 0; k < 6; k++) v[k] = half_bits_to_float((w[2 * k + (c >> 1)] >> ((c & 1) * 16)) & 0xffffu);
        const bool empty = (int)ref[c] == MCRT_BVH4_EMPTY;
        if (empty) { v[0] = v[1] = v[2] = INFINITY; v[3] = v[4] = v[5] = -INFINITY; }                 // the builders' own form of an unused slot
        out[8 * (size_t)i + 2 * c] = make_float4(v[0], v[1], v[2], v[3]);
        out[8 * (size_t)i + 2 * c + 1] = make_float4(v[4], v[5], __int_as_float((int)ref[c]), 0.0f);
    }
}

// position of the r-th (0-based) set bit of a 64-bit mask (r < popcount): binary search on popcounts
MCRT_DEV int nth_set_bit(unsigned long long m, uint32_t r)
{
    int base = 0;
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) {
        const unsigned long long low = m & ((1ull << w) - 1ull);
        const uint32_t c = (uint32_t)__popcll(low);
        if (r >= c) { r -= c; m >>= w; base += w; } else m = low;
    }
    return base;
}

// x = taken ? nx : x, in place (the hand-over of a subtree replaces a lane's ray state: trace_lane_body)
MCRT_DEV void take_if(float &x, float nx, unsigned long long m) { asm volatile("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(x) : "v"(nx), "s"(m)); }
MCRT_DEV void take_if(int &x, int nx, unsigned long long m) { asm volatile("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(x) : "v"(nx), "s"(m)); }
MCRT_DEV void take_if(uint32_t &x, uint32_t nx, unsigned long long m) { asm volatile("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(x) : "v"(nx), "s"(m)); }

template <bool STATS, int STACK, bool DYN>
MCRT_DEV void trace_lane_body(const FrameArgs &a, const uint32_t b)
{
    // the traversal stacks in LDS, [STACK][256]: entry sp of thread t at sp*256 + t -> conflict-free (DYN: sized at the launch, see k_trace_lane_wide)
    extern __shared__ int stack_dyn[];
    __shared__ int stack_fix[DYN ? 1 : STACK * 256];
    int *const stack = DYN ? stack_dyn : stack_fix;
    const int tid = threadIdx.x, lane = tid & 63;
    // Bounce 0 is special: every sample path of a scan-line starts as a copy of the same first_ray (scene.cpp:83-101), so only
    // ONE ray per (frame, scan-line) is walked -- the first sample's -- and k_shade hands its hit to all S samples.
    const uint32_t n_rays = (b == 0u) ? a.ne : a.counts[b];
    // When a bounce has far fewer rays than the GPU has lanes, each ray is cut into K sub-ranges of its parameter interval inside
    // the scene bounds and the K pieces are walked by K different lanes: the launch then lasts as long as the longest PIECE
    // instead of the longest ray.  Sub-ranges are half-open and partition [0,1), and every find goes through the ray's atomicMin
    // word, so the result is exactly the single-walk answer.
    const uint32_t K = ksplit(n_rays, a.ksplit_limit);
    const uint32_t n = n_rays * K;
    const size_t st_half = (size_t)(b & 1u) * a.ne * a.S;      // path state and closest-hit words in queue order, ping-pong by bounce parity
    const float4 *st0 = a.st0 + st_half, *st1 = a.st1 + st_half;   // (the ray is rebuilt from origin | length factor and direction: ray_of)
    const uint32_t ray_stride = (b == 0u) ? a.S : 1u;          // bounce 0: the first sample of each queued scan-line stands for all
    unsigned long long *keys = (b & 1u) ? a.key1 : a.key0;
    unsigned long long st_nodes = 0, st_tris = 0, st_q = 0;
    // (overflow entries of this lane: [entry - MCRT_LANE_STACK][grid thread])
    const LaneStackT<STACK> S = { stack, a.stack_ovf + ((size_t)blockIdx.x * 256 + tid), (size_t)gridDim.x * 256, tid };

    // WORK DISTRIBUTION, XCD-aware.  Workgroups are dealt round-robin to the 8 XCDs (workgroup w runs on XCD w % 8), each with
    // its own L2.  The queue is cut into 8 contiguous sub-queues, one per XCD, each with its own cursor: an XCD sweeps ITS part
    // of the queue in order, so the rays in flight on it belong to a few scan-lines (small L2 working set), and the returning
    // atomics that hand out the work go to 8 addresses instead of one (same-address atomics serialise in L2 at ~6 ns each).  A
    // wavefront whose sub-queue has run dry moves on to the next one, so the XCDs finish together.  Bounces with few items use
    // one queue.  The kernel is PERSISTENT over the bounce's queue: a lane whose ray is finished writes its hit word and takes
    // the next unclaimed item (from a wave-private pool refilled with one atomic on its XCD's cursor).
    const uint32_t X = (n >= (uint32_t)MCRT_XCD_MIN_ITEMS) ? (uint32_t)MCRT_XCDS : 1u;
    if (X == 1u && blockIdx.x * 256u >= n) return;
    const uint32_t x_shift = (X == 1u) ? 0u : 3u;
    uint32_t cur_x = blockIdx.x & (X - 1u), visited = 0;
#define MCRT_SUB_LO(sq) ((uint32_t)(((unsigned long long)n * (sq)) >> x_shift))
#define MCRT_SUB_STATIC(sq) (((gridDim.x - (sq) + X - 1u) >> x_shift) * 256u)
    uint32_t *cursors = a.cursors + (size_t)b * MCRT_XCDS * MCRT_CURSOR_STRIDE;
    uint32_t i = MCRT_SUB_LO(cur_x) + (blockIdx.x >> x_shift) * 256u + (uint32_t)tid;      // the first item of each lane is assigned statically
    if (i >= MCRT_SUB_LO(cur_x + 1u)) i = 0xffffffffu;
    uint32_t ray_id = 0;                         // queue position of the ray (and of its closest-hit word)
    bool exhausted = false, fresh = true;
    f3 f2 = mk(0, 0, 0), to = mk(1, 1, 1), inv = mk(1, 1, 1);
    float t_lo = 0.0f;
    Best best; best.frac = 1.0f; best.tri = -1;
    int sp = 0, sb = 0, cur = CUR_IDLE;          // the lane's stack entries live in [sb, sp): sb moves up when the bottom entry is given away (see below)
    bool shared = false;                         // another lane of the wavefront works on a subtree of this lane's ray: results meet in the ray's word
    bool helper = false;                         // this lane walks an adopted subtree: it starts from the owner's closest fraction WITHOUT the owner's
                                                 // triangle, so a triangle at exactly that fraction is a candidate (the word's atomicMin applies the id rule)
    uint32_t pool_next = 0, pool_end = 0; bool queue_empty = false;   // wave-uniform
    const uint32_t fetch = n >= (uint32_t)MCRT_LANE_FETCH_FROM ? (uint32_t)MCRT_LANE_FETCH : (uint32_t)MCRT_LANE_FETCH_SMALL;
    unsigned long long poll_old = 0; uint32_t poll_ray = 0; bool poll_pending = false;      // (see the end of the loop)
    MCRT_WATCHDOG_DECL()
    for (;;) {
        MCRT_WATCHDOG_CHECK()
        // ---- finished rays report and idle lanes take new ones, once enough of them wait (the code runs for the whole wavefront) ----
        // (once the queue has run dry, finished lanes report at once: they are the helpers of the donation step below)
        const bool do_refill = popc_mask(__ballot(cur == CUR_IDLE && !exhausted)) >= (uint32_t)MCRT_LANE_REFILL || MCRT_WALKING(cur) == 0ull ||
                               (queue_empty && __any(cur == CUR_IDLE && !fresh));
        if (do_refill) {
            if (cur == CUR_IDLE && !fresh) {
                if (best.tri >= 0) {
                    const unsigned long long word = ((unsigned long long)__float_as_uint(best.frac) << 32) | (unsigned long long)(uint32_t)best.tri;
                    if (K == 1u && !shared) keys[ray_id] = word;   // the only walker of this ray: a plain store
                    else atomicMin(&keys[ray_id], word);
                }
                fresh = true; shared = false; helper = false; i = 0xffffffffu;
            }
            // (Publishing finished rays WHILE the launch runs -- so that k_shade could start on them in the launch's tail -- needs a device-scope
            //  release here: the XCDs' L2s are not coherent with each other inside a launch.  Measured, round 4: __threadfence() + one atomic per
            //  refill round make a launch of the 20-frame pass 3.11 ms instead of 0.67, of a 128-frame pass 13.6 instead of 3.08.  Not done.)
            const bool need = fresh && !exhausted;
            const unsigned long long dynm = __ballot(need && i == 0xffffffffu);
            if (dynm) {
                while (pool_next >= pool_end && !queue_empty) {
                    uint32_t base = 0;
                    if (lane == 0) base = atomicAdd(&cursors[(size_t)cur_x * MCRT_CURSOR_STRIDE], fetch);
                    base = __shfl(base, 0, 64);
                    const uint32_t hi = MCRT_SUB_LO(cur_x + 1u);
                    const unsigned long long start = (unsigned long long)MCRT_SUB_LO(cur_x) + MCRT_SUB_STATIC(cur_x) + base;
                    if (start < hi) {
                        pool_next = (uint32_t)start; pool_end = min((uint32_t)start + fetch, hi);
                    }
                    else if (++visited >= X) queue_empty = true;      // (the launch enters its TAIL: it only finishes the rays in flight from here on.  Round 4 let the
                                                                      //  accumulation's stream wait for this moment -- a device word + hipStreamWaitValue32 --: slower)
                    else cur_x = (cur_x + 1u) & (X - 1u);
                }
                if (need && i == 0xffffffffu) {
                    const uint32_t mine = pool_next + (uint32_t)__popcll(dynm & ((1ull << lane) - 1ull));
                    if (queue_empty) i = n;
                    else if (mine < pool_end) i = mine;
                }
                const uint32_t taken = (uint32_t)__popcll(dynm);
                pool_next = (pool_next + taken < pool_end) ? pool_next + taken : pool_end;
            }
            if (need && i != 0xffffffffu) {
                if (i < n) {
                    uint32_t piece = 0u;                                 // the pieces of one ray land in different wavefronts
                    if (K == 1u) ray_id = i;                             // (no division on the common path)
                    else { piece = i / n_rays; ray_id = i - piece * n_rays; }
                    const float4 s0 = st0[(size_t)ray_id * ray_stride], s1 = st1[(size_t)ray_id * ray_stride];
                    const Ray ry = ray_of(mk(s0.x, s0.y, s0.z), mk(s1.x, s1.y, s1.z), s0.w, a);
                    f2 = ry.f2; to = ry.to;
                    const f3 d = to - f2;
                    inv = mk(rcp_dir(d.x), rcp_dir(d.y), rcp_dir(d.z));
                    t_lo = 0.0f;
                    float t_hi = 1.0f;
                    if (K > 1u) {
                        float tin, tout;
                        if (slab(mk(a.scene_lo[0], a.scene_lo[1], a.scene_lo[2]), mk(a.scene_hi[0], a.scene_hi[1], a.scene_hi[2]), f2, inv, 0.0f, 1.0f, tin, tout)) {
                            const float w = tout - tin;
                            if (piece > 0u) t_lo = tin + w * ((float)piece / (float)K);
                            if (piece + 1u < K) t_hi = tin + w * ((float)(piece + 1u) / (float)K);
                        } else if (piece > 0u) t_hi = 0.0f;
                    }
                    best.frac = t_hi; best.tri = -1;
                    sp = 0; sb = 0; shared = false; helper = false; cur = (a.n_nodes != 0u && t_lo < t_hi) ? 0 : CUR_IDLE; fresh = false;
                    if (STATS && piece == 0u) st_q++;
                } else exhausted = true;
            }
        }
        // (This block stands BEFORE the test below for a reason of code generation only -- without walking lanes there are no donors --: behind it the compiler
        //  kept a second copy of the ray's state and moved 16 registers over at the top of every round and back at its end; here it needs 73 registers, not 80.)
        // ---- the END of a launch (and one frame at a time, where a bounce has fewer rays than the GPU has lanes): the queue is
        // empty, lanes run out of rays while a few long walks go on.  Idle lanes then TAKE OVER SUBTREES: the k-th idle lane adopts
        // the bottom stack entry (the farthest, usually largest pending subtree) of the k-th lane that has one, with a copy of its
        // ray and its current closest fraction, walks it on its own stack, and reports through the ray's closest-hit word, whose
        // atomicMin is exactly the contract's (smaller fraction, then smaller triangle id) rule -- the answer is the single walk's.
        // A launch then ends after its wavefronts' remaining WORK, not after their longest walk.  (Not in the counting build, whose
        // visit counts are those of one walk per ray.)
        // Measured and not kept: the same hand-over BETWEEN wavefronts through tickets and entries in global memory
        // (the heaviest wavefront's walks are chains with little to give away: its 230-odd node steps stayed, the pushes' round
        // trips were added); one ray per four lanes at the start of a small launch; rays dealt out across the wavefronts.
        if (!STATS && __builtin_amdgcn_readfirstlane((int)queue_empty)) {      // (a SCALAR branch: as a lane condition the compiler copied the whole ray state, 16 registers, at the top of every round)
            const bool thief = cur == CUR_IDLE && fresh;
            const bool donor = cur != CUR_IDLE && sp > sb && sb < STACK;
            const unsigned long long tm = __ballot(thief), dm = __ballot(donor);
            if (tm != 0ull && dm != 0ull) {
                const unsigned long long below = (1ull << lane) - 1ull;
                const uint32_t pairs = (uint32_t)min(__popcll(tm), __popcll(dm));
                const uint32_t trank = (uint32_t)__popcll(tm & below), drank = (uint32_t)__popcll(dm & below);
                const bool take = thief && trank < pairs, give = donor && drank < pairs;
                const int src = take ? nth_set_bit(dm, trank) : lane;       // (k_path posts the donors' lanes in LDS instead: worth 4 % there, nothing here -- the hand-over only runs in a launch's tail)
                const int d_sb = __shfl(sb, src, 64);
                const float c0 = __shfl(f2.x, src, 64), c1 = __shfl(f2.y, src, 64), c2 = __shfl(f2.z, src, 64);
                const float c3 = __shfl(to.x, src, 64), c4 = __shfl(to.y, src, 64), c5 = __shfl(to.z, src, 64);
                const float c6 = __shfl(inv.x, src, 64), c7 = __shfl(inv.y, src, 64), c8 = __shfl(inv.z, src, 64);
                const float c9 = __shfl(t_lo, src, 64), c10 = __shfl(best.frac, src, 64);
                const uint32_t c11 = (uint32_t)__shfl((int)ray_id, src, 64);
                const int c12 = __shfl(best.tri, src, 64), c13 = __shfl((int)helper, src, 64);
                // (the state is replaced IN PLACE, one select per register on the takers' mask: written as assignments under `if (take)` the compiler kept
                //  a second copy of the ray's state for the branch and moved 16 registers over at the top of EVERY round of the walk, and back at its end)
                const unsigned long long tk = __ballot(take);
                const int got = stack[take ? d_sb * 256 + (tid & ~63) + src : tid];      // the donor's bottom entry (same wavefront, read before the donor moves on)
                take_if(cur, got, tk);
                take_if(f2.x, c0, tk); take_if(f2.y, c1, tk); take_if(f2.z, c2, tk);
                take_if(to.x, c3, tk); take_if(to.y, c4, tk); take_if(to.z, c5, tk);
                take_if(inv.x, c6, tk); take_if(inv.y, c7, tk); take_if(inv.z, c8, tk);
                take_if(t_lo, c9, tk); take_if(best.frac, c10, tk); take_if(best.tri, -1, tk); take_if(ray_id, c11, tk);
                take_if(sp, 0, tk); take_if(sb, 0, tk);
                fresh = fresh && !take;
                helper = take ? (c12 >= 0 || c13 != 0) : helper;         // (an owner without a find so far passes on the ray's own bound, which stays exclusive;
                                                                         // a lane that is itself a helper passes its owner's fraction on)
                sb += give ? 1 : 0;
                shared = shared || take || give;
            }
        }

        // (ONE way round the loop: with a second back edge from here -- `continue` -- the compiler kept two copies of the ray's state, one across the
        //  refill and one across the walk, and moved 16 registers over at the top of every round and back at its end)
        if (MCRT_WALKING(cur) == 0ull) { if (!__any(!exhausted)) break; }
        else {

        // ---- phase 1: inner nodes, until enough lanes are parked on a leaf ----
        const float tcap = fminf(1.0f, best.frac);               // best only changes in phase 2
        // (then phase 1 is cut short: see MCRT_LANE_ADOPT_STEPS; held as scalars -- as a per-lane condition it made the whole loop a divergent one)
        const int thieves_wait = __builtin_amdgcn_readfirstlane((!STATS && queue_empty && __any(cur == CUR_IDLE && fresh)) ? 1 : 0);
        int steps_left = thieves_wait ? MCRT_LANE_ADOPT_STEPS : 0x7fffffff;      // (one counter, no second condition in the loop)
        const f3 rc = ray_c(f2, inv);
        const LaneRay lr = { rc.x, rc.y, rc.z, inv.x, inv.y, inv.z, inv.x < 0.0f, inv.y < 0.0f, inv.z < 0.0f };
        for (;;) {
            const unsigned long long inner = MCRT_ON_INNER(cur);
            if (inner == 0ull) break;
            if (popc_mask(MCRT_ON_LEAF(cur)) >= (uint32_t)MCRT_LANE_LEAF_BATCH) break;     // (as 32-bit scalars: a 64-bit comparison is a vector instruction)
            if (--steps_left < 0) break;
            if (cur >= 0) {
                if (STATS) st_nodes++;
                lane_node_step(a, S, lr, t_lo, tcap, cur, sp, sb);
            }
        }
        // ---- phase 2: the parked leaves; the triangle test of the contract (btTriangleRaycastCallback::processTriangle behind
        // the padded-bounds rule), one lane per ray, same expressions as the quad walk's shared test ----
        if ((uint32_t)cur > 0x80000000u) {
            const uint32_t cnt = lane_leaf_test(a, S, f2, to, inv, rc, t_lo, helper, best, cur, sp, sb);
            if (STATS) st_tris += cnt;
        }

        // ---- walkers of ONE ray (the pieces of a cut ray, an owner and the lanes that took over its subtrees) meet in the ray's
        // closest-hit word: each publishes its find there and takes the smallest word back as its own closest hit, so a subtree or
        // piece behind another walker's hit is left as the single walk would leave it.  The word only ever holds real finds, and the
        // smallest of them is the answer, so cutting by it cannot cut the answer.  The returned word is looked at ONE round later
        // (its latency is then behind the node fetches of the round in between).
        if (!STATS && (K > 1u || queue_empty)) {
            if (poll_pending) {
                poll_pending = false;
                const unsigned long long mine = ((unsigned long long)__float_as_uint(best.frac) << 32) | (unsigned long long)(uint32_t)best.tri;   // (no find: id 0xffffffff)
                if (poll_ray == ray_id && cur != CUR_IDLE && poll_old < mine) {
                    best.frac = __uint_as_float((uint32_t)(poll_old >> 32)); best.tri = (int)(uint32_t)poll_old; helper = false;
                }
            }
            if ((shared || K > 1u) && cur != CUR_IDLE) {
                const unsigned long long word = (best.tri >= 0) ? (((unsigned long long)__float_as_uint(best.frac) << 32) | (unsigned long long)(uint32_t)best.tri) : ~0ull;
                poll_old = atomicMin(&keys[ray_id], word); poll_ray = ray_id; poll_pending = true;
            }
        }
        }
    }
#undef MCRT_SUB_LO
#undef MCRT_SUB_STATIC
    if (STATS) {
        unsigned long long v[3] = { st_q, st_nodes, st_tris };
#pragma unroll
        for (int k = 0; k < 3; k++) {
            long long x = wave_sum_i64((long long)v[k]);
            if (lane == 0 && x) atomicAdd(&a.stats[k], (unsigned long long)x);
        }
    }
}

// The walk comes as TWO kernels around one body.  k_trace_lane is compiled for 96 registers (budget 104): four of its wavefronts per SIMD (1024
// persistent workgroups) beside one k_march wavefront, nothing spilled -- the form for small launches, whose time is a chain of dependent
// steps.  k_trace_lane_wide is compiled for FIVE wavefronts per SIMD beside that k_march wavefront (5 x 80 + 80 registers; 1280 workgroups;
// MCRT_LANE_WIDE_STACK LDS stack entries so that five workgroups and k_march's LDS fit a CU): the compiler spills a dozen registers, all of them
// in the refill, hand-over and reporting code outside the node and leaf loops.  Sensitivity builds (profiles/round4/exp_sensitivity.txt) had shown the
// walk at the knee of its two pipes with four wavefronts to hide latency behind; the fifth is worth 3-4 % of a 128-frame pass (0.330 against
// 0.342 ms per frame; 1.8 % at 96 frames, 1.4 % at 48, 0.5 % at 32), costs a 20-frame pass 1 % and one frame at a time 6 % -- so launch_trace
// took the wide form from 4 Mi queued rays (32 frames of the headline workload) upwards through round 5.  Round 6 (kernels built without machine LICM: the
// wide form spills 20 bytes per lane instead of 48, and the small passes that the narrow form was kept for run as k_path): the wide form wins at EVERY staged
// pass size -- 5 / 6 / 8 / 12 / 20 frames: 0.678 / 0.614 / 0.512 / 0.426 / 0.359 against 0.699 / 0.628 / 0.530 / 0.446 / 0.381 ms per frame -- so it is the
// default from the first ray (MCRT_LANE_WIDE_FROM), for trees the caches hold (mcrt_trace.cpp: fill_pass); the narrow form stays for larger trees, CU-masked
// streams and the counting build.  (Its stack is sized at the launch: with a static LDS array the compiler caps the kernel's occupancy
// by LDS and hands the registers back.)  Late round 6: with the hand-over in front of the walking test (trace_lane_body) the body needs 67 registers and no scratch in
// either form; a SIXTH walk wavefront per SIMD then fits (MCRT_LANE_WIDE_WAVES 7, 1536 workgroups): 0.345-0.348 against 0.340 ms on the 20-frame pass, 0.295-0.298
// against 0.300 at 128 frames -- five stay.
#ifndef MCRT_LANE_WIDE_STACK
#define MCRT_LANE_WIDE_STACK 24          // (28: 0.332 against 0.3295 ms per frame; deeper walks go on in the overflow array, as in the other form)
#endif
#ifndef MCRT_LANE_WIDE_FROM
#define MCRT_LANE_WIDE_FROM 1u
#endif
template <bool STATS>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_num_vgpr(MCRT_LANE_VGPRS))) k_trace_lane(FrameArgs a, uint32_t b)
{
    trace_lane_body<STATS, MCRT_LANE_STACK, false>(a, b);
}
#ifndef MCRT_LANE_WIDE_WAVES
#define MCRT_LANE_WIDE_WAVES 6           // wavefronts per SIMD k_trace_lane_wide's registers are budgeted for: five of its own + one of k_march (512 / 6 -> 80 registers)
#endif
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(MCRT_LANE_WIDE_WAVES, MCRT_LANE_WIDE_WAVES))) k_trace_lane_wide(FrameArgs a, uint32_t b)
{
    trace_lane_body<false, MCRT_LANE_WIDE_STACK, true>(a, b);
}

// =============================================================================================================
// k_trace_packet -- north_star's literal traversal: ONE WAVEFRONT PER RAY PACKET.  The 64 lanes of a wavefront hold 64 consecutive rays
// of the queue (neighbours: the sample paths of one scan-line with one reflect / refract history) and walk the BVH4 TOGETHER: one
// traversal stack for the wavefront (64 entries in ONE vector register, entry e in lane e), the current node wave-uniform and fetched
// through the SCALAR cache (one s_load_dwordx16 per node and wavefront instead of 64 lanes x four 16-byte pieces through the vector memory
// pipe -- the pipe that binds the lane walk), every lane tests the four child boxes against ITS ray with ITS closest fraction (the lane
// walk's arithmetic), a child is entered when ANY lane passes it, nearest first by the first passing lane's t_near; a leaf's triangles are
// fetched the same way and tested by every lane.  Legal under the contract: the closest hit (smaller fraction, then smaller triangle id, of
// the triangles whose padded bounds the ray passes) does not depend on the visiting order, boxes only cull, and a lane that does not pass a
// box passes nothing inside it -- so every lane gets exactly the lane walk's answer, bit for bit (the parity tests do not know which kernel ran).
// What it costs is counted in profiles/round5/packet_count_*.json: the packet visits the UNION of its rays' nodes -- 1.1 x the longest ray's at
// bounce 1, 1.7 x at bounce 2, 7 x at bounce 9 (a wavefront's 64 neighbours then belong to several histories) -- so launch_trace takes it only
// for the bounces named in FrameArgs::packet_mask.
// =============================================================================================================
// entry `l` (wave-uniform) of the wavefront's stack register becomes the wave-uniform value `v`: a vector compare and select (v_writelane_b32 wants the lane
// number in M0 and its moves on the scalar ALU, the pipe this kernel is short of)
MCRT_DEV int writelane(int v, int l, int old) { return (int)(threadIdx.x & 63u) == l ? v : old; }

// the same with the node's packed word in a SCALAR register (k_trace_packet: the node is wave-uniform)
MCRT_DEV Planes4 planes4_s(uint32_t w01, uint32_t w23, float c, float inv)
{
    Planes4 r;
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel_hi:[1,0,0]" : "=v"(r.a0) : "s"(w01), "v"(inv), "v"(c));
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r.a1) : "s"(w01), "v"(inv), "v"(c));
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel_hi:[1,0,0]" : "=v"(r.b0) : "s"(w23), "v"(inv), "v"(c));
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r.b1) : "s"(w23), "v"(inv), "v"(c));
    return r;
}

// one compare-and-swap of the packet's sorting network: the pair with the smaller key goes first
MCRT_DEV void pk_cas(uint32_t &ka, int &ra, uint32_t &kb, int &rb)
{
    const bool sw = kb < ka;
    const uint32_t kl = sw ? kb : ka, kh = sw ? ka : kb;
    const int rl = sw ? rb : ra, rh = sw ? ra : rb;
    ka = kl; kb = kh; ra = rl; rb = rh;
}

// the packet's walk.  SGN: 0..7 = every ray of the packet runs the same way along every axis, bit 0 / 1 / 2 = towards -x / -y / -z (a bundle's rays differ by a
// fraction of a degree: the common case) -- which plane of a slab is the near one is then a COMPILE-TIME pick and the 24 plane distances read the node's words
// straight from scalar registers; 8 = mixed directions, picked per lane.  (The scalar ALU is this kernel's scarce pipe -- one per CU, and every step of every
// wavefront needs its ballots, keys and stack moves there: 12 selects per step are worth eight copies of the loop.)
template <int SGN>
MCRT_DEV void packet_walk(const FrameArgs &a, const LaneRay &lr, const f3 f2, const f3 to, const f3 inv, const f3 rc, Best &best)
{
    constexpr bool UNI = SGN < 8, NX = (SGN & 1) != 0, NY = (SGN & 2) != 0, NZ = (SGN & 4) != 0;
    int stk = 0;                                                          // the wavefront's traversal stack: entry e in lane e
    int sp = 0, cur = 0;                                                  // wave-uniform
    const unsigned long long wd_start = wall_clock64(); uint32_t wd_iter = 0;
    for (;;) {
        if ((++wd_iter & 4095u) == 0u && wall_clock64() - wd_start > (unsigned long long)MCRT_WATCHDOG_SECONDS * 100000000ull) { if ((threadIdx.x & 63) == 0) atomicOr(a.error_flag, 2u); break; }
        if (cur >= 0) {
            // the node: through the scalar cache, one load per wavefront
            // (words: lo.x[4] lo.y[4] | lo.z[4] hi.x[4] | hi.y[4] hi.z[4] | ref[4]; two halves per word)
            const u32x16 N = sload16((const char *)a.nodes_walk + ((size_t)(uint32_t)cur << 6));
            const uint32_t lox0 = N[0], lox1 = N[1], loy0 = N[2], loy1 = N[3], loz0 = N[4], loz1 = N[5], hix0 = N[6], hix1 = N[7], hiy0 = N[8], hiy1 = N[9], hiz0 = N[10], hiz1 = N[11];
            const float tcap = fminf(1.0f, best.frac);
            float tn0, tn1, tn2, tn3;
            bool h0, h1, h2, h3;
            if (UNI) {
                const Planes4 XN = planes4_s(NX ? hix0 : lox0, NX ? hix1 : lox1, lr.cx, lr.ix), XF = planes4_s(NX ? lox0 : hix0, NX ? lox1 : hix1, lr.cx, lr.ix);
                const Planes4 YN = planes4_s(NY ? hiy0 : loy0, NY ? hiy1 : loy1, lr.cy, lr.iy), YF = planes4_s(NY ? loy0 : hiy0, NY ? loy1 : hiy1, lr.cy, lr.iy);
                const Planes4 ZN = planes4_s(NZ ? hiz0 : loz0, NZ ? hiz1 : loz1, lr.cz, lr.iz), ZF = planes4_s(NZ ? loz0 : hiz0, NZ ? loz1 : hiz1, lr.cz, lr.iz);
                h0 = slab_near_far(XN.a0, YN.a0, ZN.a0, XF.a0, YF.a0, ZF.a0, 0.0f, tcap, tn0);
                h1 = slab_near_far(XN.a1, YN.a1, ZN.a1, XF.a1, YF.a1, ZF.a1, 0.0f, tcap, tn1);
                h2 = slab_near_far(XN.b0, YN.b0, ZN.b0, XF.b0, YF.b0, ZF.b0, 0.0f, tcap, tn2);
                h3 = slab_near_far(XN.b1, YN.b1, ZN.b1, XF.b1, YF.b1, ZF.b1, 0.0f, tcap, tn3);
            } else {
                const Planes4 XN = planes4(lr.nx ? hix0 : lox0, lr.nx ? hix1 : lox1, lr.cx, lr.ix), XF = planes4(lr.nx ? lox0 : hix0, lr.nx ? lox1 : hix1, lr.cx, lr.ix);
                const Planes4 YN = planes4(lr.ny ? hiy0 : loy0, lr.ny ? hiy1 : loy1, lr.cy, lr.iy), YF = planes4(lr.ny ? loy0 : hiy0, lr.ny ? loy1 : hiy1, lr.cy, lr.iy);
                const Planes4 ZN = planes4(lr.nz ? hiz0 : loz0, lr.nz ? hiz1 : loz1, lr.cz, lr.iz), ZF = planes4(lr.nz ? loz0 : hiz0, lr.nz ? loz1 : hiz1, lr.cz, lr.iz);
                h0 = slab_near_far(XN.a0, YN.a0, ZN.a0, XF.a0, YF.a0, ZF.a0, 0.0f, tcap, tn0);
                h1 = slab_near_far(XN.a1, YN.a1, ZN.a1, XF.a1, YF.a1, ZF.a1, 0.0f, tcap, tn1);
                h2 = slab_near_far(XN.b0, YN.b0, ZN.b0, XF.b0, YF.b0, ZF.b0, 0.0f, tcap, tn2);
                h3 = slab_near_far(XN.b1, YN.b1, ZN.b1, XF.b1, YF.b1, ZF.b1, 0.0f, tcap, tn3);
            }
            // WHICH children: any lane's.  In WHICH ORDER: nearest first by the t_near of the FIRST lane that passes each (one v_readlane per entered child; bits
            // order like the value, t_near >= 0; the slot in the two low bits makes the keys distinct).  Sorted pushes cost scalar work but save visits: with the
            // lane walk's rule instead (nearest first, the others in slot order: one v_readlane, no sort) the packet ran 1 % slower (profiles/round5/exp_packet.txt).
            const unsigned long long m0 = __ballot(h0), m1 = __ballot(h1), m2 = __ballot(h2), m3 = __ballot(h3);
            const int r0 = (int)N[12], r1 = (int)N[13], r2 = (int)N[14], r3 = (int)N[15];
            const uint32_t nh = (m0 ? 1u : 0u) + (m1 ? 1u : 0u) + (m2 ? 1u : 0u) + (m3 ? 1u : 0u);
            if (nh == 1u) { cur = m0 ? r0 : m1 ? r1 : m2 ? r2 : r3; continue; }          // one child entered: no order to work out, nothing to stack
            if (nh >= 2u) {
                uint32_t k0 = 0xffffffffu, k1 = 0xffffffffu, k2 = 0xffffffffu, k3 = 0xffffffffu;
                if (m0) k0 = ((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(tn0), __ffsll((long long)m0) - 1) & ~3u) | 0u;
                if (m1) k1 = ((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(tn1), __ffsll((long long)m1) - 1) & ~3u) | 1u;
                if (m2) k2 = ((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(tn2), __ffsll((long long)m2) - 1) & ~3u) | 2u;
                if (m3) k3 = ((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(tn3), __ffsll((long long)m3) - 1) & ~3u) | 3u;
                // a sorting network on the four (key, reference) pairs: five compare-and-swaps
                int a0 = r0, a1 = r1, a2 = r2, a3 = r3;
                pk_cas(k0, a0, k1, a1); pk_cas(k2, a2, k3, a3); pk_cas(k0, a0, k2, a2); pk_cas(k1, a1, k3, a3); pk_cas(k1, a1, k2, a2);
                if (sp + nh - 1u > (uint32_t)MCRT_STACK) { if ((threadIdx.x & 63) == 0) atomicOr(a.error_flag, 1u); break; }      // nh - 1 entries go onto the 64-lane stack register; trees whose worst case needs more than MCRT_STACK are refused at upload, so this guards the register, never silently
                if (k3 != 0xffffffffu) { stk = writelane(a3, sp, stk); sp++; }     // farthest first: the nearest pops first
                if (k2 != 0xffffffffu) { stk = writelane(a2, sp, stk); sp++; }
                stk = writelane(a1, sp, stk); sp++;
                cur = a0;
                continue;
            }
        } else {
            const uint32_t v = (uint32_t)~cur;
            const uint32_t first = v >> 3, cnt = (v & 7u) + 1u;
            for (uint32_t k = 0; k < cnt; k++) {
                const char *T = (const char *)a.tris + (size_t)(first + k) * (16u * MCRT_TRI_PIECES);
                const u32x8 A = sload8(T); const u32x4 C2 = sload4(T + 32);
                packet_tri_test(A, C2, f2, to, inv, rc, a.pad_abs, true, best);
            }
        }
        if (sp == 0) break;
        sp = __builtin_amdgcn_readfirstlane(sp - 1);
        cur = __builtin_amdgcn_readlane(stk, sp);
    }
}

__global__ void __launch_bounds__(64) k_trace_packet(FrameArgs a, uint32_t b)
{
    const uint32_t n_rays = a.counts[b];
    const uint32_t lane = threadIdx.x;
    const uint32_t base = blockIdx.x * 64u;
    if (base >= n_rays || a.n_nodes == 0u) return;
    const uint32_t i = base + lane;
    const bool live = i < n_rays;
    const uint32_t ray_id = live ? i : n_rays - 1u;
    const size_t st_half = (size_t)(b & 1u) * a.ne * a.S;
    const float4 s0 = a.st0[st_half + ray_id], s1 = a.st1[st_half + ray_id];
    const Ray ry = ray_of(mk(s0.x, s0.y, s0.z), mk(s1.x, s1.y, s1.z), s0.w, a);
    const f3 f2 = ry.f2, to = ry.to;
    const f3 d = to - f2;
    const f3 inv = mk(rcp_dir(d.x), rcp_dir(d.y), rcp_dir(d.z));
    const f3 rc = ray_c(f2, inv);
    const LaneRay lr = { rc.x, rc.y, rc.z, inv.x, inv.y, inv.z, inv.x < 0.0f, inv.y < 0.0f, inv.z < 0.0f };
    Best best; best.frac = live ? 1.0f : -1.0f; best.tri = -1;            // (a lane beyond the queue passes no box: its closest fraction is negative)
    // do all the packet's rays run the same way along every axis?  (lane 0 is live: base < n_rays)
    const int sgn = (lr.nx ? 1 : 0) | (lr.ny ? 2 : 0) | (lr.nz ? 4 : 0);
    const int sgn0 = __builtin_amdgcn_readfirstlane(sgn);
    const int which = __all(!live || sgn == sgn0) ? sgn0 : 8;               // wave-uniform
    switch (which) {
    case 0: packet_walk<0>(a, lr, f2, to, inv, rc, best); break;
    case 1: packet_walk<1>(a, lr, f2, to, inv, rc, best); break;
    case 2: packet_walk<2>(a, lr, f2, to, inv, rc, best); break;
    case 3: packet_walk<3>(a, lr, f2, to, inv, rc, best); break;
    case 4: packet_walk<4>(a, lr, f2, to, inv, rc, best); break;
    case 5: packet_walk<5>(a, lr, f2, to, inv, rc, best); break;
    case 6: packet_walk<6>(a, lr, f2, to, inv, rc, best); break;
    case 7: packet_walk<7>(a, lr, f2, to, inv, rc, best); break;
    default: packet_walk<8>(a, lr, f2, to, inv, rc, best); break;
    }
    if (live && best.tri >= 0) {
        unsigned long long *keys = (b & 1u) ? a.key1 : a.key0;
        keys[i] = ((unsigned long long)__float_as_uint(best.frac) << 32) | (unsigned long long)(uint32_t)best.tri;
    }
}

hipError_t launch_nodes_walk(const float4 *nodes, uint32_t n_nodes, uint4 *out, hipStream_t st)
{
    hipLaunchKernelGGL(k_nodes_walk, dim3((n_nodes + 255u) / 256u), dim3(256), 0, st, nodes, n_nodes, out);
    return hipGetLastError();
}
hipError_t launch_nodes_walk_decode(const uint4 *walk, uint32_t n_nodes, float4 *out, hipStream_t st)
{
    hipLaunchKernelGGL(k_nodes_walk_decode, dim3((n_nodes + 255u) / 256u), dim3(256), 0, st, walk, n_nodes, out);
    return hipGetLastError();
}

uint32_t lane_stack_entries() { return MCRT_LANE_STACK < MCRT_LANE_WIDE_STACK ? MCRT_LANE_STACK : MCRT_LANE_WIDE_STACK; }   // (the smaller of the two forms' LDS parts: sizes the overflow array)
uint32_t lane_wide_from() { return MCRT_LANE_WIDE_FROM; }

hipError_t launch_trace(const FrameArgs &a, uint32_t b, bool stats, hipStream_t st)
{
    // persistent over the bounce's queue: at most trace_blocks workgroups (the rest of the queue is fetched dynamically);
    // the live-ray count is only known on the device, surplus blocks read it and leave
    uint32_t np = (b == 0u) ? a.ne : a.ne * a.S;
    if (np < a.ksplit_limit) np = a.ksplit_limit;          // small bounces are cut into up to ksplit_limit pieces
    const uint32_t blocks = (np + 255u) / 256u;
    const dim3 grid(blocks < a.trace_blocks ? blocks : a.trace_blocks), blk(256);
    if (!stats && a.trace_blocks_wide != 0u && np >= a.wide_from && !(b >= 1u && b < 32u && ((a.packet_mask >> b) & 1u))) {          // a large launch: five wavefronts per SIMD (k_trace_lane_wide)
        const dim3 gridw(blocks < a.trace_blocks_wide ? blocks : a.trace_blocks_wide);
        hipLaunchKernelGGL(k_trace_lane_wide, gridw, blk, (size_t)MCRT_LANE_WIDE_STACK * 256 * sizeof(int), st, a, b);
        return hipGetLastError();
    }
    if (!stats && b >= 1u && b < 32u && ((a.packet_mask >> b) & 1u)) {       // a bounce walked a wavefront per ray packet (k_trace_packet)
        hipLaunchKernelGGL(k_trace_packet, dim3((a.ne * a.S + 63u) / 64u), dim3(64), 0, st, a, b);
        return hipGetLastError();
    }
    if (stats) hipLaunchKernelGGL((k_trace_lane<true>), grid, blk, 0, st, a, b);
    else hipLaunchKernelGGL((k_trace_lane<false>), grid, blk, 0, st, a, b);
    return hipGetLastError();
}

}  // namespace mcrt
