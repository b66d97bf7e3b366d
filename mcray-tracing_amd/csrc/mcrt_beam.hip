// mcrt_beam.hip -- bounces 1 .. MCRT_BEAM_LAST of a staged pass with ONE probe pose.  The rays of a scan-line leave bounce 0's hit point in a few narrow
// bundles, the same for every frame of the pass; at the next bounces the rays that left ONE triangle of a scan-line in one medium are such bundles again (their
// origins spread over the triangle).  Instead of walking the tree once per ray or per 64 rays, the triangles a bundle can meet are collected ONCE per bundle and
// every ray tests that short list, nearest first:
//
//   k_beam_clear    the reduction words, the group table, the bounce's counters, the leftover walk's counts and cursors
//   k_beam_bounds   per BEAM the bounds of the two slopes d_other / |d_dom|, of the start point f2 and of its coordinates' size, over (a sample of) the bounce's
//                   queue.  Bounce 1: a beam is scan-line x history (the medium says whether bounce 0 reflected) x dominant axis x its sign, addressed directly.
//                   Bounce b >= 2: the GROUP (scan-line, the triangle the ray left -- FrameArgs::from_tri, written by k_shade(b - 1) --, medium) claims a slot of
//                   a hash table with a compare-and-swap on its key word (MCRT_BEAM_PROBES slots are tried); a beam is slot x dominant axis x sign.  A ray whose
//                   group found no slot, or was not in the sample, is no member of any beam and is walked.
//   k_beam_rank     (bounces of MCRT_BEAM_ORDER) one lane per ray in queue order: its beam looked up (bounces >= 2: from the word k_shade(b - 1) stored for it, no ray rebuilt), one atomic per (wavefront, beam) on the beam's counter; every ray
//                   keeps its beam and its rank among the beam's rays.  A ray without a beam is counted into a pseudo-beam behind the last
//   k_beam_scan     ... a workgroup per 256 beams, none waiting for another: where every beam's SEGMENT of the order begins, each rounded up to whole wavefronts; the padding words, the totals
//   k_beam_place    ... order[base[beam] + rank] = the ray's queue position: a permutation of the queue grouped by beam
//   k_beam_collect  one workgroup per beam (bounce b >= 2: per slot, its 6 beams in turn): one traversal of the BVH4 with a conservative beam-against-box test, the leaf triangles tested by their own
//                   padded bounds, sorted by the depth at which they begin, the first `cap` copied into the beam's list (bounce b >= 2: a list of a pool,
//                   handed out to the beams that have members).  An entry is stored in two parts: the vertices, id, begin depth and edge tolerance (`list`, 64 bytes,
//                   mcrt_debug_beam_records' layout) and, beside them, what depends on the triangle alone and every test of the entry needs -- its plane and its
//                   padded bounds, by tri_plane / tri_padded_bounds -- with the begin depth and the id (`hot`, 48 bytes)
//   k_beam_test     one lane per ray in queue order, or through the beam order (then every wavefront holds ONE beam's rays): its beam looked up (the group's key compared), the contract's triangle test (list_tri_test: packet_tri_test's expressions on the stored plane and bounds,
//                   the vertices fetched only for the edge tests) over the beam's list in order, until the hit lies before everything not yet tested; lanes that cannot be decided are appended to a leftover queue
//   k_beam_gather, the lane walk, k_beam_scatter     the leftovers, walked as any other queue, in the halves of the other bounce parity
//
// EXACT: a ray's answer is the smallest (fraction, id) among the triangles that pass the contract's test, whatever the order and
// whatever else is tested.  A ray counts as a MEMBER of a beam only where comparisons prove it inside the beam's bounds (a NaN proves nothing) -- how rays are
// GROUPED into beams only decides how narrow the beams are --, the
// collection keeps every triangle whose padded bounds come within a margin m of the beam's volume -- m = 2^-18 x the largest coordinate of the start
// points and the scene, 16 x the rounding of the slab test and of the arithmetic here --, and a member is FINAL only when its hit lies more than 2 m before the depth at which
// the first untested triangle's padded bounds begin: a triangle accepted at a smaller or equal fraction has its hit inside its own padded bounds.
// The origins of a bounce b >= 2 spread over a triangle: the volume starts from the bounds of f2 (w is their extent along the dominant axis), and a ray whose
// coordinates are larger than the sampled members' is refused by the comparison with the record's size.  The triangle a ray left is among its candidates and is
// rejected by the contract's test exactly as the walk rejects it.
#include <hip/hip_fp16.h>
#include "mcrt_device.h"
#include "mcrt_walk.h"

// (20 KB of LDS in all: a beam's workgroup has to find room on a compute unit beside k_march of bounce 0, which runs on the side stream at that time -- with 40 KB
//  the launch ended when k_march did)
#define BEAM_CT 256u          // k_beam_collect: threads of a beam's workgroup (a level of the traversal holds up to a few hundred nodes)
#define BEAM_QN 512           // k_beam_collect: nodes of one level of the traversal (LDS)
#define BEAM_EN 1024          // ... and triangles of a beam before the cut to its capacity (LDS; the largest capacity)
#define BEAM_LN 2048          // ... and triangles of the leaves the traversal reaches, before their own bounds are tested (LDS)

namespace mcrt {

// floats as unsigned words of the same order (atomicMin / atomicMax)
MCRT_DEV uint32_t ford(float f) { const uint32_t b = __float_as_uint(f); return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
MCRT_DEV float funord(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }
MCRT_DEV float comp(f3 v, int k) { return k == 0 ? v.x : k == 1 ? v.y : v.z; }

// the slot of the group table that holds `key`, or -1.  claim: a free slot is taken (one compare-and-swap on its key word).  Slots are never given back during
// a bounce, so a key that is in the table is found by the same probes that put it there.
MCRT_DEV int beam_slot(const BeamArgs &g, unsigned long long key, bool claim)
{
    uint32_t h = ((uint32_t)key ^ (uint32_t)(key >> 32) * 0x9e3779b1u) * 2654435761u;
    h ^= h >> 15;
    for (uint32_t p = 0; p < MCRT_BEAM_PROBES; p++) {
        const uint32_t s = (h + p) & (g.groups - 1u);
        // (k_beam_test only reads the table: plain loads, served by the vector cache)
        unsigned long long k = claim ? __hip_atomic_load(&g.gkey[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : g.gkey[s];
        if (k == 0ull && claim) {
            k = atomicCAS(&g.gkey[s], 0ull, key);
            if (k == 0ull) { k = key; atomicAdd(&g.lcount[7], 1u); }
        }
        if (k == key) return (int)s;
        if (k == 0ull) return -1;
    }
    return -1;
}

// a queued ray of bounce g.b and the beam it would belong to (bid < 0: none)
struct BeamRay { f3 f2, to; float u, v, cmax, dd; int dom, bid; bool neg; };
MCRT_DEV bool beam_ray(const FrameArgs &a, const BeamArgs &g, uint32_t i, bool claim, BeamRay &r)
{
    const size_t half = (size_t)(g.b & 1u) * a.ne * a.S;
    const uint32_t pid = a.queue[half + i];
    const uint32_t line = pid / a.S, scan = line - (line / a.ne_frame) * a.ne_frame;
    const float4 s0 = a.st0[half + i], s1 = a.st1[half + i];
    const Ray ry = ray_of(mk(s0.x, s0.y, s0.z), mk(s1.x, s1.y, s1.z), s0.w, a);
    r.f2 = ry.f2; r.to = ry.to;
    const BeamDir bd = beam_dir(ry);      // (the one statement of dominant axis and sign: k_shade stores the same code for k_beam_rank)
    const f3 D = bd.D;
    r.dom = bd.dom;
    r.dd = comp(D, r.dom);
    const float ad = fabsf(r.dd);
    r.u = comp(D, (r.dom + 1) % 3) / ad; r.v = comp(D, (r.dom + 2) % 3) / ad;
    r.cmax = fmaxf(fmaxf(fabsf(r.f2.x), fabsf(r.f2.y)), fabsf(r.f2.z));
    r.neg = bd.neg;
    // every coordinate a number, the dominant component not 0 (then |u|, |v| <= 1)
    const float sum = fabsf(r.f2.x) + fabsf(r.f2.y) + fabsf(r.f2.z) + fabsf(r.to.x) + fabsf(r.to.y) + fabsf(r.to.z);
    const bool ok = sum < 1e30f && ad > 0.0f && fabsf(r.u) <= 1.0f && fabsf(r.v) <= 1.0f;
    const uint32_t code = beam_code(bd);
    if (g.groups == 0u) {
        const uint32_t hist = __float_as_int(s1.w) != (int)a.start_mat ? 1u : 0u;
        r.bid = (int)((scan * 2u + hist) * 6u + code);
    } else {
        r.bid = -1;
        if (ok) {
            const unsigned long long key = (1ull << 63) | ((unsigned long long)scan << 40) | ((unsigned long long)((uint32_t)__float_as_int(s1.w) & 0xffu) << 32)
                                           | (unsigned long long)a.from_tri[pid];
            const int slot = beam_slot(g, key, claim);
            if (slot >= 0) r.bid = slot * 6 + (int)code;
        }
    }
    return ok;
}

MCRT_DEV float wave_min(float x) { for (int o = 32; o > 0; o >>= 1) x = fminf(x, __shfl_xor(x, o, 64)); return x; }
MCRT_DEV float wave_max(float x) { for (int o = 32; o > 0; o >>= 1) x = fmaxf(x, __shfl_xor(x, o, 64)); return x; }

// reduction words of a beam: 0-4 minima (u, v, f2), 8-13 maxima (u, v, f2, size)
__global__ void __launch_bounds__(256) k_beam_clear(BeamArgs g)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < g.n_beams * MCRT_BEAM_REC) g.red[i] = (i & 8u) ? 0u : 0xffffffffu;
    if (i < g.groups) g.gkey[i] = 0ull;
    if (i < MCRT_BEAM_COUNTERS) g.lcount[i] = 0u;
    if (g.ordered && i <= g.n_beams) g.ocount[i] = 0u;
    if (i <= MCRT_MAX_BOUNCES) g.l_counts[i] = 0u;
    if (i < MCRT_MAX_BOUNCES * MCRT_XCDS) g.l_cursors[(size_t)i * MCRT_CURSOR_STRIDE] = 0u;
}

__global__ void __launch_bounds__(256) k_beam_bounds(FrameArgs a, BeamArgs g)
{
    const uint32_t n = a.counts[g.b];
    const uint32_t wave = (blockIdx.x * 256u + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    // one packet of 64 queue neighbours out of every `stride` is a sample of its beams -- WHICH one of the stride is a hash of the wavefront's number: k_shade
    // queues a workgroup's reflected rays first, so a fixed position repeats with the queue's period and can miss a history for good (every 16th packet of
    // 1024-sample scan-lines left a tenth of the rays without a beam)
    const uint32_t base = (wave * g.stride + ((wave * 2654435761u) >> 16) % g.stride) * 64u;
    if (base >= n) return;
    const uint32_t i = base + lane;
    BeamRay r; r.bid = -1;
    bool live = i < n && beam_ray(a, g, i, true, r);
    if (g.groups != 0u) {
        const unsigned long long lost = __ballot(live && r.bid < 0);
        if (lost && lane == 0u) atomicAdd(&g.lcount[6], (uint32_t)__popcll(lost));
        live = live && r.bid >= 0;
    }
    unsigned long long todo = __ballot(live);
    while (todo) {
        const int cb = __builtin_amdgcn_readlane(r.bid, __ffsll((long long)todo) - 1);
        const bool mine = live && r.bid == cb;
        todo &= ~__ballot(mine);
        const float lo[5] = { r.u, r.v, r.f2.x, r.f2.y, r.f2.z }, hi[6] = { r.u, r.v, r.f2.x, r.f2.y, r.f2.z, r.cmax };
        uint32_t *w = g.red + (size_t)cb * MCRT_BEAM_REC;
#pragma unroll
        // (an atomic only where the word would change: after a beam's first few packets hardly any does, and the packets of a scan-line all meet in the same words)
        for (int k = 0; k < 5; k++) { const uint32_t m = ford(wave_min(mine ? lo[k] : INFINITY)); if ((int)lane == k && m < __hip_atomic_load(&w[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&w[k], m); }
#pragma unroll
        for (int k = 0; k < 6; k++) { const uint32_t m = ford(wave_max(mine ? hi[k] : -INFINITY)); if ((int)lane == 8 + k && m > __hip_atomic_load(&w[8 + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&w[8 + k], m); }
    }
}

// ---- the beam order: the bounce's queue positions grouped by beam, so that a wavefront of k_beam_test runs ONE list.  The order decides which
// lanes sit together and nothing else: k_beam_test proves every ray a member by the same comparisons and tests it against the same list under the same rule ----
#define BEAM_ST 256u          // k_beam_scan: threads of a workgroup, and the counters it owns.  (Four wavefronts, one per SIMD, as a workgroup of k_march: it finds room on a
                              // compute unit whenever one of those ends.  With 1024 threads the launch ended when k_march on the side stream did: 1495 us, profiles/beam_order_fast)

#define BEAM_RANK_WAYS 128u    // k_beam_rank: pieces of the queue its workgroups interleave (the grid is a multiple of it)

// the members of a (wavefront, beam) get consecutive ranks: they land in the order as one run, and the gathers of st0 / st1 through it come in runs
__global__ void __launch_bounds__(256) k_beam_rank(FrameArgs a, BeamArgs g)
{
    const uint32_t n = a.counts[g.b];
    const uint32_t lane = threadIdx.x & 63u;
    // the workgroups that run at the same time take pieces of the queue that lie far apart (BEAM_RANK_WAYS pieces, launch_beam): neighbours in the queue are rays of
    // one scan-line, whose wavefronts all add to the same few counters
    const uint32_t per = gridDim.x / BEAM_RANK_WAYS, blk = (blockIdx.x % BEAM_RANK_WAYS) * per + blockIdx.x / BEAM_RANK_WAYS;
    const uint32_t base = (blk * 256u + threadIdx.x) & ~63u;
    if (base >= n) return;
    const uint32_t i = base + lane;
    const bool live = i < n;
    int bid = (int)g.n_beams;                                       // no beam (not a number, no slot): the pseudo-beam, placed last
    if (g.groups == 0u) {                                           // bounce 1: the history is in the state
        BeamRay r;
        if (beam_ray(a, g, live ? i : 0u, false, r) && r.bid >= 0) bid = r.bid;
    } else {
        // bounces >= 2: the queue word, the word k_shade(b - 1) stored beside it and from_tri are the whole key -- 12 bytes of a ray in place of its 40, no ray
        // rebuilt.  (A ray beam_ray refuses may get a beam here: k_beam_test refuses it all the same.)
        const uint32_t at = live ? i : 0u;
        const uint32_t pid = a.queue[(size_t)(g.b & 1u) * a.ne * a.S + at], word = beam_words(a)[at];
        const uint32_t line = pid / a.S, scan = line - (line / a.ne_frame) * a.ne_frame;
        const unsigned long long key = (1ull << 63) | ((unsigned long long)scan << 40) | ((unsigned long long)((word >> 8) & 0xffu) << 32) | (unsigned long long)a.from_tri[pid];
        const int slot = beam_slot(g, key, false);
        const uint32_t code = word & 0xffu;
        if (slot >= 0 && code < 6u) bid = slot * 6 + (int)code;
    }
    // the (wavefront, beam) runs first, without memory: every lane learns its run's first lane and its place in the run.  Then the first lanes of ALL runs add to
    // their beams' counters in ONE instruction -- a round trip per wavefront, not per beam it holds (five at bounce 3 in queue order)
    uint32_t rank = 0, run = 0;
    int lead = 0;
    unsigned long long todo = __ballot(live);
    while (todo) {
        const int first = __ffsll((long long)todo) - 1;
        const int cb = __builtin_amdgcn_readlane(bid, first);
        const bool mine = live && bid == cb;
        const unsigned long long mm = __ballot(mine);
        todo &= ~mm;
        if (mine) { lead = first; rank = (uint32_t)__popcll(mm & ((1ull << lane) - 1ull)); }
        if ((int)lane == first) run = (uint32_t)__popcll(mm);
    }
    uint32_t at = 0;
    if (live && (int)lane == lead) at = atomicAdd(&g.ocount[bid], run);
    rank += (uint32_t)__shfl((int)at, lead, 64);
    if (live) { g.rbeam[i] = (uint32_t)bid; g.rrank[i] = rank; }
}

// exclusive prefix over the n_beams + 1 segments; the pads are written here (a few thousand segments of at most 63 words: cheaper than clearing the order).
// Workgroup w owns the counters [BEAM_ST w, BEAM_ST (w + 1)), one per thread.  It sums the segments of every counter before its own by itself (coalesced loads
// that hit in L2, one reduction) and so waits for no other workgroup: beside a low-priority k_march nothing says that another workgroup is running.  The last
// workgroup has then seen every counter and writes the totals.  The layout is mcrt_debug_beam_layout's.
MCRT_DEV uint32_t wave_sum_u32(uint32_t x) { for (int o = 32; o > 0; o >>= 1) x += (uint32_t)__shfl_xor((int)x, o, 64); return x; }
__global__ void __launch_bounds__(BEAM_ST) k_beam_scan(BeamArgs g)
{
    __shared__ uint32_t wsum[3][BEAM_ST / 64u];      // per wavefront: words before (segments), rays, segments with rays
    __shared__ uint32_t wown[BEAM_ST / 64u];         // per wavefront: words of its own 64 segments
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6, n = g.n_beams + 1u, first = blockIdx.x * BEAM_ST;
    uint32_t before = 0, placed = 0, segs = 0;
    for (uint32_t k = t; k < first; k += BEAM_ST) { const uint32_t c = g.ocount[k]; before += beam_segment(c); placed += c; segs += c != 0u ? 1u : 0u; }
    const uint32_t k = first + t;
    const uint32_t c = k < n ? g.ocount[k] : 0u, w = beam_segment(c);
    placed += c; segs += c != 0u ? 1u : 0u;
    // inclusive prefix of the own segments inside the wavefront
    uint32_t inc = w;
    for (int o = 1; o < 64; o <<= 1) { const uint32_t v = (uint32_t)__shfl_up((int)inc, o, 64); if ((int)lane >= o) inc += v; }
    before = wave_sum_u32(before); placed = wave_sum_u32(placed); segs = wave_sum_u32(segs);
    if (lane == 63u) wown[wv] = inc;
    if (lane == 0u) { wsum[0][wv] = before; wsum[1][wv] = placed; wsum[2][wv] = segs; }
    __syncthreads();
    uint32_t at = 0, own = 0, all_placed = 0, all_segs = 0;
    for (uint32_t v = 0; v < BEAM_ST / 64u; v++) { at += wsum[0][v]; all_placed += wsum[1][v]; all_segs += wsum[2][v]; if (v < wv) at += wown[v]; own += wown[v]; }
    at += inc - w;      // every segment before this workgroup's, before this wavefront's, before this lane's
    if (k < n) {
        g.obase[k] = at;
        for (uint32_t j = c; j < w; j++) g.order[at + j] = MCRT_BEAM_PAD;
    }
    if (blockIdx.x == gridDim.x - 1u && t == 0u) {
        uint32_t len = own;
        for (uint32_t v = 0; v < BEAM_ST / 64u; v++) len += wsum[0][v];
        g.lcount[8] = all_placed; g.lcount[9] = all_segs; g.lcount[10] = len - all_placed; g.lcount[12] = len;
    }
}
// k_beam_scan over the n_beams + 1 counters of g (launch_beam; mcrt_debug_beam_scan runs it alone)
hipError_t launch_beam_scan(const BeamArgs &g, hipStream_t st)
{
    hipLaunchKernelGGL(k_beam_scan, dim3((g.n_beams + 1u + BEAM_ST - 1u) / BEAM_ST), dim3(BEAM_ST), 0, st, g);
    return hipGetLastError();
}

__global__ void __launch_bounds__(256) k_beam_place(FrameArgs a, BeamArgs g)
{
    const uint32_t n = a.counts[g.b], i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) g.order[g.obase[g.rbeam[i]] + g.rrank[i]] = i;
}

// A beam's volume: at depth s = +-(x_dom - xref) >= 0 a member's point lies at s_r = s - (0 .. w) along ITS ray, and its other two coordinates at
// f2 + s_r * slope.  Everything is padded by m.
struct BeamGeom { int dom; bool neg; float xref, w, m, umin, umax, vmin, vmax, alo, ahi, blo, bhi, smax; };
// does the box come within m of the volume?  s_begin: the depth at which the box begins, less m
MCRT_DEV bool beam_box(const BeamGeom &B, f3 lo, f3 hi, float &s_begin)
{
    const float lod = comp(lo, B.dom), hid = comp(hi, B.dom);
    const float sb0 = B.neg ? B.xref - hid : lod - B.xref, sb1 = B.neg ? B.xref - lod : hid - B.xref;
    s_begin = sb0 - B.m;
    const float s0 = fmaxf(s_begin, -B.m), s1 = fminf(sb1 + B.m, B.smax);
    if (!(s0 <= s1)) return false;
    const float sa = s0 - B.w;
    const int ka = (B.dom + 1) % 3, kb = (B.dom + 2) % 3;
    {
        const float p1 = sa * B.umin, p2 = sa * B.umax, p3 = s1 * B.umin, p4 = s1 * B.umax;
        const float l = B.alo + fminf(fminf(p1, p2), fminf(p3, p4)) - B.m, h = B.ahi + fmaxf(fmaxf(p1, p2), fmaxf(p3, p4)) + B.m;
        if (!(l <= comp(hi, ka) && h >= comp(lo, ka))) return false;
    }
    {
        const float p1 = sa * B.vmin, p2 = sa * B.vmax, p3 = s1 * B.vmin, p4 = s1 * B.vmax;
        const float l = B.blo + fminf(fminf(p1, p2), fminf(p3, p4)) - B.m, h = B.bhi + fmaxf(fmaxf(p1, p2), fmaxf(p3, p4)) + B.m;
        if (!(l <= comp(hi, kb) && h >= comp(lo, kb))) return false;
    }
    return true;
}

// the beam's record, as k_beam_test reads it: 0-3 umin umax vmin vmax | 4-6 f2 lo | 7-9 f2 hi | 10 size | 11 m | 12 xref | 13 s_end | 14 entries | 15 its list
// (a beam without members, or refused: the slope bounds are an empty interval, so that no ray proves itself inside)
MCRT_DEV void beam_collect(const FrameArgs &a, const BeamArgs &g, const uint32_t beam)
{
    __shared__ int q[2][BEAM_QN];
    __shared__ unsigned long long ent[BEAM_EN];
    __shared__ uint32_t leaf[BEAM_LN];
    __shared__ uint32_t nq[2], n_leaf, n_ent, overflow, list_at;
    const uint32_t lane = threadIdx.x;
    const uint32_t *w = g.red + (size_t)beam * MCRT_BEAM_REC;
    uint32_t *rec = g.rec + (size_t)beam * MCRT_BEAM_REC;
    float umin = funord(w[0]), vmin = funord(w[1]), umax = funord(w[8]), vmax = funord(w[9]);
    const bool empty = w[0] == 0xffffffffu;
    bool refused = !empty && !(umax - umin <= g.spread_cap && vmax - vmin <= g.spread_cap);
    if (!empty && lane == 0u) atomicAdd(&g.lcount[4], 1u);
    // the beam's list: its own (bounce 1), or the next of the pool -- a beam that finds the pool empty is refused
    uint32_t li = beam;
    if (g.groups != 0u) {
        if (lane == 0u) list_at = (empty || refused) ? 0u : atomicAdd(&g.lcount[5], 1u);
        __syncthreads();
        li = list_at;
        if (li >= g.n_lists) refused = !empty;
    }
    if (empty || refused) {
        if (lane < MCRT_BEAM_REC) rec[lane] = lane == 0u || lane == 2u ? __float_as_uint(INFINITY) : lane == 1u || lane == 3u || lane == 13u ? __float_as_uint(-INFINITY) : 0u;
        if (refused && lane == 0u) atomicAdd(&g.lcount[3], 1u);
        return;
    }
    // the bounds come from a sample of the members: padded a little, and a ray outside them is no member
    // the size of every coordinate that matters: the start points and the scene.  (Not the rays' far ends, which lie 10^9 cm away in a medium that hardly
    // attenuates: a plane distance fl(plane * inv + c) is off by 2^-24 of itself and of c = -(o * inv), i.e. the crossing by 2^-24 (|o| + |plane - o|) in space.)
    float cmax = funord(w[13]);
    for (int k = 0; k < 3; k++) cmax = fmaxf(cmax, fmaxf(fabsf(a.scene_lo[k]), fabsf(a.scene_hi[k])));
    cmax *= 1.0625f;
    const float m = cmax * 0x1p-18f;
    { const float pu = 0.0625f * (umax - umin) + 1e-6f, pv = 0.0625f * (vmax - vmin) + 1e-6f; umin -= pu; umax += pu; vmin -= pv; vmax += pv; }
    float flo[3], fhi[3];
    for (int k = 0; k < 3; k++) { const float l = funord(w[2 + k]), h = funord(w[10 + k]), p = 0.0625f * (h - l) + m; flo[k] = l - p; fhi[k] = h + p; }
    const uint32_t code = beam % 6u;
    BeamGeom B;
    B.dom = (int)(code >> 1); B.neg = (code & 1u) != 0u;
    const int ka = (B.dom + 1) % 3, kb = (B.dom + 2) % 3;
    B.xref = B.neg ? fhi[B.dom] : flo[B.dom]; B.w = fhi[B.dom] - flo[B.dom]; B.m = m;
    B.umin = umin; B.umax = umax; B.vmin = vmin; B.vmax = vmax; B.alo = flo[ka]; B.ahi = fhi[ka]; B.blo = flo[kb]; B.bhi = fhi[kb]; B.smax = 2.0f * cmax + m;

    // one traversal, level by level: a lane per node of the level
    // (the leaves' triangles are only listed on the way and tested afterwards, a lane each: a level then costs one round trip to memory, the node's)
    if (lane == 0u) { nq[0] = 1u; nq[1] = 0u; n_leaf = 0u; n_ent = 0u; overflow = 0u; q[0][0] = 0; }
    __syncthreads();
    for (uint32_t level = 0; ; level++) {
        const uint32_t cur = level & 1u, cnt = nq[cur];
        if (cnt == 0u) break;
        if (level >= 256u) { if (lane == 0u) overflow = 1u; break; }
        for (uint32_t t = lane; t < cnt; t += BEAM_CT) {
            const uint4 *N = a.nodes_walk + 4 * (size_t)(uint32_t)q[cur][t];
            const uint4 q0 = N[0], q1 = N[1], q2 = N[2], q3 = N[3];
            const uint32_t wd[12] = { q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w };      // lo.x lo.y lo.z hi.x hi.y hi.z, two words each
            const int ref[4] = { (int)q3.x, (int)q3.y, (int)q3.z, (int)q3.w };
#pragma unroll
            for (int c = 0; c < 4; c++) {
                if (ref[c] == MCRT_BVH4_EMPTY) continue;
                float bx[6];
#pragma unroll
                for (int k = 0; k < 6; k++) bx[k] = __half2float(__ushort_as_half((unsigned short)((wd[2 * k + (c >> 1)] >> ((c & 1) * 16)) & 0xffffu)));
                float sb;
                if (!beam_box(B, mk(bx[0], bx[1], bx[2]), mk(bx[3], bx[4], bx[5]), sb)) continue;
                if (ref[c] >= 0) {
                    const uint32_t at = atomicAdd(&nq[cur ^ 1u], 1u);
                    if (at < BEAM_QN) q[cur ^ 1u][at] = ref[c]; else overflow = 1u;
                } else {
                    const uint32_t v = (uint32_t)~ref[c], first = v >> 3, nt = (v & 7u) + 1u;
                    const uint32_t at = atomicAdd(&n_leaf, nt);
                    if (at + nt <= BEAM_LN) { for (uint32_t k = 0; k < nt; k++) leaf[at + k] = first + k; } else overflow = 1u;
                }
            }
        }
        __syncthreads();
        if (lane == 0u) nq[cur] = 0u;
        if (nq[cur ^ 1u] > BEAM_QN) break;                      // (overflow is set)
        __syncthreads();
    }
    __syncthreads();
    for (uint32_t t = lane; t < (overflow ? 0u : n_leaf); t += BEAM_CT) {
        const float4 *T = a.tris + (size_t)leaf[t] * MCRT_TRI_PIECES;
        f3 plo, phi;
        float sb;
        tri_padded_bounds(xyz(T[0]), xyz(T[1]), xyz(T[2]), a.pad_abs, plo, phi);
        if (!beam_box(B, plo, phi, sb)) continue;
        const uint32_t at = atomicAdd(&n_ent, 1u);
        if (at < BEAM_EN) ent[at] = ((unsigned long long)ford(sb) << 32) | (unsigned long long)leaf[t]; else overflow = 1u;
    }
    __syncthreads();
    const bool lost = overflow != 0u;
    const uint32_t N = lost ? 0u : n_ent;
    // sorted by the depth at which they begin (bitonic, padded with +infinity to a power of two)
    uint32_t P = 1u; while (P < N) P <<= 1;
    for (uint32_t t = N + lane; t < P; t += BEAM_CT) ent[t] = ~0ull;
    __syncthreads();
    for (uint32_t k = 2u; k <= P; k <<= 1)
        for (uint32_t j = k >> 1; j > 0u; j >>= 1) {
            for (uint32_t t = lane; t < P; t += BEAM_CT) {
                const uint32_t l = t ^ j;
                if (l > t) {
                    const unsigned long long x = ent[t], y = ent[l];
                    if ((x > y) == ((t & k) == 0u)) { ent[t] = y; ent[l] = x; }
                }
            }
            __syncthreads();
        }
    const uint32_t keep = N < g.cap ? N : g.cap;
    for (uint32_t e = lane; e < keep; e += BEAM_CT) {
        const unsigned long long x = ent[e];
        const float4 *T = a.tris + (size_t)(uint32_t)x * MCRT_TRI_PIECES;
        const float4 t0 = T[0], t1 = T[1], t2 = T[2];
        float4 *L = (float4 *)(g.list + 4 * ((size_t)li * g.cap + e));
        const float begin = funord((uint32_t)(x >> 32));
        L[0] = t0; L[1] = make_float4(t1.x, t1.y, t1.z, begin); L[2] = t2; L[3] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        // the hot part: what packet_tri_test rebuilds of the triangle alone, by the same two functions -- once per entry here, not per wavefront and entry in k_beam_test
        const float4 P = tri_plane(xyz(t0), xyz(t1), xyz(t2));
        f3 plo, phi;
        tri_padded_bounds(xyz(t0), xyz(t1), xyz(t2), a.pad_abs, plo, phi);
        float4 *H = (float4 *)(g.hot + MCRT_BEAM_HOT * ((size_t)li * g.cap + e));
        H[0] = P; H[1] = make_float4(plo.x, plo.y, plo.z, begin); H[2] = make_float4(phi.x, phi.y, phi.z, t0.w);
    }
    // s_end: the depth up to which the list is complete
    const float s_end = lost ? -INFINITY : N > g.cap ? funord((uint32_t)(ent[g.cap] >> 32)) : INFINITY;
    if (lane == 0u) {
        rec[0] = __float_as_uint(umin); rec[1] = __float_as_uint(umax); rec[2] = __float_as_uint(vmin); rec[3] = __float_as_uint(vmax);
        for (int k = 0; k < 3; k++) { rec[4 + k] = __float_as_uint(flo[k]); rec[7 + k] = __float_as_uint(fhi[k]); }
        rec[10] = __float_as_uint(cmax); rec[11] = __float_as_uint(m); rec[12] = __float_as_uint(B.xref); rec[13] = __float_as_uint(s_end); rec[14] = keep; rec[15] = li;
        if (lost || N > g.cap) atomicAdd(&g.lcount[2], 1u);
    }
}

// bounce 1: a workgroup per beam.  Bounces >= 2: a workgroup per slot of the group table takes the slot's 6 beams in turn -- nearly every group has one dominant
// axis and sign, and most slots are free: a sixth of the workgroups, which find their beams empty with one load each
__global__ void __launch_bounds__(BEAM_CT) k_beam_collect(FrameArgs a, BeamArgs g)
{
    const uint32_t per = g.groups != 0u ? 6u : 1u;
    for (uint32_t k = 0; k < per; k++) {
        beam_collect(a, g, blockIdx.x * per + k);
        __syncthreads();
    }
}

// ---- the contract's triangle test of one list entry.  packet_tri_test (mcrt_walk.h) rebuilds the triangle's plane and padded bounds from its
// vertices in every wavefront; here the record is a list entry, whose plane and bounds k_beam_collect stored (BeamArgs::hot) -- computed by the same two functions
// from the same floats, so every expression and comparison below sees packet_tri_test's operands bit for bit.  The vertices (the COLD part, BeamArgs::list) are
// fetched only by a wavefront that reaches the edge tests ----
// The wave-level exits are scalar.  `if (!__any(ok)) return;` compiles to a v_cndmask of 0 / 1 and a v_cmp before the branch, and so does a ballot of `ok`: the flag
// is a combination of compares, not a compare.  A ballot of a COMPARE is the v_cmp itself, written to a scalar pair; so the lanes still in the test are kept as a
// 64-bit mask `m` beside the lanes' own flag, every compare is balloted by itself, the pairs are combined by scalar instructions and the branch reads the scalar
// condition code.  `m` starts as the ballot of `on` (the caller has it per beam, outside the loop over the entries).
MCRT_DEV unsigned long long wave_of(bool c) { return __builtin_amdgcn_ballot_w64(c); }
// H: plane | padded lo, begin depth; H2: padded hi | id; cold: the entry of BeamArgs::list (v0 | id, v1 | begin, v2 | edge tolerance)
MCRT_DEV void list_tri_test(const u32x8 H, const u32x4 H2, const char *cold, const f3 f2, const f3 to, const f3 inv, const f3 rc, const bool on, unsigned long long m, Best &best)
{
    const f3 nrm = mk(__uint_as_float(H[0]), __uint_as_float(H[1]), __uint_as_float(H[2]));
    const float pw = __uint_as_float(H[3]);
    const f3 plo = mk(__uint_as_float(H[4]), __uint_as_float(H[5]), __uint_as_float(H[6])), phi = mk(__uint_as_float(H2[0]), __uint_as_float(H2[1]), __uint_as_float(H2[2]));
    const int id = (int)H2[3];
    float tmin, tmax;
    bool ok = on;
    const float da = dot(nrm, f2) - pw;
    const float db = dot(nrm, to) - pw;
    const bool sides = da * db < 0.0f;
    ok = ok & sides;
    m &= wave_of(sides);
    if (m == 0ull) return;
    const float proj = da - db;
    const float frac = da / proj;
    const bool nearer = frac < best.frac, tie = frac == best.frac, smaller = id < best.tri, ahead = frac >= 0.0f;
    ok = ok & (nearer | (tie & smaller)) & ahead;
    m &= (wave_of(nearer) | (wave_of(tie) & wave_of(smaller))) & wave_of(ahead);
    if (m == 0ull) return;
    const bool box = slab_c(plo, phi, rc, inv, 0.0f, 1.0f, tmin, tmax), after = frac >= tmin, before = frac <= tmax;
    ok = ok & box & after & before;
    m &= wave_of(box) & wave_of(after) & wave_of(before);
    if (m == 0ull) return;
    // (wave-uniform control flow up to here: one scalar fetch of the vertices for the wavefront)
    u32x8 A; u32x4 C2;
    asm volatile("s_load_dwordx8 %0, %2, 0x0\n\ts_load_dwordx4 %1, %2, 0x20\n\ts_waitcnt lgkmcnt(0)" : "=&s"(A), "=&s"(C2) : "s"(cold) : "memory");
    const f3 v0 = mk(__uint_as_float(A[0]), __uint_as_float(A[1]), __uint_as_float(A[2])), v1 = mk(__uint_as_float(A[4]), __uint_as_float(A[5]), __uint_as_float(A[6]));
    const f3 v2 = mk(__uint_as_float(C2[0]), __uint_as_float(C2[1]), __uint_as_float(C2[2]));
    const float edge_tol = __uint_as_float(C2[3]);
    const float s = 1.0f - frac;
    const f3 p = mk(s * f2.x + frac * to.x, s * f2.y + frac * to.y, s * f2.z + frac * to.z);
    const f3 p0 = v0 - p, p1 = v1 - p, p2 = v2 - p;
    ok = ok && dot(cross(p0, p1), nrm) >= edge_tol && dot(cross(p1, p2), nrm) >= edge_tol && dot(cross(p2, p0), nrm) >= edge_tol;
    if (ok) { best.frac = frac; best.tri = id; }
}

// every lane `on` has its hit (and the margin) before `begin`: nothing that begins there or later can change it
MCRT_DEV bool beam_all_before(const bool on, const unsigned long long on_m, const float reach, const float begin)
{
    return (on_m & wave_of(!(reach < begin))) == 0ull;
}

// pass 0: every ray of the bounce's queue against entries [0, near) of its beam's list -- in queue order, or (g.ordered) through the beam order, whose length
// k_beam_scan left in lcount[12] and whose pad words are lanes without a ray; pass 1: the leftovers of pass 0 against the rest
__global__ void __launch_bounds__(256) k_beam_test(FrameArgs a, BeamArgs g, uint32_t pass)
{
    const bool ordered = pass == 0u && g.ordered != 0u;
    const uint32_t n = pass != 0u ? g.lcount[0] : ordered ? g.lcount[12] : a.counts[g.b];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t base = (blockIdx.x * 256u + threadIdx.x) & ~63u;
    if (base >= n) return;
    const uint32_t j = base + lane;
    bool live = j < n;
    uint32_t ray = !live ? 0u : ordered ? g.order[j] : pass == 0u ? j : g.lq0[j];
    if (ordered && ray == MCRT_BEAM_PAD) { live = false; ray = 0u; }
    BeamRay r;
    bool member = beam_ray(a, g, ray, false, r) && live && r.bid >= 0;
    const uint32_t *rec = g.rec + (size_t)(member ? r.bid : 0) * MCRT_BEAM_REC;
    {
        const float4 b0 = ((const float4 *)rec)[0], b1 = ((const float4 *)rec)[1], b2 = ((const float4 *)rec)[2];
        member = member && r.u >= b0.x && r.u <= b0.y && r.v >= b0.z && r.v <= b0.w
                 && r.f2.x >= b1.x && r.f2.y >= b1.y && r.f2.z >= b1.z && r.f2.x <= b1.w && r.f2.y <= b2.x && r.f2.z <= b2.y && r.cmax <= b2.z;
    }
    const f3 f2 = r.f2, to = r.to;
    const f3 d = to - f2;
    const f3 inv = mk(rcp_dir(d.x), rcp_dir(d.y), rcp_dir(d.z));
    const f3 rc = ray_c(f2, inv);
    unsigned long long *keys = (g.b & 1u) ? a.key1 : a.key0;
    Best best; best.frac = 1.0f; best.tri = -1;
    if (pass != 0u && live) { const unsigned long long k = keys[ray]; best.frac = __uint_as_float((uint32_t)(k >> 32)); best.tri = (int)(uint32_t)k; }
    const float f2d = comp(f2, r.dom), sg = r.neg ? -1.0f : 1.0f;
    bool left = live && !member;
    unsigned long long todo = __ballot(member);
    uint32_t met = 0;
    const uint32_t first = pass == 0u ? 0u : g.near, cut = pass == 0u ? g.near : 0xffffffffu;
    while (todo) {
        const int cb = __builtin_amdgcn_readlane(r.bid, __ffsll((long long)todo) - 1);
        const bool mine = member && r.bid == cb;
        const unsigned long long mine_m = __ballot(mine);
        todo &= ~mine_m;
        met++;
        const u32x8 R = sload8(g.rec + (size_t)cb * MCRT_BEAM_REC + 8);      // ..., m, xref, s_end, entries, list
        const float m2 = 2.0f * __uint_as_float(R[3]), xref = __uint_as_float(R[4]);
        const uint32_t n_ent = R[6];
        // the depth of the hit, plus the margin: what begins beyond it cannot be accepted before it
        float reach = best.tri >= 0 ? sg * ((f2d + best.frac * r.dd) - xref) + m2 : INFINITY;
        float limit = __uint_as_float(R[5]);
        const char *L = (const char *)(g.list + 4 * (size_t)R[7] * g.cap), *Hh = (const char *)(g.hot + MCRT_BEAM_HOT * (size_t)R[7] * g.cap);
        // (the hot parts of two entries per round trip to the scalar cache; the second of the last pair may lie past the list: it is fetched, not looked at)
        for (uint32_t k = first; k < n_ent; k += 2u) {
            u32x8 A, A2; u32x4 C2, C22;
            const char *E = Hh + (size_t)k * (MCRT_BEAM_HOT * 4u);
            asm volatile("s_load_dwordx8 %0, %4, 0x0\n\ts_load_dwordx4 %1, %4, 0x20\n\ts_load_dwordx8 %2, %4, 0x30\n\ts_load_dwordx4 %3, %4, 0x50\n\ts_waitcnt lgkmcnt(0)"
                         : "=&s"(A), "=&s"(C2), "=&s"(A2), "=&s"(C22) : "s"(E) : "memory");
            float begin = __uint_as_float(A[7]);
            if (k >= cut || beam_all_before(mine, mine_m, reach, begin)) { limit = begin; break; }
            int before = best.tri;
            list_tri_test(A, C2, L + ((size_t)k << 6), f2, to, inv, rc, mine, mine_m, best);
            if (best.tri != before) reach = sg * ((f2d + best.frac * r.dd) - xref) + m2;
            if (k + 1u >= n_ent) break;
            begin = __uint_as_float(A2[7]);
            if (k + 1u >= cut || beam_all_before(mine, mine_m, reach, begin)) { limit = begin; break; }
            before = best.tri;
            list_tri_test(A2, C22, L + ((size_t)(k + 1u) << 6), f2, to, inv, rc, mine, mine_m, best);
            if (best.tri != before) reach = sg * ((f2d + best.frac * r.dd) - xref) + m2;
        }
        left = left || (mine && !(reach < limit || limit == INFINITY));
    }
    if (g.pairs && pass == 0u && met && lane == 0u) atomicAdd(&g.lcount[11], met);
    if (live && best.tri >= 0) keys[ray] = ((unsigned long long)__float_as_uint(best.frac) << 32) | (unsigned long long)(uint32_t)best.tri;
    const unsigned long long lm = __ballot(left);
    if (lm) {
        uint32_t at = 0;
        if (lane == 0u) at = atomicAdd(&g.lcount[pass], (uint32_t)__popcll(lm));
        at = __shfl(at, 0, 64);
        if (left) (pass == 0u ? g.lq0 : g.lq1)[at + (uint32_t)__popcll(lm & ((1ull << lane) - 1ull))] = ray;
    }
}

// the leftovers' state, compact, where the lane walk of a bounce of the OTHER parity reads it: that half of st0 / st1 and its key words, which nothing reads
// between k_shade(b - 1) and k_shade(b) (k_march of bounce b - 1, on its side stream, reads mrec and seg_count)
MCRT_DEV uint32_t beam_walk_as(uint32_t b) { return (b & 1u) ? 2u : 1u; }      // the bounce the leftovers are walked as, in an argument block of their own
__global__ void __launch_bounds__(256) k_beam_gather(FrameArgs a, BeamArgs g, uint32_t which)
{
    const uint32_t n = g.lcount[which];
    const uint32_t *lq = which == 0u ? g.lq0 : g.lq1;
    const size_t np = (size_t)a.ne * a.S, in = (g.b & 1u) ? np : 0, out = np - in;
    unsigned long long *keys = (g.b & 1u) ? a.key0 : a.key1;
    if (blockIdx.x == 0u && threadIdx.x == 0u) g.l_counts[beam_walk_as(g.b)] = n;
    for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < n; j += gridDim.x * 256u) {
        const uint32_t r = lq[j];
        a.st0[out + j] = a.st0[in + r]; a.st1[out + j] = a.st1[in + r]; keys[j] = MCRT_KEY_MISS;
    }
}
__global__ void __launch_bounds__(256) k_beam_scatter(FrameArgs a, BeamArgs g, uint32_t which)
{
    const uint32_t n = g.lcount[which];
    const uint32_t *lq = which == 0u ? g.lq0 : g.lq1;
    unsigned long long *keys = (g.b & 1u) ? a.key1 : a.key0;
    const unsigned long long *walked = (g.b & 1u) ? a.key0 : a.key1;
    for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < n; j += gridDim.x * 256u) keys[lq[j]] = walked[j];
}

// bounce g.b's closest hits by beams, in place of launch_trace(a, g.b): the same key words
hipError_t launch_beam(const FrameArgs &a, const BeamArgs &g, hipStream_t st)
{
    const uint32_t np = a.ne * a.S, blocks = (np + 255u) / 256u;
    uint32_t setup = g.n_beams * MCRT_BEAM_REC;
    if (setup < MCRT_MAX_BOUNCES * MCRT_XCDS) setup = MCRT_MAX_BOUNCES * MCRT_XCDS;
    if (setup < g.groups) setup = g.groups;
    hipLaunchKernelGGL(k_beam_clear, dim3((setup + 255u) / 256u), dim3(256), 0, st, g);
    hipLaunchKernelGGL(k_beam_bounds, dim3((blocks + g.stride - 1u) / g.stride), dim3(256), 0, st, a, g);
    if (g.ordered) {      // (the group table holds its keys)
        hipLaunchKernelGGL(k_beam_rank, dim3((blocks + BEAM_RANK_WAYS - 1u) / BEAM_RANK_WAYS * BEAM_RANK_WAYS), dim3(256), 0, st, a, g);
        launch_beam_scan(g, st);
        hipLaunchKernelGGL(k_beam_place, dim3(blocks), dim3(256), 0, st, a, g);
    }
    hipLaunchKernelGGL(k_beam_collect, dim3(g.groups != 0u ? g.groups : g.n_beams), dim3(BEAM_CT), 0, st, a, g);
    // (the order's length is a device word: the worst case is launched, and the wavefronts past the length return at once)
    const uint32_t blocks0 = g.ordered ? (uint32_t)(((size_t)np + 64u * ((size_t)g.n_beams + 1u) + 255u) / 256u) : blocks;
    hipLaunchKernelGGL(k_beam_test, dim3(blocks0), dim3(256), 0, st, a, g, 0u);
    const uint32_t which = g.near < g.cap ? 1u : 0u;
    if (which) hipLaunchKernelGGL(k_beam_test, dim3(blocks), dim3(256), 0, st, a, g, 1u);
    const uint32_t few = blocks < 2048u ? blocks : 2048u;
    hipLaunchKernelGGL(k_beam_gather, dim3(few), dim3(256), 0, st, a, g, which);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    // the leftovers as the queue of a bounce of the other parity: counts and cursors of their own, no packets
    FrameArgs w = a;
    w.counts = g.l_counts; w.cursors = g.l_cursors; w.packet_mask = 0u;
    e = launch_trace(w, (g.b & 1u) ? 2u : 1u, false, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_beam_scatter, dim3(few), dim3(256), 0, st, a, g, which);
    return hipGetLastError();
}

}  // namespace mcrt
