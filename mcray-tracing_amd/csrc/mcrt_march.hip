// mcrt_march.hip -- k_march, the RF accumulation loop (main.cpp:106-144, rfimage.h:33-40, volume.h:46-61): a lane pair / quad per segment,
// a generic variant and a fast one for the reference's 256^3 texture and time axis; k_material_table, the per-material table it reads.
#include "mcrt_device.h"

#ifndef MCRT_MARCH_PAIRS_FROM
#define MCRT_MARCH_PAIRS_FROM 1048576    // k_march: lane pairs per segment for passes with at least this many paths, quads below
#endif
#ifndef MCRT_MARCH_WAVES
#define MCRT_MARCH_WAVES 6           // waves per SIMD the register budget of k_march is set for (7: 14 spilled registers, 789 vs 750 us per launch; 5: 777)
#endif
#ifndef MCRT_MARCH_TILE
#define MCRT_MARCH_TILE 256          // slots a wavefront of k_march sorts by segment length at a time (a multiple of 64, at most 256: one byte per slot)
#endif
#ifndef MCRT_MARCH_MTAB
#define MCRT_MARCH_MTAB 32           // rows of the per-material table k_march keeps in LDS (scenes with more materials read it from memory)
#endif

namespace mcrt {

MCRT_DEV uint32_t vox_index(float q, uint32_t n, uint32_t mask)
{
    long long i;
    if (!(fabsf(q) < 9.2233720368547758e18f)) i = (long long)0x8000000000000000ull;
    else if (fabsf(q) < 2147483648.0f) i = (long long)(int)q;
    else i = (long long)q;
    return mask ? ((uint32_t)i & mask) : ((uint32_t)i) % n;   // mask = n-1 when n is a power of two (the reference's 256)
}

// ---- quad (4-lane) exchanges on the DPP path: no LDS, VALU rate.  Control flow around them is quad-uniform (the four
// lanes of a path hold identical state), so the source lanes are always active.
template <int CTRL> MCRT_DEV int dpp_i(int v) { return __builtin_amdgcn_mov_dpp(v, CTRL, 0xF, 0xF, true); }

#define QP_BCAST(k) ((k) * 0x55)

// The LDS image of a scan-line in k_march: entry r = { thr[r], bin[r] }, 16 bytes -- a step's two thresholds and its bin are then
// three constant offsets from ONE address (row << 4), with no base register.
struct RowBin { double thr; long long bin; };

// row = (int)(t / row_dt) if that quotient is < R, else -1 (rfimage.h:33-40), WITHOUT the double division:
// thr[r] (host-computed, mcrt_row_thresholds) is the smallest double t whose IEEE quotient fl(t/row_dt) is >= r, so the
// row is the largest r with thr[r] <= t.  Exactly equivalent to the division for every double t >= 0.
MCRT_DEV int row_of(double t, const RowBin *rb, uint32_t R, double inv_dt, double thr_end)
{
    if (!(t < thr_end) || !(t >= 0.0)) return -1;
    int r = (int)(t * inv_dt);                                   // within one row of the answer
    r = r < 0 ? 0 : (r > (int)R - 1 ? (int)R - 1 : r);
    const double lo = rb[r].thr, hi = rb[r + 1].thr;
    if ((t < lo) | !(t < hi)) {                                  // the estimate missed by a rounding: walk to the row
        while (t < rb[r].thr) r--;
        while (t >= rb[r + 1].thr) r++;
    }
    return r;
}

// the same row when a good guess is at hand: two threshold reads confirm it.  (k_march's guess is t * inv_dt itself, which misses
// only by a rounding: a guess from the lane's previous row + its stride misses whenever the row advances by one more than the
// stride -- every tenth step or so, i.e. in EVERY step of a wavefront some lane would take the search below, for all 64.)
// PADDED: the image holds entries up to the largest guess a valid step can make ((int)(max_travel * inv_dt), + 1), those beyond
// thr[R] filled with -inf -- the guess needs no clamp, and a time beyond the image fails "t < hi" and is sorted out by row_of.
template <bool PADDED>
MCRT_DEV int row_near(double t, int guess, const RowBin *rb, uint32_t R, double inv_dt, double thr_end)
{
    const int r = PADDED ? guess : (guess < 0 ? 0 : (guess > (int)R - 1 ? (int)R - 1 : guess));
    const double lo = rb[r].thr, hi = rb[r + 1].thr;
    if ((t >= lo) & (t < hi)) return r;                          // (false for NaN, negative times and times beyond the image)
    return row_of(t, rb, R, inv_dt, thr_end);
}

// x / tex_res, correctly rounded, as two fmas around a multiply by the rounded reciprocal (Markstein's correction).
// Used only when the GPU itself has verified (k_verify_div, exhaustive over the gated range) that the sequence
// equals IEEE division for this tex_res; otherwise, and outside the gate, the division instruction sequence is used.
MCRT_DEV float div_res(float x, const FrameArgs &a)
{
    const float ax = fabsf(x);
    if (a.fast_div && ((ax > 1e-18f && ax < 1e18f) || x == 0.0f)) {
        const float q0 = x * a.tex_rcp;
        const float r = fmaf(-q0, a.tex_res, x);
        return fmaf(r, a.tex_rcp, q0);
    }
    return x / a.tex_res;
}

// texture cell of a point, volume.h:46-61 (x / resolution, (int) cast, modulo), for any texture size and magnitude
MCRT_DEV size_t vox_cell(f3 p, const FrameArgs &a)
{
    const uint32_t vx = vox_index(div_res(p.x, a), a.tex_n, a.tex_mask), vy = vox_index(div_res(p.y, a), a.tex_n, a.tex_mask), vz = vox_index(div_res(p.z, a), a.tex_n, a.tex_mask);
    return ((size_t)vx * a.tex_n + vy) * a.tex_n + vz;
}
// the same cell when every coordinate is below lean_bound in magnitude and the size is a power of two: branch-free.
// |x / res| < 2^31 there, and the corrected reciprocal multiply is the verified quotient for |x| > 1e-18 and x == 0; for
// the tiny values in between both it and the true quotient are below 1 in magnitude (tex_res > 1e-16), so the cell is 0
// either way.
MCRT_DEV uint32_t vox_lean1(float x, const FrameArgs &a)
{
    const float q0 = x * a.tex_rcp;
    const float r = fmaf(-q0, a.tex_res, x);
    return (uint32_t)(int)fmaf(r, a.tex_rcp, q0) & a.tex_mask;
}
MCRT_DEV uint32_t vox_cell_lean(f3 p, const FrameArgs &a)
{
    return (((vox_lean1(p.x, a) << a.tex_shift) | vox_lean1(p.y, a)) << a.tex_shift) | vox_lean1(p.z, a);
}
// ... and when the texture is the reference's 256^3 (volume.h:19): the three low bytes packed by two v_perm_b32.
// (The device copy keeps the reference's cell order, (x * 256 + y) * 256 + z.  Round 6 counted and measured other orders -- x fastest, 128-byte
//  lines as 4 x 2 x 2 bricks or 4 x 1 x 4 tiles -- and the quotients as packed fp32: all slower, the kernel is bound by the instructions it issues,
//  not by its gathers.  DESIGN.md A.8, profiles/round6/exp_march_layout.txt, tools/variants/round6_march_layout.patch.)
MCRT_DEV uint32_t vox_q(float x, const FrameArgs &a)
{
    const float q0 = x * a.tex_rcp;
    const float r = fmaf(-q0, a.tex_res, x);
    return (uint32_t)(int)fmaf(r, a.tex_rcp, q0);
}
MCRT_DEV uint32_t vox_cell_lean256(f3 p, const FrameArgs &a)
{
    const uint32_t yz = __builtin_amdgcn_perm(vox_q(p.y, a), vox_q(p.z, a), 0x0c0c0400u);      // { z.b0, y.b0, 0, 0 }
    return __builtin_amdgcn_perm(vox_q(p.x, a), yz, 0x0c040100u);                                // { z.b0, y.b0, x.b0, 0 }
}
// The same with the reciprocal and the resolution held in VECTOR registers.  gfx950 issues v_mul_f32 / v_fma_f32 / v_add_f32 in 2 cycles per wavefront when every register
// operand is a vector register, and in 4 as soon as one is a SCALAR register (profiles/round6/valu_classes.json: the same for v_add_u32, v_and_b32 ...; min / max / compare /
// convert / shift / packed / f64 / fma_mix instructions take 4 either way).  The three instructions of a quotient read the wave-uniform constants: as scalar operands -- what the
// compiler picks by itself -- the 36 of an iteration of k_march cost twice what they need to.  (vgpr(): an empty asm the compiler cannot see through.)
MCRT_DEV float vgpr(float s) { float v = s; asm volatile("" : "+v"(v)); return v; }
MCRT_DEV uint32_t vox_q_v(float x, float rcp_v, float res_v)
{
    const float q0 = x * rcp_v;
    const float r = fmaf(-q0, res_v, x);
    return (uint32_t)(int)fmaf(r, rcp_v, q0);
}
MCRT_DEV uint32_t vox_cell_lean256_v(f3 p, float rcp_v, float res_v)
{
    const uint32_t yz = __builtin_amdgcn_perm(vox_q_v(p.y, rcp_v, res_v), vox_q_v(p.z, rcp_v, res_v), 0x0c0c0400u);
    return __builtin_amdgcn_perm(vox_q_v(p.x, rcp_v, res_v), yz, 0x0c040100u);
}
MCRT_DEV float abs_sum(f3 p) { return (fabsf(p.x) + fabsf(p.y)) + fabsf(p.z); }   // >= every |coordinate|; NaN/inf propagate

// one echo into the scan-line's fixed-point LDS bins (2^-40 units; integer adds commute, so the image does not depend
// on the order lanes, waves or workgroups arrive in)
MCRT_DEV void rf_add(RowBin *rb, uint32_t *lflags, int row, float echo)
{
    if (row < 0) return;
    if (!(fabsf(echo) < 1024.0f)) { atomicOr(&lflags[row >> 5], 1u << (row & 31)); return; }
    const long long v = fix40(echo);
    if (v != 0) atomicAdd((unsigned long long *)&rb[row].bin, (unsigned long long)v);
}

// ---- RF accumulation (main.cpp:112-140) of the segments produced in bounce b.  A workgroup owns a range of the sample
// slots of ONE scan-line ("line" = frame * ne_frame + scan-line), so its fixed-point bins live in LDS and are flushed once
// with global integer atomics.  Inside it every wavefront runs its slots as a task pool: a group of G lanes (template parameter: 2 or 4) per
// segment; a group that has finished (or found a dead path's empty slot) takes the next slot, so short, long and missing
// segments do not wait for each other.  Eight consecutive steps per iteration, lane j of the group owns steps j, j+G, ...
// (that many texture gathers per lane in flight).
// Tried on top of this and measured slower (MI355X, 32 frames per pass, per launch alone): one task pool per workgroup instead of
// a quarter of its slots per wavefront (an LDS cursor: 891 vs 829 us -- the extra scalar work outweighs the better balance); a
// one-read row stepper for steps after a segment's first (the row advances by G or G + 1: no gain, the two threshold reads were
// never the cost); fewer resident workgroups per CU so that k_shade / the next k_trace find registers at once (LDS padding: no gain);
// one wavefront per scan-line, four lines and four bin arrays per workgroup (a pool of S slots per wavefront instead of S/4: the GPU is
// then a quarter as finely cut and the heaviest lines set the pace -- 1714 vs 827 us).
// With the sorted tiles (750 us): the steps' echoes as straight-line code (row confirmed by two reads, zero adds into a spare bin, the
// rest left to a general path entered when any lane needs it) -- the loop issues two scalar instructions for three vector ones, but
// the straight line keeps four echoes and rows alive: 20 spilled registers at 6 waves/SIMD (1255 us), 784 us at 5; the zero adds
// all meet in one LDS word (869 / 757 us).  Round 3, the same idea with the add itself the only masked instruction (common case = estimate
// confirmed and echo small; the rest collected in a bit mask for a general path entered when any lane needs it): 2341 vs 2263 us per
// 128-frame launch -- the work done for steps that are not valid costs more than the branches it replaces.  Taking parts of the step out (wrong images, timing only): no gathers 693, no row
// search 679, no adds 707, none of the three 570 us, no loop at all 8 us (cycle stamps of the full kernel: hand-out 17 %, advance 4 %, voxel + gathers 27 %,
// rows and bins with the wait for the gathers 51 %).
// With the fast path (1397 us per 128-frame launch alone): one lane per segment instead of a pair (four steps per lane and iteration, no
// redundant advance): 1420 us; the row guessed from the lane's previous row + G instead of from its time (two double operations less per
// step): 1426 us.
// FAST (round 3): the reference's 256^3 texture with the branch-free cell, and an LDS image padded to the largest row guess of a
// valid step -- no texture size, shift, row count or LDS base in the step's instructions (the generic kernel had spilled those
// scalars: ~13 v_readlane per four steps).
template <bool STATS, int G, bool FAST>
__global__ void __launch_bounds__(256, MCRT_MARCH_WAVES) k_march(FrameArgs a, uint32_t b, uint32_t chunks)
{
    constexpr int H = 8 / G;                 // RF steps per lane and iteration: a group does G*H = 8 consecutive steps
#ifndef MCRT_MARCH_REFILL_DIV
#define MCRT_MARCH_REFILL_DIV 4
#endif
    constexpr int REFILL = (64 / G) / MCRT_MARCH_REFILL_DIV;   // new segments are handed out while at least a quarter of the wavefront's groups are idle or finished
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wv = tid >> 6, j = tid & (G - 1);
    const uint32_t R = a.R, nf = (R + 31u) >> 5, nrt = FAST ? a.march_rows : R + 1u;      // entries of the LDS image (march_lds_bytes)
    RowBin *rb = (RowBin *)smem;
    uint32_t *lflags = (uint32_t *)(rb + nrt);
    uint32_t *sort_cnt = lflags + ((nf + 3u) & ~3u) + wv * 64;                              // this wavefront's 64 length classes ...
    unsigned char *sort_list = (unsigned char *)(lflags + ((nf + 3u) & ~3u) + 4 * 64) + wv * MCRT_MARCH_TILE;   // ... its tile's slots, longest first ...
    unsigned char *sort_cls = (unsigned char *)(lflags + ((nf + 3u) & ~3u) + 4 * 64) + 4 * MCRT_MARCH_TILE + wv * MCRT_MARCH_TILE;   // ... and their classes (worked out once)
    // the per-material table (a few 16-byte rows) in LDS: the tile sort and every segment load look it up -- as reads of the vector memory pipe
    // they were a tenth of this kernel's cache accesses, and the frame is bound by the sum of its kernels' accesses
    float4 *mtab_l = (float4 *)((unsigned char *)(lflags + ((nf + 3u) & ~3u) + 4 * 64) + 8 * MCRT_MARCH_TILE);
    const bool mtab_in_lds = a.n_mat <= (uint32_t)MCRT_MARCH_MTAB;
    for (uint32_t r = tid; r < nrt; r += nthr) { rb[r].thr = r <= R ? a.row_thr[r] : -__builtin_inf(); rb[r].bin = 0; }
    for (uint32_t r = tid; r < nf; r += nthr) lflags[r] = 0u;
    if (mtab_in_lds) for (uint32_t r = tid; r < a.n_mat; r += nthr) mtab_l[r] = a.mtab[r];
    __syncthreads();
    // (a scalar branch picks the load; the empty asm keeps the LDS side a ds_read -- merged, the compiler emits ONE flat load through a selected pointer)
    auto mtab_row = [&](int m) -> float4 { float4 v; if (mtab_in_lds) { v = mtab_l[m]; asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w)); } else v = a.mtab[m]; return v; };
#define MCRT_MTAB(m) mtab_row(m)

    // XCD-aware numbering: workgroup w runs on XCD w % 8; give every XCD a CONTIGUOUS range of scan-lines, so that the texture
    // cells its segments touch (neighbouring scan-lines cross the same tissue) are shared in ITS L2
    uint32_t bid = blockIdx.x;
    if (gridDim.x % MCRT_XCDS == 0u) bid = (blockIdx.x % MCRT_XCDS) * (gridDim.x / MCRT_XCDS) + blockIdx.x / MCRT_XCDS;
    // ... and within it the F frames of a scan-line one after the other (they cross exactly the same tissue)
    const uint32_t F = a.ne / a.ne_frame, ol = bid / chunks, chunk = bid % chunks;
    const uint32_t line = (ol % F) * a.ne_frame + ol / F;
    // this wavefront's slot range: the line's S slots are cut into chunks*4 contiguous pieces
    const uint32_t per = (a.S + chunks * 4u - 1u) / (chunks * 4u);
    const uint32_t s_begin = min(a.S, (chunk * 4u + (uint32_t)wv) * per), s_end = min(a.S, s_begin + per);
    const size_t pid0 = (size_t)line * a.S;
    unsigned long long st_steps = 0;

    // The wavefront takes its slots in TILES of MCRT_MARCH_TILE, and the segments of a tile LONGEST FIRST (counting sort by the
    // number of 8-step iterations a segment needs, dead paths' slots left out): groups that start together then finish together,
    // so the hand-out code below -- which the whole wavefront executes -- runs for many groups at once and seldom, and the lanes
    // of a wavefront step in lockstep.  (RF bins are integer sums: the order is free.)
    uint32_t tile0 = s_begin, list_base = s_begin, list_n = 0, list_pos = 0;      // wave-uniform: first slot of the next tile; of the tile in hand: first slot, live segments, the next one to hand out
    bool tiles_left = s_begin < s_end;
    const double thr_end = a.row_thr[R];
    bool busy = false;
    // A GROUP of G lanes (a DPP quad, or half of one) owns a segment.  Lane j of the group carries the segment's running
    // state (point, time, intensity) j steps AHEAD of the group's base step: every lane does the same sequential updates the
    // reference does, shifted, and owns steps j, j+G, j+2G, ...
    f3 point = mk(0, 0, 0), delta = mk(0, 0, 0);
    double t = 0.0, t_start = 0.0;
    float inten = 0.0f, k_att = 0.0f, seg_refl = 0.0f, m_dens = 0.0f, m_sigma = 0.0f, m_mu = 0.0f;
    uint32_t sidx = 0, steps = 0;
    bool more = false;
    // b == MCRT_ALL_BOUNCES: the launch accumulates EVERY bounce's segments; a group then walks its path's segments one after
    // the other (seg_b = the one in progress, seg_n = how many the path has) before it takes the next slot
    const bool all_b = b == MCRT_ALL_BOUNCES;
    uint32_t seg_b = all_b ? 0u : b, seg_n = 0; size_t seg_pid = 0;
    const float rcp_v = vgpr(a.tex_rcp), res_v = vgpr(a.tex_res);      // (vector-register copies: see vox_cell_lean256_v)
#define MCRT_LOAD_SEGMENT() { \
        const float4 *mr = a.mrec + 3 * ((size_t)seg_b * a.ne * a.S + seg_pid); \
        const float4 g0 = mr[0], g1 = mr[1], g2 = mr[2]; \
        const float4 mt = MCRT_MTAB(__float_as_int(g2.w)); \
        point = mk(g0.x, g0.y, g0.z); seg_refl = g0.w; \
        delta = mk(g1.x, g1.y, g1.z); inten = g1.w; \
        t_start = __hiloint2double(__float_as_int(g2.y), __float_as_int(g2.x)); \
        steps = __float_as_uint(g2.z); \
        m_mu = mt.x; m_dens = mt.y; m_sigma = mt.z; k_att = mt.w; \
        t = t_start; sidx = (uint32_t)j; \
        /* scattering is exactly +0 for every voxel when mu0 == sigma == 0 (finite texture): the adds are no-ops */ \
        const bool silent = a.tex_finite && m_mu == 0.0f && m_sigma == 0.0f; \
        more = !silent && steps > 0u && t < a.max_travel; \
        _Pragma("unroll") for (int u = 1; u < G; u++) if (j >= u) MCRT_ADVANCE() \
        busy = true; }
#define MCRT_ADVANCE() { point = point + delta; t = t + a.time_step; inten *= k_att; }
    for (;;) {
        // ---- finished segments and idle quads.  The boundary echo of a finished segment (main.cpp:139) and the probing of new
        // slots are code the whole wavefront runs however few quads need it, so both wait until REFILL quads are
        // finished or idle (or nothing is left to step) ----
        const bool fin = busy && !more;
        if (popc_mask(__ballot((!busy || fin) && j == 0)) >= (uint32_t)REFILL || !__any(busy && more)) {
            if (fin) {
                if (j == 0) {
                    const double te = t_start + a.time_step * (double)(uint32_t)(steps - 1u);
                    rf_add(rb, lflags, row_of(te, rb, R, a.inv_row_dt, thr_end), seg_refl / (float)a.S);
                }
                busy = false;
                if (all_b && seg_b + 1u < seg_n) { seg_b++; MCRT_LOAD_SEGMENT() }      // the path's next segment
            }
            while (list_pos < list_n || tiles_left) {
                if (list_pos >= list_n) {
                    // ---- the next tile: classes 0 (longest) .. 63, a slot's class from its segment's step count ----
                    const uint32_t t1 = min(s_end, tile0 + (uint32_t)MCRT_MARCH_TILE);
                    sort_cnt[lane] = 0u;
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier();
                    // (the class of a slot is worked out once, while counting, and kept in LDS for the placing pass: worked out twice -- rounds 2-3 --
                    //  it cost the placing pass the same three global reads per slot again)
                    auto slot_class = [&](uint32_t slot) -> uint32_t {
                        if (slot >= t1) return 0xffffffffu;
                        const uint32_t sn = a.seg_count[pid0 + slot], sb0 = all_b ? 0u : b;
                        if (sb0 >= sn) return 0xffffffffu;
                        uint32_t its = 0u;
                        if (!all_b) {
                            const float4 g2 = a.mrec[3 * ((size_t)sb0 * a.ne * a.S + pid0 + slot) + 2];
                            const float4 mt = MCRT_MTAB(__float_as_int(g2.w));
                            const bool silent = a.tex_finite && mt.x == 0.0f && mt.z == 0.0f;
                            its = silent ? 0u : (__float_as_uint(g2.z) + 7u) >> 3;
                        }
                        return 63u - (its < 63u ? its : 63u);
                    };
                    for (int k = 0; k < MCRT_MARCH_TILE / 64; k++) {
                        const uint32_t c = slot_class(tile0 + (uint32_t)(k * 64 + lane));
                        sort_cls[k * 64 + lane] = (unsigned char)c;                      // (0xff: no live segment in this slot)
                        if (c != 0xffffffffu) atomicAdd(&sort_cnt[c], 1u);
                    }
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
                    const uint32_t mine_cnt = sort_cnt[lane];
                    uint32_t incl = mine_cnt;                                    // inclusive prefix sum over the 64 classes
#pragma unroll
                    for (int d = 1; d < 64; d <<= 1) { const uint32_t o = (uint32_t)__shfl_up((int)incl, d, 64); if (lane >= d) incl += o; }
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
                    sort_cnt[lane] = incl - mine_cnt;                            // now the class's next free position in the list
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
                    for (int k = 0; k < MCRT_MARCH_TILE / 64; k++) {
                        const uint32_t c = (uint32_t)sort_cls[k * 64 + lane];
                        if (c != 0xffu) sort_list[atomicAdd(&sort_cnt[c], 1u)] = (unsigned char)(k * 64 + lane);
                    }
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
                    list_n = (uint32_t)__shfl((int)incl, 63, 64); list_pos = 0u;
                    list_base = tile0; tile0 = t1; tiles_left = t1 < s_end;
                    continue;
                }
                const unsigned long long want = __ballot(!busy && j == 0);
                if (popc_mask(want) < (uint32_t)REFILL) break;
                const uint32_t mine = list_pos + (uint32_t)__popcll(want & ((1ull << (lane & ~(G - 1))) - 1ull));
                if (!busy && mine < list_n) {
                    seg_pid = pid0 + list_base + (uint32_t)sort_list[mine];
                    seg_b = all_b ? 0u : b;
                    seg_n = all_b ? a.seg_count[seg_pid] : b + 1u;           // (the list holds live slots only: no need to ask again)
                    if (seg_b < seg_n) MCRT_LOAD_SEGMENT()
                }
                const uint32_t nw = (uint32_t)__popcll(want);
                list_pos = (list_pos + nw < list_n) ? list_pos + nw : list_n;
            }
        }
        if (!__any(busy)) { if (list_pos >= list_n && !tiles_left) break; else continue; }

        // ---- G*H steps of every running segment ----
        if (busy && more) {
            f3 myp[H]; double myt[H]; float myin[H]; bool myv[H];
            float reach = 0.0f;
#pragma unroll
            for (int h = 0; h < H; h++) {
                myp[h] = point; myt[h] = t; myin[h] = inten; myv[h] = sidx < steps && t < a.max_travel;           // the reference's loop test
                if (h == 0 || h == H - 1) reach += abs_sum(point);   // every coordinate moves monotonically: first and last bound them all
#pragma unroll
                for (int u = 0; u < G; u++) MCRT_ADVANCE()
                sidx += (uint32_t)G;
            }
            // the quad goes on while its base step (lane 0's) passes the loop test
            more = dpp_i<G == 4 ? QP_BCAST(0) : 0xA0>((sidx < steps && t < a.max_travel) ? 1 : 0) != 0;   // (0xA0: quad_perm [0,0,2,2])
            float2 vox[H];
            if (reach < a.lean_bound) {
#pragma unroll
                for (int h = 0; h < H; h++) vox[h] = a.tex[FAST ? vox_cell_lean256_v(myp[h], rcp_v, res_v) : vox_cell_lean(myp[h], a)];
            } else {
#pragma unroll
                for (int h = 0; h < H; h++) vox[h] = myv[h] ? a.tex[vox_cell(myp[h], a)] : make_float2(0.0f, 0.0f);
            }
            // the steps' rows while the gathers are in flight (LDS reads do not wait for them, and the times are dead afterwards:
            // 1407 -> 1382 us per 128-frame launch against looking each row up just before its add); a step's row is guessed from its
            // time, which misses only by a rounding -- the lane's previous row + its stride misses whenever the row advances by one more
            int rows[H];
#pragma unroll
            for (int h = 0; h < H; h++)
                rows[h] = myv[h] ? row_near<FAST>(myt[h], (int)(myt[h] * a.inv_row_dt), rb, R, a.inv_row_dt, thr_end) : -1;
#pragma unroll
            for (int h = 0; h < H; h++) {
                if (myv[h]) {
                    const float scattering = vox[h].y >= m_dens ? vox[h].x * m_sigma + m_mu : 0.0f;
                    rf_add(rb, lflags, rows[h], myin[h] * scattering);
                    if (STATS) st_steps++;
                }
            }
        }
    }
#undef MCRT_ADVANCE
#undef MCRT_LOAD_SEGMENT
#undef MCRT_MTAB
    if (STATS) {
        long long x = wave_sum_i64((long long)st_steps);
        if (lane == 0 && x) atomicAdd(&a.stats[4], (unsigned long long)x);
    }
    __syncthreads();
    // row of the frame's RF block: [frame][scan-line of the whole block]; this launch covers scan-lines [acc_off, acc_off+ne_frame)
    const size_t row = (size_t)(line / a.ne_frame) * a.acc_stride + a.acc_off + line % a.ne_frame;
    for (uint32_t r = tid; r < R; r += nthr) {
        const long long v = rb[r].bin;
        if (v != 0) atomicAdd((unsigned long long *)&a.acc[row * R + r], (unsigned long long)v);
    }
    for (uint32_t r = tid; r < nf; r += nthr) { const uint32_t f = lflags[r]; if (f) atomicOr(&a.flags[row * nf + r], f); }
}

// per material, what k_march reads: mu0, mu1, sigma and the per-step attenuation factor of main.cpp:118-119
// (the segment's attenuation is its medium's, so the factor depends on the material only)
__global__ void k_material_table(const float4 *mats, uint32_t n_mat, float axial_res_f, float freq, float4 *mtab)
{
    const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_mat) return;
    const float4 s0 = mats[2 * m], s1 = mats[2 * m + 1];
    mtab[m] = make_float4(s0.z, s0.w, s1.x, det_expf(-s0.y * axial_res_f * 0.01f * freq * 1.0f));
}

size_t march_lds_bytes(uint32_t R, uint32_t rows)               // rows: entries of the { threshold, bin } image (R + 1, or FrameArgs::march_rows)
{
    const size_t img = (size_t)rows * 16, flg = (size_t)((((R + 31u) >> 5) + 3u) & ~3u) * 4;
    return img + flg + 4 * (64 * 4 + 2 * MCRT_MARCH_TILE) + 16 * MCRT_MARCH_MTAB;        // + per wavefront: 64 length-class counters, one tile of slot numbers and of their classes; + the material table
}

// RF accumulation of the segments of bounce b
hipError_t launch_march(const FrameArgs &a, uint32_t b, bool stats, hipStream_t st)
{
    // chunks per scan-line (every chunk zeroes and flushes its own copy of the line's bins): about ONE round of resident workgroups
    // (6 per CU).  Measured on the MI355X, 128 x 1024 paths per frame, ms per frame with 1024 / 2048 / 4096 workgroups aimed at: one
    // frame at a time (128 lines) 1.72 / 1.86 / 1.86; 4 frames in flight (512 lines) 0.96 / 0.90 / 0.95; 20 frames (2560 lines, so at
    // least that many workgroups) 0.512 / 0.512 / 0.525; from 16 frames on a line is one chunk either way.
    // The time is (work + workgroups x fixed cost) / throughput + the last workgroup's own length (work / workgroups): the best count
    // grows with the SQUARE ROOT of the work -- 1024 per 131072 paths fits all of the above (chunks rounded down).
    uint32_t target = a.march_blocks;
    if (!target) { target = (uint32_t)(1024.0 * sqrt((double)a.ne * a.S / 131072.0)); if (target < 1024u) target = 1024u; }
    uint32_t chunks = a.ne >= target ? 1u : (a.march_blocks ? (target + a.ne - 1u) / a.ne : target / a.ne);
    const uint32_t max_chunks = (a.S + 63u) / 64u;
    if (chunks > max_chunks) chunks = max_chunks;
    if (chunks < 1u) chunks = 1u;
    const dim3 grid(a.ne * chunks), blk(256);
    const bool fast = !stats && a.march_rows != 0u;            // (FrameArgs::march_rows: set when the fast kernel's conditions hold)
    const size_t lds = march_lds_bytes(a.R, fast ? a.march_rows : a.R + 1u);
    // lanes per segment: pairs give the higher throughput when there is plenty of work (515 vs 524 us per launch with 16 frames in
    // flight), quads the shorter iterations that matter when one frame at a time is traced (2.19 vs 2.37 ms per frame)
    const bool pairs = (size_t)a.ne * a.S >= (size_t)MCRT_MARCH_PAIRS_FROM;
    if (stats) { if (pairs) hipLaunchKernelGGL((k_march<true, 2, false>), grid, blk, lds, st, a, b, chunks); else hipLaunchKernelGGL((k_march<true, 4, false>), grid, blk, lds, st, a, b, chunks); }
    else if (fast) { if (pairs) hipLaunchKernelGGL((k_march<false, 2, true>), grid, blk, lds, st, a, b, chunks); else hipLaunchKernelGGL((k_march<false, 4, true>), grid, blk, lds, st, a, b, chunks); }
    else { if (pairs) hipLaunchKernelGGL((k_march<false, 2, false>), grid, blk, lds, st, a, b, chunks); else hipLaunchKernelGGL((k_march<false, 4, false>), grid, blk, lds, st, a, b, chunks); }
    return hipGetLastError();
}

hipError_t launch_material_table(const float4 *mats, uint32_t n_mat, float axial_res_f, float freq, float4 *mtab, hipStream_t st)
{
    hipLaunchKernelGGL(k_material_table, dim3((n_mat + 63u) / 64u), dim3(64), 0, st, mats, n_mat, axial_res_f, freq, mtab);
    return hipGetLastError();
}

}  // namespace mcrt
