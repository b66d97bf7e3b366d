// mcrt_shade.hip -- the stages of the wavefront pipeline around the walk: k_init (the first ray of every path) and k_shade (the interface
// physics of a bounce's live rays, survivors compacted into the next bounce's queue).
#include "mcrt_device.h"
#include "mcrt_shade.h"

#ifndef MCRT_SHADE_WAVES
#define MCRT_SHADE_WAVES 5             // k_shade wavefronts per SIMD the register budget is set for
#endif

namespace mcrt {

// =============================================================================================================
// The frame is a WAVEFRONT pipeline that mirrors the reference's own structure (scene::cast_rays produces segments,
// main.cpp:106-144 consumes them), one launch per stage and bounce, queues of live paths in HBM between stages:
//
//   k_init            first_ray of every (scan-line, sample) path, scene.cpp:83-101            1 lane  / path
//   for bounce b:
//     k_trace_lane    closest hit of every live ray: BVH4 walk                                  1 lane  / ray
//     k_shade         thickness draw, travel, hit_boundary, segment record, next ray;           1 lane  / ray
//                     survivors are compacted into the next bounce's queue (wave ballot + prefix)
//   k_march           RF accumulation of every segment (main.cpp:112-140)                       2 lanes / segment
//
// Every stage therefore runs with full wavefronts of lanes doing the same thing: dead paths cost nothing after the
// bounce they die in, the fp64-heavy interface physics is not replicated, and the lean walk kernel keeps 5 waves/SIMD.
// Paths draw random numbers from their own (scan-line, sample, bounce) counter and RF bins are integer sums, so the
// image does not depend on queue order.  Path state, rays and closest-hit words live in QUEUE ORDER and are compacted with
// the queue every bounce (ping-pong halves by bounce parity): every launch reads and writes them densely and coalesced.
// (Round 3 measured the alternative the sample loop of scene.cpp:102-110 suggests -- queues SORTED into bundles of the sample
// paths of a scan-line with the same reflect / refract history, path state in place by path id: 58 vs 56 % of the walk's lanes
// active, the pass 8 % slower; DESIGN.md A.4, profiles/round3/exp_*.)
// =============================================================================================================

__global__ void __launch_bounds__(256) k_init(FrameArgs a)
{
    const uint32_t pos = blockIdx.x * blockDim.x + threadIdx.x;          // this thread fills queue position `pos`
    const uint32_t np = a.ne * a.S;
    if (pos == 0) { a.counts[0] = np; for (uint32_t b = 1; b <= a.B; b++) a.counts[b] = 0u; }
    if (pos < MCRT_MAX_BOUNCES * MCRT_XCDS) a.cursors[(size_t)pos * MCRT_CURSOR_STRIDE] = 0u;   // k_trace_lane's queue cursors (relative, see there)
    if (pos >= np) return;
    // Queue position -> path.  Paths are numbered frame-major (pid = (frame * ne_frame + scan-line) * S + sample) but QUEUED
    // scan-line-major: the F frames of a scan-line sit next to each other.  The queue is swept in order, so the rays in flight
    // then belong to a few scan-lines (times all frames) and walk the same part of the BVH; later bounces inherit the order
    // from the order-preserving compaction of k_shade.
    const uint32_t F = a.ne / a.ne_frame;
    const uint32_t qline = pos / a.S, sample = pos % a.S;
    const uint32_t scan = qline / F, fr = qline % F;
    const uint32_t pid = (fr * a.ne_frame + scan) * a.S + sample;
    const size_t pe = (size_t)fr * a.pose_stride + a.e_begin + scan;      // pose_stride = 0: one probe pose for every frame of the pass (transducer.h:64-67)
    const f3 from = mk(a.el_pos[3 * pe], a.el_pos[3 * pe + 1], a.el_pos[3 * pe + 2]);
    const f3 dir = mk(a.el_dir[3 * pe], a.el_dir[3 * pe + 1], a.el_dir[3 * pe + 2]);
    const float intensity = a.I0 / (float)a.S;
    // Every sample path of a scan-line starts as a copy of the same first_ray (scene.cpp:83-101): the state of bounce 0 is written ONCE per queued
    // (scan-line, frame), at its first sample's position -- where the walk reads it (ray_stride) and where k_shade / k_path look it up for all S samples
    // (MCRT_STATE0_AT) -- instead of S times (48 B x 2.6 M paths per 20-frame pass written here and read back by k_shade).
    if (sample == 0u) {
        a.st0[pos] = make_float4(from.x, from.y, from.z, ray_len(intensity, a.mats[2 * a.start_mat].y, a));   // origin | length factor of the ray (ray_of)
        a.st1[pos] = make_float4(dir.x, dir.y, dir.z, __int_as_float((int)a.start_mat));
        a.st2[pos] = make_float4(0.0f, 0.0f, __int_as_float(OUT_NONE), intensity);  // distance_traveled (double) | outside | intensity
    }
    a.queue[pos] = pid;                                  // queue of bounce 0 (buffer 0 of two)
    a.seg_count[pid] = 0u;
    if (pos < a.ne) a.key0[pos] = MCRT_KEY_MISS;          // bounce 0: one closest-hit word per queued (scan-line, frame)
}

// ---- interface interaction of a bounce's live rays: one lane per ray ----
// FOLD (launched for b == 0 only, FrameArgs::fold_b0): the start medium is silent, so all that bounce 0 adds to the image is every path's boundary
// echo (main.cpp:139).  The workgroup -- 256 paths of ONE queued scan-line, S % 256 == 0 -- adds them into LDS bins exactly as k_march's rf_add
// does and flushes with the same global integer atomics into the same row: integer sums commute, the image is bit-identical.  No march record of
// bounce 0 is written (48 B per path) and no k_march(0) sorts, hands out and reloads them.
template <bool STATS, bool FOLD>
MCRT_DEV void shade_bounce(const FrameArgs &a, uint32_t b)
{
    const uint32_t n = a.counts[b];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (blockIdx.x * blockDim.x >= n) return;
    const int lane = threadIdx.x & 63;
    // the scene's material and mesh tables in LDS when they fit (they nearly always do: the reference's scenes have 9 materials and <= 11 meshes):
    // a ray looks up five material rows and one mesh row -- a quarter of this kernel's cache accesses, and the frame is bound by their sum
    __shared__ float4 mats_l[2 * MCRT_SHADE_TABLE];
    __shared__ uint4 meshes_l[MCRT_SHADE_TABLE];
    const bool tables_in_lds = a.n_mat <= (uint32_t)MCRT_SHADE_TABLE && a.n_mesh <= (uint32_t)MCRT_SHADE_TABLE;
    if (tables_in_lds) {
        for (uint32_t r = threadIdx.x; r < 2u * a.n_mat; r += blockDim.x) mats_l[r] = a.mats[r];
        for (uint32_t r = threadIdx.x; r < a.n_mesh; r += blockDim.x) meshes_l[r] = a.meshes[r];
        __syncthreads();
    }
    __shared__ long long fold_bin[FOLD ? MCRT_MAX_ROWS : 1];
    __shared__ uint32_t fold_flag[FOLD ? MCRT_MAX_ROWS / 32 : 1];
    if (FOLD) {
        for (uint32_t r = threadIdx.x; r < a.R; r += blockDim.x) fold_bin[r] = 0;
        for (uint32_t r = threadIdx.x; r < (a.R + 31u) >> 5; r += blockDim.x) fold_flag[r] = 0u;
        __syncthreads();
    }
    const ShadeTables tb = { a.mats, a.meshes, mats_l, meshes_l, tables_in_lds };
    // two queue buffers, ping-pong by bounce parity (like the path state)
    const uint32_t *q_in = a.queue + (size_t)(b & 1u) * a.ne * a.S;
    uint32_t *q_out = a.queue + (size_t)((b + 1u) & 1u) * a.ne * a.S;
    const bool valid = i < n;
    bool alive = false, reflected = false;
    uint32_t pid = 0;
    PathState ps; ps.from = mk(0, 0, 0); ps.dir = mk(0, 0, 1); ps.intensity = 0.0f; ps.media = 0; ps.outside = OUT_NONE; ps.dist_mm = 0.0;
    unsigned long long st_seg = 0, st_hits = 0;
    if (valid) {
        pid = q_in[i];
        // path state lives in queue order (ping-pong halves by bounce parity), so a wavefront reads and writes it coalesced
        const size_t sin = (size_t)(b & 1u) * a.ne * a.S + (b == 0u ? MCRT_STATE0_AT(i, a.S) : i);
        const float4 s0 = a.st0[sin], s1 = a.st1[sin], s2 = a.st2[sin];
        ps.from = mk(s0.x, s0.y, s0.z); ps.intensity = s2.w;
        ps.dir = mk(s1.x, s1.y, s1.z); ps.media = __float_as_int(s1.w);
        ps.dist_mm = __hiloint2double(__float_as_int(s2.y), __float_as_int(s2.x));
        ps.outside = __float_as_int(s2.z);
        const Ray ry = ray_of(ps.from, ps.dir, s0.w, a);          // the segment the walk tested (same expressions, same bits)
        const f3 f2 = ry.f2, to = ry.to;
        const size_t hi = (b == 0u) ? (size_t)(i / a.S) : (size_t)i;            // bounce 0: one walk per queued (scan-line, frame) (see k_trace_lane, k_init)
        const unsigned long long key = ((b & 1u) ? a.key1 : a.key0)[hi];
        // the triangle this ray ends on and its successor leaves, for the beams of the next bounce (mcrt_beam.hip), by path -- stored here, before shade_path, so that
        // nothing more is live across it (k_shade stays at 64 registers), and only where that bounce runs by beams: the branch is wave-uniform
        if ((a.beam_mask >> (b + 1u)) & 1u) a.from_tri[pid] = (uint32_t)key;
        FoldEcho fo;
        alive = shade_path<STATS, FOLD>(a, tb, b, pid, ps, f2, to, key, reflected, st_seg, st_hits, &fo);
        if (FOLD) {
            // the boundary echo of the finished segment, as k_march adds it: time, row, rf_add
            const double te = fo.t_start + a.time_step * (double)(uint32_t)(fo.steps - 1u);
            const int row = row_of_thr(te, a.row_thr, a.R, a.inv_row_dt, a.thr_end);
            if (row >= 0) {
                const float echo = fo.refl / (float)a.S;
                if (!(fabsf(echo) < 1024.0f)) atomicOr(&fold_flag[row >> 5], 1u << (row & 31));
                else { const long long v = fix40(echo); if (v != 0) atomicAdd((unsigned long long *)&fold_bin[row], (unsigned long long)v); }
            }
        }
    }
    const f3 from = ps.from, dir = ps.dir; const float intensity = ps.intensity; const int media = ps.media, outside = ps.outside; const double dist_mm = ps.dist_mm;

    // survivors -> next bounce's queue (ballot + prefix; ONE atomic per workgroup: tens of thousands of returning atomics on the
    // single counter would serialise in L2 and bound the kernel).  Inside a workgroup's block the reflected rays
    // come first, then the refracted ones, each in queue order: the samples of a scan-line that took the same decisions stay
    // adjacent, so the rays of a k_trace_lane wavefront mostly belong to a few tight bundles (same nodes, similar walk length).
    __shared__ uint32_t wave_live[4], wave_refl[4], block_base;
    const unsigned long long live = __ballot(alive);
    const unsigned long long live_refl = __ballot(alive && reflected);
    const int wv = threadIdx.x >> 6;
    if (lane == 0) { wave_live[wv] = (uint32_t)__popcll(live); wave_refl[wv] = (uint32_t)__popcll(live_refl); }
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t total = wave_live[0] + wave_live[1] + wave_live[2] + wave_live[3];
        block_base = total ? atomicAdd(&a.counts[b + 1u], total) : 0u;
    }
    __syncthreads();
    if (live) {
        // (round 5: reflected-first over the WORKGROUP's 256 rays, not per wavefront -- three of the next bounce's four 64-ray blocks are then of one history,
        //  which is what a ray packet wants, k_trace_packet)
        const uint32_t refl_all = wave_refl[0] + wave_refl[1] + wave_refl[2] + wave_refl[3];
        uint32_t refl_before = 0, refr_before = 0;
        for (int w = 0; w < wv; w++) { refl_before += wave_refl[w]; refr_before += wave_live[w] - wave_refl[w]; }
        if (alive) {
            const unsigned long long below = (1ull << lane) - 1ull;
            const uint32_t pos = block_base + (reflected ? refl_before + (uint32_t)__popcll(live_refl & below)
                                                         : refl_all + refr_before + (uint32_t)__popcll(live & ~live_refl & below));
            q_out[pos] = pid;
            ((b & 1u) ? a.key0 : a.key1)[pos] = MCRT_KEY_MISS;            // the next bounce's closest-hit word of this ray
            const size_t so = (size_t)((b + 1u) & 1u) * a.ne * a.S + pos;
            const float Ls = ray_len(intensity, tb.mat(2 * media).y, a);
            a.st0[so] = make_float4(from.x, from.y, from.z, Ls);   // origin | the next ray's length factor
            a.st1[so] = make_float4(dir.x, dir.y, dir.z, __int_as_float(media));
            // the next ray's beam code and medium for k_beam_rank (mcrt_beam.hip), which then reads 4 bytes of this ray in place of its state -- only where that
            // bounce is tested in the beam order: the branch is wave-uniform
            if ((a.order_mask >> (b + 1u)) & 1u) beam_words(a)[pos] = beam_word_of(from, dir, Ls, media, a);
            a.st2[so] = make_float4(__int_as_float(__double2loint(dist_mm)), __int_as_float(__double2hiint(dist_mm)), __int_as_float(outside), intensity);
        }
    }
    if (STATS) {
        long long x = wave_sum_i64((long long)st_seg), y = wave_sum_i64((long long)st_hits);
        if (lane == 0) { if (x) atomicAdd(&a.stats[3], (unsigned long long)x); if (y) atomicAdd(&a.stats[5], (unsigned long long)y); }
    }
    if (FOLD) {
        // (the barriers above are past every echo's LDS add.)  The workgroup's queue positions are those of ONE queued scan-line (k_init's order: the F frames of
        // a scan-line next to each other); its row of the frames' RF block as in k_march's epilogue
        const uint32_t F = a.ne / a.ne_frame, ql = (blockIdx.x * blockDim.x) / a.S;
        const uint32_t line = (ql % F) * a.ne_frame + ql / F;
        const size_t row = (size_t)(line / a.ne_frame) * a.acc_stride + a.acc_off + line % a.ne_frame;
        const uint32_t nf = (a.R + 31u) >> 5;
        for (uint32_t r = threadIdx.x; r < a.R; r += blockDim.x) {
            const long long v = fold_bin[r];
            if (v != 0) atomicAdd((unsigned long long *)&a.acc[row * a.R + r], (unsigned long long)v);
        }
        for (uint32_t r = threadIdx.x; r < nf; r += blockDim.x) { const uint32_t f = fold_flag[r]; if (f) atomicOr(&a.flags[row * nf + r], f); }
    }
}

template <bool STATS>
__global__ void __launch_bounds__(256, MCRT_SHADE_WAVES) k_shade(FrameArgs a, uint32_t b) { shade_bounce<STATS, false>(a, b); }
// bounce 0 with its boundary echoes folded in: a kernel of its own, so that k_shade keeps its registers (64, eight wavefronts per SIMD; this one 67, seven)
__global__ void __launch_bounds__(256, MCRT_SHADE_WAVES) k_shade_fold(FrameArgs a) { shade_bounce<false, true>(a, 0u); }

hipError_t launch_init(const FrameArgs &a, hipStream_t st)
{
    const uint32_t np = a.ne * a.S;
    hipLaunchKernelGGL(k_init, dim3((np + 255u) / 256u), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_shade(const FrameArgs &a, uint32_t b, bool stats, hipStream_t st)
{
    const uint32_t np = a.ne * a.S;
    const dim3 grid((np + 255u) / 256u), blk(256);
    if (stats) hipLaunchKernelGGL((k_shade<true>), grid, blk, 0, st, a, b);
    else if (a.fold_b0 && b == 0u) hipLaunchKernelGGL(k_shade_fold, grid, blk, 0, st, a);      // (fill_pass sets fold_b0 only where S % 256 == 0 and nothing is counted)
    else hipLaunchKernelGGL((k_shade<false>), grid, blk, 0, st, a, b);
    return hipGetLastError();
}

}  // namespace mcrt
