// mcrt_label3d.hip -- the ground truth of the 3-D products (contracts in include/mcrt.h): k_recon_label_splat and k_recon_label_resolve, a
// freehand label volume by majority vote (mcrt_recon_label_frames), and k_render_label, the label of what a rendering shows
// (mcrt_render_label_frames).  The reference has no counterpart.  Integers only: every result is order-free.
#include "mcrt_voxels.h"

namespace mcrt {

// The vote table is [voxel][label] ([label][voxel] is tools/variants/recon_label_by_label.patch): a sample's word, which is also
// the key its run is recognised by.  Below 2^31 (mcrt_recon_label_frames refuses a larger table).
__device__ __forceinline__ int vote_word(uint32_t vox, uint32_t label, uint32_t n_vox, uint32_t n_labels)
{
    return (int)(vox * n_labels + label);
}

// A lane owns one sample, consecutive lanes consecutive rows; the voxel is sample_voxel's, the one k_recon_splat bins into (mcrt_voxels.h).
// Tissue maps are piecewise constant along a scan-line, so runs of equal (voxel, label) inside a wavefront are the common case; they are found
// on the vote word (wave_runs), and a run's LAST lane issues one atomic add of the run's length -- nothing is scanned, a vote has no value.
// Lanes that vote for nothing (outside the block, a label >= n_labels, past the stack's end) carry word -1: they break runs, and a run of
// them issues nothing.
__global__ void __launch_bounds__(256) k_recon_label_splat(ReconLabelArgs a)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    int word = -1;
    bool outside = false, no_label = false;
    if (g < a.blk.n_samples) {
        const int vox = sample_voxel(a.blk, g);
        const uint32_t l = a.stack[g];
        const bool inside = vox >= 0;
        outside = !inside; no_label = inside && l >= a.n_labels;
        if (inside && l < a.n_labels) word = vote_word(vox, l, a.n_vox, a.n_labels);
    }
    wave_stats(a.blk.stats, lane, outside, no_label);
    const WaveRuns run = wave_runs(word, lane);
    if (run.last && word >= 0) atomicAdd(&a.votes[word], lane - run.start + 1u);
}

// A workgroup of 256 lanes owns k_recon_resolve's tile of RECON_TW x RECON_TV x RECON_TU voxels.  It stages ONE BYTE per voxel of the tile and a
// halo of H = fill_radius voxels in LDS: the winning label, 255 where nothing voted (a point outside the block too).  The winner is found
// while staging, labels ascending with a strict >, so the smallest label wins a tie; a staged voxel of the tile itself also writes its
// count and its winner's votes.  A hole looks through the cubes of h = 1..H in LDS and reads only sampled voxels.  Its tally is no array per
// lane: a 256-bit presence mask of the cube's labels in four words, then one count over the cube per present label, ascending with a strict
// > again.  LDS: (8 + 2H)(8 + 2H)(32 + 2H) bytes, 2 KB at H = 0, 7.3 KB at H = 3.
__global__ void __launch_bounds__(256) k_recon_label_resolve(ReconLabelArgs a)
{
    extern __shared__ unsigned char swin[];                         // [RW][RV][RU] (launch_recon_label_resolve sizes it)
    const VoxelTile t = voxel_tile(a.blk);

    for (int idx = threadIdx.x; idx < t.RU * t.RV * t.RW; idx += 256) {
        uint32_t vox;
        bool own;
        uint32_t win = MCRT_LABEL_NONE;
        if (staged_voxel(t, idx, vox, own)) {
            uint32_t count = 0u, best = 0u;
            for (uint32_t l = 0; l < a.n_labels; l++) {
                const uint32_t n = a.votes[vote_word(vox, l, a.n_vox, a.n_labels)];
                count += n;
                if (n > best) { best = n; win = l; }
            }
            if (own) {
                if (a.count_out) a.count_out[vox] = count;
                if (a.votes_out) a.votes_out[vox] = best;
            }
        }
        swin[idx] = (unsigned char)win;
    }
    if (!a.out) return;                                             // (uniform: only counts or votes were asked for)
    __syncthreads();

    for (int idx = threadIdx.x; idx < RECON_TU * RECON_TV * RECON_TW; idx += 256) {
        size_t vox;
        int li;
        if (!tile_voxel(t, idx, vox, li)) continue;
        uint32_t label = swin[li];
        if (label == MCRT_LABEL_NONE)
            for (int h = 1; h <= t.H; h++) {
                unsigned long long m0 = 0ull, m1 = 0ull, m2 = 0ull, m3 = 0ull;     // which labels the cube holds (four words, never indexed: no scratch)
                uint32_t n = 0u;
                cube_walk(t, li, h, [&](int lj) {
                    const uint32_t s = swin[lj];
                    if (s == MCRT_LABEL_NONE) return;
                    const unsigned long long bit = 1ull << (s & 63u);
                    const uint32_t k = s >> 6;
                    m0 |= k == 0u ? bit : 0ull; m1 |= k == 1u ? bit : 0ull; m2 |= k == 2u ? bit : 0ull; m3 |= k == 3u ? bit : 0ull;
                    n++;
                });
                if (n < a.blk.fill_min) continue;
                uint32_t best = 0u;
                for (uint32_t k = 0; k < 4u; k++) {
                    unsigned long long m = k == 0u ? m0 : k == 1u ? m1 : k == 2u ? m2 : m3;
                    while (m) {
                        const uint32_t l = 64u * k + (uint32_t)__ffsll((long long)m) - 1u;
                        m &= m - 1ull;
                        uint32_t tally = 0u;
                        for (int dw = -h; dw <= h; dw++)                    // (written out: through cube_walk this walk costs 17 instructions, profiles/voxel_block)
                            for (int dv = -h; dv <= h; dv++)
                                for (int du = -h; du <= h; du++) tally += swin[li + (dw * t.RV + dv) * t.RU + du] == l ? 1u : 0u;
                        if (tally > best) { best = tally; label = l; }
                    }
                }
                break;
            }
        a.out[vox] = (uint8_t)label;
    }
}

// One lane per pixel in k_render's picture tile, one frame per blockIdx.y.  The point is pixel_base plus the depth buffer's step in (float)s's
// place, so it is bit for bit the point k_render sampled; the voxel is nearest_voxel's (mcrt_voxels.h).  No LDS, no scratch.
__global__ void __launch_bounds__(256) k_render_label(RenderLabelArgs a)
{
    uint32_t i, j;
    picture_tile(a.view, i, j);
    if (i >= a.view.nx || j >= a.view.ny) return;
    const uint32_t f = blockIdx.y;
    const size_t o = ((size_t)f * a.view.ny + j) * a.view.nx + i;
    const float s = a.depth[o];
    uint32_t label = MCRT_LABEL_NONE;
    if (s >= 0.0f && s < (float)a.view.n_steps) {                  // (a NaN compares false)
        float b[3];
        size_t vox;
        pixel_base(a.view, i, j, b);
        if (nearest_voxel(a.view, b[0] + s * a.view.ds[0], b[1] + s * a.view.ds[1], b[2] + s * a.view.ds[2], vox))
            label = a.labels[(size_t)f * a.view.nu * a.view.nv * a.view.nw + vox];
    }
    a.out[o] = (uint8_t)label;
}

hipError_t launch_recon_label_splat(const ReconLabelArgs &a, hipStream_t st)
{
    if (a.blk.n_samples == 0u || a.blk.n_samples >= 0x80000000u || (uint64_t)a.n_vox * a.n_labels >= 0x80000000ull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_recon_label_splat, dim3((a.blk.n_samples + 255u) / 256u), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_recon_label_resolve(ReconLabelArgs a, hipStream_t st) { return launch_resolve(k_recon_label_resolve, a, 1u, st); }

hipError_t launch_render_label(const RenderLabelArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(k_render_label, dim3((picture_tile_waves(a.view.nx, a.view.ny) + 3u) / 4u, a.view.F), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace mcrt
