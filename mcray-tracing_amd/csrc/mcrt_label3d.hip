// mcrt_label3d.hip -- the ground truth of the 3-D products (contracts in include/mcrt.h): k_recon_label_splat and k_recon_label_resolve, a
// freehand label volume by majority vote (mcrt_recon_label_frames), and k_render_label, the label of what a rendering shows
// (mcrt_render_label_frames).  The reference has no counterpart.  Integers only: every result is order-free.
#include "mcrt_device.h"

namespace mcrt {

// The vote table is [voxel][label] ([label][voxel] is tools/variants/recon_label_by_label.patch): a sample's word, which is also
// the key its run is recognised by.  Below 2^31 (mcrt_recon_label_frames refuses a larger table).
__device__ __forceinline__ int vote_word(uint32_t vox, uint32_t label, uint32_t n_vox, uint32_t n_labels)
{
    return (int)(vox * n_labels + label);
}

// A lane owns one sample, consecutive lanes consecutive rows, and the position is mcrt_recon_frames' contract restated expression by expression
// (k_recon_splat is left as it is: the two kernels share the contract, not code).  Tissue maps are piecewise constant along a scan-line, so
// runs of equal (voxel, label) inside a wavefront are the common case; they are found with k_recon_splat's head ballot on the vote word, and a
// run's LAST lane issues one atomic add of the run's length -- nothing is scanned, a vote has no value.  Lanes that vote for nothing (outside
// the block, a label >= n_labels, past the stack's end) carry word -1: they break runs, and a run of them issues nothing.  The two statistics
// are one atomic per wavefront each.
__global__ void __launch_bounds__(256) k_recon_label_splat(ReconLabelArgs a)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    int word = -1;
    bool outside = false, no_label = false;
    if (g < a.n_samples) {
        const uint32_t line = g / a.R, r = g - line * a.R;
        const float *p = a.pos + 3u * (size_t)line, *d = a.dir + 3u * (size_t)line;
        const float t = (float)r * a.row_u;
        const float Px = p[0] + d[0] * t, Py = p[1] + d[1] * t, Pz = p[2] + d[2] * t;
        const float iu = floorf((((a.b[0] + Px * a.A[0]) + Py * a.A[1]) + Pz * a.A[2]) + 0.5f);
        const float iv = floorf((((a.b[1] + Px * a.A[3]) + Py * a.A[4]) + Pz * a.A[5]) + 0.5f);
        const float iw = floorf((((a.b[2] + Px * a.A[6]) + Py * a.A[7]) + Pz * a.A[8]) + 0.5f);
        const bool inside = iu >= 0.0f && iu < (float)a.nu && iv >= 0.0f && iv < (float)a.nv && iw >= 0.0f && iw < (float)a.nw;   // (a NaN compares false)
        const uint32_t l = a.stack[g];
        outside = !inside; no_label = inside && l >= a.n_labels;
        if (inside && l < a.n_labels)
            word = vote_word(((uint32_t)iw * a.nv + (uint32_t)iv) * a.nu + (uint32_t)iu, l, a.n_vox, a.n_labels);
    }
    if (a.stats) {
        const uint32_t n_out = (uint32_t)__popcll(__ballot(outside)), n_bad = (uint32_t)__popcll(__ballot(no_label));
        if (lane == 0u) {
            if (n_out) atomicAdd(&a.stats[0], n_out);
            if (n_bad) atomicAdd(&a.stats[1], n_bad);
        }
    }
    const int before = __shfl_up(word, 1, 64);
    const unsigned long long heads = __ballot(lane == 0u || before != word);
    const uint32_t start = 63u - (uint32_t)__clzll((long long)(heads & (~0ull >> (63u - lane))));    // (bit 0 is always set)
    const bool last = lane == 63u || ((heads >> (lane + 1u)) & 1ull);
    if (last && word >= 0) atomicAdd(&a.votes[word], lane - start + 1u);
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
    const int H = (int)a.fill_radius, RU = RECON_TU + 2 * H, RV = RECON_TV + 2 * H, RW = RECON_TW + 2 * H;
    const int nu = (int)a.nu, nv = (int)a.nv, nw = (int)a.nw;
    const uint32_t bu = blockIdx.x % a.tu, bv = (blockIdx.x / a.tu) % a.tv, bw = blockIdx.x / (a.tu * a.tv);
    const int u0 = (int)bu * RECON_TU, v0 = (int)bv * RECON_TV, w0 = (int)bw * RECON_TW;        // the tile's first voxel

    for (int idx = threadIdx.x; idx < RU * RV * RW; idx += 256) {
        const int lu = idx % RU, lv = (idx / RU) % RV, lw = idx / (RU * RV);
        const int gu = u0 - H + lu, gv = v0 - H + lv, gw = w0 - H + lw;
        uint32_t win = MCRT_LABEL_NONE;
        if (gu >= 0 && gu < nu && gv >= 0 && gv < nv && gw >= 0 && gw < nw) {
            const uint32_t vox = ((uint32_t)gw * a.nv + (uint32_t)gv) * a.nu + (uint32_t)gu;
            uint32_t count = 0u, best = 0u;
            for (uint32_t l = 0; l < a.n_labels; l++) {
                const uint32_t n = a.votes[vote_word(vox, l, a.n_vox, a.n_labels)];
                count += n;
                if (n > best) { best = n; win = l; }
            }
            if (lu >= H && lu < H + RECON_TU && lv >= H && lv < H + RECON_TV && lw >= H && lw < H + RECON_TW) {     // the tile's own: no other workgroup writes it
                if (a.count_out) a.count_out[vox] = count;
                if (a.votes_out) a.votes_out[vox] = best;
            }
        }
        swin[idx] = (unsigned char)win;
    }
    if (!a.out) return;                                             // (uniform: only counts or votes were asked for)
    __syncthreads();

    for (int idx = threadIdx.x; idx < RECON_TU * RECON_TV * RECON_TW; idx += 256) {
        const int tu = idx % RECON_TU, tv = (idx / RECON_TU) % RECON_TV, tw = idx / (RECON_TU * RECON_TV);
        const int gu = u0 + tu, gv = v0 + tv, gw = w0 + tw;
        if (gu >= nu || gv >= nv || gw >= nw) continue;
        const int li = ((tw + H) * RV + (tv + H)) * RU + (tu + H);
        uint32_t label = swin[li];
        if (label == MCRT_LABEL_NONE)
            for (int h = 1; h <= H; h++) {
                unsigned long long m0 = 0ull, m1 = 0ull, m2 = 0ull, m3 = 0ull;     // which labels the cube holds (four words, never indexed: no scratch)
                uint32_t n = 0u;
                for (int dw = -h; dw <= h; dw++)
                    for (int dv = -h; dv <= h; dv++)
                        for (int du = -h; du <= h; du++) {
                            const uint32_t s = swin[li + (dw * RV + dv) * RU + du];       // (inside the staged halo: h <= H)
                            if (s == MCRT_LABEL_NONE) continue;
                            const unsigned long long bit = 1ull << (s & 63u);
                            const uint32_t k = s >> 6;
                            m0 |= k == 0u ? bit : 0ull; m1 |= k == 1u ? bit : 0ull; m2 |= k == 2u ? bit : 0ull; m3 |= k == 3u ? bit : 0ull;
                            n++;
                        }
                if (n < a.fill_min) continue;
                uint32_t best = 0u;
                for (uint32_t k = 0; k < 4u; k++) {
                    unsigned long long m = k == 0u ? m0 : k == 1u ? m1 : k == 2u ? m2 : m3;
                    while (m) {
                        const uint32_t l = 64u * k + (uint32_t)__ffsll((long long)m) - 1u;
                        m &= m - 1ull;
                        uint32_t tally = 0u;
                        for (int dw = -h; dw <= h; dw++)
                            for (int dv = -h; dv <= h; dv++)
                                for (int du = -h; du <= h; du++)
                                    tally += swin[li + (dw * RV + dv) * RU + du] == l ? 1u : 0u;
                        if (tally > best) { best = tally; label = l; }
                    }
                }
                break;
            }
        a.out[((size_t)gw * a.nv + (size_t)gv) * a.nu + (size_t)gu] = (uint8_t)label;
    }
}

// One lane per pixel, an 8 x 8 tile of the picture per wavefront as k_render's default, one frame per blockIdx.y.  The point is
// mcrt_render_frames' own expression with the depth buffer's step in (float)s's place, so it is bit for bit the point k_render sampled; the
// voxel is the nearest rule of the label gathers.  The indices are made only where they are inside: 0 <= k < n < 2^24 holds in float and
// (uint32_t)k is exact.  No LDS, no scratch.
__global__ void __launch_bounds__(256) k_render_label(RenderLabelArgs a)
{
    const uint32_t lane = threadIdx.x & 63u, wave = blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint32_t tx = (a.nx + 7u) / 8u, i = (wave % tx) * 8u + (lane & 7u), j = (wave / tx) * 8u + (lane >> 3);
    if (i >= a.nx || j >= a.ny) return;
    const uint32_t f = blockIdx.y;
    const size_t o = ((size_t)f * a.ny + j) * a.nx + i;
    const float s = a.depth[o];
    uint32_t label = MCRT_LABEL_NONE;
    if (s >= 0.0f && s < (float)a.n_steps) {                       // (a NaN compares false)
        const float fi = (float)i, fj = (float)j;
        const float pu = ((a.origin[0] + fi * a.di[0]) + fj * a.dj[0]) + s * a.ds[0];
        const float pv = ((a.origin[1] + fi * a.di[1]) + fj * a.dj[1]) + s * a.ds[1];
        const float pw = ((a.origin[2] + fi * a.di[2]) + fj * a.dj[2]) + s * a.ds[2];
        const float fu = floorf(pu), fv = floorf(pv), fw = floorf(pw);
        const float ku = fu + (pu - fu >= 0.5f ? 1.0f : 0.0f), kv = fv + (pv - fv >= 0.5f ? 1.0f : 0.0f), kw = fw + (pw - fw >= 0.5f ? 1.0f : 0.0f);
        if (ku >= 0.0f && ku < (float)a.nu && kv >= 0.0f && kv < (float)a.nv && kw >= 0.0f && kw < (float)a.nw)
            label = a.labels[(size_t)f * a.nu * a.nv * a.nw + ((size_t)(uint32_t)kw * a.nv + (uint32_t)kv) * a.nu + (uint32_t)ku];
    }
    a.out[o] = (uint8_t)label;
}

hipError_t launch_recon_label_splat(const ReconLabelArgs &a, hipStream_t st)
{
    if (a.n_samples == 0u || a.n_samples >= 0x80000000u || (uint64_t)a.n_vox * a.n_labels >= 0x80000000ull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_recon_label_splat, dim3((a.n_samples + 255u) / 256u), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_recon_label_resolve(ReconLabelArgs a, hipStream_t st)
{
    if (a.fill_radius > RECON_MAX_FILL) return hipErrorInvalidValue;
    a.tu = (a.nu + RECON_TU - 1u) / RECON_TU; a.tv = (a.nv + RECON_TV - 1u) / RECON_TV;
    const uint32_t tw = (a.nw + RECON_TW - 1u) / RECON_TW;
    if ((uint64_t)a.tu * a.tv * tw >= RECON_MAX_TILES) return hipErrorInvalidValue;     // (mcrt_recon_label_frames refuses such a grid before anything is enqueued)
    const uint32_t H2 = 2u * a.fill_radius, cells = (RECON_TU + H2) * (RECON_TV + H2) * (RECON_TW + H2);
    hipLaunchKernelGGL(k_recon_label_resolve, dim3(a.tu * a.tv * tw), dim3(256), cells, st, a);
    return hipGetLastError();
}

hipError_t launch_render_label(const RenderLabelArgs &a, hipStream_t st)
{
    const uint32_t waves = ((a.nx + 7u) / 8u) * ((a.ny + 7u) / 8u);          // (nx * ny < 2^31: no overflow)
    hipLaunchKernelGGL(k_render_label, dim3((waves + 3u) / 4u, a.F), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace mcrt
