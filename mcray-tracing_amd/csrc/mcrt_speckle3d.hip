// mcrt_speckle3d.hip -- 3-D speckle reduction over voxel blocks (mcrt_speckle_volume_frames; contract in include/mcrt.h): k_srad3, the
// conservative 6-neighbour form of k_srad's diffusion with a weight per axis, one iteration per launch over a stack [F][nw][nv][nu].
// The reference has no counterpart.
#include "mcrt_device.h"

namespace mcrt {

// A workgroup of 256 lanes owns a tile of SRAD3_TV x SRAD3_TU voxels of (v, u) and marches it along w through a chunk of SRAD3_CW slices.
// X' at slice l reads c at l and l + 1 and X at l - 1 .. l + 1, and c at l + 1 reads X at l + 2: the window in LDS holds four slices of X
// (slice s in slot s & 3) and two of c (slot s & 1).  A slice of X is the tile plus 1 voxel on the low and 2 on the high in-plane sides,
// intersected with the block; c is computed on the tile plus 1 voxel on the high sides (what X' of the tile reads), once per slice of the
// march; the rings and the chunk's 1 + 2 halo slices are recomputed by the neighbouring workgroups.  Neighbour indices are clamped against
// the BLOCK (a clamped neighbour is the voxel itself, in LDS too), and nothing outside the block is read or computed.  c never goes to memory.
// A step of the march, for slice l:   the registers -> X[l + 2]'s slot  |  fetch X[l + 3] into registers  |  sync  |  c[l + 1] from X[l .. l + 2]  |
// sync  |  X'[l] -> dst  |  sync  -- the fetch of the next step's slice is in flight while this one is computed.
// Every voxel's arithmetic is the contract's, expression by expression, whatever the tile and the chunk: the tiling changes no bit.
// LDS: (TV + 3) x (TU + 3) floats, six times: 11 x 35 x 6 floats = 9.0 KB (a pitch of 35 dwords: a wavefront's consecutive voxels fall on consecutive banks).
// The march is bound by instruction issue and by its three barriers per slice, not by memory: a small tile and a short chunk (one voxel per
// lane and slice, many workgroups per CU) measured faster than 16 x 64 x 16 on every block.
constexpr int S3_RV = SRAD3_TV + 3, S3_RU = SRAD3_TU + 3, S3_RN = S3_RV * S3_RU;     // a staged slice; LDS (lj, li) is voxel (j0 - 1 + lj, i0 - 1 + li)
constexpr int S3_PER = (S3_RN + 255) / 256;                                         // its floats per lane

struct Srad3Tile { int j0, i0, nv, nu; size_t base; };      // the tile's first voxel, the block's size, the frame's offset

// a slice's staged voxels into registers; step 0 of the contract (X = |v| when finite, else 0) on the first launch of a call only
__device__ __forceinline__ void srad3_fetch(const Speckle3Args &a, const Srad3Tile &t, int l, float (&r)[S3_PER])
{
#pragma unroll
    for (int k = 0; k < S3_PER; k++) {
        const int idx = (int)threadIdx.x + 256 * k, lj = idx / S3_RU, li = idx - lj * S3_RU, gj = t.j0 - 1 + lj, gi = t.i0 - 1 + li;
        float v = 0.0f;
        if (idx < S3_RN && gj >= 0 && gj < t.nv && gi >= 0 && gi < t.nu) {
            v = a.src[t.base + ((size_t)l * (size_t)t.nv + (size_t)gj) * (size_t)t.nu + (size_t)gi];
            if (a.first) { v = fabsf(v); v = v <= 3.402823466e+38f ? v : 0.0f; }
        }
        r[k] = v;
    }
}
__device__ __forceinline__ void srad3_store(float *X, const float (&r)[S3_PER])
{
#pragma unroll
    for (int k = 0; k < S3_PER; k++) {
        const int idx = (int)threadIdx.x + 256 * k;
        if (idx < S3_RN) X[idx] = r[k];
    }
}

// c of slice l on the tile grown by one voxel on the high sides, inside the block; Xd, Xu: the slices below and above, or X itself at the block's ends
__device__ __forceinline__ void srad3_coeff(const Speckle3Args &a, const Srad3Tile &t, const float *Xd, const float *X, const float *Xu, float *c)
{
    constexpr int CU = SRAD3_TU + 1, CN = (SRAD3_TV + 1) * CU;
    for (int k = threadIdx.x; k < CN; k += 256) {
        const int cj = k / CU, ci = k - cj * CU, gj = t.j0 + cj, gi = t.i0 + ci;
        if (gj < t.nv && gi < t.nu) {
            const int idx = (cj + 1) * S3_RU + ci + 1;
            const float x = X[idx];
            const float dN = X[gj > 0 ? idx - S3_RU : idx] - x, dS = X[gj < t.nv - 1 ? idx + S3_RU : idx] - x;
            const float dW = X[gi > 0 ? idx - 1 : idx] - x, dE = X[gi < t.nu - 1 ? idx + 1 : idx] - x;
            const float dD = Xd[idx] - x, dU = Xu[idx] - x;
            const float gN = a.wv * dN, gS = a.wv * dS, gW = a.wu * dW, gE = a.wu * dE, gD = a.ww * dD, gU = a.ww * dU;
            const float S1 = ((((gN + gS) + gW) + gE) + gD) + gU;
            const float S2 = ((((gN * dN + gS * dS) + gW * dW) + gE * dE) + gD * dD) + gU * dU;
            const float m = x + a.hs * S1;
            const float q2 = (a.a * S2 - a.b * (S1 * S1)) / (m * m);
            c[idx] = fminf(fmaxf(1.0f / (1.0f + (q2 - a.q0sq) * a.kq), 0.0f), 1.0f);
        }
    }
}

// X' of slice l on the tile inside the block -> dst; c, cu: c of this slice and of the one above (c itself at the block's end)
__device__ __forceinline__ void srad3_update(const Speckle3Args &a, const Srad3Tile &t, int l, const float *Xd, const float *X, const float *Xu,
                                             const float *c, const float *cu)
{
    for (int k = threadIdx.x; k < SRAD3_TV * SRAD3_TU; k += 256) {
        const int tj = k / SRAD3_TU, ti = k - tj * SRAD3_TU, gj = t.j0 + tj, gi = t.i0 + ti;
        if (gj < t.nv && gi < t.nu) {
            const int idx = (tj + 1) * S3_RU + ti + 1;
            const int iS = gj < t.nv - 1 ? idx + S3_RU : idx, iE = gi < t.nu - 1 ? idx + 1 : idx;
            const float x = X[idx], cc = c[idx];
            const float dN = X[gj > 0 ? idx - S3_RU : idx] - x, dS = X[iS] - x;
            const float dW = X[gi > 0 ? idx - 1 : idx] - x, dE = X[iE] - x;
            const float dD = Xd[idx] - x, dU = Xu[idx] - x;
            const float gN = a.wv * dN, gS = a.wv * dS, gW = a.wu * dW, gE = a.wu * dE, gD = a.ww * dD, gU = a.ww * dU;
            const float D = ((((cc * gN + c[iS] * gS) + cc * gW) + c[iE] * gE) + cc * gD) + cu[idx] * gU;
            a.dst[t.base + ((size_t)l * (size_t)t.nv + (size_t)gj) * (size_t)t.nu + (size_t)gi] = x + a.lamw * D;
        }
    }
}

__global__ void __launch_bounds__(256) k_srad3(Speckle3Args a)
{
    __shared__ float sx[4][S3_RN];
    __shared__ float sc[2][S3_RN];
    const int nw = (int)a.nw;
    uint32_t b = blockIdx.x;
    const uint32_t tu = b % a.tx; b /= a.tx;
    const uint32_t tv = b % a.ty; b /= a.ty;
    const uint32_t ch = b % a.tc, f = b / a.tc;
    Srad3Tile t;
    t.j0 = (int)tv * SRAD3_TV; t.i0 = (int)tu * SRAD3_TU; t.nv = (int)a.nv; t.nu = (int)a.nu;
    t.base = (size_t)f * a.nw * a.nv * a.nu;
    const int l0 = (int)ch * SRAD3_CW, l1 = min(l0 + SRAD3_CW, nw) - 1;       // the chunk's slices, l0 <= l1 < nw
    float r[S3_PER];

    // the slices l0 - 1, l0, l0 + 1 that lie in the block, then c[l0]
    for (int s = max(l0 - 1, 0); s <= min(l0 + 1, nw - 1); s++) {
        srad3_fetch(a, t, s, r);
        srad3_store(sx[s & 3], r);
    }
    __syncthreads();
    srad3_coeff(a, t, sx[max(l0 - 1, 0) & 3], sx[l0 & 3], sx[min(l0 + 1, nw - 1) & 3], sc[l0 & 1]);
    // (c[l0] is ordered against its readers by the first sync of the loop; slot (l0 + 2) & 3 is read by nobody yet)
    if (l0 + 2 < nw) srad3_fetch(a, t, l0 + 2, r);

    for (int l = l0; l <= l1; l++) {
        const int ld = max(l - 1, 0), lu = min(l + 1, nw - 1), lu2 = min(l + 2, nw - 1);
        // X[l + 2] into its slot: the slot held slice l - 2, last read by X'[l - 1] before the sync that ended the previous step
        if (l + 2 < nw) srad3_store(sx[(l + 2) & 3], r);
        if (l < l1 && l + 3 < nw) srad3_fetch(a, t, l + 3, r);
        __syncthreads();
        // c[l + 1] into the slot of c[l - 1], last read by X'[l - 1]
        if (l + 1 < nw) srad3_coeff(a, t, sx[l & 3], sx[lu & 3], sx[lu2 & 3], sc[lu & 1]);
        __syncthreads();
        srad3_update(a, t, l, sx[ld & 3], sx[l & 3], sx[lu & 3], sc[l & 1], sc[lu & 1]);
        __syncthreads();
    }
}

// one iteration over F blocks
hipError_t launch_srad3(Speckle3Args a, uint32_t F, hipStream_t st)
{
    a.tx = (a.nu + SRAD3_TU - 1u) / SRAD3_TU; a.ty = (a.nv + SRAD3_TV - 1u) / SRAD3_TV; a.tc = (a.nw + SRAD3_CW - 1u) / SRAD3_CW;
    const dim3 grid(a.tx * a.ty * a.tc * F), blk(256);      // (no more workgroups than voxels: below 2^31)
    hipLaunchKernelGGL(k_srad3, grid, blk, 0, st, a);
    return hipGetLastError();
}

}  // namespace mcrt
