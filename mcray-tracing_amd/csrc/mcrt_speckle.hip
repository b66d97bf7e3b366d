// mcrt_speckle.hip -- speckle reduction (mcrt_speckle_frames; contract in include/mcrt.h): k_srad, Yu & Acton's speckle-reducing anisotropic
// diffusion in its conservative 4-neighbour form, iterated over a stack of float frames [F][H][W].  The reference has no counterpart.
#include "mcrt_device.h"

namespace mcrt {

// A workgroup of 256 lanes owns a tile of SRAD_TH x SRAD_TW pixels of one frame and carries it through a.n <= TT iterations in LDS.  One
// iteration's X' at (i, j) reads c at (i, j), (i+1, j), (i, j+1) and X at the four neighbours, and c at a pixel reads X at its four
// neighbours: an iteration eats 1 pixel of the low sides and 2 of the high sides.  So the tile is staged with a halo of n low and 2n high,
// and iteration s = 1..n is computed on the tile grown by n - s low and 2 (n - s) high, intersected with the image -- every pixel that a
// later iteration of this launch reads, and no other; the rings are recomputed by the neighbouring workgroups.  Neighbour indices are
// clamped against the IMAGE border (a clamped neighbour is the pixel itself, in LDS too), and nothing outside the image is read or
// computed.  c goes to LDS (the tile plus one pixel on the high sides) and never to memory; the last iteration's X' goes straight to dst.
// Every pixel's arithmetic is the contract's, expression by expression, whatever the tile and TT: the tiling changes no bit.
// LDS: (TH + 3 TT) x (TW + 3 TT) floats, X twice (once for TT = 1: there is no second iteration to hand X' to) and c.
//   TT = 2: 22 x 70 x 3 floats = 18.5 KB,   TT = 4: 28 x 76 x 3 = 25.5 KB   (160 KB per CU)
// Built: k_srad<2>, the default, and k_srad<4> (MCRT_SPECKLE_FUSE=4), which is faster for a single frame.  The un-fused k_srad<1> (19 x 67 x 2
// floats) was measured slower than <2> everywhere and is tools/variants/srad_unfused.patch.
template <int TT>
__global__ void __launch_bounds__(256) k_srad(SpeckleArgs a)
{
    constexpr int RH = SRAD_TH + 3 * TT, RW = SRAD_TW + 3 * TT, RN = RH * RW;
    __shared__ float sx[TT > 1 ? 2 : 1][RN];
    __shared__ float sc[RN];
    const int H = (int)a.H, W = (int)a.W, n = (int)a.n;
    const uint32_t tj = blockIdx.x % a.tx, ti = (blockIdx.x / a.tx) % a.ty, f = blockIdx.x / (a.tx * a.ty);
    const int i0 = (int)ti * SRAD_TH, j0 = (int)tj * SRAD_TW;       // the tile's first pixel
    const int r0 = i0 - n, c0 = j0 - n;                              // LDS (li, lj) is pixel (r0 + li, c0 + lj)
    const size_t frame = (size_t)f * a.H * a.W;

    // the tile and its halo; step 0 of the contract (X = |v| when finite, else 0) on the first launch of a call only
    for (int idx = threadIdx.x; idx < RN; idx += 256) {
        const int li = idx / RW, lj = idx - li * RW, gi = r0 + li, gj = c0 + lj;
        if (li < SRAD_TH + 3 * n && lj < SRAD_TW + 3 * n && gi >= 0 && gi < H && gj >= 0 && gj < W) {
            float v = a.src[frame + (size_t)gi * a.W + (size_t)gj];
            if (a.first) { v = fabsf(v); v = v <= 3.402823466e+38f ? v : 0.0f; }
            sx[0][idx] = v;
        }
    }
    __syncthreads();

    for (int s = 1; s <= n; s++) {
        const float *X = sx[TT > 1 ? (s - 1) & 1 : 0];
        // X' of this iteration: rows lo_i .. hi_i, columns lo_j .. hi_j; c one further on the high sides
        const int lo_i = max(i0 - (n - s), 0), hi_i = min(i0 + SRAD_TH - 1 + 2 * (n - s), H - 1);
        const int lo_j = max(j0 - (n - s), 0), hi_j = min(j0 + SRAD_TW - 1 + 2 * (n - s), W - 1);
        const int hc_i = min(hi_i + 1, H - 1), hc_j = min(hi_j + 1, W - 1);
        const float q0sq = a.q0sq[s - 1], kq = a.kq[s - 1];
        for (int idx = threadIdx.x; idx < RN; idx += 256) {
            const int li = idx / RW, lj = idx - li * RW, gi = r0 + li, gj = c0 + lj;
            if (gi >= lo_i && gi <= hc_i && gj >= lo_j && gj <= hc_j) {
                const float x = X[idx];
                const float dN = X[gi > 0 ? idx - RW : idx] - x, dS = X[gi < H - 1 ? idx + RW : idx] - x;
                const float dW = X[gj > 0 ? idx - 1 : idx] - x, dE = X[gj < W - 1 ? idx + 1 : idx] - x;
                const float S1 = ((dN + dS) + dW) + dE;
                const float S2 = ((dN * dN + dS * dS) + dW * dW) + dE * dE;
                const float m = x + 0.25f * S1;
                const float q2 = (0.5f * S2 - 0.0625f * (S1 * S1)) / (m * m);
                sc[idx] = fminf(fmaxf(1.0f / (1.0f + (q2 - q0sq) * kq), 0.0f), 1.0f);
            }
        }
        __syncthreads();
        for (int idx = threadIdx.x; idx < RN; idx += 256) {
            const int li = idx / RW, lj = idx - li * RW, gi = r0 + li, gj = c0 + lj;
            if (gi >= lo_i && gi <= hi_i && gj >= lo_j && gj <= hi_j) {
                const int iS = gi < H - 1 ? idx + RW : idx, iE = gj < W - 1 ? idx + 1 : idx;
                const float x = X[idx], c = sc[idx];
                const float dN = X[gi > 0 ? idx - RW : idx] - x, dS = X[iS] - x;
                const float dW = X[gj > 0 ? idx - 1 : idx] - x, dE = X[iE] - x;
                const float D = ((c * dN + sc[iS] * dS) + c * dW) + sc[iE] * dE;
                const float xn = x + a.lam4 * D;
                if (s == n) a.dst[frame + (size_t)gi * a.W + (size_t)gj] = xn;     // (the region is the tile inside the image)
                else sx[TT > 1 ? s & 1 : 0][idx] = xn;
            }
        }
        __syncthreads();
    }
}

// one launch of a.n <= fuse iterations over F frames; fuse: 2 or 4 (SRAD_FUSE_MAX), the instantiation
hipError_t launch_srad(SpeckleArgs a, uint32_t F, uint32_t fuse, hipStream_t st)
{
    a.tx = (a.W + SRAD_TW - 1u) / SRAD_TW; a.ty = (a.H + SRAD_TH - 1u) / SRAD_TH;
    const dim3 grid(a.tx * a.ty * F), blk(256);      // (no more tiles than pixels: below 2^31)
    if (a.n == 0u || a.n > fuse) return hipErrorInvalidValue;
    if (fuse == 2u) hipLaunchKernelGGL((k_srad<2>), grid, blk, 0, st, a);
    else if (fuse == 4u) hipLaunchKernelGGL((k_srad<4>), grid, blk, 0, st, a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace mcrt
