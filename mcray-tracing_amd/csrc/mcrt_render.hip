// mcrt_render.hip -- volume rendering (mcrt_render_frames; contract in include/mcrt.h): k_render, a block of voxels [nw][nv][nu] seen from a
// direction -- one orthographic ray per pixel, n_steps trilinear samples along it, folded into the maximum, the mean or a front-to-back
// composited surface.  The reference has one plane and no counterpart.
#include "mcrt_pixels.h"
#include "mcrt_voxels.h"

namespace mcrt {

// one step of one ray: the 8 voxels around the sample point (t[du + 2 dv + 4 dw]; a voxel outside the block is 0.0f and is not read), the
// three fractions, and whether the step counts at all
struct RenderSample { float t[8]; float au, av, aw; bool covered; };

// p = b + (float)s * ds per component (b: the pixel's base point, pixel_base, so that p is the contract's expression and no running sum).
// The indices are made only where the step is covered: -1 <= f < n then holds in float, n < 2^24, and (int)f is exact.
template <bool IN8>
__device__ __forceinline__ RenderSample render_fetch(const ViewArgs &a, const void *blk, const float (&b)[3], uint32_t s)
{
    RenderSample r;
    const float fs = (float)s;
    const float pu = b[0] + fs * a.ds[0], pv = b[1] + fs * a.ds[1], pw = b[2] + fs * a.ds[2];
    const float fu = floorf(pu), fv = floorf(pv), fw = floorf(pw);
    r.au = pu - fu; r.av = pv - fv; r.aw = pw - fw;
    r.covered = pu == pu && pv == pv && pw == pw && fu >= -1.0f && fu < (float)a.nu && fv >= -1.0f && fv < (float)a.nv && fw >= -1.0f && fw < (float)a.nw;
    const int iu = r.covered ? (int)fu : 0, iv = r.covered ? (int)fv : 0, iw = r.covered ? (int)fw : 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const uint32_t u = (uint32_t)(iu + (k & 1)), v = (uint32_t)(iv + ((k >> 1) & 1)), w = (uint32_t)(iw + (k >> 2));   // (-1 wraps to 2^32 - 1: outside)
        float t = 0.0f;
        if (r.covered && u < a.nu && v < a.nv && w < a.nw) {
            const uint32_t idx = (w * a.nv + v) * a.nu + u;                   // (nu * nv * nw < 2^31)
            t = IN8 ? (float)((const uint8_t *)blk)[idx] : ((const float *)blk)[idx];
        }
        r.t[k] = t;
    }
    return r;
}

// One lane per pixel, one frame per blockIdx.y.  Which pixels a wavefront owns decides how far apart the 64 x 8 taps of one gather step lie in
// the block: an 8 x 8 tile of the picture (row_tile = 0, the default) keeps them inside a patch about 8 pixel pitches across for ANY view
// direction; 64 pixels of one picture row (row_tile = 1) are a line 64 pitches long, compact in memory only when di runs along u.  The next
// step's 8 taps are asked for before this step is blended (the last step asks for its own again: no branch); a step that is not covered
// reads nothing.  The exact per-step `covered` test decides every step: there is no per-ray clip.  IN8: the block is bytes (the voxels of
// mcrt_bmode_volume_frames), else floats (mcrt_volume_frames).  The mode is wave-uniform.  No LDS, no scratch.
template <bool IN8>
__global__ void __launch_bounds__(256) k_render(RenderArgs a)
{
    const ViewArgs &vw = a.view;
    uint32_t i, j;
    if (a.row_tile) { const uint32_t wave = blockIdx.x * 4u + (threadIdx.x >> 6), per_row = (vw.nx + 63u) / 64u; i = (wave % per_row) * 64u + (threadIdx.x & 63u); j = wave / per_row; }
    else picture_tile(vw, i, j);
    if (i >= vw.nx || j >= vw.ny) return;
    const uint32_t f = blockIdx.y, mode = a.mode, n_steps = vw.n_steps;
    const size_t nvox = (size_t)vw.nu * vw.nv * vw.nw;
    const void *blk = IN8 ? (const void *)((const uint8_t *)a.vol + (size_t)f * nvox) : (const void *)((const float *)a.vol + (size_t)f * nvox);
    float b[3];
    pixel_base(vw, i, j, b);
    float m = 0.0f, depth = -1.0f, sum = 0.0f, C = 0.0f, T = 1.0f;     // (depth is MIP's arg as well)
    uint32_t cnt = 0u;
    RenderSample cur = render_fetch<IN8>(vw, blk, b, 0u);
    for (uint32_t s = 0; s < n_steps; s++) {
        const RenderSample nxt = render_fetch<IN8>(vw, blk, b, min(s + 1u, n_steps - 1u));
        if (cur.covered) {
            const float wu = 1.0f - cur.au, wv = 1.0f - cur.av, ww = 1.0f - cur.aw;
            const float c00 = cur.t[0] * wu + cur.t[1] * cur.au, c01 = cur.t[2] * wu + cur.t[3] * cur.au;
            const float c10 = cur.t[4] * wu + cur.t[5] * cur.au, c11 = cur.t[6] * wu + cur.t[7] * cur.au;
            const float e0 = c00 * wv + c01 * cur.av, e1 = c10 * wv + c11 * cur.av;
            float v = e0 * ww + e1 * cur.aw;
            v = (v == v) ? v : 0.0f;
            const float x = fminf(fmaxf((v - a.lo) * a.inv_range, 0.0f), 1.0f);
            if (mode == MCRT_RENDER_MIP) {
                if (x > m) { m = x; depth = (float)s; }
            } else if (mode == MCRT_RENDER_MEAN) {
                sum = sum + x; cnt++;
            } else {
                const float al = fminf(fmaxf((x - a.threshold) * a.inv_ramp, 0.0f), 1.0f) * a.opacity;
                const float shade = 1.0f - a.depth_cue * ((float)s * a.inv_steps);
                C = C + (T * al) * (x * shade);
                T = T * (1.0f - al);
                if (depth < 0.0f && T <= 0.5f) depth = (float)s;
                if (T < a.t_cut) break;
            }
        }
        cur = nxt;
    }
    const float out = mode == MCRT_RENDER_MIP ? m : mode == MCRT_RENDER_MEAN ? (cnt ? sum / (float)cnt : 0.0f) : C;
    const size_t o = ((size_t)f * vw.ny + j) * vw.nx + i;
    if (a.out) a.out[o] = out;
    if (a.out8) a.out8[o] = quantise(fminf(fmaxf(out, 0.0f), 1.0f));
    if (a.depth) a.depth[o] = mode == MCRT_RENDER_MEAN ? -1.0f : depth;
}

hipError_t launch_render(const RenderArgs &a, bool in8, hipStream_t st)
{
    const uint32_t waves = a.row_tile ? ((a.view.nx + 63u) / 64u) * a.view.ny : picture_tile_waves(a.view.nx, a.view.ny);   // (nx * ny < 2^31: no overflow)
    const dim3 grid((waves + 3u) / 4u, a.view.F), blk(256);
    if (in8) hipLaunchKernelGGL((k_render<true>), grid, blk, 0, st, a);
    else hipLaunchKernelGGL((k_render<false>), grid, blk, 0, st, a);
    return hipGetLastError();
}

}  // namespace mcrt
