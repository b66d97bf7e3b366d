// mcrt_voxels.h -- the voxel block of the 3-D stages, stated once: where a sample of a tracked stack lands and how a wavefront finds its runs
// and counts its statistics (k_recon_splat, k_recon_label_splat), the resolve tile with its staged halo and its launch (k_recon_resolve,
// k_recon_label_resolve; mcrt_image.cpp's limit check), the 8 x 8 picture tile and a pixel's base point (k_render, k_render_label), the
// nearest voxel of a point (k_render_label).  These are CONTRACTS (include/mcrt.h): the label volume registers with the float volume, and
// k_render_label lands on the point k_render sampled, because both sides run these lines.  Float expressions keep the contract's order,
// one rounding per operation.
#pragma once
#include "mcrt_device.h"

namespace mcrt {

// Sample g of the stack [F][E][R], row r = g % R of (frame, scan-line) g / R: t = r row_u, P = pos + dir t, x_c = ((b_c + P_x A_c0) +
// P_y A_c1) + P_z A_c2, i_c = floorf(x_c + 0.5f), inside when 0 <= i_c < n_c in float (a NaN compares false).  The voxel's index in
// [nw][nv][nu] (nu * nv * nw < 2^31), or -1 outside the block.
MCRT_DEV int sample_voxel(const ReconBlock &k, uint32_t g)
{
    const uint32_t line = g / k.R, r = g - line * k.R;
    const float *p = k.pos + 3u * (size_t)line, *d = k.dir + 3u * (size_t)line;
    const float t = (float)r * k.row_u;
    const float Px = p[0] + d[0] * t, Py = p[1] + d[1] * t, Pz = p[2] + d[2] * t;
    const float iu = floorf((((k.b[0] + Px * k.A[0]) + Py * k.A[1]) + Pz * k.A[2]) + 0.5f);
    const float iv = floorf((((k.b[1] + Px * k.A[3]) + Py * k.A[4]) + Pz * k.A[5]) + 0.5f);
    const float iw = floorf((((k.b[2] + Px * k.A[6]) + Py * k.A[7]) + Pz * k.A[8]) + 0.5f);
    const bool inside = iu >= 0.0f && iu < (float)k.nu && iv >= 0.0f && iv < (float)k.nv && iw >= 0.0f && iw < (float)k.nw;
    return inside ? (int)(((uint32_t)iw * k.nv + (uint32_t)iv) * k.nu + (uint32_t)iu) : -1;
}

// A wavefront's runs of equal keys: a lane is a run's head when its key differs from the lane's before it, the run's start is the last head
// at or below the lane, and the run's LAST lane (which issues the run's atomics, with lane - start + 1 as the length) stands before the next head.
struct WaveRuns { uint32_t start; bool last, all_heads; };          // all_heads: every lane is a run of its own
MCRT_DEV WaveRuns wave_runs(int key, uint32_t lane)
{
    const int before = __shfl_up(key, 1, 64);
    const unsigned long long heads = __ballot(lane == 0u || before != key);
    const uint32_t start = 63u - (uint32_t)__clzll((long long)(heads & (~0ull >> (63u - lane))));    // (bit 0 is always set)
    return WaveRuns{ start, lane == 63u || ((heads >> (lane + 1u)) & 1ull) != 0ull, heads == ~0ull };
}
// the two statistics of a splat, one atomic per wavefront each: lanes outside the block, lanes inside it that bin nothing
MCRT_DEV void wave_stats(uint32_t *stats, uint32_t lane, bool outside, bool rejected)
{
    if (!stats) return;
    const uint32_t n_out = (uint32_t)__popcll(__ballot(outside)), n_bad = (uint32_t)__popcll(__ballot(rejected));
    if (lane == 0u) { if (n_out) atomicAdd(&stats[0], n_out); if (n_bad) atomicAdd(&stats[1], n_bad); }
}

// The resolve tile: a workgroup of 256 lanes owns RECON_TW x RECON_TV x RECON_TU voxels and stages them with a halo of H = fill_radius on
// every side, [RW][RV][RU].  recon_tiling: the tiles along the axes and the staged cells of one; false for a radius or a grid that
// mcrt_recon_frames and mcrt_recon_label_frames refuse before anything is enqueued (recon_limits).
struct ReconTiling { uint32_t tu, tv, tw, cells; };
inline bool recon_tiling(uint32_t nu, uint32_t nv, uint32_t nw, uint32_t fill_radius, ReconTiling &t)
{
    const uint32_t H2 = 2u * fill_radius;
    t = ReconTiling{ (nu + RECON_TU - 1u) / RECON_TU, (nv + RECON_TV - 1u) / RECON_TV, (nw + RECON_TW - 1u) / RECON_TW, (RECON_TU + H2) * (RECON_TV + H2) * (RECON_TW + H2) };
    return fill_radius <= RECON_MAX_FILL && (uint64_t)t.tu * t.tv * t.tw < RECON_MAX_TILES;
}
// the launch of a resolve kernel over a's block, cell_bytes of LDS per staged cell
template <class Args> hipError_t launch_resolve(void (*kernel)(Args), Args a, uint32_t cell_bytes, hipStream_t st)
{
    ReconTiling t;
    if (!recon_tiling(a.blk.nu, a.blk.nv, a.blk.nw, a.blk.fill_radius, t)) return hipErrorInvalidValue;
    a.blk.tu = t.tu; a.blk.tv = t.tv;
    hipLaunchKernelGGL(kernel, dim3(t.tu * t.tv * t.tw), dim3(256), cell_bytes * t.cells, st, a);
    return hipGetLastError();
}
struct VoxelTile { int H, RU, RV, RW, u0, v0, w0, nu, nv, nw; };    // (u0, v0, w0): the tile's first voxel
MCRT_DEV VoxelTile voxel_tile(const ReconBlock &k)
{
    const int H = (int)k.fill_radius;
    const uint32_t bu = blockIdx.x % k.tu, bv = (blockIdx.x / k.tu) % k.tv, bw = blockIdx.x / (k.tu * k.tv);
    return VoxelTile{ H, RECON_TU + 2 * H, RECON_TV + 2 * H, RECON_TW + 2 * H, (int)bu * RECON_TU, (int)bv * RECON_TV, (int)bw * RECON_TW, (int)k.nu, (int)k.nv, (int)k.nw };
}
// staged cell idx < RU * RV * RW -> its voxel (Index: uint32_t or size_t, as the kernel goes on to use it; nu * nv * nw < 2^31); false: a point outside the
// block.  own: a voxel of the tile itself (no other workgroup writes it)
template <class Index> MCRT_DEV bool staged_voxel(const VoxelTile &t, int idx, Index &vox, bool &own)
{
    const int lu = idx % t.RU, lv = (idx / t.RU) % t.RV, lw = idx / (t.RU * t.RV);
    const int gu = t.u0 - t.H + lu, gv = t.v0 - t.H + lv, gw = t.w0 - t.H + lw;
    own = lu >= t.H && lu < t.H + RECON_TU && lv >= t.H && lv < t.H + RECON_TV && lw >= t.H && lw < t.H + RECON_TW;
    vox = ((Index)gw * (Index)t.nv + (Index)gv) * (Index)t.nu + (Index)gu;
    return gu >= 0 && gu < t.nu && gv >= 0 && gv < t.nv && gw >= 0 && gw < t.nw;
}
// the tile's own voxel idx < RECON_TU * RECON_TV * RECON_TW -> its voxel and its staged cell li; false: past the block's end
template <class Index> MCRT_DEV bool tile_voxel(const VoxelTile &t, int idx, Index &vox, int &li)
{
    const int tu = idx % RECON_TU, tv = (idx / RECON_TU) % RECON_TV, tw = idx / (RECON_TU * RECON_TV);
    const int gu = t.u0 + tu, gv = t.v0 + tv, gw = t.w0 + tw;
    vox = ((Index)gw * (Index)t.nv + (Index)gv) * (Index)t.nu + (Index)gu;
    li = ((tw + t.H) * t.RV + (tv + t.H)) * t.RU + (tu + t.H);
    return gu < t.nu && gv < t.nv && gw < t.nw;
}
// visit(cell) over the cube of h <= H voxels around staged cell li, w outermost and u innermost (inside the staged halo)
template <typename Visit> MCRT_DEV void cube_walk(const VoxelTile &t, int li, int h, Visit visit)
{
    for (int dw = -h; dw <= h; dw++)
        for (int dv = -h; dv <= h; dv++)
            for (int du = -h; du <= h; du++) visit(li + (dw * t.RV + dv) * t.RU + du);
}

// The picture tile: one lane per pixel, 8 x 8 pixels per wavefront, four wavefronts per workgroup (why: mcrt_render.hip).  The lane's pixel
// (i, j) may lie outside the picture.
inline uint32_t picture_tile_waves(uint32_t nx, uint32_t ny) { return ((nx + 7u) / 8u) * ((ny + 7u) / 8u); }   // (nx * ny < 2^31: no overflow)
MCRT_DEV void picture_tile(const ViewArgs &v, uint32_t &i, uint32_t &j)
{
    const uint32_t lane = threadIdx.x & 63u, wave = blockIdx.x * 4u + (threadIdx.x >> 6), tx = (v.nx + 7u) / 8u;
    i = (wave % tx) * 8u + (lane & 7u); j = (wave / tx) * 8u + (lane >> 3);
}
// pixel (i, j)'s base point b_c = (origin_c + i di_c) + j dj_c; step s of its ray is b_c + s ds_c: the contract's expression, no running sum
MCRT_DEV void pixel_base(const ViewArgs &v, uint32_t i, uint32_t j, float (&b)[3])
{
    const float fi = (float)i, fj = (float)j;
#pragma unroll
    for (int c = 0; c < 3; c++) b[c] = (v.origin[c] + fi * v.di[c]) + fj * v.dj[c];
}
// the nearest voxel of a point, the rule of the label gathers: k_c = f + (p_c - f >= 0.5f), f = floorf(p_c); false outside the block (a NaN
// too).  The index is made only where it is inside: 0 <= k < n < 2^24 holds in float and (uint32_t)k is exact.
MCRT_DEV bool nearest_voxel(const ViewArgs &v, float pu, float pv, float pw, size_t &vox)
{
    const float fu = floorf(pu), fv = floorf(pv), fw = floorf(pw);
    const float ku = fu + (pu - fu >= 0.5f ? 1.0f : 0.0f), kv = fv + (pv - fv >= 0.5f ? 1.0f : 0.0f), kw = fw + (pw - fw >= 0.5f ? 1.0f : 0.0f);
    const bool inside = ku >= 0.0f && ku < (float)v.nu && kv >= 0.0f && kv < (float)v.nv && kw >= 0.0f && kw < (float)v.nw;
    vox = inside ? ((size_t)(uint32_t)kw * v.nv + (uint32_t)kv) * v.nu + (uint32_t)ku : 0u;
    return inside;
}

}  // namespace mcrt
