// mcrt_volume.hip -- volume imaging (mcrt_volume_frames, mcrt_bmode_volume_frames; contract in include/mcrt.h): k_volume, the K tilted planes
// of every frame of a swept probe gathered through three maps (plane, column, row) into the points of a grid -- Cartesian voxels, or the
// pixels of any cut.  A trilinear scan conversion; the reference has one plane and no counterpart.
#include "mcrt_pixels.h"

namespace mcrt {

// out[f][p] = v0 * (1 - az) + v1 * az, v0 and v1 the bilinear blends -- remap_point / remap_taps / remap_blend, the one statement of the scan
// conversion -- of the planes floor(map_plane) and the next of frame f at the point the column and row maps give for p; a plane outside the
// sweep counts 0 and is not read (its taps are asked for in an image of no scan-lines).  One rounding per operation.  OUT8 = false writes
// that float from the RF stack (mcrt_volume_frames); OUT8 = true takes the grey levels of k_bmode_grey, quantises as k_bmode does and stores
// one 32-bit word per frame and lane (mcrt_bmode_volume_frames).
// The layout, the frame chunks and the stores are the pixel tile's (mcrt_pixels.h): the 64 lanes of a gather ask for 64 NEIGHBOURING points
// along u.  Neighbouring points are a fraction of a scan-line apart and every scan-line is a cache line of its own (R x 4 bytes), and here a
// point has 8 taps in 8 different lines: with 4 consecutive points per lane an instruction would reach four times as far along u.  A lane
// reads its 3 x 4 map values once, makes its four points and plane fractions once, and walks the frames of its chunk: per frame 32 gathers
// in flight, nothing else from memory.  (A padded point reads plane 0.)  No LDS, no scratch.
template <bool OUT8>
__global__ void __launch_bounds__(256) k_volume(VolumeArgs a)
{
    PixelTile tile;
    if (!pixel_tile(a.pass, tile)) return;
    const uint32_t n = a.pass.n, E = a.E, R = a.R, K = a.K;
    const size_t plane = (size_t)E * R;
    const float *mz = a.maps + tile.p0, *mc = mz + a.pass.n_pad, *mr = mc + a.pass.n_pad;
    RemapPoint pt[4];
    float az[4];
    uint32_t z[4];                                                            // the first plane read, 0 when neither is
    uint32_t E0[4], E1[4];                                                    // scan-lines of the planes z0 and z0 + 1: E inside the sweep, else 0 (no tap is read)
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const float pz = mz[64 * j], mx = mc[64 * j], my = mr[64 * j];
        pt[j] = remap_point(mx, my);
        const float fz = floorf(pz);
        az[j] = pz - fz;
        const bool mapped = (pz == pz) && (mx == mx) && (my == my);
        const bool in0 = mapped && fz >= 0.0f && fz < (float)K;               // 0 <= z0 < K (K <= 256: exact in float)
        const bool in1 = mapped && fz >= -1.0f && fz < (float)K - 1.0f;       // 0 <= z0 + 1 < K
        E0[j] = in0 ? E : 0u; E1[j] = in1 ? E : 0u;
        z[j] = in0 ? (uint32_t)fz : 0u;                                       // (in1 alone: z0 = -1, plane z0 + 1 = 0 = z + 0 -- see o1 below)
    }
    for (uint32_t f = tile.f0; f < tile.f1; f++) {
        const float *img = a.src + (size_t)f * K * plane;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const float *g0 = img + (size_t)z[j] * plane;
            const float *g1 = E0[j] ? g0 + plane : g0;                        // plane z0 + 1: the next one, or plane 0 when z0 = -1
            float t0[2][2], t1[2][2];
            remap_taps(pt[j], E0[j], R, [=](long long x, long long yy) { return g0[(size_t)x * R + (size_t)yy]; }, t0);
            remap_taps(pt[j], E1[j], R, [=](long long x, long long yy) { return g1[(size_t)x * R + (size_t)yy]; }, t1);
            const float v0 = remap_blend(pt[j], t0), v1 = remap_blend(pt[j], t1);
            v[j] = v0 * (1.0f - az[j]) + v1 * az[j];
        }
        if (OUT8) tile_store_u8((uint8_t *)a.out + (size_t)f * n, tile, n, quantise4(v), a.pass.vec != 0u);
        else tile_store_f32((float *)a.out + (size_t)f * n, tile, n, v);
    }
}

hipError_t launch_volume(const VolumeArgs &a, bool out8, hipStream_t st)
{
    const dim3 grid = pixel_grid(a.pass), blk(256);
    if (out8) hipLaunchKernelGGL((k_volume<true>), grid, blk, 0, st, a);
    else hipLaunchKernelGGL((k_volume<false>), grid, blk, 0, st, a);
    return hipGetLastError();
}

}  // namespace mcrt
