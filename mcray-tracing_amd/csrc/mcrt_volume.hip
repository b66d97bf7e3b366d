// mcrt_volume.hip -- volume imaging (mcrt_volume_frames, mcrt_bmode_volume_frames; contract in include/mcrt.h): k_volume, the K tilted planes
// of every frame of a swept probe gathered through three maps (plane, column, row) into the points of a grid -- Cartesian voxels, or the
// pixels of any cut.  A trilinear scan conversion; the reference has one plane and no counterpart.
#include "mcrt_device.h"

namespace mcrt {

// out[f][p] = v0 * (1 - az) + v1 * az, v0 and v1 the bilinear blends -- remap_point / remap_taps / remap_blend, the one statement of the scan
// conversion -- of the planes floor(map_plane) and the next of frame f at the point the column and row maps give for p; a plane outside the
// sweep counts 0 and is not read (its taps are asked for in an image of no scan-lines).  One rounding per operation.  OUT8 = false writes
// that float from the RF stack (mcrt_volume_frames); OUT8 = true takes the grey levels of k_bmode_grey, quantises as k_bmode does and stores
// one 32-bit word per frame and lane (mcrt_bmode_volume_frames).
// The layout is k_compound's (measured there: which points a lane owns decides the speed): a wavefront owns 256 consecutive
// points, a lane the four points wb + 64 j + lane, j = 0..3, so in every gather instruction the 64 lanes ask for 64 NEIGHBOURING points along
// u.  Neighbouring points are a fraction of a scan-line apart and every scan-line is a cache line of its own (R x 4 bytes), and here a point
// has 8 taps in 8 different lines: with 4 consecutive points per lane an instruction would reach four times as far along u.  A lane reads
// its 3 x 4 map values once, makes its four points and plane fractions once, and walks the frames [f0, f1) of its chunk (blockIdx.y): per
// frame 32 gathers in flight, nothing else from memory.  The maps are padded to a multiple of 256 points (zeros: the points past the grid's
// end read plane 0, tap (0, 0), which exists, and are not stored).  The float form stores 256 contiguous bytes per instruction as it is; the
// 8-bit form first turns the wavefront's 4 x 64 bytes round with four ds_bpermute, so that lane L holds the bytes of points wb + 4 L ..
// 4 L + 3 (a.vec: the grid's size and the output pointer keep the words aligned; a wavefront at the grid's end stores its bytes one by one).
// No LDS, no scratch.
template <bool OUT8>
__global__ void __launch_bounds__(256) k_volume(VolumeArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wb = blockIdx.x * 1024u + (threadIdx.x >> 6) * 256u;      // the wavefront's first point
    if (wb >= a.n) return;                                                    // (the whole wavefront)
    const uint32_t p0 = wb + lane, E = a.E, R = a.R, K = a.K;                 // the lane's points: p0 + 64 j
    const bool whole = wb + 256u <= a.n;
    const size_t plane = (size_t)E * R;
    const uint32_t f0 = blockIdx.y * a.frames_per_chunk, f1 = min(a.F, f0 + a.frames_per_chunk);
    const float *mz = a.maps + p0, *mc = mz + a.n_pad, *mr = mc + a.n_pad;    // (n_pad % 256 == 0: p0 + 192 < n_pad)
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
    for (uint32_t f = f0; f < f1; f++) {
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
        if (OUT8) {
            uint32_t bytes = 0u;                            // byte j: point p0 + 64 j
#pragma unroll
            for (int j = 0; j < 4; j++) bytes |= (uint32_t)(uint8_t)(v[j] * 255.0f + 0.5f) << (8 * j);
            uint8_t *o = (uint8_t *)a.out + (size_t)f * a.n;
            if (a.vec && whole) {                           // point wb + 4 L + i is byte L / 16 of lane (4 L + i) % 64: every lane is active here
                uint32_t word = 0u;
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const uint32_t got = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(((4u * lane + (uint32_t)i) & 63u) * 4u), (int)bytes);
                    word |= ((got >> (8u * (lane >> 4))) & 0xffu) << (8 * i);
                }
                *(uint32_t *)(o + wb + 4u * lane) = word;
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++) if (p0 + 64u * j < a.n) o[p0 + 64u * j] = (uint8_t)(bytes >> (8 * j));
            }
        } else {
            float *o = (float *)a.out + (size_t)f * a.n;
#pragma unroll
            for (int j = 0; j < 4; j++) if (p0 + 64u * j < a.n) o[p0 + 64u * j] = v[j];
        }
    }
}

hipError_t launch_volume(const VolumeArgs &a, bool out8, hipStream_t st)
{
    const uint32_t chunks = (a.F + a.frames_per_chunk - 1u) / a.frames_per_chunk;
    const dim3 grid((a.n + 1023u) / 1024u, chunks), blk(256);
    if (out8) hipLaunchKernelGGL((k_volume<true>), grid, blk, 0, st, a);
    else hipLaunchKernelGGL((k_volume<false>), grid, blk, 0, st, a);
    return hipGetLastError();
}

}  // namespace mcrt
