// mcrt_recon.hip -- freehand 3-D reconstruction (mcrt_recon_frames; contract in include/mcrt.h): k_recon_splat bins every sample of a tracked
// stack [F][E][R] into the voxel its pose puts it in, k_recon_resolve turns the accumulators into voxels and fills the holes.  The
// reference has no counterpart.
#include "mcrt_voxels.h"

namespace mcrt {

constexpr unsigned long long RECON_BIAS = 0x8000000000000000ull;   // MAX mode keeps q + 2^63 as an unsigned word: a cleared word is below every q

// A lane owns one sample; consecutive lanes own consecutive rows of a scan-line (a wavefront may run over a scan-line's end into the
// next one: nothing below asks for a scan-line).  The voxel is sample_voxel's (mcrt_voxels.h).  At a voxel of a few row pitches
// neighbouring rows land in the same voxel, and atomics on one address serialise in L2, so the runs of equal voxels inside a wavefront
// are combined first (wave_runs): a segmented inclusive scan adds (MEAN) or maximises (MAX) q from the run's start, and the run's LAST
// lane issues one atomic pair with the run's length as the count.  A wavefront in which every lane is a head skips the scan.  Lanes that
// bin nothing (outside the block, an unusable value, past the stack's end) carry voxel -1: they break runs, and a run of them issues
// nothing.  Integer sums and maxima commute and associate: the combining changes no bit.
template <bool MAXMODE>
__global__ void __launch_bounds__(256) k_recon_splat(ReconArgs a)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    int vox = -1;
    long long q = 0;
    bool outside = false, unusable = false;
    if (g < a.blk.n_samples) {
        const int at = sample_voxel(a.blk, g);
        const float v = a.stack[g];
        const bool inside = at >= 0, usable = fabsf(v) < a.value_max;       // (value_max is finite: a NaN or an infinity is not below it)
        outside = !inside; unusable = inside && !usable;
        if (inside && usable) { vox = at; q = (long long)((double)v * a.qscale); }
    }
    wave_stats(a.blk.stats, lane, outside, unusable);
    const WaveRuns run = wave_runs(vox, lane);
    if (!run.all_heads)
        for (uint32_t d = 1u; d < 64u; d <<= 1) {
            const long long o = __shfl_up(q, d, 64);
            if (lane >= run.start + d) q = MAXMODE ? (o > q ? o : q) : q + o;
        }
    if (run.last && vox >= 0) {
        atomicAdd(&a.count[vox], lane - run.start + 1u);
        if (MAXMODE) atomicMax(&a.sum[vox], (unsigned long long)q ^ RECON_BIAS);
        else atomicAdd(&a.sum[vox], (unsigned long long)q);
    }
}

// A workgroup of 256 lanes owns a tile of RECON_TW x RECON_TV x RECON_TU voxels.  It stages the RESOLVED value and a sampled flag of the
// tile and a halo of H = fill_radius voxels on every side in LDS, straight from the accumulators (a point outside the block: not
// sampled); the resolved block never goes through memory on its own.  A sampled voxel is its staged value.  A hole looks through the
// cubes of h = 1..H around it in LDS, w outermost and u innermost, and reads only sampled voxels -- never a filled one, so neither the
// tiling nor any order shows in the bits.  LDS is sized by the call's H at launch: (8 + 2H)(8 + 2H)(32 + 2H) floats, then as many bytes --
// 10 KB at H = 0, 16.6 KB at the default H = 1, 36.4 KB at H = 3.
__device__ __forceinline__ float recon_value(unsigned long long s, uint32_t n, uint32_t mode, double qscale)
{
    return mode == MCRT_RECON_MAX ? (float)((double)(long long)(s ^ RECON_BIAS) / qscale) : (float)((double)(long long)s / ((double)n * qscale));
}

__global__ void __launch_bounds__(256) k_recon_resolve(ReconArgs a)
{
    extern __shared__ float sval[];                                 // [RW][RV][RU] resolved values, then as many flags (launch_recon_resolve sizes them)
    const VoxelTile t = voxel_tile(a.blk);
    const int cells = t.RU * t.RV * t.RW;
    unsigned char *sflag = (unsigned char *)(sval + cells);

    for (int idx = threadIdx.x; idx < cells; idx += 256) {
        size_t vox;
        bool own;
        float val = 0.0f;
        unsigned char flag = 0;
        if (staged_voxel(t, idx, vox, own)) {
            const uint32_t n = a.count[vox];
            if (n) { val = recon_value(a.sum[vox], n, a.mode, a.qscale); flag = 1; }
        }
        sval[idx] = val; sflag[idx] = flag;
    }
    __syncthreads();

    for (int idx = threadIdx.x; idx < RECON_TU * RECON_TV * RECON_TW; idx += 256) {
        size_t vox;
        int li;
        if (!tile_voxel(t, idx, vox, li)) continue;
        float value = a.empty;
        uint32_t n_here = 0u;
        if (sflag[li]) { value = sval[li]; if (a.count_out) n_here = a.count[vox]; }
        else
            for (int h = 1; h <= t.H; h++) {
                float s = 0.0f;
                uint32_t n = 0u;
                cube_walk(t, li, h, [&](int lj) { if (sflag[lj]) { s = s + sval[lj]; n++; } });
                if (n >= a.blk.fill_min) { value = s / (float)n; break; }
            }
        a.out[vox] = value;
        if (a.count_out) a.count_out[vox] = n_here;
    }
}

hipError_t launch_recon_splat(const ReconArgs &a, hipStream_t st)
{
    if (a.blk.n_samples == 0u || a.blk.n_samples >= 0x80000000u) return hipErrorInvalidValue;
    const dim3 grid((a.blk.n_samples + 255u) / 256u), blk(256);
    if (a.mode == MCRT_RECON_MAX) hipLaunchKernelGGL((k_recon_splat<true>), grid, blk, 0, st, a);
    else hipLaunchKernelGGL((k_recon_splat<false>), grid, blk, 0, st, a);
    return hipGetLastError();
}

hipError_t launch_recon_resolve(ReconArgs a, hipStream_t st) { return launch_resolve(k_recon_resolve, a, 5u, st); }   // (a float and a flag per staged cell)

}  // namespace mcrt
