// mcrt_recon.hip -- freehand 3-D reconstruction (mcrt_recon_frames; contract in include/mcrt.h): k_recon_splat bins every sample of a tracked
// stack [F][E][R] into the voxel its pose puts it in, k_recon_resolve turns the accumulators into voxels and fills the holes.  The
// reference has no counterpart.
#include "mcrt_device.h"

namespace mcrt {

constexpr unsigned long long RECON_BIAS = 0x8000000000000000ull;   // MAX mode keeps q + 2^63 as an unsigned word: a cleared word is below every q

// A lane owns one sample; consecutive lanes own consecutive rows of a scan-line (a wavefront may run over a scan-line's end into the
// next one: nothing below asks for a scan-line).  The position is pos + dir * t and three dot products, the contract's expressions one
// by one.  At a voxel of a few row pitches neighbouring rows land in the same voxel, and atomics on one address serialise in L2, so the
// runs of equal voxels inside a wavefront are combined first: a lane is a run's head when its voxel differs from the lane's before it,
// the run's start is the last head at or below the lane, a segmented inclusive scan adds (MEAN) or maximises (MAX) q from the start, and
// the run's LAST lane issues one atomic pair with the run's length as the count.  A wavefront in which every lane is a head skips the
// scan.  Lanes that bin nothing (outside the block, an unusable value, past the stack's end) carry voxel -1: they break runs, and a run
// of them issues nothing.  Integer sums and maxima commute and associate: the combining changes no bit.  The two statistics are one
// atomic per wavefront each.
template <bool MAXMODE>
__global__ void __launch_bounds__(256) k_recon_splat(ReconArgs a)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    int vox = -1;
    long long q = 0;
    bool outside = false, unusable = false;
    if (g < a.n_samples) {
        const uint32_t line = g / a.R, r = g - line * a.R;
        const float *p = a.pos + 3u * (size_t)line, *d = a.dir + 3u * (size_t)line;
        const float t = (float)r * a.row_u;
        const float Px = p[0] + d[0] * t, Py = p[1] + d[1] * t, Pz = p[2] + d[2] * t;
        const float iu = floorf((((a.b[0] + Px * a.A[0]) + Py * a.A[1]) + Pz * a.A[2]) + 0.5f);
        const float iv = floorf((((a.b[1] + Px * a.A[3]) + Py * a.A[4]) + Pz * a.A[5]) + 0.5f);
        const float iw = floorf((((a.b[2] + Px * a.A[6]) + Py * a.A[7]) + Pz * a.A[8]) + 0.5f);
        const bool inside = iu >= 0.0f && iu < (float)a.nu && iv >= 0.0f && iv < (float)a.nv && iw >= 0.0f && iw < (float)a.nw;   // (a NaN compares false)
        const float v = a.stack[g];
        const bool usable = fabsf(v) < a.value_max;       // (value_max is finite: a NaN or an infinity is not below it)
        outside = !inside; unusable = inside && !usable;
        if (inside && usable) {
            vox = (int)(((uint32_t)iw * a.nv + (uint32_t)iv) * a.nu + (uint32_t)iu);     // (below nu * nv * nw < 2^31)
            q = (long long)((double)v * a.qscale);
        }
    }
    if (a.stats) {
        const uint32_t n_out = (uint32_t)__popcll(__ballot(outside)), n_bad = (uint32_t)__popcll(__ballot(unusable));
        if (lane == 0u) {
            if (n_out) atomicAdd(&a.stats[0], n_out);
            if (n_bad) atomicAdd(&a.stats[1], n_bad);
        }
    }
    const int before = __shfl_up(vox, 1, 64);
    const unsigned long long heads = __ballot(lane == 0u || before != vox);
    const uint32_t start = 63u - (uint32_t)__clzll((long long)(heads & (~0ull >> (63u - lane))));    // (bit 0 is always set)
    if (heads != ~0ull)
        for (uint32_t d = 1u; d < 64u; d <<= 1) {
            const long long o = __shfl_up(q, d, 64);
            if (lane >= start + d) q = MAXMODE ? (o > q ? o : q) : q + o;
        }
    const bool last = lane == 63u || ((heads >> (lane + 1u)) & 1ull);
    if (last && vox >= 0) {
        atomicAdd(&a.count[vox], lane - start + 1u);
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
    const int H = (int)a.fill_radius, RU = RECON_TU + 2 * H, RV = RECON_TV + 2 * H, RW = RECON_TW + 2 * H;
    unsigned char *sflag = (unsigned char *)(sval + RU * RV * RW);
    const int nu = (int)a.nu, nv = (int)a.nv, nw = (int)a.nw;
    const uint32_t bu = blockIdx.x % a.tu, bv = (blockIdx.x / a.tu) % a.tv, bw = blockIdx.x / (a.tu * a.tv);
    const int u0 = (int)bu * RECON_TU, v0 = (int)bv * RECON_TV, w0 = (int)bw * RECON_TW;        // the tile's first voxel

    for (int idx = threadIdx.x; idx < RU * RV * RW; idx += 256) {
        const int lu = idx % RU, lv = (idx / RU) % RV, lw = idx / (RU * RV);
        const int gu = u0 - H + lu, gv = v0 - H + lv, gw = w0 - H + lw;
        float val = 0.0f;
        unsigned char flag = 0;
        if (gu >= 0 && gu < nu && gv >= 0 && gv < nv && gw >= 0 && gw < nw) {
            const size_t vox = ((size_t)gw * a.nv + (size_t)gv) * a.nu + (size_t)gu;
            const uint32_t n = a.count[vox];
            if (n) { val = recon_value(a.sum[vox], n, a.mode, a.qscale); flag = 1; }
        }
        sval[idx] = val; sflag[idx] = flag;
    }
    __syncthreads();

    for (int idx = threadIdx.x; idx < RECON_TU * RECON_TV * RECON_TW; idx += 256) {
        const int tu = idx % RECON_TU, tv = (idx / RECON_TU) % RECON_TV, tw = idx / (RECON_TU * RECON_TV);
        const int gu = u0 + tu, gv = v0 + tv, gw = w0 + tw;
        if (gu >= nu || gv >= nv || gw >= nw) continue;
        const size_t vox = ((size_t)gw * a.nv + (size_t)gv) * a.nu + (size_t)gu;
        const int li = ((tw + H) * RV + (tv + H)) * RU + (tu + H);
        float value = a.empty;
        uint32_t n_here = 0u;
        if (sflag[li]) { value = sval[li]; if (a.count_out) n_here = a.count[vox]; }
        else
            for (int h = 1; h <= H; h++) {
                float s = 0.0f;
                uint32_t n = 0u;
                for (int dw = -h; dw <= h; dw++)
                    for (int dv = -h; dv <= h; dv++)
                        for (int du = -h; du <= h; du++) {
                            const int lj = li + (dw * RV + dv) * RU + du;         // (inside the staged halo: h <= H)
                            if (sflag[lj]) { s = s + sval[lj]; n++; }
                        }
                if (n >= a.fill_min) { value = s / (float)n; break; }
            }
        a.out[vox] = value;
        if (a.count_out) a.count_out[vox] = n_here;
    }
}

hipError_t launch_recon_splat(const ReconArgs &a, hipStream_t st)
{
    if (a.n_samples == 0u || a.n_samples >= 0x80000000u) return hipErrorInvalidValue;
    const dim3 grid((a.n_samples + 255u) / 256u), blk(256);
    if (a.mode == MCRT_RECON_MAX) hipLaunchKernelGGL((k_recon_splat<true>), grid, blk, 0, st, a);
    else hipLaunchKernelGGL((k_recon_splat<false>), grid, blk, 0, st, a);
    return hipGetLastError();
}

hipError_t launch_recon_resolve(ReconArgs a, hipStream_t st)
{
    if (a.fill_radius > RECON_MAX_FILL) return hipErrorInvalidValue;
    a.tu = (a.nu + RECON_TU - 1u) / RECON_TU; a.tv = (a.nv + RECON_TV - 1u) / RECON_TV;
    const uint32_t tw = (a.nw + RECON_TW - 1u) / RECON_TW;
    if ((uint64_t)a.tu * a.tv * tw >= RECON_MAX_TILES) return hipErrorInvalidValue;     // (mcrt_recon_frames refuses such a grid before anything is enqueued)
    const dim3 grid(a.tu * a.tv * tw), blk(256);
    const uint32_t H2 = 2u * a.fill_radius, cells = (RECON_TU + H2) * (RECON_TV + H2) * (RECON_TW + H2);
    hipLaunchKernelGGL(k_recon_resolve, grid, blk, 5u * cells, st, a);
    return hipGetLastError();
}

}  // namespace mcrt
