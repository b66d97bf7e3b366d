// mcrt_mmode.hip -- M-mode (mcrt_mmode_lines_frames, mcrt_mmode_picture_frames; contracts in include/mcrt.h): k_mmode_lines moves one
// scan-line's tissue over slow time and reads every pulse's analytic line out of the one traced line; k_mmode_peak takes the column
// means and each line's largest one; k_mmode_picture compresses a column to grey levels and resamples it in depth.  The reference has no
// counterpart.
#include "mcrt_device.h"
#include "mcrt_warp.h"              // warp_read: the reading of a line at a sub-row displacement, shared with mcrt_strain.hip and mcrt_shear.hip

namespace mcrt {

#define MMODE_ENV 1u
#define MMODE_IQ 2u
#define MMODE_DISP 4u
#define MMODE_LABEL 8u

// the dynamic LDS of k_mmode_lines, every part on a 16-byte boundary: D [R] (int64), the pre pairs [R], the four waves' partial sums,
// the labels [R] -- 16 KB + 16 KB + 64 B + 2 KB at R = 2048, so four workgroups share a CU's 160 KB and the launch sizes it by R
__host__ __device__ inline uint32_t mmode_rows_padded(uint32_t R) { return (R + 1u) & ~1u; }
static size_t mmode_lines_lds(uint32_t R) { return (size_t)16u * mmode_rows_padded(R) + 64u + ((R + 15u) & ~15u); }

// ONE workgroup of four wavefronts owns one M-line and MMODE_PULSE_CHUNK consecutive pulses.  It stages the line's pairs and labels in
// LDS, because pulse t's row q reads the rows q + (U >> 24) and the next one, wherever that pulse's displacement sends them, and builds
// D, the running sum of the rows' dilations, once: per tile of 256 rows a lane looks its row's dilation up by its label, six shuffle
// steps give the inclusive sum within a wavefront, the wavefronts' totals meet in LDS and the tile's total is carried on -- integers, so
// the order of the sum is free.  Then the pulses, the lanes across the rows: w_q16[t] and bulk_q24[t] are uniform, the displacement is
// two integer operations and a clamp, and every store runs along R (4 bytes a lane, 8 for the pairs, 1 for the labels).  The outputs
// are the instantiation (M: a mask of MMODE_*): one that is not asked for costs nothing, and the truths alone read no line and draw no
// noise.  Every float operation is the contract's, rounded once (compiled -ffp-contract=off).
template <uint32_t M>
__global__ void __launch_bounds__(MMODE_THREADS) k_mmode_lines(MmodeLinesArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char mmode_smem[];
    const uint32_t R = a.R, Rp = mmode_rows_padded(R);
    long long *D = (long long *)mmode_smem;
    float2 *pre = (float2 *)(mmode_smem + (size_t)8u * Rp);
    long long *part = (long long *)(mmode_smem + (size_t)16u * Rp);
    uint8_t *lab = mmode_smem + (size_t)16u * Rp + 64u;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t j = blockIdx.x / a.chunks, chunk = blockIdx.x - j * a.chunks;
    const uint32_t image = a.lines[2u * j], e = a.lines[2u * j + 1u];
    const size_t from = ((size_t)image * a.E + e) * R;
    const float2 *src = a.iq + from;
    const uint8_t *tissue = a.tissue + from;
    if (M & (MMODE_ENV | MMODE_IQ))
        for (uint32_t q = tid; q < R; q += MMODE_THREADS) pre[q] = src[q];
    long long carry = 0;
    for (uint32_t q0 = 0; q0 < R; q0 += MMODE_THREADS) {
        const uint32_t q = q0 + tid;
        const bool in = q < R;
        const uint32_t l = in ? tissue[q] : 255u;
        if (in) lab[q] = (uint8_t)l;
        const long long d = l < a.n_labels ? (long long)a.dil[l] : 0ll;
        long long incl = d;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const long long up = __shfl_up(incl, s);
            if ((int)lane >= s) incl += up;
        }
        if (lane == 63u) part[wave] = incl;
        __syncthreads();
        long long before = carry;
        for (uint32_t w = 0; w < wave; w++) before += part[w];
        if (in) D[q] = before + (incl - d);
        carry += (part[0] + part[1]) + (part[2] + part[3]);
        __syncthreads();                                    // (the partial sums are rewritten by the next tile)
    }
    const float sigma = a.sigma_dev ? a.sigma_dev[image] : a.sigma;
    const float k = sigma * a.inv_std;
    const long long carrier = a.carrier_q32;
    const uint32_t t0 = chunk * MMODE_PULSE_CHUNK, t1 = min(a.T, t0 + MMODE_PULSE_CHUNK);
    for (uint32_t t = t0; t < t1; t++) {
        const long long w = (long long)a.w[t], bulk = (long long)a.bulk[t];
        const size_t row = ((size_t)j * a.T + t) * R;
        for (uint32_t q = tid; q < R; q += MMODE_THREADS) {
            long long u = ((D[q] * w) >> 16) + bulk;
            u = u < -(127ll << 24) ? -(127ll << 24) : u > (127ll << 24) ? (127ll << 24) : u;
            const int32_t U = (int32_t)u;
            if (M & MMODE_DISP) a.truth_disp[row + q] = (float)U * 0x1p-24f;
            if (M & MMODE_LABEL) {
                const int32_t sr = ((int32_t)q + (U >> 24)) + ((U & 0xFFFFFF) >> 23);      // warp_read's s0 and fr: the nearer of its two samples
                a.truth_label[row + q] = sr >= 0 && sr < (int32_t)R ? lab[sr] : (uint8_t)255u;
            }
            if (M & (MMODE_ENV | MMODE_IQ)) {
                const float2 x = warp_read(pre, 0, (int32_t)R, (int32_t)q, U, carrier, a.lut);
                float xr = x.x, xi = x.y;
                if (k != 0.0f) {
                    uint32_t o[4];
                    philox4x32_10(e, q, 0x4D4D4F44u, t, a.seed, a.first_id + image, o);
                    int32_t di, dq;
                    irwin_hall(o, di, dq);
                    xr = xr + k * (float)di; xi = xi + k * (float)dq;
                }
                if (M & MMODE_IQ) a.iq_out[row + q] = make_float2(xr, xi);
                if (M & MMODE_ENV) {
                    const float rr = xr * xr, ii = xi * xi;
                    a.env[row + q] = sqrtf(rr + ii);
                }
            }
        }
    }
}

// one workgroup per (M-line, chunk of pulses): n_lines <= 65535 and T <= 16384, so the grid stays below 2^31
hipError_t launch_mmode_lines(const MmodeLinesArgs &a, hipStream_t st)
{
    if (a.n_lines == 0u || a.chunks == 0u || a.R == 0u || a.R > MCRT_MAX_ROWS) return hipErrorInvalidValue;
    const uint32_t m = (a.env ? MMODE_ENV : 0u) | (a.iq_out ? MMODE_IQ : 0u) | (a.truth_disp ? MMODE_DISP : 0u) | (a.truth_label ? MMODE_LABEL : 0u);
    const dim3 grid(a.n_lines * a.chunks);
    const size_t lds = mmode_lines_lds(a.R);
    switch (m) {
#define MMODE_CASE(M) case M: hipLaunchKernelGGL(k_mmode_lines<M>, grid, dim3(MMODE_THREADS), lds, st, a); break;
    MMODE_CASE(1) MMODE_CASE(2) MMODE_CASE(3) MMODE_CASE(4) MMODE_CASE(5) MMODE_CASE(6) MMODE_CASE(7) MMODE_CASE(8)
    MMODE_CASE(9) MMODE_CASE(10) MMODE_CASE(11) MMODE_CASE(12) MMODE_CASE(13) MMODE_CASE(14) MMODE_CASE(15)
#undef MMODE_CASE
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// whether a column mean counts in the display: finite and > 0 (a NaN, an infinity, a zero and anything negative count as 0)
MCRT_DEV bool mmode_counts(float v) { return v > 0.0f && __float_as_uint(v) < 0x7f800000u; }

// a[c][r] of one line: the mean of the column's hop pulses at row r, ascending from 0.0f (lanes across r: the reads are coalesced)
MCRT_DEV float mmode_mean(const float *env_line, uint32_t R, uint32_t hop, uint32_t c, uint32_t r)
{
    const float *p = env_line + (size_t)c * hop * R + r;
    float s = 0.0f;
    for (uint32_t k = 0; k < hop; k++) s = s + p[(size_t)k * R];
    return s / (float)hop;
}

// The column means and each line's largest one over the shown rows: positive floats order as their bit patterns do, so the maximum is
// an integer maximum -- exact and independent of the order -- taken per lane, across the wavefront and then by one atomic per wavefront
// into peak[j] (zeroed before), as k_sonogram_peak takes its.  With a mean_dev every row of the line is visited and written, otherwise
// the shown rows alone.
__global__ void __launch_bounds__(256) k_mmode_peak(MmodePictureArgs a)
{
    const uint32_t j = blockIdx.y;
    const uint32_t lo = a.mean ? 0u : a.row_lo, hi = a.mean ? a.R : a.row_hi, nr = hi - lo, per = a.W * nr;
    const float *env_line = a.env + (size_t)j * a.T * a.R;
    uint32_t m = 0u;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < per; i += gridDim.x * 256u) {
        const uint32_t c = i / nr, r = lo + (i - c * nr);
        const float v = mmode_mean(env_line, a.R, a.hop, c, r);
        if (a.mean) a.mean[((size_t)j * a.W + c) * a.R + r] = v;
        if (r >= a.row_lo && r < a.row_hi && mmode_counts(v)) m = max(m, __float_as_uint(v));
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) m = max(m, (uint32_t)__shfl_xor((int)m, d));
    if (a.peak && (threadIdx.x & 63u) == 0u && m != 0u) atomicMax((unsigned int *)(a.peak + j), m);
}

// W * R < 2^31 / n_lines (the entry point's limit), so `per` fits
hipError_t launch_mmode_peak(const MmodePictureArgs &a, hipStream_t st)
{
    const uint32_t nr = a.mean ? a.R : a.row_hi - a.row_lo, blocks = (a.W * nr + 255u) / 256u;
    hipLaunchKernelGGL(k_mmode_peak, dim3(blocks < 256u ? blocks : 256u, a.n_lines), dim3(256), 0, st, a);
    return hipGetLastError();
}

// One workgroup per (line, column): it takes the column's means again (the same sums: the same bits), holds the grey levels g[c][.] of
// the shown rows in LDS (8 KB at the most) and writes the column's H bytes and the truths registered with them.  The picture is the
// lines transposed, so a column's bytes are W apart: the stores of a wavefront are 64 single bytes, which the L2 merges with the
// neighbouring columns' (the picture is small beside the env stack the call reads).
__global__ void __launch_bounds__(256) k_mmode_picture(MmodePictureArgs a)
{
    __shared__ float g[MCRT_MAX_ROWS];
    const uint32_t c = blockIdx.x, j = blockIdx.y, nr = a.row_hi - a.row_lo;
    const float *env_line = a.env + (size_t)j * a.T * a.R;
    const float ref = a.peak ? a.peak[j] : a.ref;
    for (uint32_t i = threadIdx.x; i < nr; i += 256u) {
        const float v = mmode_mean(env_line, a.R, a.hop, c, a.row_lo + i);
        float x = 0.0f;
        if (mmode_counts(v)) {
            x = ((20.0f * log10f(v / ref) + a.gain) + a.dr) / a.dr;
            x = x < 0.0f ? 0.0f : x; x = x > 1.0f ? 1.0f : x;
        }
        g[i] = x;
    }
    __syncthreads();
    const size_t first = ((size_t)j * a.T + (size_t)c * a.hop) * a.R;         // pulse c * hop of this line
    for (uint32_t y = threadIdx.x; y < a.H; y += 256u) {
        const uint32_t i0 = a.idx[y], i1 = min(i0 + 1u, a.row_hi - 1u);
        const float wt = a.wt[y];
        const float v = (1.0f - wt) * g[i0 - a.row_lo] + wt * g[i1 - a.row_lo];
        const size_t at = ((size_t)j * a.H + y) * a.W + c;
        a.out[at] = (uint8_t)(v * 255.0f + 0.5f);
        const uint32_t rn = min(i0 + (wt >= 0.5f ? 1u : 0u), a.row_hi - 1u);
        if (a.label_out) a.label_out[at] = a.truth_label[first + rn];
        if (a.disp_out) a.disp_out[at] = a.truth_disp[first + rn];
    }
}

hipError_t launch_mmode_picture(const MmodePictureArgs &a, hipStream_t st)
{
    if (a.W == 0u || a.n_lines == 0u || a.n_lines > 65535u || a.row_hi <= a.row_lo || a.row_hi - a.row_lo > MCRT_MAX_ROWS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_mmode_picture, dim3(a.W, a.n_lines), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace mcrt
