// mcrt_autogain.hip -- automatic gain (mcrt_autogain_frames; contract in include/mcrt.h): k_autogain_hist (the amplitude histograms of every
// frame's depth bands), k_autogain_curve (the floor, the bands' levels, the target, the gains of bands and rows, the penetration depth: what
// mcrt_autogain_curve does on the host, bit for bit) and k_autogain_apply (the multiply).  The reference has no counterpart.
#include "mcrt_device.h"

namespace mcrt {

// bin(a) of the contract: bits(|v|) >> 20 where v is finite, else 0
MCRT_DEV uint32_t autogain_bin(float v)
{
    const uint32_t bits = __float_as_uint(v) & 0x7fffffffu;
    return bits >= 0x7f800000u ? 0u : bits >> 20;
}

// Step 2.  A workgroup (256 lanes) histograms one (frame, band, run of scan-lines) in LDS and flushes its non-zero bins with one integer
// atomic each: the counts do not depend on any order.  The band's rows are contiguous within a scan-line, so consecutive lanes take
// consecutive rows and then the next scan-line: with 16-row bands a wavefront's load is whole 64-byte runs, four scan-lines (VEC: sixteen,
// a lane taking four rows as one 16-byte load, where the base, R and band_rows allow) at a time.
// Speckle of one band falls into a few dozen neighbouring bins, so many lanes of one LDS atomic meet on one address, and those are served
// one after the other.  COPIES interleaved histograms (bin * COPIES + lane % COPIES: the copies of a bin lie in neighbouring banks) divide
// the lanes that can meet by COPIES at 8 KiB of LDS each; the flush adds the copies up.  Measured, four copies lose to one,
// 17.6 against 10.1 us on 20 x 512 x 465: a workgroup reads 16 KiB, and clearing and flushing 32 KiB of LDS costs it more than the meetings
// do.  One is the default; both forms are built (MCRT_AUTOGAIN_COPIES).  Bin 0 -- the exact zeros that fill a traced frame below its
// last echo -- would put a whole wavefront on one address: a lane counts its zeros in a register and a wavefront adds them once.
template <bool VEC, uint32_t COPIES>
__global__ void __launch_bounds__(256) k_autogain_hist(AutogainArgs a)
{
    __shared__ uint32_t h[AUTOGAIN_BINS * COPIES];
    const uint32_t t = threadIdx.x, b = blockIdx.y, f = blockIdx.z;
    for (uint32_t i = t; i < AUTOGAIN_BINS * COPIES; i += 256u) h[i] = 0u;
    __syncthreads();
    const uint32_t R = a.R, r_lo = b * a.band_rows, nb = min(a.band_rows, R - r_lo);
    const uint32_t per = (a.lines + a.shares - 1u) / a.shares, l0 = blockIdx.x * per, l1 = min(a.lines, l0 + per);
    constexpr uint32_t U = VEC ? 4u : 1u;                       // rows of a lane's unit
    const uint32_t nu = nb / U;                                 // units of a scan-line's band: 1 .. 256 (VEC: nb % 4 == 0)
    const uint32_t dl = 256u / nu, du = 256u % nu;              // the workgroup's stride, in scan-lines and units
    uint32_t line = l0 + t / nu, u = t % nu, zeros = 0u;
    const float *base = a.rf + (size_t)f * a.lines * R + r_lo;
    const uint32_t copy = t & (COPIES - 1u);
    auto count = [&](float v) {
        const uint32_t bin = autogain_bin(v);
        if (bin) atomicAdd(&h[bin * COPIES + copy], 1u); else zeros++;
    };
    while (line < l1) {
        const float *p = base + (size_t)line * R + u * U;
        if (VEC) { const float4 q = *(const float4 *)p; count(q.x); count(q.y); count(q.z); count(q.w); }
        else count(*p);
        u += du; line += dl;
        if (u >= nu) { u -= nu; line++; }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) zeros += (uint32_t)__shfl_xor((int)zeros, d, 64);
    if ((t & 63u) == 0u && zeros) atomicAdd(&h[0], zeros);
    __syncthreads();
    uint32_t *g = a.hist + ((size_t)f * a.n_bands + b) * AUTOGAIN_BINS;
    for (uint32_t bin = t; bin < AUTOGAIN_BINS; bin += 256u) {
        uint32_t c = 0u;
#pragma unroll
        for (uint32_t k = 0; k < COPIES; k++) c += h[bin * COPIES + k];
        if (c) atomicAdd(&g[bin], c);
    }
}

MCRT_DEV float autogain_centre(int32_t bin) { return __uint_as_float(((uint32_t)bin << 20) | (1u << 19)); }

// Steps 3 to 8, one workgroup of 16 wavefronts per frame.  A wavefront takes a band at a time: its 2048 counts are eight 16-byte loads per
// lane (lane l reads the bins 256 j + 4 l .. + 3 of chunk j), the counts at or below the floor's bin are dropped, a sum over the wavefront is
// n_t, and the lower median is found from the chunks' sums and one prefix scan -- the chunk in which twice the cumulative count reaches n_t, the
// first lane of it, and that lane's four bins.  The target is found by rank-counting over the (at most 512) bands in LDS, a thread per band;
// the hold fill walks back to the nearest valid band; then a thread per row makes the row gains.  Integers decide; the float operations are
// the contract's (compiled -ffp-contract=off, the divisions correctly rounded).
__global__ void __launch_bounds__(1024) k_autogain_curve(AutogainArgs a)
{
    __shared__ int32_t m_s[AUTOGAIN_MAX_BANDS];
    __shared__ float k_s[AUTOGAIN_MAX_BANDS];
    __shared__ int32_t tgt_s, first_s, last_s;
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6, f = blockIdx.x, nB = a.n_bands, R = a.R;
    const float floor_f = a.floor_dev ? a.floor_dev[f] : a.floor;
    const float thr = floor_f * a.floor_scale;
    const uint32_t thr_bin = (isfinite(thr) && thr > 0.0f) ? __float_as_uint(thr) >> 20 : 0u;
    if (t == 0u) { tgt_s = -1; first_s = 0x7fffffff; last_s = -1; }
    for (uint32_t b = wave; b < nB; b += 16u) {
        const uint4 *hb = (const uint4 *)(a.hist + ((size_t)f * nB + b) * AUTOGAIN_BINS);
        // chunk j of the band's counts as lane l holds it, without the counts at or below the floor's bin
        auto tissue = [&](uint32_t j) {
            uint4 v = hb[j * 64u + lane];
            int32_t cut = (int32_t)thr_bin - (int32_t)(j * 256u + lane * 4u);   // the lane's entries 0 .. cut are no tissue
            asm volatile("" : "+v"(cut));                       // (made here: hoisted out of the band loop, the 32 comparisons hold 64 scalar registers across it)
            v.x = cut >= 0 ? 0u : v.x; v.y = cut >= 1 ? 0u : v.y; v.z = cut >= 2 ? 0u : v.z; v.w = cut >= 3 ? 0u : v.w;
            return v;
        };
        uint32_t tot[8], n_t = 0u;
#pragma unroll
        for (uint32_t j = 0; j < 8u; j++) {
            const uint4 v = tissue(j);
            uint32_t c = v.x + v.y + v.z + v.w;
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) c += (uint32_t)__shfl_xor((int)c, d, 64);
            tot[j] = (uint32_t)__builtin_amdgcn_readfirstlane((int)c);   // the chunk's tissue count
            n_t += tot[j];
        }
        const uint32_t rows = min(a.band_rows, R - b * a.band_rows);
        const bool valid = n_t > 0u && (unsigned long long)n_t * 1000ull >= (unsigned long long)a.min_permille * ((unsigned long long)a.lines * rows);
        int32_t m = -1;
        if (valid) {                                            // (the wavefront's)
            const unsigned long long need = n_t;
            uint32_t carry = 0u, js = 8u;                       // the chunk in which twice the cumulative count reaches n_t, and the count before it
#pragma unroll
            for (uint32_t j = 0; j < 8u; j++) {
                if (js == 8u) {
                    if (2ull * (carry + tot[j]) >= need) js = j;
                    else carry += tot[j];
                }
            }
            const uint4 vj = tissue(js);                        // (read again: the eight chunks are not kept in registers)
            const uint32_t sj = vj.x + vj.y + vj.z + vj.w;
            uint32_t incl = sj;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { const uint32_t o = (uint32_t)__shfl_up((int)incl, d, 64); if ((int)lane >= d) incl += o; }
            const unsigned long long mask = __ballot(2ull * (carry + incl) >= need);
            const int first = __ffsll((long long)mask) - 1;     // (the chunk's last lane satisfies it)
            uint32_t c = carry + incl - sj;
            const int32_t bin0 = (int32_t)(js * 256u + lane * 4u);
            int32_t bin = bin0 + 3;
            c += vj.x; const bool at0 = 2ull * c >= need;
            c += vj.y; const bool at1 = 2ull * c >= need;
            c += vj.z; const bool at2 = 2ull * c >= need;
            bin = at2 ? bin0 + 2 : bin; bin = at1 ? bin0 + 1 : bin; bin = at0 ? bin0 : bin;
            m = __shfl(bin, first, 64);
        }
        if (lane == 0u) m_s[b] = m;
    }
    __syncthreads();
    // the target: the valid band whose (level, index) has rank (V - 1) / 2
    if (t < nB && m_s[t] >= 0) {
        const int32_t mi = m_s[t];
        uint32_t V = 0u, rank = 0u;
        for (uint32_t j = 0; j < nB; j++) {
            const int32_t mj = m_s[j];
            if (mj < 0) continue;
            V++;
            if (mj < mi || (mj == mi && j < t)) rank++;
        }
        if (rank == (V - 1u) / 2u) tgt_s = mi;
        atomicMin(&first_s, (int32_t)t);
        atomicMax(&last_s, (int32_t)t);
    }
    __syncthreads();
    const int32_t tgt = tgt_s, last = last_s;
    if (t < nB) {
        float k = 1.0f;
        if (tgt >= 0) {
            int32_t j = (int32_t)t;
            while (j >= 0 && m_s[j] < 0) j--;                   // the nearest valid band shallower
            if (j < 0) j = first_s;
            k = fminf(fmaxf(autogain_centre(tgt) / autogain_centre(m_s[j]), a.inv_max_gain), a.max_gain);
        }
        k_s[t] = k;
        if (a.band_bin) a.band_bin[(size_t)f * nB + t] = m_s[t];
    }
    if (t == 0u && a.pen) a.pen[f] = last < 0 ? 0u : min(R, ((uint32_t)last + 1u) * a.band_rows);
    __syncthreads();
    const int32_t two_b = 2 * (int32_t)a.band_rows;
    for (uint32_t r = t; r < R; r += 1024u) {
        const int32_t n = 2 * (int32_t)r - ((int32_t)a.band_rows - 1);
        float k;
        if (n <= 0) k = k_s[0];
        else {
            const int32_t b = n / two_b;
            if (b >= (int32_t)nB - 1) k = k_s[nB - 1u];
            else {
                const float tt = (float)(n - two_b * b) / (float)two_b;
                const float k0 = k_s[b], d = k_s[b + 1] - k0, p = d * tt;
                k = k0 + p;
            }
        }
        a.gain[(size_t)f * R + r] = k;
    }
}

// Step 9 in k_noise's shape: a wavefront owns NOISE_WAVE_ROWS consecutive rows of one scan-line, a lane NOISE_LANE_ROWS of them -- one 16-byte
// load of the stack, one of the gains and one store where the addresses and R allow, row by row elsewhere and at the ragged end.
__global__ void __launch_bounds__(256) k_autogain_apply(AutogainArgs a, uint32_t n_lines)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    const uint32_t line = w / a.chunks, chunk = w - line * a.chunks;
    if (line >= n_lines) return;
    const uint32_t R = a.R, f = line / a.lines;
    const uint32_t r0 = chunk * NOISE_WAVE_ROWS + lane * NOISE_LANE_ROWS;
    if (r0 >= R) return;
    const uint32_t cnt = min(NOISE_LANE_ROWS, R - r0);
    float *p = a.rf + (size_t)line * R + r0;
    const float *g = a.gain + (size_t)f * R + r0;
    if (cnt == NOISE_LANE_ROWS && (uintptr_t)p % 16u == 0u && (uintptr_t)g % 16u == 0u) {
        const float4 q = *(const float4 *)p, k = *(const float4 *)g;
        *(float4 *)p = make_float4(q.x * k.x, q.y * k.y, q.z * k.z, q.w * k.w);
    } else {
        for (uint32_t i = 0; i < cnt; i++) p[i] = p[i] * g[i];
    }
}

// grid (shares, bands, frames); VEC where every band of every scan-line starts on 16 bytes and holds whole units of four rows
hipError_t launch_autogain_hist(const AutogainArgs &a, uint32_t F, uint32_t copies, hipStream_t st)
{
    if (F == 0u || a.shares == 0u || a.n_bands == 0u || a.n_bands > AUTOGAIN_MAX_BANDS) return hipErrorInvalidValue;
    const bool vec = (uintptr_t)a.rf % 16u == 0u && a.R % 4u == 0u && a.band_rows % 4u == 0u;
    const dim3 grid(a.shares, a.n_bands, F);
    if (copies == 4u) {
        if (vec) hipLaunchKernelGGL((k_autogain_hist<true, 4u>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((k_autogain_hist<false, 4u>), grid, dim3(256), 0, st, a);
    } else {
        if (vec) hipLaunchKernelGGL((k_autogain_hist<true, 1u>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((k_autogain_hist<false, 1u>), grid, dim3(256), 0, st, a);
    }
    return hipGetLastError();
}

hipError_t launch_autogain_curve(const AutogainArgs &a, uint32_t F, hipStream_t st)
{
    if (F == 0u || a.n_bands == 0u || a.n_bands > AUTOGAIN_MAX_BANDS || a.R > MCRT_MAX_ROWS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_autogain_curve, dim3(F), dim3(1024), 0, st, a);
    return hipGetLastError();
}

// one wavefront per (scan-line, chunk of NOISE_WAVE_ROWS rows), four to a workgroup (the stack has fewer than 2^31 samples: so has the grid)
hipError_t launch_autogain_apply(const AutogainArgs &a, uint32_t F, hipStream_t st)
{
    if (F == 0u || a.lines == 0u || a.chunks == 0u) return hipErrorInvalidValue;
    const uint32_t n_lines = F * a.lines, waves = n_lines * a.chunks;
    hipLaunchKernelGGL(k_autogain_apply, dim3((waves + 3u) / 4u), dim3(256), 0, st, a, n_lines);
    return hipGetLastError();
}

}  // namespace mcrt
