// mcrt_spectral.hip -- spectral Doppler (mcrt_spectral_series_frames, mcrt_spectral_frames, mcrt_sonogram_frames; contracts in include/mcrt.h):
// k_gate_series synthesises a sample gate's slow-time series from the two detected images, the integer phase table and the rows' rates;
// k_spectrum<N> takes one windowed FFT of N pulses per (gate, column), orders its power by velocity and writes the mean velocity;
// k_sonogram_peak and k_sonogram turn a gate's spectra into the displayed picture.  The reference has no counterpart.
#include "mcrt_device.h"

namespace mcrt {

// A WAVEFRONT owns 64 consecutive pulses of one gate, a lane one pulse.  The gate, its rows' pairs, weights and rates are the
// wavefront's: their addresses are built from scalar registers only, so they arrive through the scalar path and the products
// w_r * M_r are formed once per row in every lane alike (no LDS, nothing to synchronise).  What differs from lane to lane is the phase,
// one 8-byte load, and the rotor it selects.  The rotor table (32 KB) stays in global memory and is read through the vector cache: a
// copy per workgroup in the LDS would cost 32 KB of loads for 256 pulses x G lookups of 8 bytes -- more traffic than the gathers
// themselves up to G = 16 -- and neighbouring pulses turn by neighbouring phases, so a wavefront's 64 lookups of a row fall into a few
// cache lines.  Every float operation is the contract's, rounded once (compiled -ffp-contract=off).
__global__ void __launch_bounds__(256) k_gate_series(GateSeriesArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    const uint32_t j = w / a.chunks, chunk = w - j * a.chunks;
    if (j >= a.n_gates) return;
    const uint32_t t = chunk * 64u + lane;
    if (t >= a.T) return;
    const uint32_t image = a.gates[3u * j], line = a.gates[3u * j + 1u], row0 = a.gates[3u * j + 2u];
    const size_t at = ((size_t)image * a.E + line) * a.R + row0;
    const int32_t *rate = a.rate + (size_t)j * a.G;
    const long long ph = a.phase[t];
    const bool has_static = a.iq_static != nullptr;
    float zr = 0.0f, zi = 0.0f, ar = 0.0f, ai = 0.0f;
    for (uint32_t i = 0; i < a.G; i++) {
        const float wr = a.weight[i];
        if (has_static) {
            const float2 s = a.iq_static[at + i];
            zr = zr + wr * s.x; zi = zi + wr * s.y;
        }
        const float2 m = a.iq_moving[at + i];
        const float Ar = wr * m.x, Ai = wr * m.y;
        const uint32_t theta = (uint32_t)((ph * (long long)rate[i]) >> 16);
        const float2 cs = a.lut[((theta + 0x80000u) >> 20) & 4095u];
        const float rc = Ar * cs.x, is = Ai * cs.y, rs = Ar * cs.y, ic = Ai * cs.x;
        ar = ar + (rc - is); ai = ai + (rs + ic);
    }
    float xr = zr + ar, xi = zi + ai;
    const float sigma = a.sigma_dev ? a.sigma_dev[image] : a.sigma;
    const float k = (sigma * a.wnorm) * a.inv_std;
    if (k != 0.0f) {
        uint32_t o[4];
        philox4x32_10(line, row0, 0x53504543u, t, a.seed, a.first_id + image, o);
        const int32_t di = (int32_t)(((o[0] & 0xffffu) + (o[0] >> 16)) + ((o[1] & 0xffffu) + (o[1] >> 16))) - 131070;   // |d| < 2^24: the conversions are exact
        const int32_t dq = (int32_t)(((o[2] & 0xffffu) + (o[2] >> 16)) + ((o[3] & 0xffffu) + (o[3] >> 16))) - 131070;
        xr = xr + k * (float)di; xi = xi + k * (float)dq;
    }
    a.series[(size_t)j * a.T + t] = make_float2(xr, xi);
}

// one wavefront per (gate, chunk of 64 pulses), four to a workgroup (n_gates * T < 2^28: so is the grid)
hipError_t launch_gate_series(const GateSeriesArgs &a, hipStream_t st)
{
    if (a.n_gates == 0u || a.chunks == 0u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_gate_series, dim3((a.n_gates * a.chunks + 3u) / 4u), dim3(256), 0, st, a);
    return hipGetLastError();
}

// the contract's pairwise sum over the N values a wavefront holds, lane l the P consecutive ones from l * P: the levels inside a lane in
// registers, the log2 LANES levels above them by an exchange with the lane whose number differs in one bit -- both partners add the same
// two terms, and a + b is b + a bit for bit, so every lane ends with the sum of the plain tree.  Lanes past LANES only meet each other.
template <uint32_t P, uint32_t LANES>
MCRT_DEV float wave_pair_sum(const float (&v)[P])
{
    float t[P];
#pragma unroll
    for (uint32_t i = 0; i < P; i++) t[i] = v[i];
#pragma unroll
    for (uint32_t n = P; n > 1u; n /= 2u) {
#pragma unroll
        for (uint32_t i = 0; i < P / 2u; i++)
            if (i < n / 2u) t[i] = t[2u * i] + t[2u * i + 1u];
    }
    float s = t[0];
#pragma unroll
    for (uint32_t m = 1u; m < LANES; m <<= 1) s = s + __shfl_xor(s, (int)m);
    return s;
}

// ONE wavefront is the workgroup and owns one (gate, column): no wavefront depends on another, and the barrier between two stages is
// the wavefront's own.  A lane loads the P = N / 64 consecutive pulses from lane * P (N = 32: one pulse, half the wavefront idle),
// which is the layout the pairwise sums of the wall filter and of the mean velocity want; the windowed points go to the workgroup's
// 8 N bytes of LDS in bit-reversed order and every stage runs there, a lane taking the butterflies lane, lane + 64, ...: from half = 32
// on a wavefront's two 8-byte accesses are 512 contiguous bytes each (no bank conflict), below that the stride of 2 half pairs costs
// up to two LDS cycles per access -- five short stages of at most four butterflies a lane.  The twiddles come from the context's table
// of this N through the vector cache.  Every float operation is the contract's, rounded once.
template <uint32_t N>
__global__ void __launch_bounds__(64) k_spectrum(SpectrumArgs a)
{
    constexpr uint32_t P = N >= 64u ? N / 64u : 1u, LANES = N / P, HALF = N / 2u;
    constexpr uint32_t LOG = N == 32u ? 5u : N == 64u ? 6u : N == 128u ? 7u : N == 256u ? 8u : 9u;
    __shared__ float2 y[N];
    const uint32_t lane = threadIdx.x;
    const uint32_t g = blockIdx.x / a.n_cols, c = blockIdx.x - g * a.n_cols;
    const bool on = lane < LANES;
    const float2 *x = a.series + (size_t)g * a.T + (size_t)c * a.hop;
    float xr[P], xi[P];
#pragma unroll
    for (uint32_t p = 0; p < P; p++) {
        const float2 v = on ? x[lane * P + p] : make_float2(0.0f, 0.0f);
        xr[p] = v.x; xi[p] = v.y;
    }
    if (a.wall == MCRT_SPECTRAL_WALL_MEAN) {
        const float mr = wave_pair_sum<P, LANES>(xr) / (float)N, mi = wave_pair_sum<P, LANES>(xi) / (float)N;
#pragma unroll
        for (uint32_t p = 0; p < P; p++) { xr[p] = xr[p] - mr; xi[p] = xi[p] - mi; }
    }
    if (on) {
#pragma unroll
        for (uint32_t p = 0; p < P; p++) {
            const uint32_t n = lane * P + p;
            const float h = a.window[n];
            y[__brev(n) >> (32u - LOG)] = make_float2(xr[p] * h, xi[p] * h);
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t s = 1u; s <= LOG; s++) {
        const uint32_t half = 1u << (s - 1u);
#pragma unroll
        for (uint32_t q = 0; q < (HALF + 63u) / 64u; q++) {
            const uint32_t k = lane + 64u * q;
            if (k < HALF) {
                const uint32_t j = k & (half - 1u), lo = ((k >> (s - 1u)) << s) + j, hi = lo + half;
                const float2 tw = a.tw[j * (N >> s)], u = y[lo], v = y[hi];
                const float rr = v.x * tw.x, ii = v.y * tw.y, ri = v.x * tw.y, ir = v.y * tw.x;
                const float tr = rr - ii, ti = ri + ir;
                y[lo] = make_float2(u.x + tr, u.y + ti);
                y[hi] = make_float2(u.x - tr, u.y - ti);
            }
        }
        __syncthreads();
    }
    float pw[P], mo[P];
#pragma unroll
    for (uint32_t p = 0; p < P; p++) {
        const uint32_t i = lane * P + p;
        pw[p] = 0.0f; mo[p] = 0.0f;
        if (on) {
            const float2 X = y[(i + HALF) & (N - 1u)];
            const float rr = X.x * X.x, ii = X.y * X.y;
            const int d = (int)i - (int)HALF;
            const uint32_t ad = (uint32_t)(d < 0 ? -d : d);
            pw[p] = ad < a.wall_bins ? 0.0f : rr + ii;
            mo[p] = pw[p] * (float)d;
        }
    }
    if (a.power && on) {
        float *o = a.power + ((size_t)g * a.n_cols + c) * N + lane * P;
#pragma unroll
        for (uint32_t p = 0; p < P; p++) o[p] = pw[p];
    }
    if (a.mean) {
        const float num = wave_pair_sum<P, LANES>(mo), den = wave_pair_sum<P, LANES>(pw);
        if (lane == 0u) a.mean[(size_t)g * a.n_cols + c] = den > 0.0f ? (num / den) * a.vscale : 0.0f;
    }
}

// one workgroup of one wavefront per (gate, column) (n_gates * T < 2^28: so is the grid)
hipError_t launch_spectrum(const SpectrumArgs &a, hipStream_t st)
{
    if (a.n_gates == 0u || a.n_cols == 0u) return hipErrorInvalidValue;
    const dim3 grid(a.n_gates * a.n_cols);
    switch (a.N) {
#define SPECTRUM_CASE(N) case N: hipLaunchKernelGGL(k_spectrum<N>, grid, dim3(64), 0, st, a); break;
    SPECTRUM_CASE(32) SPECTRUM_CASE(64) SPECTRUM_CASE(128) SPECTRUM_CASE(256) SPECTRUM_CASE(512)
#undef SPECTRUM_CASE
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// whether p counts in the display: finite and > 0 (a NaN, an infinity, a zero and anything negative count as 0)
MCRT_DEV bool sonogram_counts(float p) { return p > 0.0f && __float_as_uint(p) < 0x7f800000u; }

// The largest finite power of each gate: positive floats order as their bit patterns do, so the maximum is an integer maximum -- exact
// and independent of the order -- taken per lane, across the wavefront and then by one atomic per wavefront into peak[g] (zeroed before).
__global__ void __launch_bounds__(256) k_sonogram_peak(SonogramArgs a)
{
    const uint32_t g = blockIdx.y, per = a.n_cols * a.N;
    const float *p = a.power + (size_t)g * per;
    uint32_t m = 0u;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < per; i += gridDim.x * 256u) {
        const float v = p[i];
        if (sonogram_counts(v)) m = max(m, __float_as_uint(v));
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) m = max(m, (uint32_t)__shfl_xor((int)m, d));
    if ((threadIdx.x & 63u) == 0u && m != 0u) atomicMax((unsigned int *)(a.peak + g), m);
}

hipError_t launch_sonogram_peak(const SonogramArgs &a, hipStream_t st)
{
    const uint32_t per = a.n_cols * a.N, blocks = (per + 255u) / 256u;
    hipLaunchKernelGGL(k_sonogram_peak, dim3(blocks < 64u ? blocks : 64u, a.n_gates), dim3(256), 0, st, a);
    return hipGetLastError();
}

// The picture is the spectra transposed and turned upside down.  A workgroup owns a tile of 16 columns x 16 bins: it reads 16 runs of 16
// consecutive bins (64 bytes each), forms the bytes, and writes them through a 16 x 17 LDS tile as 16 runs of 16 consecutive bytes of
// 16 picture rows.  (The pixel tile of mcrt_pixels.h owns 256 consecutive points of ONE picture and gathers; this stage transposes.)
__global__ void __launch_bounds__(256) k_sonogram(SonogramArgs a)
{
    __shared__ uint8_t tile[16][17];
    const uint32_t tx = threadIdx.x & 15u, ty = threadIdx.x >> 4, g = blockIdx.z;
    const uint32_t c0 = blockIdx.x * 16u, i0 = blockIdx.y * 16u;
    const float ref = a.peak ? a.peak[g] : a.ref;
    if (c0 + ty < a.n_cols) {
        const float p = a.power[((size_t)g * a.n_cols + c0 + ty) * a.N + i0 + tx];
        float v = 0.0f;
        if (sonogram_counts(p)) {
            v = ((10.0f * log10f(p / ref) + a.gain) + a.dr) / a.dr;
            v = v < 0.0f ? 0.0f : v; v = v > 1.0f ? 1.0f : v;
        }
        tile[ty][tx] = (uint8_t)(v * 255.0f + 0.5f);
    }
    __syncthreads();
    if (c0 + tx < a.n_cols) a.out[((size_t)g * a.N + (a.N - 1u - (i0 + ty))) * a.n_cols + c0 + tx] = tile[tx][ty];
}

hipError_t launch_sonogram(const SonogramArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(k_sonogram, dim3((a.n_cols + 15u) / 16u, a.N / 16u, a.n_gates), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace mcrt
