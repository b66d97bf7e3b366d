// mcrt_flow.hip -- colour Doppler (mcrt_flow_split_frames, mcrt_flow_frames, mcrt_colour_frames; contracts in include/mcrt.h): k_flow_split cuts
// the raw trace by tissue label into what stands still and what moves; k_flow<N, WALL> synthesises a sample's slow-time ensemble from the two
// detected images, filters it and takes its autocorrelation at lags 0 and 1; k_flow_avg averages the three planes over a window and writes
// the Kasai estimates; k_colour lays the estimate over the B-mode picture.  The reference has no counterpart.
#include "mcrt_device.h"
#include "mcrt_pixels.h"

namespace mcrt {

// One lane per sample, grid-strided: 5 bytes in, 8 out.  The table of moving labels is 256 bits in scalar registers; a lane picks its word
// by eight selects (an index into the argument block would go through scratch).
__global__ void __launch_bounds__(256) k_flow_split(FlowSplitArgs a)
{
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < a.n; i += gridDim.x * 256u) {
        const uint32_t l = a.tissue[i];
        uint32_t word = 0u;
#pragma unroll
        for (uint32_t k = 0; k < 8u; k++) word = (l >> 5) == k ? a.moving[k] : word;
        const bool mv = ((word >> (l & 31u)) & 1u) != 0u;
        const float v = a.rf[i];
        const uint32_t f = i / a.plane;
        float *o = a.out + (size_t)f * a.plane + i;                 // image 0 of frame f; image 1 is a.plane further
        o[0] = mv ? 0.0f : v;
        o[a.plane] = mv ? v : 0.0f;
    }
}

hipError_t launch_flow_split(const FlowSplitArgs &a, hipStream_t st)
{
    const uint32_t blocks = (a.n + 255u) / 256u;
    hipLaunchKernelGGL(k_flow_split, dim3(blocks < 4096u ? blocks : 4096u), dim3(256), 0, st, a);
    return hipGetLastError();
}

// k_noise's shape: a WAVEFRONT owns FLOW_WAVE_ROWS consecutive rows of one scan-line, a lane one of them -- the frame, the scan-line e, the
// image's id and k = sigma_f * inv_std are the wavefront's (scalar registers and scalar loads), the I/Q pairs are one 8-byte load per lane
// and 512 contiguous bytes per wavefront.  The N packets of a sample stay in registers: N and the wall filter are the instantiation and
// every loop over n is unrolled in full, so z[] is never indexed at run time (no scratch).  The phasor is gathered by the lane's label from
// the context's table [n_labels][E] -- at most 254 x E pairs, which stay in the vector cache.  With noise a sample costs N Philox4x32-10
// blocks (20 N products with both halves) against 17 bytes in and 12 out: the integer multiplier binds, as in k_noise; without it the
// kernel streams.  Every float operation is the contract's, rounded once (compiled -ffp-contract=off).  No LDS.
// the pairwise sum of the contract's mean: level by level neighbours are added in pairs, an odd last term is carried up as it is.  N equal
// terms at a power of two sum to N times the term exactly, so what stands still leaves the mean filter as +0.0f, not as rounding noise.
template <uint32_t N>
MCRT_DEV float pair_sum(const float (&z)[N])
{
    float t[N];
#pragma unroll
    for (uint32_t i = 0; i < N; i++) t[i] = z[i];
    uint32_t n = N;
#pragma unroll
    for (uint32_t level = 0; level < 4u; level++) {              // N <= 16: four levels at most
        if (n < 2u) break;
        const uint32_t half = n / 2u;
#pragma unroll
        for (uint32_t i = 0; i < N / 2u; i++)
            if (i < half) t[i] = t[2u * i] + t[2u * i + 1u];
        if (n & 1u) t[half] = t[n - 1u];
        n = half + (n & 1u);
    }
    return t[0];
}

template <uint32_t N, uint32_t WALL>
__global__ void __launch_bounds__(256) k_flow(FlowArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    const uint32_t line = w / a.chunks, chunk = w - line * a.chunks;
    if (line >= a.lines) return;
    const uint32_t R = a.R, E = a.E, f = line / E, e = line - f * E;
    const uint32_t r = chunk * FLOW_WAVE_ROWS + lane;
    if (r >= R) return;
    const size_t at = (size_t)line * R + r;
    const uint32_t l = a.tissue[at], id = a.first_id + f;
    const bool known = l < a.n_labels;
    const float2 p = known ? a.phasor[(size_t)l * E + e] : make_float2(1.0f, 0.0f);
    if (a.truth_out) a.truth_out[at] = known ? a.truth[(size_t)l * E + e] : 0.0f;
    const float sigma = a.sigma_dev ? a.sigma_dev[f] : a.sigma;
    const float k = sigma * a.inv_std;
    const bool has_static = a.iq_static != nullptr;
    const float2 s = has_static ? a.iq_static[at] : make_float2(0.0f, 0.0f);
    float2 m = a.iq_moving[at];
    float zr[N], zi[N];
#pragma unroll
    for (uint32_t n = 0; n < N; n++) {
        float xr = has_static ? s.x + m.x : m.x, xi = has_static ? s.y + m.y : m.y;
        if (k != 0.0f) {
            uint32_t o[4];
            philox4x32_10(e, r, 0x464C4F57u, n, a.seed, id, o);
            const int32_t di = (int32_t)(((o[0] & 0xffffu) + (o[0] >> 16)) + ((o[1] & 0xffffu) + (o[1] >> 16))) - 131070;   // |d| < 2^24: the conversions are exact
            const int32_t dq = (int32_t)(((o[2] & 0xffffu) + (o[2] >> 16)) + ((o[3] & 0xffffu) + (o[3] >> 16))) - 131070;
            xr = xr + k * (float)di; xi = xi + k * (float)dq;
        }
        zr[n] = xr; zi[n] = xi;
        if (n + 1u < N) {
            const float ac = m.x * p.x, bs = m.y * p.y, as = m.x * p.y, bc = m.y * p.x;
            m.x = ac - bs; m.y = as + bc;
        }
    }
    if (WALL != MCRT_FLOW_WALL_NONE) {
        const float mr = pair_sum<N>(zr) / (float)N, mi = pair_sum<N>(zi) / (float)N;
#pragma unroll
        for (uint32_t n = 0; n < N; n++) { zr[n] = zr[n] - mr; zi[n] = zi[n] - mi; }
    }
    if (WALL == MCRT_FLOW_WALL_LINEAR) {
        float nr = 0.0f, ni = 0.0f, den = 0.0f;
#pragma unroll
        for (uint32_t n = 0; n < N; n++) {
            const float t = (float)(2 * (int)n - ((int)N - 1));
            nr = nr + t * zr[n]; ni = ni + t * zi[n]; den = den + t * t;
        }
        const float br = nr / den, bi = ni / den;
#pragma unroll
        for (uint32_t n = 0; n < N; n++) {
            const float t = (float)(2 * (int)n - ((int)N - 1));
            zr[n] = zr[n] - t * br; zi[n] = zi[n] - t * bi;
        }
    }
    float r0 = 0.0f, re = 0.0f, im = 0.0f;
#pragma unroll
    for (uint32_t n = 0; n < N; n++) {
        const float rr = zr[n] * zr[n], ii = zi[n] * zi[n];
        r0 = r0 + (rr + ii);
    }
#pragma unroll
    for (uint32_t n = 0; n + 1u < N; n++) {
        const float ac = zr[n + 1u] * zr[n], bd = zi[n + 1u] * zi[n], bc = zi[n + 1u] * zr[n], ad = zr[n + 1u] * zi[n];
        re = re + (ac + bd); im = im + (bc - ad);
    }
    const size_t plane = (size_t)E * R;
    float *o = a.raw + (size_t)f * 3u * plane + (size_t)e * R + r;
    o[0] = r0; o[plane] = re; o[2u * plane] = im;
}

// The window average and the estimates, k_flow's layout: a wavefront owns 64 rows of one scan-line.  The separable order of the contract is
// taken as it is written -- per line of the window the sum along the rows, then the sum of those across the lines -- from the per-sample
// planes in the context's buffer: the (2 a + 1)(2 b + 1) reads of a lane (15 by default) are coalesced across the wavefront and hit the
// vector cache, a line being read by its 2 b + 1 neighbours at once.  The line loop is the wavefront's (scalar), the row test a lane's.
__global__ void __launch_bounds__(256) k_flow_avg(FlowArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    const uint32_t line = w / a.chunks, chunk = w - line * a.chunks;
    if (line >= a.lines) return;
    const uint32_t R = a.R, E = a.E, f = line / E, e = line - f * E;
    const uint32_t r = chunk * FLOW_WAVE_ROWS + lane;
    if (r >= R) return;
    const uint32_t e0 = e > a.avg_lines ? e - a.avg_lines : 0u, e1 = min(E - 1u, e + a.avg_lines);
    const uint32_t q0 = r > a.avg_rows ? r - a.avg_rows : 0u, q1 = min(R - 1u, r + a.avg_rows);
    const size_t plane = (size_t)E * R;
    const float *x = a.raw + (size_t)f * 3u * plane;
    float S[3] = { 0.0f, 0.0f, 0.0f };
    for (uint32_t ee = e0; ee <= e1; ee++) {
        const float *xl = x + (size_t)ee * R;
        float s[3] = { 0.0f, 0.0f, 0.0f };
        for (uint32_t q = q0; q <= q1; q++) {
#pragma unroll
            for (uint32_t c = 0; c < 3u; c++) s[c] = s[c] + xl[c * plane + q];
        }
#pragma unroll
        for (uint32_t c = 0; c < 3u; c++) S[c] = S[c] + s[c];
    }
    const float cnt = (float)((q1 - q0 + 1u) * (e1 - e0 + 1u));
    const float r0 = S[0] / cnt, re = S[1] / cnt, im = S[2] / cnt;
    const size_t at = (size_t)e * R + r;
    if (a.corr) {
        float *o = a.corr + (size_t)f * 3u * plane + at;
        o[0] = r0; o[plane] = re; o[2u * plane] = im;
    }
    if (a.vel) a.vel[(size_t)f * plane + at] = det_atan2f(im, re) * a.vscale;
    if (a.var) {
        const float rr = re * re, ii = im * im;
        float v = 1.0f - sqrtf(rr + ii) / r0;
        v = v < 0.0f ? 0.0f : v; v = v > 1.0f ? 1.0f : v;
        a.var[(size_t)f * plane + at] = r0 > 0.0f ? v : 0.0f;
    }
}

template <uint32_t N>
static void launch_flow_wall(const FlowArgs &a, dim3 grid, hipStream_t st)
{
    switch (a.wall) {
    case MCRT_FLOW_WALL_NONE: hipLaunchKernelGGL((k_flow<N, MCRT_FLOW_WALL_NONE>), grid, dim3(256), 0, st, a); break;
    case MCRT_FLOW_WALL_MEAN: hipLaunchKernelGGL((k_flow<N, MCRT_FLOW_WALL_MEAN>), grid, dim3(256), 0, st, a); break;
    default: hipLaunchKernelGGL((k_flow<N, MCRT_FLOW_WALL_LINEAR>), grid, dim3(256), 0, st, a); break;
    }
}

// one wavefront per (scan-line, chunk of FLOW_WAVE_ROWS rows), four to a workgroup (the stack has fewer than 2^31 samples: so has the grid)
hipError_t launch_flow(const FlowArgs &a, hipStream_t st)
{
    if (a.lines == 0u || a.chunks == 0u || a.wall > MCRT_FLOW_WALL_LINEAR) return hipErrorInvalidValue;
    const dim3 grid((a.lines * a.chunks + 3u) / 4u);
    switch (a.n_packets) {
#define FLOW_CASE(N) case N: launch_flow_wall<N>(a, grid, st); break;
    FLOW_CASE(2) FLOW_CASE(3) FLOW_CASE(4) FLOW_CASE(5) FLOW_CASE(6) FLOW_CASE(7) FLOW_CASE(8) FLOW_CASE(9)
    FLOW_CASE(10) FLOW_CASE(11) FLOW_CASE(12) FLOW_CASE(13) FLOW_CASE(14) FLOW_CASE(15) FLOW_CASE(16)
#undef FLOW_CASE
    default: return hipErrorInvalidValue;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_flow_avg, grid, dim3(256), 0, st, a);
    return hipGetLastError();
}

// The overlay over the pixel tile (mcrt_pixels.h): a lane owns the points p0 + 64 j of a picture, so the three planes and the grey bytes
// are read, and the velocity leaves, as neighbouring words of neighbouring lanes; the three bytes of a pixel leave one by one (a
// wavefront's 192 bytes are contiguous).  The colour table is 256 floats of the context's, each the exact integer r | g << 8 | b << 16.
__global__ void __launch_bounds__(256) k_colour(ColourArgs a)
{
    PixelTile tile;
    if (!pixel_tile(a.pass, tile)) return;
    const uint32_t n = a.pass.n;
    for (uint32_t f = tile.f0; f < tile.f1; f++) {
        const float *x = a.corr + (size_t)f * 3u * n;
        const uint8_t *grey = a.grey + (size_t)f * n;
        uint8_t *rgb = a.rgb + (size_t)f * 3u * n;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t p = tile.p0 + 64u * j;
            v[j] = 0.0f;
            if (p >= n) continue;
            const float r0 = x[p], re = x[n + p], im = x[2u * (size_t)n + p];
            const uint32_t g = grey[p];
            const float ang = det_atan2f(im, re), vel = ang * a.vscale;
            const bool show = r0 > a.power_thr && fabsf(vel) >= a.vel_thr && g <= a.grey_max;      // (a NaN compares false)
            uint32_t c = g | g << 8 | g << 16;
            if (show) {
                int idx = 128 + (int)rintf(ang * a.iscale);
                idx = idx < 1 ? 1 : idx > 255 ? 255 : idx;
                c = (uint32_t)a.lut[idx];
                v[j] = vel;
            }
            rgb[3u * (size_t)p] = (uint8_t)c; rgb[3u * (size_t)p + 1u] = (uint8_t)(c >> 8); rgb[3u * (size_t)p + 2u] = (uint8_t)(c >> 16);
        }
        if (a.vel) tile_store_f32(a.vel + (size_t)f * n, tile, n, v);
    }
}

hipError_t launch_colour(const ColourArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(k_colour, pixel_grid(a.pass), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace mcrt
