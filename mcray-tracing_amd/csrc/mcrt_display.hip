// mcrt_display.hip -- the displayed picture (mcrt_bmode_frames, contract in include/mcrt.h): k_bmode_peak (each frame's reference amplitude),
// k_bmode_grey (TGC and log compression of every RF tap) and k_bmode (the scan conversion of the grey levels, persistence and 8-bit
// quantisation, every frame of a pass in one launch).  Spatial compounding (mcrt_compound_frames, mcrt_bmode_compound_frames): k_compound, the
// N steered views of every frame gathered through their N map pairs into one float or 8-bit picture.
// The reference stops at rfimage.h:131-136 (log10(v+1)/log10(max+1), commented out) and rfimage.h:142-147 (convertTo CV_8U, 255).
#include "mcrt_device.h"

namespace mcrt {

// a = |v| * k[row]; a non-finite a (a NaN or infinite tap -- the reference's TIR scan-lines -- or an overflowing product) is no echo
MCRT_DEV float bmode_amp(float v, const float *tgc, uint32_t row)
{
    const float a = fabsf(v) * (tgc ? tgc[row] : 1.0f);
    return isfinite(a) ? a : 0.0f;
}

// Step 2, the largest a of every frame: grid (blocks per frame, F), 1024 lanes; frame f's E*R floats are grid-strided two float4 per lane
// at a time (scalars where the frame's size or the pointer do not allow float4), reduced over the wavefront, then the block, and leave as
// one atomicMax per block on the float's bits (a >= 0: the unsigned order of the bits is the float order, so the maximum is exact and
// independent of the order).  Atomics on one address are serialised (about 0.17 us each, measured): few, large blocks per frame.
// peak[] is zeroed before the launch.
template <bool VEC>
__global__ void __launch_bounds__(1024) k_bmode_peak(const float *rf, uint32_t E, uint32_t R, const float *tgc, float *peak)
{
    const size_t n = (size_t)E * R;
    const float *img = rf + (size_t)blockIdx.y * n;
    const size_t stride = (size_t)gridDim.x * 1024u;
    uint32_t m = 0u;
    auto amp4 = [&](float4 v, size_t i) {
        uint32_t r = (uint32_t)((4u * i) % R);
        m = max(m, __float_as_uint(bmode_amp(v.x, tgc, r))); r = r + 1u == R ? 0u : r + 1u;
        m = max(m, __float_as_uint(bmode_amp(v.y, tgc, r))); r = r + 1u == R ? 0u : r + 1u;
        m = max(m, __float_as_uint(bmode_amp(v.z, tgc, r))); r = r + 1u == R ? 0u : r + 1u;
        m = max(m, __float_as_uint(bmode_amp(v.w, tgc, r)));
    };
    if (VEC) {
        const float4 *img4 = (const float4 *)img;
        const size_t n4 = n / 4u;
        for (size_t i = (size_t)blockIdx.x * 1024u + threadIdx.x; i < n4; i += 2u * stride) {
            const bool two = i + stride < n4;
            const float4 v0 = img4[i];
            const float4 v1 = two ? img4[i + stride] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            amp4(v0, i);
            if (two) amp4(v1, i + stride);
        }
    } else {
        for (size_t i = (size_t)blockIdx.x * 1024u + threadIdx.x; i < n; i += stride)
            m = max(m, __float_as_uint(bmode_amp(img[i], tgc, (uint32_t)(i % R))));
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, d, 64));
    __shared__ uint32_t wave_max[16];
    if ((threadIdx.x & 63u) == 0u) wave_max[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x < 64u) {
        m = threadIdx.x < 16u ? wave_max[threadIdx.x] : 0u;
#pragma unroll
        for (int d = 8; d >= 1; d >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, d, 64));
        if (threadIdx.x == 0u && m) atomicMax((uint32_t *)&peak[blockIdx.y], m);
    }
}

// Step 3 of the contract, once per RF tap: grey[F][E][R] = g(a, ref_f) in float (grid (blocks per frame, F), float4 where the frame's size
// and the pointers allow).  Computing it per tap and not per interpolated pixel is 13x fewer log10f at 400 x 500 out of 128 x 465 (a tap
// feeds about 13 pixels' bilinear blends) -- the fused form measured 34.6 us for a 20-frame pass against k_remap's 19.0.
template <int MODE>
MCRT_DEV float bmode_grey(float amp, float ref, float den, float gain, float dr)
{
    const float g = MODE == MCRT_BMODE_DB ? (amp > 0.0f ? (20.0f * log10f(amp / ref) + gain + dr) / dr : 0.0f)
                                          : log10f(amp + 1.0f) / den;
    return fminf(fmaxf(g, 0.0f), 1.0f);                  // (fmaxf: a NaN quotient is 0)
}
template <int MODE, bool VEC>
__global__ void __launch_bounds__(256) k_bmode_grey(const float *rf, uint32_t E, uint32_t R, const float *tgc, const float *peak, float ref_fixed,
                                                    float *peak_out, float gain, float dr, float *grey)
{
    const size_t n = (size_t)E * R;
    const uint32_t f = blockIdx.y;
    const float *img = rf + (size_t)f * n;
    float *g = grey + (size_t)f * n;
    const float ref = peak ? peak[f] : ref_fixed;
    if (peak_out && blockIdx.x == 0u && threadIdx.x == 0u) peak_out[f] = ref;
    const bool black = !(ref > 0.0f);                    // ref_f == 0: the frame is black
    const float den = MODE == MCRT_BMODE_REF_LOG ? log10f(ref + 1.0f) : 0.0f;
    const size_t stride = (size_t)gridDim.x * 256u;
    auto one = [&](float v, uint32_t r) { return black ? 0.0f : bmode_grey<MODE>(bmode_amp(v, tgc, r), ref, den, gain, dr); };
    if (VEC) {
        for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n / 4u; i += stride) {
            const float4 v = ((const float4 *)img)[i];
            uint32_t r = (uint32_t)((4u * i) % R);
            float4 o;
            o.x = one(v.x, r); r = r + 1u == R ? 0u : r + 1u;
            o.y = one(v.y, r); r = r + 1u == R ? 0u : r + 1u;
            o.z = one(v.z, r); r = r + 1u == R ? 0u : r + 1u;
            o.w = one(v.w, r);
            ((float4 *)g)[i] = o;
        }
    } else {
        for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += stride) g[i] = one(img[i], (uint32_t)(i % R));
    }
}

// Steps 4-6.  Each lane owns the 4 consecutive output pixels 4q .. 4q+3 (fewer at the end of a frame) and walks the frames [f0, f1) of its
// chunk (blockIdx.y): the maps are read once, persistence is a register recurrence, and each frame's 4 pixels leave as one 32-bit store
// where the frame size and the output pointer keep them aligned (VEC_OUT).  The 16 taps of frame f+1 are loaded before frame f is blended
// (the recurrence is short; the gathers are what a lane waits for).  Frames are cut into chunks only without persistence (alpha = 0),
// where every frame stands alone.  The blend is remap_bilinear, k_remap's own expression, over the grey levels of k_bmode_grey.
template <bool VEC_OUT>
__global__ void __launch_bounds__(256) k_bmode(BmodeArgs a)
{
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    const uint32_t p0 = 4u * q;
    if (p0 >= a.n) return;
    const uint32_t cnt = min(4u, a.n - p0), E = a.E, R = a.R;
    float mx[4], my[4], y[4];
    RemapPoint pt[4];
    if (cnt == 4u) {                                    // the maps are hipMalloc'd and p0 % 4 == 0: 16-byte aligned
        const float4 c4 = *(const float4 *)(a.map_col + p0), r4 = *(const float4 *)(a.map_row + p0);
        mx[0] = c4.x; mx[1] = c4.y; mx[2] = c4.z; mx[3] = c4.w;
        my[0] = r4.x; my[1] = r4.y; my[2] = r4.z; my[3] = r4.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) { mx[j] = (uint32_t)j < cnt ? a.map_col[p0 + j] : 0.0f; my[j] = (uint32_t)j < cnt ? a.map_row[p0 + j] : 0.0f; }
    }
#pragma unroll
    for (int j = 0; j < 4; j++) pt[j] = remap_point(mx[j], my[j]);
    const uint32_t f0 = blockIdx.y * a.frames_per_chunk, f1 = min(a.F, f0 + a.frames_per_chunk);
    const bool smooth = a.alpha > 0.0f;
    bool have_prev = false;
    if (smooth && a.state && !a.reset) {
#pragma unroll
        for (int j = 0; j < 4; j++) y[j] = (uint32_t)j < cnt ? a.state[p0 + j] : 0.0f;
        have_prev = true;
    }
    const size_t frame = (size_t)E * R;
    float t[4][2][2], tn[4][2][2];                      // the taps of frame f and of frame f+1
    auto gather = [&](uint32_t f, float (*dst)[2][2]) {
        const float *g = a.grey + (size_t)f * frame;
#pragma unroll
        for (int j = 0; j < 4; j++) remap_taps(pt[j], E, R, [=](long long x, long long yy) { return g[(size_t)x * R + (size_t)yy]; }, dst[j]);
    };
    if (f0 < f1) gather(f0, t);
    for (uint32_t f = f0; f < f1; f++) {
        if (f + 1u < f1) gather(f + 1u, tn);
        uint32_t bytes = 0u;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const float s = remap_blend(pt[j], t[j]);
            if (!smooth) y[j] = s;
            else y[j] = fmaf(a.alpha, have_prev ? y[j] : s, (1.0f - a.alpha) * s);
            bytes |= (uint32_t)(uint8_t)(y[j] * 255.0f + 0.5f) << (8 * j);
        }
        have_prev = true;
        uint8_t *o = a.out + (size_t)f * a.n + p0;
        if (VEC_OUT && cnt == 4u) *(uint32_t *)o = bytes;
        else for (uint32_t j = 0; j < cnt; j++) o[j] = (uint8_t)(bytes >> (8 * j));
#pragma unroll
        for (int j = 0; j < 4; j++) { t[j][0][0] = tn[j][0][0]; t[j][0][1] = tn[j][0][1]; t[j][1][0] = tn[j][1][0]; t[j][1][1] = tn[j][1][1]; }
    }
    if (a.state && f1 == a.F && f0 < f1) {
#pragma unroll
        for (int j = 0; j < 4; j++) if ((uint32_t)j < cnt) a.state[p0 + j] = y[j];
    }
}

// Spatial compounding (contract in include/mcrt.h): out[f][p] = the mean, over the views n that cover pixel p, of view n of frame f blended
// at the point view n's maps give for p -- k_remap's expression per view, summed in n order, one rounding per operation.  OUT8 = false
// writes that float (mcrt_compound_frames); OUT8 = true takes the grey levels of k_bmode_grey and goes on as k_bmode does: persistence as
// a register recurrence, quantisation, one 32-bit store per frame and lane (mcrt_bmode_compound_frames).
// A wavefront owns 256 consecutive pixels, a lane the four pixels wb + 64 j + lane, j = 0..3: in every gather the 64 lanes then ask for 64
// NEIGHBOURING pixels, as k_remap's do.  (With four consecutive pixels per lane, k_bmode's layout, the lanes of one gather are four pixels
// apart and reach 2.5 times as many scan-lines, each a cache line of its own: measured)  The lane walks the frames [f0, f1)
// of its chunk (blockIdx.y) in groups of up to 8.  The loop of a group is VIEWS-outer: a view's 4 points are made once per group (16 views'
// points at once would take 16 x 4 x 6 registers), then that view is gathered and blended for each frame of the group into per-frame sums
// in registers.  Which views cover a pixel depends on the maps alone, so the count is made once per group.  The maps are padded to a
// multiple of 256 pixels per view (zeros: the pixels past the picture's end read tap (0, 0), which exists, and are not stored).  The float
// form stores 256 contiguous bytes per instruction as it is; the 8-bit form first turns the wavefront's 4 x 64 bytes round with four
// ds_bpermute, so that lane L holds the bytes of pixels wb + 4 L .. 4 L + 3 and stores them as one word (VEC_OUT: the picture's size and
// the output pointer keep them aligned; a wavefront at the picture's end stores its bytes one by one).  Frames are cut into chunks only
// without persistence, as in k_bmode.
constexpr int COMPOUND_GROUP = 8;
template <bool OUT8, bool VEC_OUT>
__global__ void __launch_bounds__(256) k_compound(CompoundArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wb = blockIdx.x * 1024u + (threadIdx.x >> 6) * 256u;      // the wavefront's first pixel
    if (wb >= a.n) return;                                                    // (the whole wavefront)
    const uint32_t p0 = wb + lane, E = a.E, R = a.R, N = a.N;                 // the lane's pixels: p0 + 64 j
    const bool whole = wb + 256u <= a.n;
    const size_t view = (size_t)E * R;
    const uint32_t f0 = blockIdx.y * a.frames_per_chunk, f1 = min(a.F, f0 + a.frames_per_chunk);
    const bool smooth = OUT8 && a.alpha > 0.0f;
    float y[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    bool have_prev = false;
    if (smooth && a.state && !a.reset) {
#pragma unroll
        for (int j = 0; j < 4; j++) y[j] = p0 + 64u * j < a.n ? a.state[p0 + 64u * j] : 0.0f;
        have_prev = true;
    }
    for (uint32_t g0 = f0; g0 < f1; g0 += (uint32_t)COMPOUND_GROUP) {
        const uint32_t ng = min((uint32_t)COMPOUND_GROUP, f1 - g0);
        float sum[COMPOUND_GROUP][4];
        float looks[4] = { 0.0f, 0.0f, 0.0f, 0.0f };       // views that cover each pixel (at most 16: exact in float)
#pragma unroll
        for (int k = 0; k < COMPOUND_GROUP; k++)
#pragma unroll
            for (int j = 0; j < 4; j++) sum[k][j] = 0.0f;
        for (uint32_t n = 0; n < N; n++) {
            const float *mc = a.maps + (size_t)(2u * n) * a.n_pad + p0, *mr = mc + a.n_pad;   // (n_pad % 256 == 0: p0 + 192 < n_pad)
            RemapPoint pt[4];
            bool covered[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const float mx = mc[64 * j], my = mr[64 * j];
                pt[j] = remap_point(mx, my);
                covered[j] = (mx == mx) && (my == my) && pt[j].x0 >= -1 && pt[j].x0 < (long long)E && pt[j].y0 >= -1 && pt[j].y0 < (long long)R;
                looks[j] = covered[j] ? looks[j] + 1.0f : looks[j];
            }
#pragma unroll
            for (int k = 0; k < COMPOUND_GROUP; k++) {
                if ((uint32_t)k < ng) {                     // (the same in every lane)
                    const float *g = a.src + ((size_t)(g0 + (uint32_t)k) * N + n) * view;
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        float t[2][2];
                        remap_taps(pt[j], E, R, [=](long long x, long long yy) { return g[(size_t)x * R + (size_t)yy]; }, t);
                        const float s = remap_blend(pt[j], t);
                        sum[k][j] = covered[j] ? sum[k][j] + s : sum[k][j];
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < COMPOUND_GROUP; k++) {
            if ((uint32_t)k < ng) {
                const uint32_t f = g0 + (uint32_t)k;
                float v[4];
#pragma unroll
                for (int j = 0; j < 4; j++) v[j] = looks[j] > 0.0f ? sum[k][j] / looks[j] : 0.0f;
                if (OUT8) {
                    uint32_t bytes = 0u;                    // byte j: pixel p0 + 64 j
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        if (!smooth) y[j] = v[j];
                        else y[j] = fmaf(a.alpha, have_prev ? y[j] : v[j], (1.0f - a.alpha) * v[j]);
                        bytes |= (uint32_t)(uint8_t)(y[j] * 255.0f + 0.5f) << (8 * j);
                    }
                    have_prev = true;
                    uint8_t *o = (uint8_t *)a.out + (size_t)f * a.n;
                    if (VEC_OUT && whole) {                 // pixel wb + 4 L + i is byte L / 16 of lane (4 L + i) % 64: every lane is active here
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
    }
    if (OUT8 && a.state && f1 == a.F && f0 < f1) {
#pragma unroll
        for (int j = 0; j < 4; j++) if (p0 + 64u * j < a.n) a.state[p0 + 64u * j] = y[j];
    }
}

hipError_t launch_bmode_peak(const float *rf, uint32_t F, uint32_t E, uint32_t R, const float *tgc, float *peak, hipStream_t st)
{
    const size_t n = (size_t)E * R;
    const bool vec = n % 4u == 0u && (uintptr_t)rf % 16u == 0u;
    const size_t per_block = 1024u * 8u;                 // two float4 per lane
    const uint32_t blocks = (uint32_t)std::min<size_t>(64u, std::max<size_t>(1u, (n + per_block - 1u) / per_block));
    if (vec) hipLaunchKernelGGL((k_bmode_peak<true>), dim3(blocks, F), dim3(1024), 0, st, rf, E, R, tgc, peak);
    else hipLaunchKernelGGL((k_bmode_peak<false>), dim3(blocks, F), dim3(1024), 0, st, rf, E, R, tgc, peak);
    return hipGetLastError();
}

hipError_t launch_bmode_grey(const float *rf, uint32_t F, uint32_t E, uint32_t R, const float *tgc, const float *peak, float ref, float *peak_out,
                             uint32_t mode, float gain, float dr, float *grey, hipStream_t st)
{
    const size_t n = (size_t)E * R;
    const bool vec = n % 4u == 0u && (uintptr_t)rf % 16u == 0u && (uintptr_t)grey % 16u == 0u;
    const uint32_t blocks = (uint32_t)std::min<size_t>(256u, std::max<size_t>(1u, (n + 1023u) / 1024u));   // about 4 taps per lane
    const dim3 grid(blocks, F), blk(256);
#define MCRT_GREY(M, V) hipLaunchKernelGGL((k_bmode_grey<M, V>), grid, blk, 0, st, rf, E, R, tgc, peak, ref, peak_out, gain, dr, grey)
    if (mode == MCRT_BMODE_DB) { if (vec) MCRT_GREY(MCRT_BMODE_DB, true); else MCRT_GREY(MCRT_BMODE_DB, false); }
    else { if (vec) MCRT_GREY(MCRT_BMODE_REF_LOG, true); else MCRT_GREY(MCRT_BMODE_REF_LOG, false); }
#undef MCRT_GREY
    return hipGetLastError();
}

hipError_t launch_bmode(const BmodeArgs &a, hipStream_t st)
{
    const uint32_t groups = (a.n + 3u) / 4u, chunks = (a.F + a.frames_per_chunk - 1u) / a.frames_per_chunk;
    const dim3 grid((groups + 255u) / 256u, chunks), blk(256);
    const bool vec = a.n % 4u == 0u && (uintptr_t)a.out % 4u == 0u;
    if (vec) hipLaunchKernelGGL((k_bmode<true>), grid, blk, 0, st, a);
    else hipLaunchKernelGGL((k_bmode<false>), grid, blk, 0, st, a);
    return hipGetLastError();
}

hipError_t launch_compound(const CompoundArgs &a, bool out8, hipStream_t st)
{
    const uint32_t chunks = (a.F + a.frames_per_chunk - 1u) / a.frames_per_chunk;
    const dim3 grid((a.n + 1023u) / 1024u, chunks), blk(256);
    const bool vec = a.n % 4u == 0u && (uintptr_t)a.out % 4u == 0u;          // the 8-bit form's one word per lane
    if (!out8) hipLaunchKernelGGL((k_compound<false, false>), grid, blk, 0, st, a);
    else if (vec) hipLaunchKernelGGL((k_compound<true, true>), grid, blk, 0, st, a);
    else hipLaunchKernelGGL((k_compound<true, false>), grid, blk, 0, st, a);
    return hipGetLastError();
}

}  // namespace mcrt
