// mcrt_display.hip -- the displayed picture (mcrt_bmode_frames, contract in include/mcrt.h): k_bmode_peak (each frame's reference amplitude),
// k_bmode_grey (TGC and log compression of every RF tap) and k_bmode (the scan conversion of the grey levels, persistence and 8-bit
// quantisation, every frame of a pass in one launch).  Spatial compounding (mcrt_compound_frames, mcrt_bmode_compound_frames): k_compound, the
// N steered views of every frame gathered through their N map pairs into one float or 8-bit picture.
// The reference stops at rfimage.h:131-136 (log10(v+1)/log10(max+1), commented out) and rfimage.h:142-147 (convertTo CV_8U, 255).
#include "mcrt_pixels.h"

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
// chunk (mcrt_pixels.h: frame_window): the maps are read once, persistence is a register recurrence, and each frame's 4 pixels leave as one
// 32-bit store where the frame size and the output pointer keep them aligned (VEC_OUT: pass.vec).  The 16 taps of frame f+1 are loaded before frame f is blended
// (the recurrence is short; the gathers are what a lane waits for).  Frames are cut into chunks only without persistence (alpha = 0),
// where every frame stands alone.  The blend is remap_bilinear, k_remap's own expression, over the grey levels of k_bmode_grey.
template <bool VEC_OUT>
__global__ void __launch_bounds__(256) k_bmode(BmodeArgs a)
{
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    const uint32_t p0 = 4u * q;
    const uint32_t n = a.pass.n;
    if (p0 >= n) return;
    const uint32_t cnt = min(4u, n - p0), E = a.E, R = a.R;
    float mx[4], my[4];
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
    uint32_t f0, f1;
    frame_window(a.pass, f0, f1);
    const bool smooth = a.alpha > 0.0f;
    float y[4];
    bool have_prev = persist_load(y, smooth, a.state, a.reset, p0, 1u, n);
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
        float s[4];
#pragma unroll
        for (int j = 0; j < 4; j++) s[j] = remap_blend(pt[j], t[j]);
        persist_step(y, have_prev, smooth, a.alpha, s);
        const uint32_t bytes = quantise4(y);
        uint8_t *o = a.out + (size_t)f * n + p0;
        if (VEC_OUT && cnt == 4u) *(uint32_t *)o = bytes;
        else for (uint32_t j = 0; j < cnt; j++) o[j] = (uint8_t)(bytes >> (8 * j));
#pragma unroll
        for (int j = 0; j < 4; j++) { t[j][0][0] = tn[j][0][0]; t[j][0][1] = tn[j][0][1]; t[j][1][0] = tn[j][1][0]; t[j][1][1] = tn[j][1][1]; }
    }
    if (a.state && f1 == a.pass.F && f0 < f1) {
#pragma unroll
        for (int j = 0; j < 4; j++) if ((uint32_t)j < cnt) a.state[p0 + j] = y[j];
    }
}

// Spatial compounding (contract in include/mcrt.h): out[f][p] = the mean, over the views n that cover pixel p, of view n of frame f blended
// at the point view n's maps give for p -- k_remap's expression per view, summed in n order, one rounding per operation.  OUT8 = false
// writes that float (mcrt_compound_frames); OUT8 = true takes the grey levels of k_bmode_grey and goes on as k_bmode does: persistence as
// a register recurrence, quantisation, one 32-bit store per frame and lane (mcrt_bmode_compound_frames).
// The layout, the frame chunks and the stores are the pixel tile's (mcrt_pixels.h; with k_bmode's four consecutive pixels per lane the lanes
// of one gather reach 2.5 times as many scan-lines: measured).  The lane walks the frames [f0, f1) of its chunk in groups of up
// to 8.  The loop of a group is VIEWS-outer: a view's 4 points are made once per group (16 views' points at once would take 16 x 4 x 6
// registers), then that view is gathered and blended for each frame of the group into per-frame sums in registers.  Which views cover a
// pixel depends on the maps alone, so the count is made once per group.  VEC_OUT is pass.vec.  Frames are cut into chunks only without
// persistence, as in k_bmode.
//
// MODE (mcrt_compound_frames_opts / mcrt_bmode_compound_frames_opts; the default options run COMPOUND_PLAIN, the loop described above):
//   COMPOUND_WEIGHTED  the weighted, feathered mean.  A view's weight at a pixel (compound_weight: its view weight times the lateral edge
//                      ramp of its column map) is made with the view's points, once per view and group; the count becomes the sum of the
//                      weights, the per-frame accumulator sum + w * s.  A view whose weight is not > 0 does not contribute.
//   COMPOUND_MAX       the same loop with the accumulator m = max(m, s) from -inf (the first contributing s, then s > m ? s : m); a NaN
//                      stays: once m is NaN nothing replaces it, and a NaN s replaces any number.  The weights only gate.
//   COMPOUND_MEDIAN    a loop of its own: 16 values x 4 pixels x 8 frames do not fit a lane's registers, so the median walks its frames ONE
//                      at a time and makes the points of every view again for each frame (the maps come from the cache: two coalesced
//                      loads per view and pixel beside the four gathered taps).  The views loop is unrolled over the N bucket NB (4, 8 or
//                      16, chosen by the launcher) so that every value has a register of its own: slot n holds view n's blend, +inf where
//                      the view does not contribute, the slot is past N or the blend is NaN (the NaN is remembered in a flag beside the
//                      values).  MEDIAN_PIX pixels of the lane's four are in flight at a time.  The values are ordered by Batcher's
//                      odd-even merge network (5, 19, 63 compare-exchanges of one v_min and one v_max each; the pads end up on top), and
//                      the middle one or two are picked by a select chain on the count.
constexpr int COMPOUND_GROUP = 8;
#ifndef MCRT_MEDIAN_PIX
#define MCRT_MEDIAN_PIX 4                  // pixels of a lane's four that the median holds values for at once: 4, 2 or 1 (measured)
#endif
constexpr int MEDIAN_PIX = MCRT_MEDIAN_PIX;
static_assert(MEDIAN_PIX == 1 || MEDIAN_PIX == 2 || MEDIAN_PIX == 4, "MCRT_MEDIAN_PIX divides the lane's four pixels");

// a view's weight at a pixel whose column map is mx: one rounding per operation (include/mcrt.h; mcrt_compound_weights is the host's copy)
MCRT_DEV float compound_weight(float mx, float last_line, float view_weight, float feather)
{
    const float a = feather > 0.0f ? fminf(fmaxf(fminf(mx, last_line - mx) / feather, 0.0f), 1.0f) : 1.0f;
    return view_weight * a;
}

// Batcher's odd-even merge sort of NB values (any NB; the kernel uses 4, 8 and 16) as a list of compare-exchanges (lo, hi), made at compile time: every index the kernel
// uses is a constant, so the values stay in registers
template <int NB> struct SortNet {
    int lo[NB * 4], hi[NB * 4], n;
    constexpr SortNet() : lo(), hi(), n(0)
    {
        for (int p = 1; p < NB; p *= 2)
            for (int k = p; k >= 1; k /= 2)
                for (int j = k % p; j <= NB - 1 - k; j += 2 * k)
                    for (int i = 0; i <= (k - 1 < NB - j - k - 1 ? k - 1 : NB - j - k - 1); i++)
                        if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) { lo[n] = i + j; hi[n] = i + j + k; n++; }
    }
};
template <int NB, int I> struct SortStep { static constexpr SortNet<NB> net = SortNet<NB>(); static constexpr int lo = net.lo[I], hi = net.hi[I]; };
template <int NB, int PIX, int I> MCRT_DEV void sort_steps(float (&v)[NB][PIX])
{
    if constexpr (I < SortNet<NB>().n) {
        constexpr int lo = SortStep<NB, I>::lo, hi = SortStep<NB, I>::hi;
#pragma unroll
        for (int q = 0; q < PIX; q++) {
            const float a = v[lo][q], b = v[hi][q];
            v[lo][q] = fminf(a, b); v[hi][q] = fmaxf(a, b);
        }
        sort_steps<NB, PIX, I + 1>(v);
    }
}
// the median of the c smallest of NB ordered values (c <= NB): v[(c-1)/2] for an odd c, the mean of v[c/2-1] and v[c/2] for an even one
template <int NB, int PIX> MCRT_DEV float median_pick(const float (&v)[NB][PIX], int q, uint32_t c)
{
    const uint32_t il = (c - 1u) >> 1, ih = c >> 1;        // (c odd: the same slot)
    float lo = v[0][q], hi = v[0][q];
#pragma unroll
    for (int i = 1; i <= NB / 2; i++) {
        if (i < NB / 2) lo = il == (uint32_t)i ? v[i][q] : lo;
        hi = ih == (uint32_t)i ? v[i][q] : hi;
    }
    return (c & 1u) ? lo : (lo + hi) * 0.5f;
}

template <bool OUT8, bool VEC_OUT, int MODE = COMPOUND_PLAIN, int NB = 0>
__global__ void __launch_bounds__(256) k_compound(CompoundArgs a)
{
    PixelTile tile;
    if (!pixel_tile(a.pass, tile)) return;
    const uint32_t p0 = tile.p0, f0 = tile.f0, f1 = tile.f1, pixels = a.pass.n, n_pad = a.pass.n_pad, E = a.E, R = a.R, N = a.N;
    const size_t view = (size_t)E * R;
    const bool smooth = OUT8 && a.alpha > 0.0f;
    float y[4];
    bool have_prev = persist_load(y, smooth, a.state, a.reset, p0, 64u, pixels);
    // frame f's four compounded values of this lane leave: persistence, quantisation and the byte store, or the floats
    auto emit = [&](uint32_t f, const float (&v)[4]) {
        if (OUT8) {
            persist_step(y, have_prev, smooth, a.alpha, v);
            tile_store_u8((uint8_t *)a.out + (size_t)f * pixels, tile, pixels, quantise4(y), VEC_OUT);
        } else tile_store_f32((float *)a.out + (size_t)f * pixels, tile, pixels, v);
    };
    if constexpr (MODE == COMPOUND_MEDIAN) {
        const float last_line = (float)(E - 1u), inf = __builtin_inff();
        for (uint32_t f = f0; f < f1; f++) {
            float v[4];
#pragma unroll
            for (int j0 = 0; j0 < 4; j0 += MEDIAN_PIX) {
                float s[NB][MEDIAN_PIX];
                uint32_t cnt[MEDIAN_PIX];
                bool bad[MEDIAN_PIX];
#pragma unroll
                for (int q = 0; q < MEDIAN_PIX; q++) { cnt[q] = 0u; bad[q] = false; }
#pragma unroll
                for (int n = 0; n < NB; n++) {
                    if ((uint32_t)n < N) {                  // (the same in every lane)
                        const float *mc = a.maps + (size_t)(2u * n) * n_pad + p0, *mr = mc + n_pad;
                        const float *g = a.src + ((size_t)f * N + (uint32_t)n) * view;
                        const float wv = a.weight[n];
#pragma unroll
                        for (int q = 0; q < MEDIAN_PIX; q++) {
                            const float mx = mc[64 * (j0 + q)], my = mr[64 * (j0 + q)];
                            const RemapPoint pt = remap_point(mx, my);
                            const bool in = (mx == mx) && (my == my) && pt.x0 >= -1 && pt.x0 < (long long)E && pt.y0 >= -1 && pt.y0 < (long long)R
                                            && compound_weight(mx, last_line, wv, a.feather) > 0.0f;
                            float t[2][2];
                            remap_taps(pt, E, R, [=](long long x, long long yy) { return g[(size_t)x * R + (size_t)yy]; }, t);
                            const float b = remap_blend(pt, t);
                            const bool number = b == b;
                            cnt[q] = in ? cnt[q] + 1u : cnt[q];
                            bad[q] = bad[q] || (in && !number);
                            s[n][q] = in && number ? b : inf;
                        }
                    } else {
#pragma unroll
                        for (int q = 0; q < MEDIAN_PIX; q++) s[n][q] = inf;
                    }
                }
                sort_steps<NB, MEDIAN_PIX, 0>(s);
#pragma unroll
                for (int q = 0; q < MEDIAN_PIX; q++) {
                    const float m = median_pick<NB, MEDIAN_PIX>(s, q, cnt[q]);
                    v[j0 + q] = cnt[q] == 0u ? 0.0f : bad[q] ? __builtin_nanf("") : m + 0.0f;
                }
            }
            emit(f, v);
        }
    } else {
        const float last_line = (float)(E - 1u);
        for (uint32_t g0 = f0; g0 < f1; g0 += (uint32_t)COMPOUND_GROUP) {
            const uint32_t ng = min((uint32_t)COMPOUND_GROUP, f1 - g0);
            float sum[COMPOUND_GROUP][4];
            float looks[4] = { 0.0f, 0.0f, 0.0f, 0.0f };       // views that cover each pixel (at most 16: exact in float); WEIGHTED: the sum of their weights
#pragma unroll
            for (int k = 0; k < COMPOUND_GROUP; k++)
#pragma unroll
                for (int j = 0; j < 4; j++) sum[k][j] = MODE == COMPOUND_MAX ? -__builtin_inff() : 0.0f;
            for (uint32_t n = 0; n < N; n++) {
                const float *mc = a.maps + (size_t)(2u * n) * n_pad + p0, *mr = mc + n_pad;
                RemapPoint pt[4];
                bool covered[4];
                float w[4];
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const float mx = mc[64 * j], my = mr[64 * j];
                    pt[j] = remap_point(mx, my);
                    covered[j] = (mx == mx) && (my == my) && pt[j].x0 >= -1 && pt[j].x0 < (long long)E && pt[j].y0 >= -1 && pt[j].y0 < (long long)R;
                    if constexpr (MODE == COMPOUND_PLAIN) { w[j] = 1.0f; looks[j] = covered[j] ? looks[j] + 1.0f : looks[j]; }
                    else {
                        w[j] = compound_weight(mx, last_line, a.weight[n], a.feather);
                        covered[j] = covered[j] && w[j] > 0.0f;
                        looks[j] = covered[j] ? looks[j] + (MODE == COMPOUND_WEIGHTED ? w[j] : 1.0f) : looks[j];
                    }
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
                            if constexpr (MODE == COMPOUND_PLAIN) sum[k][j] = covered[j] ? sum[k][j] + s : sum[k][j];
                            else if constexpr (MODE == COMPOUND_WEIGHTED) sum[k][j] = covered[j] ? sum[k][j] + w[j] * s : sum[k][j];
                            else sum[k][j] = covered[j] && (sum[k][j] == sum[k][j]) && !(s <= sum[k][j]) ? s : sum[k][j];
                        }
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < COMPOUND_GROUP; k++) {
                if ((uint32_t)k < ng) {
                    float v[4];
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        if constexpr (MODE == COMPOUND_MAX) v[j] = looks[j] > 0.0f ? sum[k][j] + 0.0f : 0.0f;
                        else v[j] = looks[j] > 0.0f ? sum[k][j] / looks[j] : 0.0f;
                    }
                    emit(g0 + (uint32_t)k, v);
                }
            }
        }
    }
    if (OUT8 && a.state && f1 == a.pass.F && f0 < f1) {
#pragma unroll
        for (int j = 0; j < 4; j++) if (p0 + 64u * j < pixels) a.state[p0 + 64u * j] = y[j];
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
    const dim3 grid = pixel_grid(a.pass), blk(256);
    if (a.pass.vec) hipLaunchKernelGGL((k_bmode<true>), grid, blk, 0, st, a);
    else hipLaunchKernelGGL((k_bmode<false>), grid, blk, 0, st, a);
    return hipGetLastError();
}

// a.mode picks the instantiation; the median's views loop is unrolled over the smallest bucket that holds a.N
hipError_t launch_compound(const CompoundArgs &a, bool out8, hipStream_t st)
{
    const dim3 grid = pixel_grid(a.pass), blk(256);
#define MCRT_COMPOUND(...) do { \
        if (!out8) hipLaunchKernelGGL((k_compound<false, false, __VA_ARGS__>), grid, blk, 0, st, a); \
        else if (a.pass.vec) hipLaunchKernelGGL((k_compound<true, true, __VA_ARGS__>), grid, blk, 0, st, a); \
        else hipLaunchKernelGGL((k_compound<true, false, __VA_ARGS__>), grid, blk, 0, st, a); } while (0)
    switch (a.mode) {
    case COMPOUND_PLAIN: MCRT_COMPOUND(COMPOUND_PLAIN, 0); break;
    case COMPOUND_WEIGHTED: MCRT_COMPOUND(COMPOUND_WEIGHTED, 0); break;
    case COMPOUND_MAX: MCRT_COMPOUND(COMPOUND_MAX, 0); break;
    case COMPOUND_MEDIAN:
        if (a.N <= 4u) MCRT_COMPOUND(COMPOUND_MEDIAN, 4);
        else if (a.N <= 8u) MCRT_COMPOUND(COMPOUND_MEDIAN, 8);
        else MCRT_COMPOUND(COMPOUND_MEDIAN, 16);
        break;
    default: return hipErrorInvalidValue;
    }
#undef MCRT_COMPOUND
    return hipGetLastError();
}

}  // namespace mcrt
