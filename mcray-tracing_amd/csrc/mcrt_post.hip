// mcrt_post.hip -- after the accumulation: k_finalize (fixed-point RF bins -> float image, rf_image::clear rfimage.h:161), k_conv_*
// (rf_image::convolve, rfimage.h:93-123; k_conv_lateral_rows its lateral pass with a tap row per RF row: focal zones; k_conv_axial_bands its axial pass with a tap row per
// band and RF row: frequency compounding), k_envelope (rfimage.h:54-91), k_remap (the scan conversion of rf_image::postprocess,
// rfimage.h:125-140), k_elevation (the elevation planes of a frame folded into one image: slice thickness), k_transpose, and k_blocks_to_frames (the ranks' blocks of an mcrt_group laid out as frames).
#include "mcrt_device.h"

namespace mcrt {

// fixed-point bins -> float RF image [ne][R]; clears the bins for the next frame.  A frame whose launches set the context's device
// error word (a persistent kernel abandoned by its watchdog, a traversal stack that ran out) is written as NaN throughout: a caller that
// synchronises on its own stream and never asks mcrt_synchronize cannot mistake it for an image.
__global__ void k_finalize(long long *acc, uint32_t *flags, float *rf, uint32_t ne, uint32_t R, const uint32_t *error_flag)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)ne * R) return;
    const uint32_t e = (uint32_t)(i / R), r = (uint32_t)(i % R);
    const uint32_t nf = (R + 31u) >> 5;
    const bool bad = ((flags[(size_t)e * nf + (r >> 5)] >> (r & 31)) & 1u) || *error_flag != 0u;
    const long long v = acc[i];
    rf[i] = bad ? __uint_as_float(0x7fc00000u) : (float)((double)v * 0x1p-40);
    acc[i] = 0;
}
__global__ void k_clear_flags(uint32_t *flags, size_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flags[i] = 0u;
}

// rfimage.h:96-108 on the scan-line-major image: tmp[e][row] = sum_k img[e][row+k]*ax[k], row in [na, R-na)
// (both passes take a stack of n_img images [n_img][E][R] at once: one launch for all the frames of a pass)
__global__ void k_conv_axial(const float *img, float *tmp, uint32_t n_img, uint32_t E, uint32_t R, ConvTaps taps)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n_img * E * R) return;
    const int row = (int)(i % R), na = (int)taps.n_ax;
    if (row < na || row >= (int)R - na) return;
    float conv = 0;
    for (int k = 0; k < na; k++) conv += img[i + k] * taps.ax[k];
    tmp[i] = conv;
}
// rfimage.h:111-122: img[col][row] = sum_k tmp[col+k][row]*lat[k], row in [na,R-na), col in [nl/2, E-nl)
__global__ void k_conv_lateral(const float *tmp, float *img, uint32_t n_img, uint32_t E, uint32_t R, ConvTaps taps)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n_img * E * R) return;
    const int row = (int)(i % R), col = (int)((i / R) % E), na = (int)taps.n_ax, nl = (int)taps.n_lat;
    if (row < na || row >= (int)R - na) return;
    if (col < nl / 2 || col >= (int)E - nl) return;
    float conv = 0;
    for (int k = 0; k < nl; k++) conv += tmp[i + (size_t)k * R] * taps.lat[k];
    img[i] = conv;
}

// The lateral pass of mcrt_convolve_frames_depth: rfimage.h:111-122 with taps of their own per row (focal zones),
//     img[col][row] = sum_k tmp[col+k][row] * lat[k][row],  row in [na, R-na), col in [nl/2, E-nl),
// lat tap-major [nl][R] (the host transposes the caller's [R][nl]).  A lane owns one row of a strip of MCRT_CONV_STRIP neighbouring
// columns: it loads each tap once for the whole strip, and the strip's window slides by one column per tap, so the sums of a strip
// read nl + STRIP - 1 values of tmp instead of STRIP * nl.  Neighbouring lanes are neighbouring rows, so every tap and window load of
// a wavefront is one contiguous line.  Each sum is still sequential over k from 0, one rounding per multiply and per add.
// (8 columns measured best: 20 x 128 x 465 images 9.0 us at 2, 4 or 8 columns, 12.8 at one; 128 frames 20.3 us at 8, 29.7 at 4,
// 42.3 at 2, 67.2 at 1; k_conv_lateral 11.3 and 59.8 us -- DESIGN 5.5)
#ifndef MCRT_CONV_STRIP
#define MCRT_CONV_STRIP 8
#endif
__global__ void k_conv_lateral_rows(const float *tmp, float *img, uint32_t n_img, uint32_t E, uint32_t R, uint32_t na, uint32_t nl,
                                    uint32_t n_strips, const float *lat)
{
    constexpr int C = MCRT_CONV_STRIP;
    const uint32_t nr = R - 2u * na;                                            // rows of the window (> 0: the launcher checks)
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n_img * n_strips * nr) return;
    const uint32_t row = na + (uint32_t)(i % nr);
    const size_t sf = i / nr;                                                   // frame * n_strips + strip
    const uint32_t strip = (uint32_t)(sf % n_strips), f = (uint32_t)(sf / n_strips);
    const uint32_t col0 = nl / 2u + strip * (uint32_t)C, col_end = E - nl;      // this strip's first column, the window's end
    const float *t = tmp + ((size_t)f * E) * R + row;                           // column c of frame f at t[c * R]
    float win[C], conv[C];
#pragma unroll
    for (int j = 0; j < C; j++) {                                               // columns past the image's last are never summed: 0
        conv[j] = 0.0f;
        win[j] = col0 + (uint32_t)j < E ? t[(size_t)(col0 + j) * R] : 0.0f;
    }
    for (uint32_t k = 0; k < nl; k++) {
        const float w = lat[(size_t)k * R + row];
        const uint32_t c = col0 + (uint32_t)C + k;                              // the column the window takes in for tap k + 1
        const float next = (k + 1u < nl && c < E) ? t[(size_t)c * R] : 0.0f;
#pragma unroll
        for (int j = 0; j < C; j++) conv[j] += win[j] * w;
#pragma unroll
        for (int j = 0; j < C - 1; j++) win[j] = win[j + 1];                    // slide: win[j] = tmp[col0 + j + k + 1]
        win[C - 1] = next;
    }
    float *o = img + ((size_t)f * E) * R + row;
#pragma unroll
    for (int j = 0; j < C; j++)
        if (col0 + (uint32_t)j < col_end) o[(size_t)(col0 + j) * R] = conv[j];
}

// The axial pass of mcrt_convolve_bands_frames (frequency compounding, the depth downshift): k_conv_axial with taps of their own per band and per row,
//     tmp[f][b][e][row] = sum_k rf[f][e][row+k] * ax[b][k][row],  row in [na, R-na),   ax tap-major [B][na][R] (the host transposes the caller's [B][R][na]),
// and out[f][b][e][row] = rf[f][e][row] at EVERY pixel: the band image starts as the input's own bits, and the lateral pass then writes its window over it.
// A lane owns one row of a strip of MCRT_BANDS_STRIP neighbouring columns, for all B bands: per tap it loads the strip's input values once and each
// band's tap once, and adds into B x STRIP sums held in registers (indexed by unrolled constants only: no scratch).  So an input value is loaded once
// for all the bands, a tap once for the whole strip -- (STRIP + B) loads per tap for B * STRIP sums, where B calls of k_conv_axial take B * STRIP --
// and neighbouring lanes are neighbouring rows: every tap load and every input load of a wavefront is one contiguous line.  Each sum is still
// sequential over k from 0.0f, one rounding per multiply and per add.  (20 x 128 x 465 images, 3 bands, 7 / 13 taps, the whole
// call: 46.7 us at 4 columns, 47.9 at 8, 52.1 at 2, 54.7 at 1; three calls of mcrt_convolve_frames 62.4 us -- DESIGN 5.18)
#ifndef MCRT_BANDS_STRIP
#define MCRT_BANDS_STRIP 4
#endif
#define MCRT_MAX_BANDS 8
__global__ void k_conv_axial_bands(const float *rf, float *tmp, float *out, uint32_t F, uint32_t B, uint32_t E, uint32_t R, uint32_t na,
                                   uint32_t n_strips, const float *ax)
{
    constexpr int C = MCRT_BANDS_STRIP;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)F * n_strips * R) return;
    const uint32_t row = (uint32_t)(i % R);
    const size_t sf = i / R;                                                    // frame * n_strips + strip
    const uint32_t col0 = (uint32_t)(sf % n_strips) * (uint32_t)C, f = (uint32_t)(sf / n_strips);
    const bool inside = row >= na && row + na < R;                              // a row of the window: row + k < R for every tap
    const float *p = rf + ((size_t)f * E + col0) * R + row;                     // column col0 + j at p[j * R]
    float acc[MCRT_MAX_BANDS][C], first[C];
#pragma unroll
    for (int b = 0; b < MCRT_MAX_BANDS; b++)
#pragma unroll
        for (int j = 0; j < C; j++) acc[b][j] = 0.0f;
#pragma unroll
    for (int j = 0; j < C; j++) first[j] = col0 + (uint32_t)j < E ? p[(size_t)j * R] : 0.0f;
    const uint32_t nk = inside ? na : 0u;
    for (uint32_t k = 0; k < nk; k++) {
        float v[C];
#pragma unroll
        for (int j = 0; j < C; j++) v[j] = col0 + (uint32_t)j < E ? p[(size_t)j * R + k] : 0.0f;
#pragma unroll
        for (int b = 0; b < MCRT_MAX_BANDS; b++)
            if ((uint32_t)b < B) {
                const float w = ax[((size_t)b * na + k) * R + row];
#pragma unroll
                for (int j = 0; j < C; j++) acc[b][j] += v[j] * w;
            }
    }
#pragma unroll
    for (int b = 0; b < MCRT_MAX_BANDS; b++)
        if ((uint32_t)b < B) {
            const size_t o = (((size_t)f * B + (uint32_t)b) * E + col0) * R + row;
#pragma unroll
            for (int j = 0; j < C; j++)
                if (col0 + (uint32_t)j < E) {
                    out[o + (size_t)j * R] = first[j];
                    if (inside) tmp[o + (size_t)j * R] = acc[b][j];
                }
        }
}

// mcrt_elevation_frames (psf.h:16-18,42,77; the contract is in mcrt.h): the K elevation planes of every frame folded into one RF image,
//     rf[f][e][r] = sum_k planes[f][k][e][r] * w[k][r],   w tap-major [K][R] (the host transposes the caller's [R][K]),
// summed in k order from 0.0f, one rounding per multiply and per add.  A pure stream: F*K*E*R floats read once, F*E*R written.  A lane
// owns one V (a float4 = 4 consecutive floats of the flattened [E*R] image, or one float) and loads its planes in batches of
// MCRT_ELEV_BATCH before the first multiply of the batch, so that up to 8 loads of 16 bytes are in flight per lane (K = 7: all of them).
// A batch's loads are unconditional -- past the last plane they repeat it, which stays inside the stack -- and only the sums are guarded:
// a plane that does not exist must not reach the sum (0 * NaN).  nv = E*R / (floats per V); rows wrap inside a float4 when R % 4 != 0.
#define MCRT_ELEV_BATCH 8
__device__ __forceinline__ void elev_fold(float4 &a, const float4 &v, const float *wk, const uint32_t *r)
{
    a.x += v.x * wk[r[0]]; a.y += v.y * wk[r[1]]; a.z += v.z * wk[r[2]]; a.w += v.w * wk[r[3]];
}
__device__ __forceinline__ void elev_fold(float &a, const float &v, const float *wk, const uint32_t *r) { a += v * wk[r[0]]; }
__device__ __forceinline__ void elev_zero(float4 &a) { a = make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
__device__ __forceinline__ void elev_zero(float &a) { a = 0.0f; }
template <typename V>
__global__ void k_elevation(const V *planes, V *rf, uint32_t F, uint32_t K, size_t nv, uint32_t R, const float *w)
{
    constexpr uint32_t W = sizeof(V) / 4u;
    constexpr uint32_t B = MCRT_ELEV_BATCH;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;            // element of `rf`
    if (i >= (size_t)F * nv) return;
    const size_t f = i / nv, j = i % nv;
    const V *p = planes + f * K * nv + j;                                      // plane k of this lane at p[k * nv]
    uint32_t r[W];
    r[0] = (uint32_t)((j * W) % R);
#pragma unroll
    for (uint32_t c = 1; c < W; c++) r[c] = r[c - 1u] + 1u == R ? 0u : r[c - 1u] + 1u;
    V acc; elev_zero(acc);
    for (uint32_t k0 = 0; k0 < K; k0 += B) {
        V v[B];
#pragma unroll
        for (uint32_t b = 0; b < B; b++) v[b] = p[(size_t)min(k0 + b, K - 1u) * nv];
#pragma unroll
        for (uint32_t b = 0; b < B; b++)
            if (k0 + b < K) elev_fold(acc, v[b], w + (size_t)(k0 + b) * R, r);
    }
    rf[i] = acc;
}

// rfimage.h:54-91, one WAVEFRONT per scan-line.  The reference walks a column once: whenever the signal stops ascending at row i
// (a concave peak), the rows [last peak, i) are overwritten with the line from |last peak| to |c[i]|.  The comparisons only ever
// read rows the walk has not overwritten yet, so the peaks are a pure function of the input column:
//     peak(i) = (c[i-1] < c[i]) && !(c[i] < c[i+1]),  1 <= i <= R-2      (`ascending` after step j is exactly c[j] < c[j+1])
// and row j becomes  last*(1-alpha) + next*alpha  with last / next the peaks around it (prev <= j < next; before the first peak
// `last` is the signed c[0] at row 0, rfimage.h:64), rows after the last peak stay.  Same float expressions as the sequential loop,
// evaluated by 64 lanes from an LDS copy of the column: previous / next peak by a wave-wide max / min scan over lane-contiguous chunks.
// (One lane per column, the round-2 kernel, is a chain of 465 dependent global loads: 650 us per call however few the columns.)
__global__ void __launch_bounds__(64) k_envelope(float *img, uint32_t E, uint32_t R)
{
    __shared__ float col[MCRT_MAX_ROWS];
    __shared__ unsigned short prv[MCRT_MAX_ROWS], nxt[MCRT_MAX_ROWS];
    const uint32_t lane = threadIdx.x;
    if (blockIdx.x >= E || R < 2) return;
    float *c = img + (size_t)blockIdx.x * R;
    for (uint32_t r = lane; r < R; r += 64u) col[r] = c[r];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier();
    const uint32_t per = (R + 63u) / 64u, r0 = min(R, lane * per), r1 = min(R, r0 + per);
    constexpr uint32_t NONE = 0xffffu;
    auto peak = [&](uint32_t i) { return i >= 1u && i + 1u < R && (col[i - 1u] < col[i]) && !(col[i] < col[i + 1u]); };
    // last peak at or before each row (0 = the start of the column), first peak after it
    uint32_t last = 0u, first = NONE;
    for (uint32_t i = r0; i < r1; i++) if (peak(i)) { last = i; if (first == NONE) first = i; }
    uint32_t before = last, after = first;                    // inclusive scans over the lanes' chunks ...
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)before, d, 64), dn = (uint32_t)__shfl_down((int)after, d, 64);
        if ((int)lane >= d) before = max(before, up);
        if ((int)lane + d < 64) after = min(after, dn);
    }
    uint32_t run_prev = (uint32_t)__shfl_up((int)before, 1, 64), run_next = (uint32_t)__shfl_down((int)after, 1, 64);      // ... made exclusive
    if (lane == 0u) run_prev = 0u;
    if (lane == 63u) run_next = NONE;
    for (uint32_t i = r0; i < r1; i++) { if (peak(i)) run_prev = i; prv[i] = (unsigned short)run_prev; }
    for (uint32_t i = r1; i > r0; i--) { nxt[i - 1u] = (unsigned short)run_next; if (peak(i - 1u)) run_next = i - 1u; }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier();
    for (uint32_t j = lane; j < R; j += 64u) {
        const uint32_t p = prv[j], q = nxt[j];
        if (q == NONE) continue;                               // past the last peak: untouched
        const float last_peak = p == 0u ? col[0] : fabsf(col[p]), new_peak = fabsf(col[q]);
        const float alpha = ((float)j - (float)p) / ((float)q - (float)p);
        c[j] = last_peak * (1 - alpha) + new_peak * alpha;
    }
}

// cv::remap(src, dst, map_y, map_x, INTER_LINEAR, BORDER_CONSTANT 0) with precomputed maps (rfimage.h:139):
// src is [E][R] scan-line-major; the tap-and-blend is remap_bilinear (mcrt_device.h), shared with k_bmode.
__global__ void k_remap(const float *img, uint32_t E, uint32_t R, const float *map_col, const float *map_row, float *out, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    img += (size_t)blockIdx.y * E * R; out += (size_t)blockIdx.y * n;          // image blockIdx.y of a stack [n_img][E][R] -> [n_img][n]
    out[i] = remap_bilinear(map_col[i], map_row[i], E, R, [=](long long x, long long y) { return img[(size_t)x * R + (size_t)y]; });
}

// [E][R] -> [R][E]
__global__ void k_transpose(const float *in, float *out, uint32_t E, uint32_t R)
{
    __shared__ float tile[32][33];
    const uint32_t r0 = blockIdx.x * 32, e0 = blockIdx.y * 32;
    for (int j = threadIdx.y; j < 32; j += blockDim.y) {
        const uint32_t e = e0 + j, r = r0 + threadIdx.x;
        if (e < E && r < R) tile[j][threadIdx.x] = in[(size_t)e * R + r];
    }
    __syncthreads();
    for (int j = threadIdx.y; j < 32; j += blockDim.y) {
        const uint32_t r = r0 + j, e = e0 + threadIdx.x;
        if (e < E && r < R) out[(size_t)r * E + e] = tile[threadIdx.x][j];
    }
}

// The ranks' blocks, as they arrive from the other GPUs -- rank g's [F][ne_g][R] one after the other -- laid out as the frames
// [F][E][R] a single context would have written (mcrt_group_trace_frames): one float4 per lane where R allows, else scalars.
// off[g] = first scan-line of rank g (off[G] = E); the block of rank g starts at float offset F * off[g] * R of `blocks`.
struct GroupOffsets { uint32_t off[65]; };
template <typename V>
__global__ void k_blocks_to_frames(const V *blocks, V *frames, uint32_t F, uint32_t E, uint32_t Rv, uint32_t G, GroupOffsets o)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;          // element of `frames`
    if (i >= (size_t)F * E * Rv) return;
    const uint32_t r = (uint32_t)(i % Rv), e = (uint32_t)((i / Rv) % E), f = (uint32_t)(i / ((size_t)Rv * E));
    uint32_t g = 0;
    while (g + 1u < G && e >= o.off[g + 1u]) g++;
    const uint32_t ne = o.off[g + 1u] - o.off[g];
    frames[i] = blocks[((size_t)F * o.off[g] + (size_t)f * ne + (e - o.off[g])) * Rv + r];
}

hipError_t launch_finalize(long long *acc, uint32_t *flags, float *rf, uint32_t ne, uint32_t R, const uint32_t *error_flag, hipStream_t st)
{
    const size_t n = (size_t)ne * R;
    hipLaunchKernelGGL(k_finalize, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, acc, flags, rf, ne, R, error_flag);
    const size_t nf = (size_t)ne * ((R + 31u) >> 5);
    hipLaunchKernelGGL(k_clear_flags, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, st, flags, nf);
    return hipGetLastError();
}

// the lateral pass over n_img images, tmp -> img: k_conv_lateral_rows with the device table lat [taps.n_lat][R] where one is given, else k_conv_lateral with taps.lat
static void launch_conv_lateral(const float *tmp, float *img, uint32_t n_img, uint32_t E, uint32_t R, const ConvTaps &taps, const float *lat, hipStream_t st)
{
    const size_t n = (size_t)n_img * E * R;
    const uint32_t na = taps.n_ax, nl = taps.n_lat;
    if (!lat) hipLaunchKernelGGL(k_conv_lateral, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, tmp, img, n_img, E, R, taps);
    else if (R > 2u * na && E > nl + nl / 2u) {                                 // else the lateral window is empty (as in k_conv_lateral)
        const uint32_t n_strips = (E - nl - nl / 2u + MCRT_CONV_STRIP - 1u) / MCRT_CONV_STRIP;
        const size_t m = (size_t)n_img * n_strips * (R - 2u * na);
        hipLaunchKernelGGL(k_conv_lateral_rows, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, tmp, img, n_img, E, R, na, nl, n_strips, lat);
    }
}

hipError_t launch_convolve(float *img, float *tmp, uint32_t n_img, uint32_t E, uint32_t R, const ConvTaps &taps, hipStream_t st)
{
    const size_t n = (size_t)n_img * E * R;
    hipLaunchKernelGGL(k_conv_axial, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float *)img, tmp, n_img, E, R, taps);
    launch_conv_lateral(tmp, img, n_img, E, R, taps, nullptr, st);
    return hipGetLastError();
}

hipError_t launch_convolve_depth(float *img, float *tmp, uint32_t n_img, uint32_t E, uint32_t R, const ConvTaps &taps, const float *lat, hipStream_t st)
{
    const size_t n = (size_t)n_img * E * R;
    hipLaunchKernelGGL(k_conv_axial, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float *)img, tmp, n_img, E, R, taps);
    launch_conv_lateral(tmp, img, n_img, E, R, taps, lat, st);
    return hipGetLastError();
}

hipError_t launch_convolve_bands(const float *rf, float *tmp, float *bands, uint32_t F, uint32_t B, uint32_t E, uint32_t R, const ConvTaps &taps,
                                 const float *ax, const float *lat, hipStream_t st)
{
    const uint32_t n_strips = (E + MCRT_BANDS_STRIP - 1u) / MCRT_BANDS_STRIP;
    const size_t m = (size_t)F * n_strips * R;
    hipLaunchKernelGGL(k_conv_axial_bands, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, rf, tmp, bands, F, B, E, R, taps.n_ax, n_strips, ax);
    launch_conv_lateral(tmp, bands, F * B, E, R, taps, lat, st);
    return hipGetLastError();
}

hipError_t launch_elevation(const float *planes, float *rf, uint32_t F, uint32_t K, uint32_t E, uint32_t R, const float *w, hipStream_t st)
{
    const size_t ER = (size_t)E * R;
    const bool vec = (ER % 4u) == 0u && ((uintptr_t)planes % 16u) == 0u && ((uintptr_t)rf % 16u) == 0u;   // every plane then starts 16-byte aligned
    const size_t nv = vec ? ER / 4u : ER, n = (size_t)F * nv;
    const dim3 grid((unsigned)((n + 255) / 256)), blk(256);
    if (vec) hipLaunchKernelGGL((k_elevation<float4>), grid, blk, 0, st, (const float4 *)planes, (float4 *)rf, F, K, nv, R, w);
    else hipLaunchKernelGGL((k_elevation<float>), grid, blk, 0, st, planes, rf, F, K, nv, R, w);
    return hipGetLastError();
}

hipError_t launch_envelope(float *img, uint32_t E, uint32_t R, hipStream_t st)
{
    hipLaunchKernelGGL(k_envelope, dim3(E), dim3(64), 0, st, img, E, R);
    return hipGetLastError();
}

hipError_t launch_remap(const float *img, uint32_t n_img, uint32_t E, uint32_t R, const float *map_col, const float *map_row, float *out, uint32_t n, hipStream_t st)
{
    hipLaunchKernelGGL(k_remap, dim3((n + 255) / 256, n_img), dim3(256), 0, st, img, E, R, map_col, map_row, out, n);
    return hipGetLastError();
}

hipError_t launch_blocks_to_frames(const float *blocks, float *frames, uint32_t F, uint32_t E, uint32_t R, uint32_t G, const uint32_t *off, hipStream_t st)
{
    GroupOffsets o;
    for (uint32_t g = 0; g <= G && g < 65u; g++) o.off[g] = off[g];
    const bool vec = (R % 4u) == 0u && ((uintptr_t)blocks % 16u) == 0u && ((uintptr_t)frames % 16u) == 0u;
    const uint32_t Rv = vec ? R / 4u : R;
    const size_t n = (size_t)F * E * Rv;
    if (vec) hipLaunchKernelGGL((k_blocks_to_frames<float4>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float4 *)blocks, (float4 *)frames, F, E, Rv, G, o);
    else hipLaunchKernelGGL((k_blocks_to_frames<float>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, blocks, frames, F, E, Rv, G, o);
    return hipGetLastError();
}

hipError_t launch_transpose(const float *in, float *out, uint32_t E, uint32_t R, hipStream_t st)
{
    hipLaunchKernelGGL(k_transpose, dim3((R + 31) / 32, (E + 31) / 32), dim3(32, 8), 0, st, in, out, E, R);
    return hipGetLastError();
}

}  // namespace mcrt
