// mcrt_strain.hip -- strain elastography (mcrt_strain_compress_frames, mcrt_strain_frames, mcrt_elastogram_frames; contracts in include/mcrt.h):
// k_strain_warp compresses every scan-line as a column of springs and reads the post-compression analytic line out of the pre-compression
// one; k_strain_track finds each sample's displacement by normalised complex cross-correlation over a window and a range of lags, with
// the sub-sample part from the phase of the winning correlation; k_strain_slope takes the least-squares slope of the displacement;
// k_elastogram lays the gathered strain over the B-mode picture.  The reference has no counterpart.
#include "mcrt_device.h"
#include "mcrt_pixels.h"
#include "mcrt_warp.h"              // warp_read: the reading of a line at a sub-row displacement, shared with mcrt_shear.hip

namespace mcrt {

// ONE wavefront is the workgroup and owns one scan-line: the pre-compression line sits in its LDS (8 R bytes, 16 KB at the most), because
// row q reads the rows q + U(q) >> 24 and the next one, wherever the displacement sends them; the launch sizes it by R, so that short
// lines do not pay the occupancy of the longest.  The displacement is the running sum of the rows' strains -- integers, so the order of
// the sum is free: per chunk of 64 rows a lane looks its row's strain up by its label (the table, at most 254 words, stays in the vector
// cache), six shuffle steps give the inclusive sum and the chunk's total is carried in a scalar.  Every float operation is the
// contract's, rounded once (compiled -ffp-contract=off).
__global__ void __launch_bounds__(64) k_strain_warp(StrainWarpArgs a)
{
    extern __shared__ float2 pre[];
    const uint32_t lane = threadIdx.x, line = blockIdx.x, R = a.R;
    const uint32_t f = line / a.E, e = line - f * a.E;
    const float2 *src = a.iq + (size_t)line * R;
    const uint8_t *tissue = a.tissue + (size_t)line * R;
    for (uint32_t q = lane; q < R; q += 64u) pre[q] = src[q];
    __syncthreads();
    const float sigma = a.sigma_dev ? a.sigma_dev[f] : a.sigma;
    const float k = sigma * a.inv_std;
    const long long carrier = a.carrier_q32;
    int32_t carry = 0;
    for (uint32_t q0 = 0; q0 < R; q0 += 64u) {
        const uint32_t q = q0 + lane;
        const bool in = q < R;
        const uint32_t l = in ? tissue[q] : 255u;
        const int32_t eps = l < a.n_labels ? a.eps[l] : 0;
        int32_t incl = eps;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int32_t up = __shfl_up(incl, d);
            if ((int)lane >= d) incl += up;
        }
        const int32_t U = carry + (incl - eps);
        carry += __builtin_amdgcn_readlane(incl, 63);
        if (!in) continue;
        const size_t at = (size_t)line * R + q;
        if (a.truth_disp) a.truth_disp[at] = (float)U * 0x1p-24f;
        if (a.truth_strain) a.truth_strain[at] = (float)eps * 0x1p-24f;
        if (!a.post) continue;
        const float2 x = warp_read(pre, 0, (int32_t)R, (int32_t)q, U, carrier, a.lut);
        float xr = x.x, xi = x.y;
        if (k != 0.0f) {
            uint32_t o[4];
            philox4x32_10(e, q, 0x5354524Eu, 0u, a.seed, a.first_id + f, o);
            int32_t di, dq;
            irwin_hall(o, di, dq);
            xr = xr + k * (float)di; xi = xi + k * (float)dq;
        }
        a.post[at] = make_float2(xr, xi);
    }
}

// one workgroup of one wavefront per scan-line (the stack has fewer than 2^31 samples: so has the grid)
hipError_t launch_strain_warp(const StrainWarpArgs &a, hipStream_t st)
{
    if (a.lines == 0u || a.R == 0u || a.R > MCRT_MAX_ROWS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_strain_warp, dim3(a.lines), dim3(64), (size_t)a.R * sizeof(float2), st, a);
    return hipGetLastError();
}

// THE TILING.  ONE wavefront is the workgroup and owns STRAIN_TILE_ROWS = 64 consecutive rows of one scan-line, a lane one of them.  It
// stages the rows its lanes touch -- the pre line with a halo of a rows, the post line with a halo of a + L rows, 8 bytes a row -- and the
// post line's window energies P for its rows and L more on either side into its LDS: 2.7 KB at the largest window, which leaves the
// occupancy to the registers, where two whole 2048-row lines per wavefront (32 KB) would hold a CU to five wavefronts; the halo costs
// (64 + 2 a + 2 L) / 64 = 1.75 x the loads of whole lines at the defaults, all of them hits in the vector cache or the L2, against a
// search of (2 L + 1)(2 a + 1) = 561 complex multiply-adds per sample.  Rows outside the line are SKIPPED, not read as zeros (an infinity
// times zero would be a NaN): the window of a lane at lag k is the run of taps [lo, hi] with both rows inside, a lane's own loop bounds.
// The lags -m and +m share the pre row of a tap: three 8-byte LDS reads feed two complex multiply-adds.  The loops over the window and
// the lags are bounded at run time (a, L are options); nothing is indexed out of registers, so there is no scratch.  Every float
// operation is the contract's, rounded once (compiled -ffp-contract=off).
struct StrainBest { float re, im, rho2; int32_t k; };

// candidate k of a lane: c_k = (re, im), e1 the pre window's energy, p the post window's at row r + k; strictly greater replaces
MCRT_DEV void strain_candidate(StrainBest &best, float re, float im, float e1, float p, int32_t k, bool valid, bool first)
{
    const float rr = re * re, ii = im * im;
    const float rho2 = (rr + ii) / (e1 * p);
    if (first || (valid && rho2 > best.rho2)) { best.re = re; best.im = im; best.rho2 = rho2; best.k = k; }
}

__global__ void __launch_bounds__(64) k_strain_track(StrainTrackArgs a)
{
    __shared__ float2 pre[STRAIN_TILE_ROWS + 2u * STRAIN_MAX_WINDOW];
    __shared__ float2 post[STRAIN_TILE_ROWS + 2u * (STRAIN_MAX_WINDOW + STRAIN_MAX_SEARCH)];
    __shared__ float P[STRAIN_TILE_ROWS + 2u * STRAIN_MAX_SEARCH];
    const int32_t lane = (int32_t)threadIdx.x, R = (int32_t)a.R, aw = (int32_t)a.window, L = (int32_t)a.search;
    const uint32_t line = blockIdx.x / a.chunks, chunk = blockIdx.x - line * a.chunks;
    const int32_t r0 = (int32_t)(chunk * STRAIN_TILE_ROWS), r = r0 + lane;
    const float2 *src_pre = a.pre + (size_t)line * a.R, *src_post = a.post + (size_t)line * a.R;
    // pre[j] is row r0 - aw + j, post[j] row r0 - aw - L + j: rows outside the line are never read back, they stay unwritten
    for (int32_t j = lane; j < (int32_t)STRAIN_TILE_ROWS + 2 * aw; j += 64) {
        const int32_t q = r0 - aw + j;
        if (q >= 0 && q < R) pre[j] = src_pre[q];
    }
    for (int32_t j = lane; j < (int32_t)STRAIN_TILE_ROWS + 2 * (aw + L); j += 64) {
        const int32_t q = r0 - aw - L + j;
        if (q >= 0 && q < R) post[j] = src_post[q];
    }
    __syncthreads();
    // P[j]: the energy of the post window about row r0 - L + j
    for (int32_t j = lane; j < (int32_t)STRAIN_TILE_ROWS + 2 * L; j += 64) {
        const int32_t q = r0 - L + j;
        if (q < 0 || q >= R) continue;
        const int32_t lo = max(-aw, -q), hi = min(aw, R - 1 - q);
        float s = 0.0f;
        for (int32_t i = lo; i <= hi; i++) {
            const float2 v = post[j + aw + i];
            const float rr = v.x * v.x, ii = v.y * v.y;
            s = s + (rr + ii);
        }
        P[j] = s;
    }
    __syncthreads();
    if (r >= R) return;
    const float2 *mine = pre + lane + aw;            // mine[i]: pre row r + i
    const float2 *theirs = post + lane + aw + L;     // theirs[i]: post row r + i
    float e1 = 0.0f;
    StrainBest best;
    {
        const int32_t lo = max(-aw, -r), hi = min(aw, R - 1 - r);
        float re = 0.0f, im = 0.0f;
        for (int32_t i = lo; i <= hi; i++) {
            const float2 u = mine[i], v = theirs[i];
            const float uu = u.x * u.x, vv = u.y * u.y;
            e1 = e1 + (uu + vv);
            const float ac = v.x * u.x, bd = v.y * u.y, bc = v.y * u.x, ad = v.x * u.y;
            re = re + (ac + bd); im = im + (bc - ad);
        }
        strain_candidate(best, re, im, e1, P[lane + L], 0, true, true);
    }
    for (int32_t m = 1; m <= L; m++) {
        // the taps of lag -m are [lo_n, hi_n], those of lag +m [lo_p, hi_p]: both rows of a tap inside the line
        const int32_t lo_n = max(-aw, m - r), hi_n = min(aw, R - 1 - r);
        const int32_t lo_p = max(-aw, -r), hi_p = min(aw, R - 1 - r - m);
        float nre = 0.0f, nim = 0.0f, pre_ = 0.0f, pim = 0.0f;
        for (int32_t i = min(lo_n, lo_p); i <= max(hi_n, hi_p); i++) {
            const float2 u = mine[i];
            if (i >= lo_n && i <= hi_n) {
                const float2 v = theirs[i - m];
                const float ac = v.x * u.x, bd = v.y * u.y, bc = v.y * u.x, ad = v.x * u.y;
                nre = nre + (ac + bd); nim = nim + (bc - ad);
            }
            if (i >= lo_p && i <= hi_p) {
                const float2 v = theirs[i + m];
                const float ac = v.x * u.x, bd = v.y * u.y, bc = v.y * u.x, ad = v.x * u.y;
                pre_ = pre_ + (ac + bd); pim = pim + (bc - ad);
            }
        }
        const bool vn = r - m >= 0, vp = r + m < R;
        strain_candidate(best, nre, nim, e1, vn ? P[lane + L - m] : 0.0f, -m, vn, false);
        strain_candidate(best, pre_, pim, e1, vp ? P[lane + L + m] : 0.0f, m, vp, false);
    }
    const size_t at = (size_t)line * a.R + (size_t)r;
    a.disp[at] = det_atan2f(best.im, best.re) * a.scale - (float)best.k;
    if (a.rho) a.rho[at] = sqrtf(best.rho2);
}

// The slope, k_flow_avg's layout: a lane owns a row, its 2 g + 1 reads of the displacement are coalesced across the wavefront and hit the
// vector cache.  Both sums ascend over the rows of the clipped window.
__global__ void __launch_bounds__(256) k_strain_slope(StrainTrackArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    const uint32_t line = w / a.chunks, chunk = w - line * a.chunks;
    if (line >= a.lines) return;
    const int32_t R = (int32_t)a.R, g = (int32_t)a.lsq, r = (int32_t)(chunk * STRAIN_TILE_ROWS + lane);
    if (r >= R) return;
    const float *d = a.disp + (size_t)line * a.R;
    const int32_t j_lo = max(0, r - g), j_hi = min(R - 1, r + g);
    float num = 0.0f, den = 0.0f;
    for (int32_t j = j_lo; j <= j_hi; j++) {
        const float t = (float)(2 * j - (j_lo + j_hi));
        num = num + t * d[j]; den = den + t * t;
    }
    a.strain[(size_t)line * a.R + (size_t)r] = j_lo == j_hi ? 0.0f : (2.0f * num) / den;
}

// one wavefront per (scan-line, tile of 64 rows) (the stack has fewer than 2^31 samples: so has the grid); the slope in stream order
hipError_t launch_strain_track(const StrainTrackArgs &a, hipStream_t st)
{
    if (a.lines == 0u || a.chunks == 0u || a.window > STRAIN_MAX_WINDOW || a.search > STRAIN_MAX_SEARCH || !a.disp) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_strain_track, dim3(a.lines * a.chunks), dim3(64), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !a.strain) return e;
    hipLaunchKernelGGL(k_strain_slope, dim3((a.lines * a.chunks + 3u) / 4u), dim3(256), 0, st, a);
    return hipGetLastError();
}

// The overlay over the pixel tile (mcrt_pixels.h): a lane owns the points p0 + 64 j of a picture, so the two planes and the grey bytes
// are read as neighbouring words of neighbouring lanes; the three bytes of a pixel leave one by one, as k_colour's do (a wavefront's 192
// bytes are contiguous; laid out in LDS and stored as aligned words they took 9.7 us at 400 x 500 against 9.8: not kept).  The colour
// table is 256 floats of the context's, each the exact integer r | g << 8 | b << 16.
__global__ void __launch_bounds__(256) k_elastogram(ElastogramArgs a)
{
    PixelTile tile;
    if (!pixel_tile(a.pass, tile)) return;
    const uint32_t n = a.pass.n;
    for (uint32_t f = tile.f0; f < tile.f1; f++) {
        const float *strain = a.strain + (size_t)f * n, *rho = a.rho + (size_t)f * n;
        const uint8_t *grey = a.grey + (size_t)f * n;
        uint8_t *rgb = a.rgb + (size_t)f * 3u * n;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t p = tile.p0 + 64u * j;
            if (p >= n) continue;
            const uint32_t g = grey[p];
            const float x = strain[p] / a.ref_strain, t = rintf(x * 128.0f);
            const bool show = x == x && rho[p] >= a.rho_min && g >= a.grey_min;      // (a NaN compares false)
            uint32_t c = g | g << 8 | g << 16;
            if (show) {
                const uint32_t idx = t < 0.0f ? 0u : t > 255.0f ? 255u : (uint32_t)t;
                const uint32_t l = (uint32_t)a.lut[idx], ga = g * (256u - a.alpha) + 128u;
                c = ((ga + (l & 0xffu) * a.alpha) >> 8) | ((ga + ((l >> 8) & 0xffu) * a.alpha) >> 8) << 8 | ((ga + (l >> 16) * a.alpha) >> 8) << 16;
            }
            rgb[3u * (size_t)p] = (uint8_t)c; rgb[3u * (size_t)p + 1u] = (uint8_t)(c >> 8); rgb[3u * (size_t)p + 2u] = (uint8_t)(c >> 16);
        }
    }
}

hipError_t launch_elastogram(const ElastogramArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(k_elastogram, pixel_grid(a.pass), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace mcrt
