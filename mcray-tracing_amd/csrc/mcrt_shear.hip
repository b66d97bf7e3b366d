// mcrt_shear.hip -- shear-wave elastography (mcrt_shear_wave_frames, mcrt_shear_speed_frames; contracts in include/mcrt.h):
// k_shear_arrival walks every RF row outwards from the pushed scan-line and sums the integer crossing costs into arrival ticks;
// k_shear_track synthesises the T tracking lines of a tile from the pre line and the arrivals, estimates each pulse's displacement from
// the phase of the lag-0 correlation and keeps the time to peak; k_shear_speed takes the least-squares slope of the time to peak across
// scan-lines and turns it into a speed, a modulus and a quality.  The reference has no counterpart.
#include "mcrt_device.h"
#include "mcrt_warp.h"

namespace mcrt {

// the ticks a crossing costs that leaves a sample of this slowness in a row of this pitch (slow < 2^38 + 1, pitch < 2^24: below 2^62)
MCRT_DEV long long shear_cost(long long slow, long long pitch)
{
    return slow != 0 ? (slow * pitch) >> 24 : SHEAR_NEVER;
}

// One wavefront owns 64 consecutive rows of one frame and one direction (blockIdx & 1: 0 walks from the pushed line to line E - 1 and
// writes the pushed line itself, 1 from its left neighbour down to line 0); a lane owns a row, so the byte loads of a step are
// neighbouring and so are the stores.  The walk over the lines is serial in the sum and in nothing else: the labels of the next
// SHEAR_WALK_AHEAD lines are loaded while those of the last are added, and the two tables they index (at most 254 entries each) sit in
// LDS.  At 1 x 512 x 465 the walk takes 70 us whether 4, 8 or 32 lines are in flight: 16 wavefronts, one to a SIMD, each with 256
// dependent steps of a 64-bit product, two LDS lookups and three stores -- the chain, not the loads, is what it waits for.
#define SHEAR_WALK_AHEAD 8
__global__ void __launch_bounds__(64) k_shear_arrival(ShearWaveArgs a)
{
    __shared__ long long slow[256];
    __shared__ float spd[256];
    const uint32_t lane = threadIdx.x;
    for (uint32_t l = lane; l < 256u; l += 64u) {
        slow[l] = l < a.n_labels ? a.slow[l] : 0ll;
        spd[l] = l < a.n_labels ? a.speed_f[l] : 0.0f;
    }
    __syncthreads();
    const uint32_t dir = blockIdx.x & 1u, w = blockIdx.x >> 1, f = w / a.chunks, chunk = w - f * a.chunks;
    const uint32_t r = chunk * SHEAR_TILE_ROWS + lane, R = a.R, p = a.push_line;
    if (r >= R || (dir == 1u && p == 0u)) return;
    const size_t plane = (size_t)f * a.E * R + r;
    const uint8_t *tissue = a.tissue + plane;
    const long long pitch = (long long)a.pitch[r];
    long long A = dir == 0u ? 0ll : shear_cost(slow[tissue[(size_t)p * R]], pitch);
    const int32_t step = dir == 0u ? 1 : -1;
    int32_t e = dir == 0u ? (int32_t)p : (int32_t)p - 1, left = dir == 0u ? (int32_t)(a.E - p) : (int32_t)p;
    uint32_t l[SHEAR_WALK_AHEAD], ahead[SHEAR_WALK_AHEAD];
#pragma unroll
    for (int i = 0; i < SHEAR_WALK_AHEAD; i++) l[i] = i < left ? tissue[(size_t)(e + i * step) * R] : 255u;
    while (left > 0) {
        // the next lines' labels are on their way while these are added
#pragma unroll
        for (int i = 0; i < SHEAR_WALK_AHEAD; i++) ahead[i] = SHEAR_WALK_AHEAD + i < left ? tissue[(size_t)(e + (SHEAR_WALK_AHEAD + i) * step) * R] : 255u;
#pragma unroll
        for (int i = 0; i < SHEAR_WALK_AHEAD; i++) {
            if (i >= left) break;
            const size_t at = plane + (size_t)(e + i * step) * R;
            a.arrival[at] = A;
            if (a.truth_arrival) a.truth_arrival[at] = A >= SHEAR_NEVER ? __builtin_inff() : (float)A * 0x1p-16f;
            if (a.truth_speed) a.truth_speed[at] = spd[l[i]];
            const long long next = A + shear_cost(slow[l[i]], pitch);
            A = next < SHEAR_NEVER ? next : SHEAR_NEVER;
        }
#pragma unroll
        for (int i = 0; i < SHEAR_WALK_AHEAD; i++) l[i] = ahead[i];
        e += SHEAR_WALK_AHEAD * step; left -= SHEAR_WALK_AHEAD;
    }
}

// pulse n's line at row q of scan-line e: the pre line read at q + u, u the particle displacement of the contract, plus the receiver noise
MCRT_DEV float2 shear_line(const ShearWaveArgs &a, const float2 *pre, int32_t base, int32_t q, long long A, int32_t pa, uint32_t n, uint32_t e, uint32_t id, float k)
{
    const long long t = ((long long)n << 16) - A, idx = t >> SHEAR_SHAPE_SHIFT;
    int32_t u = 0;
    if (q >= (int32_t)a.row0 && q < (int32_t)a.row1 && A < SHEAR_NEVER && t >= 0 && idx < (long long)a.n_shape)
        u = (int32_t)(((long long)pa * (long long)a.shape[idx]) >> 16);
    float2 x = warp_read(pre, base, (int32_t)a.R, q, u, a.carrier_q32, a.lut);
    if (k != 0.0f) {
        uint32_t o[4];
        philox4x32_10(e, (uint32_t)q, 0x53484552u, n, a.seed, id, o);
        int32_t di, dq;
        irwin_hall(o, di, dq);
        x.x = x.x + k * (float)di; x.y = x.y + k * (float)dq;
    }
    return x;
}

// THE TILING is k_strain_track's: ONE wavefront is the workgroup and owns SHEAR_TILE_ROWS = 64 consecutive rows of one scan-line, a lane
// one of them.  The pre line's rows the tile touches -- its 64 rows, the window's halo of a rows and one more on either side, because a
// displacement below one row reads the row before or after -- sit in LDS, and so do two copies of the tracking line (64 + 2 a rows):
// pulse n is written into copy n & 1 while the lanes that are behind still read pulse n - 1, which leaves one barrier per pulse.  Per
// pulse a lane synthesises its own row and, if it is one of the first 2 a lanes, one halo row (the halo costs (64 + 2 a) / 64 = 1.25 x the
// warps at the default window, against 2 a + 1 = 17 complex multiply-adds per sample and pulse), then sums its window out of LDS.
// The arrival ticks of a lane's two rows stay in registers for all T pulses; the T estimates are never stored unless the movie is asked
// for: a lane keeps the running maximum and the estimates beside it.  T, a and the pushed rows are run-time bounds; nothing is indexed
// out of registers, so there is no scratch.  LDS: 8 x (98 + 2 x 96) = 2320 bytes, which bounds nothing; 68 VGPRs (the Philox rounds of two
// rows and the deterministic atan2 are live together) leave 7 of the 8 wavefronts a SIMD can hold.  Every float operation is the
// contract's, rounded once (compiled -ffp-contract=off).
__global__ void __launch_bounds__(64) k_shear_track(ShearWaveArgs a)
{
    __shared__ float2 pre[SHEAR_TILE_ROWS + 2u * SHEAR_MAX_WINDOW + 2u];
    __shared__ float2 z[2][SHEAR_TILE_ROWS + 2u * SHEAR_MAX_WINDOW];
    const int32_t lane = (int32_t)threadIdx.x, R = (int32_t)a.R, aw = (int32_t)a.window;
    const uint32_t line = blockIdx.x / a.chunks, chunk = blockIdx.x - line * a.chunks, f = line / a.E, e = line - f * a.E, T = a.T;
    const int32_t r0 = (int32_t)(chunk * SHEAR_TILE_ROWS), r = r0 + lane, base = r0 - aw - 1;
    const float2 *src = a.iq + (size_t)line * a.R;
    // pre[j] is row base + j, z[.][j] row r0 - aw + j: rows outside the line are never read back, they stay unwritten
    for (int32_t j = lane; j < (int32_t)SHEAR_TILE_ROWS + 2 * aw + 2; j += 64) {
        const int32_t q = base + j;
        if (q >= 0 && q < R) pre[j] = src[q];
    }
    // the rows this lane synthesises: q0 always (if it is inside the line), q1 in the first 2 a lanes
    const long long *arr = a.arrival + (size_t)line * a.R;
    const int32_t q0 = r0 - aw + lane, q1 = q0 + 64;
    const bool own0 = q0 >= 0 && q0 < R, own1 = lane < 2 * aw && q1 < R;
    const long long A0 = own0 ? arr[q0] : SHEAR_NEVER, A1 = own1 ? arr[q1] : SHEAR_NEVER;
    const uint32_t dist = e > a.push_line ? e - a.push_line : a.push_line - e;
    const int32_t pa = (int32_t)(((long long)a.peak_q24 * (long long)(dist < a.n_amp ? a.amp[dist] : 0u)) >> 16);
    const float sigma = a.sigma_dev ? a.sigma_dev[f] : a.sigma;
    const float k = sigma * a.inv_std;
    const uint32_t id = a.first_id + f;
    __syncthreads();
    const bool mine = r < R;
    const int32_t lo = max(-aw, -r), hi = min(aw, R - 1 - r);
    const float2 *pw = pre + lane + aw + 1;          // pw[i]: pre row r + i
    float best = 0.0f, um = 0.0f, up = 0.0f, prev = 0.0f;
    uint32_t bn = 0u;
    bool pending = false;
    for (uint32_t n = 0; n < T; n++) {
        float2 *zn = z[n & 1u];
        if (own0) zn[lane] = shear_line(a, pre, base, q0, A0, pa, n, e, id, k);
        if (own1) zn[lane + 64] = shear_line(a, pre, base, q1, A1, pa, n, e, id, k);
        __syncthreads();
        if (!mine) continue;
        const float2 *zw = zn + lane + aw;           // zw[i]: this pulse's row r + i
        float re = 0.0f, im = 0.0f;
        for (int32_t i = lo; i <= hi; i++) {
            const float2 u = pw[i], v = zw[i];
            const float ac = v.x * u.x, bd = v.y * u.y, bc = v.y * u.x, ad = v.x * u.y;
            re = re + (ac + bd); im = im + (bc - ad);
        }
        const float d = det_atan2f(im, re) * a.scale;
        if (a.disp) a.disp[(((size_t)f * T + n) * a.E + e) * a.R + (size_t)r] = d;
        if (pending) { up = d; pending = false; }
        if (n == 0u || d > best) { best = d; bn = n; um = prev; pending = true; }     // strictly greater: the first maximum wins, a NaN never does
        prev = d;
    }
    if (!mine) return;
    const size_t at = (size_t)line * a.R + (size_t)r;
    if (a.peak_disp) a.peak_disp[at] = best;
    if (a.peak_time) {
        const float den = (um - 2.0f * best) + up, num = 0.5f * (um - up);
        a.peak_time[at] = bn == 0u || bn == T - 1u || den == 0.0f ? __builtin_nanf("") : (float)bn + num / den;
    }
}

// both kernels, in stream order: one wavefront per (frame, tile of 64 rows, direction), then one per (scan-line, tile of 64 rows) (the
// stack has fewer than 2^31 samples: so have the grids)
hipError_t launch_shear_wave(const ShearWaveArgs &a, hipStream_t st)
{
    if (a.F == 0u || a.E == 0u || a.R == 0u || a.chunks != (a.R + SHEAR_TILE_ROWS - 1u) / SHEAR_TILE_ROWS || a.window > SHEAR_MAX_WINDOW || a.push_line >= a.E ||
        a.row1 > a.R || a.n_labels > 254u || !a.arrival) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_shear_arrival, dim3(a.F * a.chunks * 2u), dim3(64), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || (!a.peak_time && !a.peak_disp && !a.disp)) return e;
    hipLaunchKernelGGL(k_shear_track, dim3(a.F * a.E * a.chunks), dim3(64), 0, st, a);
    return hipGetLastError();
}

// the mean of a scan-line's peak times over the rows [i_lo, i_hi], NaN rows skipped: the sum ascends; no row left gives 0.0f / 0.0f, a NaN
MCRT_DEV float shear_row_mean(const float *pt, int32_t i_lo, int32_t i_hi)
{
    float s = 0.0f;
    uint32_t c = 0u;
    for (int32_t i = i_lo; i <= i_hi; i++) {
        const float v = pt[i];
        if (v == v) { s = s + v; c++; }
    }
    return s / (float)c;
}

// The slope across scan-lines, k_strain_slope's layout turned: a lane owns a row, so its reads of a neighbouring line's rows are coalesced
// across the wavefront and hit the vector cache.  The window's row means are taken twice (once for their mean, once for the sums about it)
// in place of a register array indexed at run time.
__global__ void __launch_bounds__(256) k_shear_speed(ShearSpeedArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    const uint32_t line = w / a.chunks, chunk = w - line * a.chunks;
    if (line >= a.F * a.E) return;
    const int32_t R = (int32_t)a.R, E = (int32_t)a.E, b = (int32_t)a.lines, v = (int32_t)a.avg, p = (int32_t)a.push_line;
    const int32_t r = (int32_t)(chunk * SHEAR_TILE_ROWS + lane);
    if (r >= R) return;
    const uint32_t f = line / a.E;
    const int32_t e = (int32_t)(line - f * a.E);
    const size_t at = (size_t)line * a.R + (size_t)r;
    const float nan = __builtin_nanf("");
    float speed = nan, modulus = nan, quality = 0.0f;
    if (e - b >= 0 && e + b < E && !(e - b <= p && p <= e + b)) {
        const float *pt = a.peak_time + (size_t)f * a.E * a.R;
        const int32_t i_lo = max(0, r - v), i_hi = min(R - 1, r + v);
        float sum = 0.0f;
        bool bad = false;
        for (int32_t j = e - b; j <= e + b; j++) {
            const float y = shear_row_mean(pt + (size_t)j * a.R, i_lo, i_hi);
            bad = bad || !(y == y);
            sum = sum + y;
        }
        const float mean = sum / (float)(2 * b + 1);
        float num = 0.0f, den = 0.0f, syy = 0.0f;
        for (int32_t j = e - b; j <= e + b; j++) {
            const float y = shear_row_mean(pt + (size_t)j * a.R, i_lo, i_hi);
            const float t = (float)(2 * j - 2 * e), dy = y - mean;
            num = num + t * y; den = den + t * t; syy = syy + dy * dy;
        }
        float slope = (2.0f * num) / den;
        if (e < p) slope = -slope;
        if (!bad && slope > 0.0f) {
            speed = (a.pitch_mm[r] * a.kf) / slope;
            modulus = a.d3 * (speed * speed);
            const float r2 = (num * num) / (den * syy);
            quality = r2 > 1.0f ? 1.0f : r2 >= 0.0f ? r2 : 0.0f;
        }
    }
    if (a.speed) a.speed[at] = speed;
    if (a.modulus) a.modulus[at] = modulus;
    if (a.quality) a.quality[at] = quality;
}

// one wavefront per (scan-line, tile of 64 rows), four to a workgroup
hipError_t launch_shear_speed(const ShearSpeedArgs &a, hipStream_t st)
{
    if (a.F == 0u || a.E == 0u || a.R == 0u || a.chunks != (a.R + SHEAR_TILE_ROWS - 1u) / SHEAR_TILE_ROWS || a.lines == 0u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_shear_speed, dim3((a.F * a.E * a.chunks + 3u) / 4u), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace mcrt
