// mcrt_warp.h -- the ONE reading of an analytic line at a sub-row displacement (the contract of mcrt_strain_compress_frames in
// include/mcrt.h): the two neighbouring samples, each turned by the carrier phase of its fractional offset through the rotor table, then
// the linear interpolation.  k_strain_warp (mcrt_strain.hip) and k_shear_track (mcrt_shear.hip) both read their lines through it.
#pragma once
#include "mcrt_device.h"

namespace mcrt {

// (c, s) of theta in 2^-32 turn from the rotor table, and z turned by it: mcrt_spectral_series_frames' index and product
MCRT_DEV float2 strain_turn(float2 z, uint32_t theta, const float2 *lut)
{
    const float2 cs = lut[((theta + 0x80000u) >> 20) & 4095u];
    const float rc = z.x * cs.x, is = z.y * cs.y, rs = z.x * cs.y, ic = z.y * cs.x;
    return make_float2(rc - is, rs + ic);
}

// the line read at row q + U * 2^-24: pre[i - base] holds row i for the rows the caller staged (every row in [0, R) that
// q + (U >> 24) and the next one can name); rows outside [0, R) read as (+0.0f, +0.0f).  Every float operation is rounded once.
MCRT_DEV float2 warp_read(const float2 *pre, int32_t base, int32_t R, int32_t q, int32_t U, long long carrier, const float2 *lut)
{
    const int32_t s0 = q + (U >> 24), fr = U & 0xFFFFFF;      // s = (q << 24) + U: its whole rows and its fraction
    const float2 zero = make_float2(0.0f, 0.0f);
    const float2 A = s0 >= 0 && s0 < R ? pre[s0 - base] : zero;
    const float2 B = s0 + 1 >= 0 && s0 + 1 < R ? pre[s0 + 1 - base] : zero;
    const float w1 = (float)fr * 0x1p-24f, w0 = 1.0f - w1;
    const uint32_t th0 = (uint32_t)((carrier * (long long)fr) >> 24);
    const uint32_t th1 = (uint32_t)((carrier * ((long long)fr - (1ll << 24))) >> 24);
    const float2 ra = strain_turn(A, th0, lut), rb = strain_turn(B, th1, lut);
    return make_float2(w0 * ra.x + w1 * rb.x, w0 * ra.y + w1 * rb.y);
}

// the two Irwin-Hall sums of one Philox block (mcrt_flow_draws'): |d| < 2^24, so the conversions to float are exact
MCRT_DEV void irwin_hall(const uint32_t o[4], int32_t &di, int32_t &dq)
{
    di = (int32_t)(((o[0] & 0xffffu) + (o[0] >> 16)) + ((o[1] & 0xffffu) + (o[1] >> 16))) - 131070;
    dq = (int32_t)(((o[2] & 0xffffu) + (o[2] >> 16)) + ((o[3] & 0xffffu) + (o[3] >> 16))) - 131070;
}

}  // namespace mcrt
