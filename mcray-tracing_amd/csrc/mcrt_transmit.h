// mcrt_transmit.h -- the impedance rule of one boundary crossing (mcrt_transmit_boundary's contract in include/mcrt.h; shade_path's own lines
// in mcrt_shade.h, without the random normal), ONE text for the host entry point (mcrt_host.cpp, plain C++) and k_transmit
// (mcrt_transmit.hip).  Every operation is rounded on its own: both sides are compiled with -ffp-contract=off.
#pragma once
#include <math.h>

#if defined(__HIP__) || defined(__HIPCC__)
#define MCRT_TRANSMIT_FN __host__ __device__ inline
#else
#define MCRT_TRANSMIT_FN inline
#endif

namespace mcrt {

MCRT_TRANSMIT_FN void transmit_boundary(float z1, float z2, float inc, float intensity, float &i_refl, float &i_refr)
{
    const float rr = z1 / z2;
    float refa = 1 - rr * rr * (1 - inc * inc);
    if (refa < 0) { i_refl = intensity; i_refr = 0.0f; return; }      // total internal reflection
    refa = sqrtf(refa);
    const float num = z1 * inc - z2 * refa;
    const float den = z1 * inc + z2 * refa;
    const float qq = num / den;
    i_refl = (float)((double)intensity * ((double)qq * (double)qq));
    i_refr = intensity - i_refl;
}

}  // namespace mcrt
