// mcrt_detect.hip -- quadrature detection (mcrt_detect_frames; contract in include/mcrt.h): k_detect, an FIR Hilbert transformer along every
// scan-line of the RF stack [lines][R] -> the envelope sqrt(x^2 + q^2) and / or the analytic pair (x, q).  The reference has no counterpart: its
// rf_image::envelope (k_envelope, mcrt_post.hip) joins the local maxima of the samples.
#include "mcrt_device.h"

namespace mcrt {

#ifndef MCRT_DETECT_WAVES
#define MCRT_DETECT_WAVES 4u          // wavefronts (scan-lines in flight) per workgroup
#endif
#define DETECT_PAD 32u                // zeros staged before and after a scan-line: the largest reach of the taps is 31 rows

// k_envelope's shape: a WAVEFRONT owns a scan-line and stages it in LDS between DETECT_PAD zeros on either side -- the contract's xz --, so
// that no tap needs a bounds test and env may be rf (the whole line is read before a row of it is written; the other wavefronts own other
// lines).  Lane l takes the rows l, l + 64, ...: neighbouring lanes read neighbouring LDS words at every offset r - m and r + m, which is
// free of bank conflicts.  The taps are kernel arguments (scalar registers) and NT, the number of them, is the instantiation: the tap loop
// is unrolled in full, without a test.  The sum runs over m = 1, 3, 5, ... in ascending order from 0.0f, the difference, every multiply
// and every add rounded once (compiled -ffp-contract=off); sqrtf is the correctly rounded one.  A workgroup's wavefronts stride over the
// lines, so that any number of lines fits a grid.  LDS: blockDim.x / 64 * (R + 2 * DETECT_PAD) floats, dynamic.  No scratch.
template <uint32_t NT>
__global__ void __launch_bounds__(MCRT_DETECT_WAVES * 64u) k_detect(DetectArgs a)
{
    extern __shared__ float detect_lds[];
    const uint32_t lane = threadIdx.x & 63u, R = a.R;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), waves = blockDim.x >> 6;
    float *s = detect_lds + (size_t)wave * (R + 2u * DETECT_PAD);
    s[lane < DETECT_PAD ? lane : R + lane] = 0.0f;             // lanes 0..31: the zeros before the line, lanes 32..63: the zeros after it
    s += DETECT_PAD;
    for (size_t line = (size_t)blockIdx.x * waves + wave; line < a.lines; line += (size_t)gridDim.x * waves) {
        const float *x = a.rf + line * R;
        for (uint32_t r = lane; r < R; r += 64u) s[r] = x[r];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier();
        for (uint32_t r = lane; r < R; r += 64u) {
            const float *p = s + r;
            float q = 0.0f;
#pragma unroll
            for (uint32_t k = 0; k < NT; k++) {
                const uint32_t m = 2u * k + 1u;
                const float d = p[-(int)m] - p[m];
                q = q + d * a.t[k];
            }
            const float v = p[0];
            if (a.env) { const float xx = v * v, qq = q * q; a.env[line * R + r] = sqrtf(xx + qq); }
            if (a.iq) a.iq[line * R + r] = make_float2(v, q);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier();      // the next line overwrites s
    }
}

hipError_t launch_detect(const DetectArgs &a, hipStream_t st)
{
    const uint32_t waves = MCRT_DETECT_WAVES;
    const size_t blocks = (a.lines + waves - 1u) / waves;
    const size_t lds = (size_t)waves * (a.R + 2u * DETECT_PAD) * sizeof(float);
    const dim3 grid((unsigned)(blocks < 0x100000u ? blocks : 0x100000u)), blk(waves * 64u);
    switch (a.nt) {
#define DETECT_CASE(NT) case NT: hipLaunchKernelGGL(k_detect<NT>, grid, blk, lds, st, a); break;
    DETECT_CASE(1) DETECT_CASE(2) DETECT_CASE(3) DETECT_CASE(4) DETECT_CASE(5) DETECT_CASE(6) DETECT_CASE(7) DETECT_CASE(8)
    DETECT_CASE(9) DETECT_CASE(10) DETECT_CASE(11) DETECT_CASE(12) DETECT_CASE(13) DETECT_CASE(14) DETECT_CASE(15) DETECT_CASE(16)
#undef DETECT_CASE
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace mcrt
