// mcrt_noise.hip -- receiver noise (mcrt_noise_frames; contract in include/mcrt.h): k_noise, a Gaussian noise floor from integer Philox sums
// and a gain per transducer element over the RF stack [F][N][E][R], in place.  The reference has no counterpart.  The frames' peaks
// (MCRT_NOISE_SNR_DB) are k_bmode_peak's (mcrt_display.hip), each frame's N * E scan-lines taken as one image.
#include "mcrt_device.h"

namespace mcrt {

// A wavefront owns NOISE_WAVE_ROWS consecutive rows of one scan-line, a lane NOISE_LANE_ROWS of them: the scan-line e, the image's id, the
// frame's k_f and element_gain[e] are the wavefront's (scalar registers and scalar loads), and a lane's rows are one 16-byte load and store
// where the scan-line's base and R allow -- with R % 4 != 0 every fourth scan-line's, the others' and the ragged end go row by row.  A
// sample costs one Philox4x32-10 block, 20 products of which the high and the low word are taken, against 8 bytes of traffic: the kernel
// is bound by the integer multiplier, not by memory.  The draw is integers only and the float operations are the
// contract's, one rounding each (compiled -ffp-contract=off).  No LDS, no scratch.
__global__ void __launch_bounds__(256) k_noise(NoiseArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    const uint32_t line = w / a.chunks, chunk = w - line * a.chunks;
    if (line >= a.lines) return;
    const uint32_t R = a.R, j = line / a.E, e = line - j * a.E, f = j / a.N;
    const float sigma = a.peak ? a.peak[f] * a.c : a.c;
    const float k = sigma * a.inv_std;
    const bool has_gain = a.gain != nullptr;
    const float g = has_gain ? a.gain[e] : 1.0f;
    if (a.sigma_out && line == f * a.N * a.E && chunk == 0u && lane == 0u) a.sigma_out[f] = sigma;   // the frame's first wavefront
    const uint32_t r0 = chunk * NOISE_WAVE_ROWS + lane * NOISE_LANE_ROWS;
    if (r0 >= R) return;
    const uint32_t cnt = min(NOISE_LANE_ROWS, R - r0), id = a.first_id + j;
    float *p = a.rf + (size_t)line * R + r0;
    const bool vec = cnt == NOISE_LANE_ROWS && (uintptr_t)p % 16u == 0u;
    float v[NOISE_LANE_ROWS];
    if (vec) { const float4 q = *(const float4 *)p; v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
    else {
#pragma unroll
        for (uint32_t i = 0; i < NOISE_LANE_ROWS; i++) v[i] = i < cnt ? p[i] : 0.0f;
    }
#pragma unroll
    for (uint32_t i = 0; i < NOISE_LANE_ROWS; i++) {
        if (i >= cnt) continue;
        uint32_t o[4];
        philox4x32_10(e, r0 + i, 0x4E4F4953u, 0u, a.seed, id, o);
        const uint32_t s = (((o[0] & 0xffffu) + (o[0] >> 16)) + ((o[1] & 0xffffu) + (o[1] >> 16))) + (((o[2] & 0xffffu) + (o[2] >> 16)) + ((o[3] & 0xffffu) + (o[3] >> 16)));
        const int32_t d = (int32_t)s - 262140;              // |d| < 2^24: the conversion is exact
        const float u = has_gain ? v[i] * g : v[i];
        v[i] = k == 0.0f ? u : u + (float)d * k;
    }
    if (vec) *(float4 *)p = make_float4(v[0], v[1], v[2], v[3]);
    else {
#pragma unroll
        for (uint32_t i = 0; i < NOISE_LANE_ROWS; i++)
            if (i < cnt) p[i] = v[i];
    }
}

// one wavefront per (scan-line, chunk of NOISE_WAVE_ROWS rows), four to a workgroup (the stack has fewer than 2^31 samples: so has the grid)
hipError_t launch_noise(const NoiseArgs &a, hipStream_t st)
{
    if (a.lines == 0u || a.chunks == 0u) return hipErrorInvalidValue;
    const uint32_t waves = a.lines * a.chunks;
    hipLaunchKernelGGL(k_noise, dim3((waves + 3u) / 4u), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace mcrt
