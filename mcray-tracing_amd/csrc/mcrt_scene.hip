// mcrt_scene.hip -- scene preparation (k_expand_tris: the walk's triangle records; k_tris_by_id: the same records in id order, for
// k_shade) and the probes through which the tests check the device's contract math (k_math_probe, k_verify_div, k_philox_probe).
#include "mcrt_device.h"

namespace mcrt {

// the walk's leaf-order triangle records once more in triangle-id order, for k_shade (refresh_soa: after every build, update and refit)
__global__ void k_tris_by_id(const float4 *tris, uint32_t n_tri, float4 *out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_tri) return;
    const float4 r0 = tris[MCRT_TRI_PIECES * (size_t)i], r1 = tris[MCRT_TRI_PIECES * (size_t)i + 1], r2 = tris[MCRT_TRI_PIECES * (size_t)i + 2];
    const uint32_t id = __float_as_uint(r0.w);
    if (id >= n_tri) return;
    out[MCRT_TRI_PIECES * (size_t)id] = r0; out[MCRT_TRI_PIECES * (size_t)id + 1] = r1; out[MCRT_TRI_PIECES * (size_t)id + 2] = r2;
}

__global__ void k_expand_tris(const float4 *in, uint32_t n_tri, float4 *out)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tri) return;
    const float4 t0 = in[3 * (size_t)t], t1 = in[3 * (size_t)t + 1], t2 = in[3 * (size_t)t + 2];
    const f3 v0 = xyz(t0), v1 = xyz(t1), v2 = xyz(t2);
    const f3 n = cross(v1 - v0, v2 - v0);
    float4 *o = out + MCRT_TRI_PIECES * (size_t)t;
    o[0] = make_float4(v0.x, v0.y, v0.z, t0.w);
    o[1] = make_float4(v1.x, v1.y, v1.z, t1.w);
    o[2] = make_float4(v2.x, v2.y, v2.z, dot(n, n) * -0.0001f);           // processTriangle's edge tolerance, -1e-4 |n|^2
}

__global__ void k_math_probe(int op, const double *x, const double *y, double *out, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double a = x[i], b = y ? y[i] : 0.0;
    double r = 0.0, s, c;
    switch (op) {
    case 0: r = det_log(a); break;
    case 1: r = det_exp(a); break;
    case 2: det_sincos(a, s, c); r = s; break;
    case 3: det_sincos(a, s, c); r = c; break;
    case 4: r = sqrt(a); break;
    case 5: r = a / b; break;
    case 6: r = (double)det_logf((float)a); break;
    case 7: r = (double)det_expf((float)a); break;
    case 8: r = (double)det_powf((float)a, (float)b); break;
    case 9: r = (double)sqrtf((float)a); break;
    case 10: r = (double)((float)a / (float)b); break;
    case 11: r = det_pow_pos(a, b); break;
    case 12: r = (double)(fix40((float)a) & 0x7fffffffll); break;          // low 31 bits of the fixed-point echo
    case 13: r = (double)(fix40((float)a) >> 31); break;                    // the rest (arithmetic shift)
    default: break;
    }
    out[i] = r;
}

// exhaustive check that the fmaf-corrected reciprocal multiply equals IEEE division by `res` for every float in
// the gate of div_res(); mismatches are counted
__global__ void k_verify_div(float res, float rcp, unsigned long long *bad)
{
    const uint64_t n = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long local = 0;
    for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < (1ull << 32); b += n) {
        const float x = __uint_as_float((uint32_t)b);
        const float ax = fabsf(x);
        if (!((ax > 1e-18f && ax < 1e18f) || x == 0.0f)) continue;
        const float q0 = x * rcp;
        const float r = fmaf(-q0, res, x);
        const float q = fmaf(r, rcp, q0);
        if (!(q == x / res)) local++;          // as VALUES: for x = -0 the sequence gives +0 where the division gives -0, and both are cell 0 (the one
                                               // bit pattern in the gate where the two differ for 0.145 -- a bitwise comparison here kept the whole fast path switched off)
    }
    if (local) atomicAdd(bad, local);
}

__global__ void k_philox_probe(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t *out)
{
    uint32_t o[4];
    philox4x32_10(c0, c1, c2, c3, k0, k1, o);
    for (int i = 0; i < 4; i++) out[i] = o[i];
}

hipError_t launch_math_probe(int op, const double *x, const double *y, double *out, uint32_t n, hipStream_t st)
{
    hipLaunchKernelGGL(k_math_probe, dim3((n + 255) / 256), dim3(256), 0, st, op, x, y, out, n);
    return hipGetLastError();
}

hipError_t launch_verify_div(float res, float rcp, unsigned long long *bad, hipStream_t st)
{
    hipLaunchKernelGGL(k_verify_div, dim3(256 * 16), dim3(256), 0, st, res, rcp, bad);
    return hipGetLastError();
}

hipError_t launch_tris_by_id(const float4 *tris, uint32_t n_tri, float4 *out, hipStream_t st)
{
    if (n_tri == 0) return hipSuccess;
    hipLaunchKernelGGL(k_tris_by_id, dim3((n_tri + 255u) / 256u), dim3(256), 0, st, tris, n_tri, out);
    return hipGetLastError();
}

hipError_t launch_expand_tris(const float4 *in48, uint32_t n_tri, float4 *out, hipStream_t st)
{
    hipLaunchKernelGGL(k_expand_tris, dim3((n_tri + 255u) / 256u), dim3(256), 0, st, in48, n_tri, out);
    return hipGetLastError();
}

hipError_t launch_philox_probe(const uint32_t c[4], const uint32_t k[2], uint32_t *out, hipStream_t st)
{
    hipLaunchKernelGGL(k_philox_probe, dim3(1), dim3(1), 0, st, c[0], c[1], c[2], c[3], k[0], k[1], out);
    return hipGetLastError();
}

}  // namespace mcrt
