// mcrt_device.h -- device code shared by the kernel translation units (mcrt_walk / shade / path / march / post / scene.hip): the
// primitives two or more of them use, and every compile-time knob read by more than one of them (so a -D reaches all its readers the
// same way).  Everything here is inline (MCRT_DEV); a helper or knob that only one unit uses stays in that unit, next to its kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mcrt.h"
#include "mcrt_internal.h"
#include "mcrt_detmath.h"
#include "mcrt_kernels.h"

#ifndef MCRT_LANE_STACK
#define MCRT_LANE_STACK 32           // (the headline workload's deepest walk stacks 16 entries, 14 at the 99.9th percentile: profiles/round4/bvh_width.json)
#endif
// Persistent kernels carry a WATCHDOG: every 4096 iterations of its outer loop a wavefront compares the 100 MHz wall clock
// with its start, and a kernel that is still running after MCRT_WATCHDOG_SECONDS sets bit 1 of the device error word and leaves
// -- a logic error then surfaces as MCRT_ERR_LIMIT from the next synchronising call instead of a hung GPU.
#ifndef MCRT_WATCHDOG_SECONDS
#define MCRT_WATCHDOG_SECONDS 20
#endif
#define MCRT_WATCHDOG_DECL() const unsigned long long wd_start = wall_clock64(); uint32_t wd_iter = 0;
#define MCRT_WATCHDOG_CHECK() { if ((++wd_iter & 4095u) == 0u && wall_clock64() - wd_start > (unsigned long long)MCRT_WATCHDOG_SECONDS * 100000000ull) { \
        if ((threadIdx.x & 63) == 0) atomicOr(a.error_flag, 2u); break; } }
#ifndef MCRT_LANE_LEAF_BATCH
#define MCRT_LANE_LEAF_BATCH 20      // leave the inner-node phase once this many lanes are parked on a leaf
#endif
#ifndef MCRT_SHADE_TABLE
#define MCRT_SHADE_TABLE 32          // rows of the material / mesh tables k_shade keeps in LDS (larger scenes read them from memory)
#endif

namespace mcrt {

struct f3 { float x, y, z; };
MCRT_DEV f3 mk(float x, float y, float z) { f3 r; r.x = x; r.y = y; r.z = z; return r; }
MCRT_DEV f3 operator+(f3 a, f3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
MCRT_DEV f3 operator-(f3 a, f3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
MCRT_DEV f3 neg(f3 a) { return mk(-a.x, -a.y, -a.z); }
MCRT_DEV f3 scale(f3 a, float s) { return mk(a.x * s, a.y * s, a.z * s); }
MCRT_DEV float dot(f3 a, f3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }                 // btVector3::dot, scalar path
MCRT_DEV f3 cross(f3 a, f3 b) { return mk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
MCRT_DEV f3 normalized(f3 a) { float inv = 1.0f / sqrtf(dot(a, a)); return scale(a, inv); }    // btVector3::normalized
MCRT_DEV f3 xyz(float4 q) { return mk(q.x, q.y, q.z); }

constexpr int OUT_NONE = -1;   // media_outside == nullptr
constexpr int OUT_SELF = -2;   // media_outside aliases the ray's own media (ray.cpp:38 + scene.cpp:154)

// The contract's plane distance (round 3): ONE fused multiply-add per plane, t = fl(plane * inv + c) with c = -(o * inv) rounded once
// per ray and axis.  For a fixed ray it is a monotone function of the plane, which is all the order-independence argument needs
// (DESIGN.md 3).  The reciprocal direction is kept FINITE: 1/0 (a ray parallel to an axis) and overflowing quotients become
// +-2^100, so every distance is a finite number (|plane| < 2^20 in any scene) and the argument needs no special cases; the sign of
// the huge distance still says on which side of the plane the origin lies.
MCRT_DEV float rcp_dir(float d) { const float r = 1.0f / d; return r > 0x1p+100f ? 0x1p+100f : (r < -0x1p+100f ? -0x1p+100f : r); }
MCRT_DEV f3 ray_c(f3 o, f3 inv) { return mk(-(o.x * inv.x), -(o.y * inv.y), -(o.z * inv.z)); }
// ray parameter interval of a box under that rule (the triangles' padded bounds: the eligibility test of the contract)
MCRT_DEV bool slab_c(f3 lo, f3 hi, f3 c, f3 inv, float tlow, float tcap, float &tmin_o, float &tmax_o)
{
    const float t0x = fmaf(lo.x, inv.x, c.x), t1x = fmaf(hi.x, inv.x, c.x);
    const float t0y = fmaf(lo.y, inv.y, c.y), t1y = fmaf(hi.y, inv.y, c.y);
    const float t0z = fmaf(lo.z, inv.z, c.z), t1z = fmaf(hi.z, inv.z, c.z);
    float lo3 = fminf(t0z, t1z), hi3 = fmaxf(t0z, t1z), tmin, tmax;
    const float lo1 = fminf(t0x, t1x), lo2 = fminf(t0y, t1y), hi1 = fmaxf(t0x, t1x), hi2 = fmaxf(t0y, t1y);
    asm("v_max_f32 %0, %1, %2" : "=v"(lo3) : "v"(lo3), "v"(tlow));
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(tmin) : "v"(lo1), "v"(lo2), "v"(lo3));
    asm("v_min_f32 %0, %1, %2" : "=v"(hi3) : "v"(hi3), "v"(tcap));
    asm("v_min3_f32 %0, %1, %2, %3" : "=v"(tmax) : "v"(hi1), "v"(hi2), "v"(hi3));
    tmin_o = tmin; tmax_o = tmax;
    return tmin <= tmax;
}

// the walk only needs (fraction, triangle): k_shade looks the plane of the winner up again
struct Best { float frac; int tri; };

// The walk's triangle record, 48 bytes = three 16-byte pieces in leaf order:
//   v0 | id, v1 | mesh     the vertices (edge tests; the plane and the triangle's own padded bounds are rebuilt from them: tri_plane, tri_padded_bounds)
//   v2 | -1e-4 |n|^2       ... and processTriangle's edge tolerance
// Rounds 1-3 stored plane AND padded bounds (96 bytes, six pieces per triangle tested), round 4 tried the plane as a fourth piece.  The walk is bound by
// the cache accesses it makes: what a few register instructions rebuild -- with the contract's own expressions, so bit for bit -- is not
// fetched.
// the plane of a triangle, n = (v1 - v0) x (v2 - v0) and dot(v0, n) (Bullet's processTriangle)
MCRT_DEV float4 tri_plane(f3 v0, f3 v1, f3 v2)
{
    const f3 n = cross(v1 - v0, v2 - v0);
    return make_float4(n.x, n.y, n.z, dot(v0, n));
}
// the triangle's own padded bounds (contract: pad = 2e-4 * largest extent + pad_abs), bit for bit what the builders put around the
// leaves (mcrt_build_bvh, k_prims): min / max are exact, the three roundings (extent, pad, the six sums) are the builders' own
MCRT_DEV void tri_padded_bounds(f3 v0, f3 v1, f3 v2, float pad_abs, f3 &lo_o, f3 &hi_o)
{
    const f3 lo = mk(fminf(v0.x, fminf(v1.x, v2.x)), fminf(v0.y, fminf(v1.y, v2.y)), fminf(v0.z, fminf(v1.z, v2.z)));
    const f3 hi = mk(fmaxf(v0.x, fmaxf(v1.x, v2.x)), fmaxf(v0.y, fmaxf(v1.y, v2.y)), fmaxf(v0.z, fmaxf(v1.z, v2.z)));
    const float ext = fmaxf(fmaxf(fmaxf(0.0f, hi.x - lo.x), hi.y - lo.y), hi.z - lo.z);
    const float pad = 2e-4f * ext + pad_abs;
    lo_o = mk(lo.x - pad, lo.y - pad, lo.z - pad);
    hi_o = mk(hi.x + pad, hi.y + pad, hi.z + pad);
}

struct Rng { uint32_t k0, k1, element, sample, bounce; };
MCRT_DEV void rng_block(const Rng &g, uint32_t block, double &a, double &b)
{
    uint32_t o[4];
    philox4x32_10(g.element, g.sample, g.bounce, block, g.k0, g.k1, o);
    a = u53(o[0], o[1]);
    b = u53(o[2], o[3]);
}

// ray.cpp:167-211
MCRT_DEV f3 random_unit_vector(f3 v, float cos_theta, const Rng &g)
{
    bool flag = false;
    float px, py, p;
    uint32_t attempt = 0;
    do {
        double ua, ur;
        rng_block(g, 2u + attempt, ua, ur);
        double a = ua * 2 * PI_D;
        double r = 0.5 * sqrt(ur);
        double sa, ca;
        det_sincos(a, sa, ca);
        px = (float)(r * ca);
        py = (float)(r * sa);
        p = px * px + py * py;
        attempt++;
    } while (!(p <= 0.25f) && attempt < 8u);
    float vx = v.x, vy = v.y, vz = v.z;
    if (fabsf(vx) > fabsf(vy)) { vx = vy; vy = v.x; flag = true; }
    float b = 1 - vx * vx;
    float radicando = 1 - cos_theta * cos_theta;
    radicando = radicando / (p * b);
    float c = sqrtf(radicando);
    px = px * c;
    py = py * c;
    float d = cos_theta - vx * px;
    float wx = vx * cos_theta - b * px;
    float wy = vy * d + vz * py;
    float wz = vz * d - vy * py;
    if (flag) { float aux = wy; wy = wx; wx = aux; }
    return mk(wx, wy, wz);
}

MCRT_DEV float std_max(float a, float b) { return (a < b) ? b : a; }

MCRT_DEV uint32_t steps_from(double q)
{
    if (!(fabs(q) < 9.2233720368547758e18)) return 0u;
    return (uint32_t)(long long)q;
}

MCRT_DEV long long wave_sum_i64(long long v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// rint(echo * 2^40) for |echo| < 1024 (so |echo * 2^40| < 2^50), round to nearest even -- in TWO floating-point instructions: the
// product echo * 2^40 is exact in double, and adding 1.5 * 2^52 to it rounds the sum to an integer (ulp = 1 in [2^52, 2^53))
// whose low mantissa bits ARE that integer, offset by 2^51; one fma does both, an integer subtract removes the offset.
MCRT_DEV long long fix40(float echo)
{
    const double x = fma((double)echo, 0x1p40, 0x1.8p52);
    return (long long)__double_as_longlong(x) - (long long)__double_as_longlong(0x1.8p52);
}

// row = (int)(t / row_dt) if that quotient is < R, else -1 (rfimage.h:33-40), from the threshold table in memory (k_shade's folded bounce 0, k_label): k_march's row_of, which reads its LDS image
MCRT_DEV int row_of_thr(double t, const double *thr, uint32_t R, double inv_dt, double thr_end)
{
    if (!(t < thr_end) || !(t >= 0.0)) return -1;
    int r = (int)(t * inv_dt);                                   // within one row of the answer
    r = r < 0 ? 0 : (r > (int)R - 1 ? (int)R - 1 : r);
    while (t < thr[r]) r--;
    while (t >= thr[r + 1]) r++;
    return r;
}

struct Ray { f3 f2, to; };

#define MCRT_KEY_MISS ((0x3f800000ull << 32) | 0xffffffffull)   // fraction 1.0, no triangle

// max_ray_length (ray.cpp:110-113) + enlarge (scene.cpp:292-298) + the 0.1 start offset (scene.cpp:115).
// The segment a ray is tested on is a pure function of the path state -- origin, direction and the length factor L / 100 -- so the
// state carries that ONE float (ray_len, evaluated once per bounce where intensity and medium are at hand) and both the walk and
// k_shade rebuild the end points from it with the same expressions (ray_of): rounds 1-3 wrote a 32-byte ray record per ray and
// bounce in k_shade and read it back twice.
MCRT_DEV float ray_len(float intensity, float att, const FrameArgs &a)
{
    const float L = 10.f * det_logf(a.eps / intensity) / -att * a.freq;
    return L / 100.0f;
}
MCRT_DEV Ray ray_of(f3 from, f3 dir, float Ls, const FrameArgs &a)
{
    Ray r;
    r.to = mk(from.x + Ls * (a.sx * dir.x), from.y + Ls * (a.sy * dir.y), from.z + Ls * (a.sz * dir.z));
    r.f2 = mk(from.x + a.offs * dir.x, from.y + a.offs * dir.y, from.z + a.offs * dir.z);
    return r;
}

// The direction a beam sorts a ray by (mcrt_beam.hip): D = to - f2 of the ray's segment, its dominant axis and the sign along it; the beam's CODE is
// 2 * axis + sign, 0 .. 5 whatever D holds.  ONE statement of it: k_shade(b - 1) stores the code of the ray it queues (FrameArgs::beam_word), k_beam_rank(b)
// sorts by the stored code, k_beam_bounds / k_beam_test rebuild it from the state (beam_ray) -- the same expressions on the same floats, the same bits.
// (From the segment, not from dir: sx / sy / sz scale the components of `to` differently.)
struct BeamDir { f3 D; int dom; bool neg; };
MCRT_DEV BeamDir beam_dir(const Ray &ry)
{
    BeamDir r;
    r.D = ry.to - ry.f2;
    const float ax = fabsf(r.D.x), ay = fabsf(r.D.y), az = fabsf(r.D.z);
    r.dom = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);
    r.neg = (r.dom == 0 ? r.D.x : r.dom == 1 ? r.D.y : r.D.z) < 0.0f;
    return r;
}
MCRT_DEV uint32_t beam_code(const BeamDir &d) { return (uint32_t)d.dom * 2u + (d.neg ? 1u : 0u); }
// the word k_shade stores per queued ray of an ordered bounce: code | (medium & 0xff) << 8 -- with from_tri all of the group key that is not in the path id
MCRT_DEV uint32_t beam_word_of(f3 from, f3 dir, float Ls, int media, const FrameArgs &a)
{
    return beam_code(beam_dir(ray_of(from, dir, Ls, a))) | (((uint32_t)media & 0xffu) << 8);
}
MCRT_DEV uint32_t *beam_words(const FrameArgs &a) { return a.from_tri + (size_t)a.ne * a.S; }      // [np] by queue position, behind from_tri's [np] by path

#define MCRT_STATE0_AT(pos, S) ((pos) - (pos) % (S))      /* queue position of the bounce-0 state of the path queued at pos: its scan-line's first sample (k_init) */

// cv::remap(src, dst, map_y, map_x, INTER_LINEAR, BORDER_CONSTANT 0) at one output pixel (rfimage.h:139), exact bilinear: mx = column
// coordinate (scan-line), my = row coordinate.  remap_taps gathers the four taps -- tap(x, y) (long long) is the source value at scan-line x,
// row y, asked for only inside the E x R image, 0 elsewhere -- and remap_blend weighs them.  The one statement of the scan conversion:
// k_remap gathers the float image with remap_bilinear, k_bmode the grey levels with the two halves (the taps of the next frame are in flight
// while a frame is blended).
struct RemapPoint { float mx, my, ax, ay; long long x0, y0; };
MCRT_DEV RemapPoint remap_point(float mx, float my)
{
    RemapPoint p;
    const float fx = floorf(mx), fy = floorf(my);
    p.mx = mx; p.my = my; p.ax = mx - fx; p.ay = my - fy;
    p.x0 = (long long)fx; p.y0 = (long long)fy;
    return p;
}
template <typename Tap>
MCRT_DEV void remap_taps(const RemapPoint &p, uint32_t E, uint32_t R, Tap tap, float v[2][2])
{
    const bool mapped = (p.mx == p.mx) && (p.my == p.my);
#pragma unroll
    for (int dy = 0; dy < 2; dy++)
#pragma unroll
        for (int dx = 0; dx < 2; dx++) {
            const long long xx = p.x0 + dx, yy = p.y0 + dy;
            const bool in = mapped && xx >= 0 && yy >= 0 && xx < (long long)E && yy < (long long)R;
            v[dy][dx] = in ? tap(xx, yy) : 0.0f;
        }
}
MCRT_DEV float remap_blend(const RemapPoint &p, const float v[2][2])
{
    const float top = v[0][0] * (1.0f - p.ax) + v[0][1] * p.ax;
    const float bot = v[1][0] * (1.0f - p.ax) + v[1][1] * p.ax;
    return top * (1.0f - p.ay) + bot * p.ay;
}
template <typename Tap>
MCRT_DEV float remap_bilinear(float mx, float my, uint32_t E, uint32_t R, Tap tap)
{
    const RemapPoint p = remap_point(mx, my);
    float v[2][2];
    remap_taps(p, E, R, tap, v);
    return remap_blend(p, v);
}

// population count of a wave mask as a 32-bit SCALAR (a comparison of __popcll's 64-bit result is compiled to a vector instruction)
MCRT_DEV uint32_t popc_mask(unsigned long long m)
{
    uint32_t n = (uint32_t)__builtin_popcount((uint32_t)m) + (uint32_t)__builtin_popcount((uint32_t)(m >> 32));
    asm volatile("" : "+s"(n));
    return n;
}

}  // namespace mcrt
