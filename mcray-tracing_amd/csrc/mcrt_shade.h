// mcrt_shade.h -- the interface interaction of one path (shade_path) and the state it works on, shared by k_shade (mcrt_shade.hip)
// and k_path (mcrt_path.hip)
#pragma once
#include "mcrt_device.h"

namespace mcrt {

struct Hit { float frac; int tri; int mesh; f3 n; float da; };

// ---- interface interaction (scene.cpp:122-165, ray.cpp:11-97) of ONE path at bounce b, given its ray and the closest-hit
// word of the walk: thickness draw, travel, hit_boundary, the segment's records, the continuing ray's state.  Returns whether
// the path goes on.
struct PathState { f3 from, dir; float intensity; int media, outside; double dist_mm; };

// the scene's material and mesh tables as k_shade reads them: its LDS copies when they fit (MCRT_SHADE_TABLE rows each), else memory.
// (`lds` is wave-uniform: a scalar branch picks the load, so the LDS side compiles to ds_read, not to a flat load)
struct ShadeTables {
    const float4 *mats_g; const uint4 *meshes_g; const float4 *mats_l; const uint4 *meshes_l; bool lds;
    // (the empty asm keeps the two sides different instructions: otherwise the compiler merges them into ONE load through a selected flat pointer)
    MCRT_DEV float4 mat(uint32_t r) const { float4 v; if (lds) { v = mats_l[r]; asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w)); } else v = mats_g[r]; return v; }
    MCRT_DEV uint4 mesh(uint32_t r) const { uint4 v; if (lds) { v = meshes_l[r]; asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w)); } else v = meshes_g[r]; return v; }
};
// FOLD (k_shade of bounce 0 in a silent start medium, FrameArgs::fold_b0): the segment's march record is not written; what its boundary echo
// needs is handed back in *fo and the caller adds the echo itself.
struct FoldEcho { float refl; uint32_t steps; double t_start; };
template <bool STATS, bool FOLD = false>
MCRT_DEV bool shade_path(const FrameArgs &a, const ShadeTables &tb, uint32_t b, uint32_t pid, PathState &ps, f3 f2, f3 to, unsigned long long key, bool &reflected,
                         unsigned long long &st_seg, unsigned long long &st_hits, FoldEcho *fo = nullptr)
{
    bool alive = false;
    f3 from = ps.from, dir = ps.dir;
    float intensity = ps.intensity; int media = ps.media, outside = ps.outside; double dist_mm = ps.dist_mm;
    reflected = false;
    {
        Hit best; best.frac = __uint_as_float((uint32_t)(key >> 32)); best.tri = (int)(uint32_t)key; best.da = 0.0f; best.mesh = 0; best.n = mk(0, 0, 0);
        if (best.tri >= 0) {
            // plane normal, mesh and the origin-side value of the winning triangle, as the walk's test evaluated them
            const float4 *T = a.tris_id + MCRT_TRI_PIECES * (size_t)best.tri;      // (the id-ordered copy: through tri_slot the fetch was a chain of two dependent random reads)
            const float4 t2 = T[1];                                     // (v1, mesh)
            const float4 P = tri_plane(xyz(T[0]), xyz(t2), xyz(T[2]));
            best.n = xyz(P);
            best.da = dot(best.n, f2) - P.w;
            best.mesh = __float_as_int(t2.w);
        }
        const uint32_t line = pid / a.S, fr = line / a.ne_frame;      // (two divisions; the remainders by multiply-subtract)
        const uint32_t e_abs = a.e_begin + (line - fr * a.ne_frame);
        Rng g; g.k0 = a.seed; g.k1 = a.frame + fr; g.element = e_abs; g.sample = pid - line * a.S; g.bounce = b;
        const float4 m0 = tb.mat(2 * media);   // imp, att, mu0, mu1  (second half: sigma, spec, shine, thick)
        const float att = m0.y;

        f3 seg_to = to;
        float seg_refl = 0.0f; const float seg_init = intensity; const double seg_dist = dist_mm;
        const f3 seg_from = from, seg_dir = dir; const int seg_media = media; int seg_tri = -1;
        if (best.tri >= 0) {
            if (STATS) st_hits++;
            f3 nn = normalized(best.n);
            if (best.da <= 0.0f) nn = neg(nn);
            const float sfr = 1.0f - best.frac;
            const f3 hp = mk(sfr * f2.x + best.frac * to.x, sfr * f2.y + best.frac * to.y, sfr * f2.z + best.frac * to.z);
            const uint4 organ = tb.mesh(best.mesh);   // mat_inside, mat_outside, vascular
            // thickness penetration scene.cpp:132-139 (Box-Muller on block 0)
            const float sigma_t = tb.mat(2 * organ.x + 1).w;
            float qpen = 0.0f;
            if (sigma_t != 0.0f) {
                double n1, n2, sn, cs;
                rng_block(g, 0u, n1, n2);
                det_sincos(n2 * 2 * PI_D, sn, cs);
                const double z = sqrt(-2.0 * det_log(1.0 - n1)) * cs;
                qpen = (float)fabs(z * (double)sigma_t + 0.0);
            }
            const f3 inside = mk(qpen * dir.x + hp.x, qpen * dir.y + hp.y, qpen * dir.z + hp.z);
            // travel ray.cpp:99-103, distance_in_mm scene.cpp:281-290
            const float xd = fabsf(from.x - inside.x) * a.sx, yd = fabsf(from.y - inside.y) * a.sy, zd = fabsf(from.z - inside.z) * a.sz;
            const double mm = sqrt((double)xd * (double)xd + (double)yd * (double)yd + (double)zd * (double)zd) * 10;
            dist_mm = dist_mm + mm;
            intensity = intensity * det_expf(-att * ((float)mm * 0.01f) * a.freq);

            // hit_boundary: material transition logic ray.cpp:14-47 (bug-compatible)
            int after_vasc, mat_after;
            if (outside != OUT_NONE) {
                if (organ.z) { after_vasc = OUT_NONE; mat_after = (outside == OUT_SELF) ? media : outside; }
                else { after_vasc = (outside == (int)organ.x) ? (int)organ.y : (int)organ.x; mat_after = media; }
            } else {
                if (organ.z) { after_vasc = OUT_SELF; mat_after = (int)organ.x; }
                else { after_vasc = OUT_NONE; mat_after = (int)organ.x; }
            }
            const float4 a0 = tb.mat(2 * mat_after), a1 = tb.mat(2 * mat_after + 1);
            double u_pc, u_x;
            rng_block(g, 1u, u_pc, u_x);
            // power_cosine_variate ray.cpp:213-224
            const int indice = (int)a1.z + 1;
            const float exponente = (float)((double)1.0 / indice);
            const float random_angle = (float)det_pow_pos(u_pc, (double)exponente);
            const f3 rn = random_unit_vector(nn, random_angle, g);

            float inc = dot(dir, neg(rn));
            if (inc < 0) inc = dot(dir, rn);
            const float rr = m0.x / a0.x;
            float refa = 1 - rr * rr * (1 - inc * inc);
            const bool tir = refa < 0;
            refa = sqrtf(refa);
            const float kk = rr * inc - refa;
            f3 refr = mk(rr * dir.x + kk * rn.x, rr * dir.y + kk * rn.y, rr * dir.z + kk * rn.z);
            refr = normalized(refr);
            const float two_c = 2 * inc;
            f3 refl = mk(dir.x + two_c * rn.x, dir.y + two_c * rn.y, dir.z + two_c * rn.z);
            refl = normalized(refl);

            float i_refl;
            if (tir) i_refl = intensity;
            else {
                const float num = m0.x * inc - a0.x * refa;
                const float den = m0.x * inc + a0.x * refa;
                const float qq = num / den;
                i_refl = (float)((double)intensity * ((double)qq * (double)qq));
            }
            const float i_refr = intensity - i_refl;

            const float ra = dot(dir, refr);
            float refraction_factor = det_powf(ra, a1.y);
            const float rb = dot(dir, refl);
            const float reflection_factor = det_powf(rb, a1.y);
            if (a.sanitize && tir) refraction_factor = 0.0f;
            seg_refl = (std_max(refraction_factor, 0.0f) + std_max(reflection_factor, 0.0f)) * random_angle;
            seg_to = inside;
            seg_tri = best.tri;

            const float x = (float)u_x;
            const float prob = i_refl / intensity;
            float i_new;
            from = hp;
            if (prob > x) { dir = refl; i_new = i_refl > a.eps ? i_refl : 0.0f; reflected = true; }
            else { dir = refr; media = mat_after; outside = after_vasc; i_new = i_refr > a.eps ? i_refr : 0.0f; }
            if (i_new > a.eps) { intensity = i_new; alive = true; }
        }
        if (STATS) st_seg++;

        // what the accumulation loop needs of this segment (main.cpp:112-121), computed once here by one lane instead of by
        // every lane of k_march's quad: start time, step count, the per-step advance
        {
            const f3 df = seg_to - seg_from;
            const float dist_f = sqrtf(dot(df, df)) * 10.0f;
            const uint32_t steps = steps_from((double)dist_f / a.axial_res_mm);
            const double t_start = (seg_dist * 1000.0) / a.sos_d;
            if (FOLD) { fo->refl = seg_refl; fo->steps = steps; fo->t_start = t_start; }
            else {
                float4 *mr = a.mrec + 3 * ((size_t)b * a.ne * a.S + pid);    // [bounce][path]: neighbouring paths are neighbours in memory
                mr[0] = make_float4(seg_from.x, seg_from.y, seg_from.z, seg_refl);
                mr[1] = make_float4(a.axial_res_f * seg_dir.x, a.axial_res_f * seg_dir.y, a.axial_res_f * seg_dir.z, seg_init);
                mr[2] = make_float4(__int_as_float(__double2loint(t_start)), __int_as_float(__double2hiint(t_start)), __uint_as_float(steps), __int_as_float(seg_media));
            }
        }
        // ray_physics::segment (ray.h:28-36) -> slot [path][bounce], for the callers that ask for the segments themselves
        if (a.want_segs) {
            mcrt_segment sg;
            sg.from[0] = seg_from.x; sg.from[1] = seg_from.y; sg.from[2] = seg_from.z;
            sg.to[0] = seg_to.x; sg.to[1] = seg_to.y; sg.to[2] = seg_to.z;
            sg.dir[0] = seg_dir.x; sg.dir[1] = seg_dir.y; sg.dir[2] = seg_dir.z;
            sg.reflected_intensity = seg_refl; sg.initial_intensity = seg_init; sg.attenuation = att;
            sg.distance_traveled = seg_dist; sg.media = seg_media; sg.tri = seg_tri;
            a.segs[(size_t)pid * a.B + b] = sg;
        }
        if (a.hits) a.hits[(size_t)pid * a.B + b] = seg_tri;
        a.seg_count[pid] = b + 1u;
        alive = alive && (b + 1u < a.B);
        // RETIRE a path that can no longer reach the image (FrameArgs::retire_late): t_next is the very expression the next bounce would store as
        // its t_start.  Once it is past BOTH limits -- max_travel, which gates the steps, and the image's end thr_end = row_thr[R], which gates
        // every echo's row; n_rows is a parameter, so neither implies the other -- the rest of the path adds nothing: dist_mm only grows (mm is a
        // non-negative square root, or NaN; rounding is monotone and sos_d, time_step > 0), so every later t_start is >= t_next or NaN.  The
        // accumulation loop's test `t < max_travel` then fails at step 0 of every later segment, and every later boundary echo's time
        // t_start + time_step * (steps - 1) is >= t_start (huge when steps == 0, through the unsigned wrap) or NaN: outside [0, thr_end), no row.
        // A NaN t_next is not retired (`t_next == t_next`): left to the loop as before.  The segment that CROSSES the limit is this one: untouched.
        if (alive && a.retire_late) {
            const double t_next = (dist_mm * 1000.0) / a.sos_d;
            if (!(t_next < a.max_travel) && !(t_next < a.thr_end) && t_next == t_next) alive = false;
        }
    }
    ps.from = from; ps.dir = dir; ps.intensity = intensity; ps.media = media; ps.outside = outside; ps.dist_mm = dist_mm;
    return alive;
}

}  // namespace mcrt
