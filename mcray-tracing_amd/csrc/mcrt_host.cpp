// mcrt_host.cpp -- host-side pieces of the hot path (no GPU needed):
//   * BVH2 builder (binned SAH) replacing btBvhTriangleMeshShape construction + the DBVT
//     broadphase (scene.cpp:255,309): ONE flattened tree over the triangles of all meshes.
//   * the reference's static tables: tissue texture (volume.h:19-35), PSF taps (psf.h:34-58),
//     transducer element geometry (transducer.h:24-62), scan-conversion maps (rfimage.h:183-215).
//   * the library's error string (mcrt_last_error).
// Plain C++ with no HIP in it: tests/test_host_sanitize.py compiles this file by itself under ASan + UBSan.
#include "../../include/mcrt.h"
#include "mcrt_internal.h"
#include "mcrt_transmit.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

namespace mcrt {
static thread_local std::string g_err;
int set_error(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    g_err = buf;
    return code;
}
}  // namespace mcrt
extern "C" const char *mcrt_last_error(void) { return mcrt::g_err.c_str(); }

// tuning knobs (mcrt_internal.h): only a process started with MCRT_TUNING=1 has any
const char *mcrt::tuning_env(const char *name)
{
    const char *e = getenv("MCRT_TUNING");       // (looked at when a knob is asked for -- mcrt_create, a BVH build --, never on the frame path)
    return (e && e[0] == '1') ? getenv(name) : nullptr;
}

namespace {

struct Prim {
    float lo[3], hi[3];   // padded bounds
    float c[3];           // centroid of the unpadded bounds
    uint32_t id;
};

struct Box {
    float lo[3], hi[3];
    void reset() { for (int i = 0; i < 3; i++) { lo[i] = INFINITY; hi[i] = -INFINITY; } }
    void grow(const float *l, const float *h) { for (int i = 0; i < 3; i++) { lo[i] = std::min(lo[i], l[i]); hi[i] = std::max(hi[i], h[i]); } }
    void grow_pt(const float *p) { for (int i = 0; i < 3; i++) { lo[i] = std::min(lo[i], p[i]); hi[i] = std::max(hi[i], p[i]); } }
    float half_area() const {
        float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
        if (!(dx >= 0) || !(dy >= 0) || !(dz >= 0)) return 0.f;
        return dx * dy + dy * dz + dz * dx;
    }
};

constexpr int kLeafMaxDefault = 4;     // (leaf size and triangle cost can be set through MCRT_SAH_LEAF_MAX / MCRT_SAH_COST_TRI for experiments: members of the Builder)
constexpr int kBins = 16;
constexpr int kMaxDepth = MCRT_BVH_MAX_DEPTH;   // deepest leaf; the traversal stack holds this many entries
constexpr float kCostNode = 1.0f, kCostTriDefault = 1.2f;

struct Builder {
    int kLeafMax = kLeafMaxDefault; float kCostTri = kCostTriDefault;
    std::vector<Prim> prims;
    std::vector<mcrt_bvh_node> nodes;
    int deepest = 0;

    int levels_needed(uint32_t n) const { int k = 0; uint64_t cap = (uint64_t)kLeafMax; while (cap < n) { cap <<= 1; k++; } return k; }

    static int32_t leaf_ref(uint32_t first, uint32_t cnt) { return ~(int32_t)((first << 3) | (cnt - 1)); }

    // returns child reference, bounds of the subtree in `out`
    int32_t build(uint32_t lo, uint32_t hi, int depth, Box &out)
    {
        const uint32_t n = hi - lo;
        out.reset();
        Box cb; cb.reset();
        for (uint32_t i = lo; i < hi; i++) { out.grow(prims[i].lo, prims[i].hi); cb.grow_pt(prims[i].c); }
        deepest = std::max(deepest, depth);

        uint32_t mid = 0;
        bool have_split = false;
        const bool force_median = depth + levels_needed(n) >= kMaxDepth;
        float best_cost = INFINITY;
        if (n > 1 && !force_median) {
            int best_axis = -1, best_bin = -1;
            const float parent_area = out.half_area();
            for (int axis = 0; axis < 3; axis++) {
                const float cmin = cb.lo[axis], cext = cb.hi[axis] - cb.lo[axis];
                if (!(cext > 0.f)) continue;
                const float scale = (float)kBins / cext;
                Box bb[kBins]; uint32_t cnt[kBins];
                for (int b = 0; b < kBins; b++) { bb[b].reset(); cnt[b] = 0; }
                for (uint32_t i = lo; i < hi; i++) {
                    int b = (int)((prims[i].c[axis] - cmin) * scale);
                    b = std::min(std::max(b, 0), kBins - 1);
                    bb[b].grow(prims[i].lo, prims[i].hi); cnt[b]++;
                }
                float right_area[kBins]; uint32_t right_cnt[kBins];
                Box acc; acc.reset(); uint32_t c = 0;
                for (int b = kBins - 1; b > 0; b--) { acc.grow(bb[b].lo, bb[b].hi); c += cnt[b]; right_area[b] = acc.half_area(); right_cnt[b] = c; }
                acc.reset(); c = 0;
                for (int b = 0; b < kBins - 1; b++) {
                    acc.grow(bb[b].lo, bb[b].hi); c += cnt[b];
                    if (c == 0 || right_cnt[b + 1] == 0) continue;
                    float cost = kCostNode + kCostTri * (acc.half_area() * (float)c + right_area[b + 1] * (float)right_cnt[b + 1]) / std::max(parent_area, 1e-30f);
                    if (cost < best_cost) { best_cost = cost; best_axis = axis; best_bin = b; }
                }
            }
            if (best_axis >= 0) {
                const float cmin = cb.lo[best_axis], scale = (float)kBins / (cb.hi[best_axis] - cb.lo[best_axis]);
                auto it = std::partition(prims.begin() + lo, prims.begin() + hi, [&](const Prim &p) {
                    int b = (int)((p.c[best_axis] - cmin) * scale);
                    b = std::min(std::max(b, 0), kBins - 1);
                    return b <= best_bin;
                });
                mid = (uint32_t)(it - prims.begin());
                have_split = mid > lo && mid < hi;
            }
        }
        if (n <= (uint32_t)kLeafMax && (n == 1 || !have_split || best_cost >= kCostTri * (float)n))
            return leaf_ref(lo, n);
        if (!have_split) {   // median split on the widest centroid axis (also the depth-limit fallback)
            int axis = 0; float ext = -1.f;
            for (int a = 0; a < 3; a++) { float e = cb.hi[a] - cb.lo[a]; if (e > ext) { ext = e; axis = a; } }
            mid = lo + n / 2;
            std::nth_element(prims.begin() + lo, prims.begin() + mid, prims.begin() + hi,
                             [axis](const Prim &a, const Prim &b) { return a.c[axis] < b.c[axis] || (a.c[axis] == b.c[axis] && a.id < b.id); });
        }
        const int32_t me = (int32_t)nodes.size();
        nodes.emplace_back();
        Box bl, br;
        int32_t cl = build(lo, mid, depth + 1, bl);
        int32_t cr = build(mid, hi, depth + 1, br);
        mcrt_bvh_node &N = nodes[me];
        for (int i = 0; i < 3; i++) { N.lo0[i] = bl.lo[i]; N.hi0[i] = bl.hi[i]; N.lo1[i] = br.lo[i]; N.hi1[i] = br.hi[i]; }
        N.c0 = cl; N.c1 = cr; N.pad0 = 0; N.pad1 = 0;
        return me;
    }
};

}  // namespace

extern "C" int mcrt_build_bvh(const float *tri, const uint32_t *tri_mesh, uint32_t n_tri, mcrt_bvh *out)
{
    if (!tri || !out || n_tri == 0) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_build_bvh: no triangles");
    if (n_tri >= (1u << 28)) return mcrt::set_error(MCRT_ERR_LIMIT, "mcrt_build_bvh: more than 2^28 triangles");
    Builder b;
    if (const char *e = mcrt::tuning_env("MCRT_SAH_LEAF_MAX")) { int v = atoi(e); if (v >= 1 && v <= 8) b.kLeafMax = v; }
    if (const char *e = mcrt::tuning_env("MCRT_SAH_COST_TRI")) { float v = (float)atof(e); if (v > 0.0f) b.kCostTri = v; }
    b.prims.resize(n_tri);
    // Padding (DESIGN.md "Closest hit"): Bullet's triangle test accepts points up to 1e-4 of the triangle's
    // height outside an edge, and the slab arithmetic rounds; each triangle's bounds are widened accordingly.
    // A triangle is eligible only while the ray overlaps ITS padded bounds (as in Bullet's per-triangle BVH
    // leaves); node boxes are exact unions of those, and the contract's plane distance fl(plane * inv + c) (one fma, finite
    // reciprocal: DESIGN.md 3) is a monotone function of the plane, so a box that contains another yields the wider interval
    // and node culling can never remove an eligible triangle.
    float scale = 0.f;
    for (size_t i = 0; i < (size_t)n_tri * 9; i++) { float a = std::fabs(tri[i]); if (a > scale && std::isfinite(a)) scale = a; }
    const float abs_pad = 4e-6f * std::max(scale, 1e-3f);
    for (uint32_t t = 0; t < n_tri; t++) {
        const float *v = tri + (size_t)t * 9;
        Prim &p = b.prims[t];
        // must equal k_expand_tris' padded bounds bit for bit: node boxes are unions of exactly these boxes
        float ext = 0.f;
        for (int a = 0; a < 3; a++) {
            float l = fminf(v[a], fminf(v[3 + a], v[6 + a]));
            float h = fmaxf(v[a], fmaxf(v[3 + a], v[6 + a]));
            p.lo[a] = l; p.hi[a] = h; p.c[a] = 0.5f * (l + h);
            ext = fmaxf(ext, h - l);
        }
        const float pad = 2e-4f * ext + abs_pad;
        for (int a = 0; a < 3; a++) { p.lo[a] = p.lo[a] - pad; p.hi[a] = p.hi[a] + pad; }
        p.id = t;
    }
    b.nodes.reserve(n_tri);
    Box root;
    int32_t r = b.build(0, n_tri, 0, root);
    if (r < 0) {   // everything fitted one leaf: wrap it in a root node (both children the same leaf)
        b.nodes.emplace_back();
        mcrt_bvh_node &N = b.nodes[0];
        for (int i = 0; i < 3; i++) { N.lo0[i] = root.lo[i]; N.hi0[i] = root.hi[i]; N.lo1[i] = root.lo[i]; N.hi1[i] = root.hi[i]; }
        N.c0 = r; N.c1 = r; N.pad0 = N.pad1 = 0;
    }
    out->n_nodes = (uint32_t)b.nodes.size();
    out->n_tri = n_tri;
    out->max_depth = (uint32_t)b.deepest;
    out->pad_abs = abs_pad;
    out->nodes = (mcrt_bvh_node *)malloc(sizeof(mcrt_bvh_node) * b.nodes.size());
    out->tri = (float *)malloc(sizeof(float) * 12 * (size_t)n_tri);
    if (!out->nodes || !out->tri) { free(out->nodes); free(out->tri); return mcrt::set_error(MCRT_ERR_NOMEM, "mcrt_build_bvh: out of memory"); }
    memcpy(out->nodes, b.nodes.data(), sizeof(mcrt_bvh_node) * b.nodes.size());
    for (uint32_t i = 0; i < n_tri; i++) {
        const uint32_t id = b.prims[i].id;
        const float *v = tri + (size_t)id * 9;
        float *o = out->tri + (size_t)i * 12;
        uint32_t mesh = tri_mesh ? tri_mesh[id] : 0u, zero = 0u;
        o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; memcpy(&o[3], &id, 4);
        o[4] = v[3]; o[5] = v[4]; o[6] = v[5]; memcpy(&o[7], &mesh, 4);
        o[8] = v[6]; o[9] = v[7]; o[10] = v[8]; memcpy(&o[11], &zero, 4);
    }
    return MCRT_OK;
}

extern "C" void mcrt_free_bvh(mcrt_bvh *bvh)
{
    if (!bvh) return;
    free(bvh->nodes); free(bvh->tri);
    bvh->nodes = nullptr; bvh->tri = nullptr; bvh->n_nodes = bvh->n_tri = 0;
}

// ---- BVH2 -> BVH4 collapse ----------------------------------------------------------------------
namespace {
struct Collapser {
    const mcrt_bvh *b2;
    std::vector<mcrt_bvh4_node> nodes;
    struct Slot { int32_t ref; float lo[3], hi[3]; };
    static float harea(const Slot &s) { float dx = s.hi[0] - s.lo[0], dy = s.hi[1] - s.lo[1], dz = s.hi[2] - s.lo[2]; return dx * dy + dy * dz + dz * dx; }
    static void kids(const mcrt_bvh_node &n, Slot &a, Slot &b)
    {
        a.ref = n.c0; b.ref = n.c1;
        for (int i = 0; i < 3; i++) { a.lo[i] = n.lo0[i]; a.hi[i] = n.hi0[i]; b.lo[i] = n.lo1[i]; b.hi[i] = n.hi1[i]; }
    }
    // returns {node4 index, worst-case stack entries needed below (and including) this node}
    std::pair<int32_t, uint32_t> build(int32_t n2)
    {
        Slot s[4]; int k = 2;
        kids(b2->nodes[n2], s[0], s[1]);
        if (s[0].ref == s[1].ref && s[0].ref < 0) k = 1;          // degenerate single-leaf root wrapper
        while (k < 4) {
            int pick = -1; float best = -1.f;
            for (int i = 0; i < k; i++) if (s[i].ref >= 0) { float a = harea(s[i]); if (a > best) { best = a; pick = i; } }
            if (pick < 0) break;
            Slot a, b; kids(b2->nodes[s[pick].ref], a, b);
            s[pick] = a; s[k++] = b;
        }
        const int32_t me = (int32_t)nodes.size();
        nodes.emplace_back();
        uint32_t deepest = 0;
        for (int i = 0; i < 4; i++) {
            mcrt_bvh4_child c;
            if (i < k) {
                int32_t ref = s[i].ref;
                if (ref >= 0) { auto r = build(ref); ref = r.first; deepest = std::max(deepest, r.second); }
                c.lo[0] = s[i].lo[0]; c.lo[1] = s[i].lo[1]; c.lo[2] = s[i].lo[2];
                c.hi_x = s[i].hi[0]; c.hi_y = s[i].hi[1]; c.hi_z = s[i].hi[2]; c.ref = ref; c.pad = 0;
            } else {
                c.lo[0] = c.lo[1] = c.lo[2] = INFINITY; c.hi_x = c.hi_y = c.hi_z = -INFINITY; c.ref = MCRT_BVH4_EMPTY; c.pad = 0;
            }
            nodes[me].c[i] = c;
        }
        return { me, (uint32_t)(k - 1) + deepest };
    }
};
}  // namespace

extern "C" int mcrt_build_bvh4(const mcrt_bvh *b2, mcrt_bvh4 *out)
{
    if (!b2 || !out || !b2->nodes || b2->n_nodes == 0) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_build_bvh4: no BVH2");
    Collapser c; c.b2 = b2;
    c.nodes.reserve(b2->n_nodes / 2 + 4);
    auto r = c.build(0);
    out->n_nodes = (uint32_t)c.nodes.size();
    out->max_stack = r.second;
    out->nodes = (mcrt_bvh4_node *)malloc(sizeof(mcrt_bvh4_node) * c.nodes.size());
    if (!out->nodes) return mcrt::set_error(MCRT_ERR_NOMEM, "mcrt_build_bvh4: out of memory");
    memcpy(out->nodes, c.nodes.data(), sizeof(mcrt_bvh4_node) * c.nodes.size());
    return MCRT_OK;
}

extern "C" void mcrt_free_bvh4(mcrt_bvh4 *b)
{
    if (!b) return;
    free(b->nodes); b->nodes = nullptr; b->n_nodes = 0;
}

// thr[r] = smallest double t with fl(t / dt) >= r (IEEE division is monotone in t), r = 0..R: the kernel's row_of()
// turns the reference's `row = t / dt; if (row < max_rows)` (rfimage.h:35-36) into table look-ups, exactly.
extern "C" int mcrt_row_thresholds(double dt, uint32_t R, double *thr)
{
    if (!thr || !(dt > 0.0)) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_row_thresholds: bad arguments");
    thr[0] = 0.0;
    for (uint32_t r = 1; r <= R; r++) {
        double t = (double)r * dt;
        while (t / dt >= (double)r) t = std::nextafter(t, -INFINITY);
        while (t / dt < (double)r) t = std::nextafter(t, INFINITY);
        thr[r] = t;
    }
    return MCRT_OK;
}

// ---- volume<n,res>::volume() (volume.h:19-35) ------------------------------------------------
// libstdc++ semantics: std::default_random_engine is minstd_rand0 (multiplier 16807, modulus 2^31-1,
// default seed 1); generate_canonical<double,53> consumes two draws; normal_distribution<double> is
// the Marsaglia polar method, which returns y*m and keeps x*m for the following call.
extern "C" int mcrt_generate_texture(float *vox, uint32_t n)
{
    if (!vox || n == 0) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_generate_texture: bad arguments");
    uint64_t state = 1;
    auto next = [&state]() -> double { state = (state * 16807ull) % 2147483647ull; return (double)(uint32_t)(state - 1); };
    const double R = 2147483646.0, RR = R * R;
    auto canonical = [&]() -> double {
        double sum = next();
        sum += next() * R;
        double r = sum / RR;
        return r >= 1.0 ? std::nextafter(1.0, 0.0) : r;
    };
    const size_t total = (size_t)n * n * n;
    for (size_t i = 0; i < total; i++) {
        double x, y, r2;
        do {
            x = 2.0 * canonical() - 1.0;
            y = 2.0 * canonical() - 1.0;
            r2 = x * x + y * y;
        } while (r2 > 1.0 || r2 == 0.0);
        const double mult = std::sqrt(-2 * std::log(r2) / r2);
        vox[2 * i] = (float)(y * mult);        // texture_noise: first variate of the pair
        vox[2 * i + 1] = (float)(x * mult);    // scattering_probability: the saved one
    }
    return MCRT_OK;
}

// ---- psf<>::psf (psf.h:34-58; psf.h:9 defines M_PI as 3.14159) --------------------------------
extern "C" int mcrt_psf_kernels(float freq, float var_x, float var_y, uint32_t res_um, float *axial, uint32_t n_ax, float *lateral, uint32_t n_lat)
{
    if (!axial || !lateral) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_psf_kernels: null output");
    const double pi_psf = 3.14159;
    const float res = (float)res_um / 1000.0f;
    const float half_ax = (float)((size_t)n_ax * res_um) / 1000.0f / 2.0f;
    const float half_lat = (float)((size_t)n_lat * res_um) / 1000.0f / 2.0f;
    for (uint32_t i = 0; i < n_ax; i++) {
        const float x = (float)i * res - half_ax;
        const double x2 = (double)x * (double)x;
        axial[i] = (float)(std::exp(-0.5f * (x2 / (double)var_x)) * std::cos(2 * pi_psf * (double)freq * (double)x));
    }
    for (uint32_t i = 0; i < n_lat; i++) {
        const float y = (float)i * res - half_lat;
        const double y2 = (double)y * (double)y;
        lateral[i] = (float)std::exp(-0.5f * (y2 / (double)var_y));
    }
    return MCRT_OK;
}

// Focal zones (the model is in include/mcrt.h): mcrt_psf_kernels' lateral taps per RF row, widened by the row's distance to the nearest
// focus and scaled by g = sqrt(var_y / var) to keep their area.  At q = 0, var == var_y and g == 1 exactly, so the row is
// mcrt_psf_kernels' own expression bit for bit.
extern "C" int mcrt_psf_focus_kernels(float var_y, uint32_t res_um, const mcrt_focus *f, uint32_t n_rows, double row_mm, float *lat_rows, uint32_t n_lat)
{
    if (!f || !lat_rows) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_psf_focus_kernels: null %s", f ? "lat_rows" : "focus");
    if (n_lat == 0 || n_lat > 32) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_psf_focus_kernels: n_lat must be 1..32 (%u)", n_lat);
    if (!(std::isfinite(var_y) && var_y > 0.0f)) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_psf_focus_kernels: var_y must be finite and > 0");
    if (!(std::isfinite(row_mm) && row_mm > 0.0)) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_psf_focus_kernels: row_mm must be finite and > 0");
    if (f->n_focus > 8) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_psf_focus_kernels: at most 8 foci (%u)", f->n_focus);
    for (uint32_t j = 0; j < f->n_focus; j++) {
        if (!(std::isfinite(f->focus_mm[j]) && f->focus_mm[j] >= 0.0f)) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_psf_focus_kernels: focus_mm[%u] must be finite and >= 0", j);
        if (j > 0 && !(f->focus_mm[j] > f->focus_mm[j - 1])) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_psf_focus_kernels: foci must be strictly ascending");
    }
    if (f->n_focus > 0 && !(std::isfinite(f->focal_range_mm) && f->focal_range_mm > 0.0f))
        return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_psf_focus_kernels: focal_range_mm must be finite and > 0");
    if (n_rows > MCRT_MAX_ROWS) return mcrt::set_error(MCRT_ERR_LIMIT, "mcrt_psf_focus_kernels: at most %d rows", MCRT_MAX_ROWS);
    const float res = (float)res_um / 1000.0f;
    const float half_lat = (float)((size_t)n_lat * res_um) / 1000.0f / 2.0f;
    for (uint32_t r = 0; r < n_rows; r++) {
        const double z = (double)r * row_mm;
        double var = (double)var_y, g = 1.0;
        if (f->n_focus > 0) {
            uint32_t best = 0;
            for (uint32_t j = 1; j < f->n_focus; j++)          // strictly nearer only: a tie keeps the shallower focus
                if (std::fabs(z - (double)f->focus_mm[j]) < std::fabs(z - (double)f->focus_mm[best])) best = j;
            const double q = (z - (double)f->focus_mm[best]) / (double)f->focal_range_mm;
            var = (double)var_y * (1.0 + q * q);
            g = std::sqrt((double)var_y / var);
        }
        for (uint32_t i = 0; i < n_lat; i++) {
            const float y = (float)i * res - half_lat;
            const double y2 = (double)y * (double)y;
            lat_rows[(size_t)r * n_lat + i] = (float)(g * std::exp(-0.5f * (y2 / var)));
        }
    }
    return MCRT_OK;
}

// Frequency compounding and the depth downshift (the model is in include/mcrt.h): mcrt_psf_kernels' axial taps per band and per RF row, the
// band's centre frequency falling with the row's depth down to a floor.  With no downshift f == (double)band_mhz[b] exactly, so the row is
// mcrt_psf_kernels' own expression bit for bit.
extern "C" int mcrt_default_bands(mcrt_bands *b, float freq, float var_x)
{
    if (!b) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_default_bands: null bands");
    memset(b, 0, sizeof *b);
    b->n_bands = 1u; b->band_mhz[0] = freq; b->band_weight[0] = 1.0f; b->var_x = var_x;
    return MCRT_OK;
}

extern "C" int mcrt_psf_band_kernels(const mcrt_bands *b, uint32_t res_um, uint32_t n_rows, double row_mm, float *ax_rows, uint32_t n_ax, float *w_rows)
{
    static const char fn[] = "mcrt_psf_band_kernels";
    if (!b || !ax_rows) return mcrt::set_error(MCRT_ERR_INVALID, "%s: null %s", fn, b ? "ax_rows" : "bands");
    if (b->n_bands == 0 || b->n_bands > 8) return mcrt::set_error(MCRT_ERR_INVALID, "%s: n_bands must be 1..8 (%u)", fn, b->n_bands);
    double S = 0.0;
    for (uint32_t k = 0; k < b->n_bands; k++) {
        if (!(std::isfinite(b->band_mhz[k]) && b->band_mhz[k] > 0.0f)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: band_mhz[%u] must be finite and > 0", fn, k);
        if (!(std::isfinite(b->band_weight[k]) && b->band_weight[k] >= 0.0f)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: band_weight[%u] must be finite and >= 0", fn, k);
        S += (double)b->band_weight[k];
    }
    if (!(S > 0.0)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: band_weight: every one of the %u bands has weight 0", fn, b->n_bands);
    if (!(std::isfinite(b->var_x) && b->var_x > 0.0f)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: var_x must be finite and > 0", fn);
    if (!(std::isfinite(b->downshift_mhz_per_mm) && b->downshift_mhz_per_mm >= 0.0f)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: downshift_mhz_per_mm must be finite and >= 0", fn);
    if (!(std::isfinite(b->min_mhz) && b->min_mhz >= 0.0f)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: min_mhz must be finite and >= 0", fn);
    if (res_um == 0) return mcrt::set_error(MCRT_ERR_INVALID, "%s: res_um must be > 0", fn);
    if (!(std::isfinite(row_mm) && row_mm > 0.0)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: row_mm must be finite and > 0", fn);
    if (n_ax == 0 || n_ax > 16) return mcrt::set_error(MCRT_ERR_INVALID, "%s: n_ax must be 1..16 (%u)", fn, n_ax);
    if (n_rows > MCRT_MAX_ROWS) return mcrt::set_error(MCRT_ERR_LIMIT, "%s: at most %d rows", fn, MCRT_MAX_ROWS);
    const double pi_psf = 3.14159;
    const float res = (float)res_um / 1000.0f;
    const float half_ax = (float)((size_t)n_ax * res_um) / 1000.0f / 2.0f;
    for (uint32_t k = 0; k < b->n_bands; k++)
        for (uint32_t r = 0; r < n_rows; r++) {
            const double z = (double)r * row_mm;
            const double f = std::max((double)b->min_mhz, (double)b->band_mhz[k] - (double)b->downshift_mhz_per_mm * z);
            for (uint32_t i = 0; i < n_ax; i++) {
                const float x = (float)i * res - half_ax;
                const double x2 = (double)x * (double)x;
                ax_rows[((size_t)k * n_rows + r) * n_ax + i] = (float)(std::exp(-0.5f * (x2 / (double)b->var_x)) * std::cos(2 * pi_psf * f * (double)x));
            }
        }
    if (w_rows)
        for (uint32_t r = 0; r < n_rows; r++)
            for (uint32_t k = 0; k < b->n_bands; k++) w_rows[(size_t)r * b->n_bands + k] = (float)((double)b->band_weight[k] / S);
    return MCRT_OK;
}

// Quadrature detection (the model is in include/mcrt.h): the taps of a type-III FIR Hilbert transformer under a Hamming window, its
// magnitude response, and the digital carrier of mcrt_psf_kernels' axial pulse.  Host only.
static bool detect_taps_ok(uint32_t n_taps) { return n_taps >= 3u && n_taps <= 63u && n_taps % 4u == 3u; }

extern "C" int mcrt_default_detect_opts(mcrt_detect_opts *o)
{
    if (!o) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_default_detect_opts: null options");
    o->n_taps = 31u;
    return MCRT_OK;
}

extern "C" int mcrt_detect_taps(const mcrt_detect_opts *o, float *taps)
{
    static const char fn[] = "mcrt_detect_taps";
    if (!o || !taps) return mcrt::set_error(MCRT_ERR_INVALID, "%s: null %s", fn, o ? "taps" : "options");
    if (!detect_taps_ok(o->n_taps)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: n_taps must be 3, 7, 11, ..., 63 (%u)", fn, o->n_taps);
    const double pi = 3.141592653589793;
    const uint32_t M = (o->n_taps - 1u) / 2u;
    for (uint32_t i = 0; i < o->n_taps; i++) taps[i] = 0.0f;
    for (uint32_t m = 1; m <= M; m += 2u) {
        const float t = (float)((2.0 / (pi * (double)m)) * (0.54 + 0.46 * std::cos(pi * (double)m / (double)(M + 1u))));
        taps[M + m] = t; taps[M - m] = -t;
    }
    return MCRT_OK;
}

extern "C" int mcrt_detect_gain(const float *taps, uint32_t n_taps, double cycles_per_row, double *gain)
{
    static const char fn[] = "mcrt_detect_gain";
    if (!taps || !gain) return mcrt::set_error(MCRT_ERR_INVALID, "%s: null %s", fn, taps ? "gain" : "taps");
    if (!detect_taps_ok(n_taps)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: n_taps must be 3, 7, 11, ..., 63 (%u)", fn, n_taps);
    const double pi = 3.141592653589793;
    const uint32_t M = (n_taps - 1u) / 2u;
    double sum = 0.0;
    for (uint32_t m = 1; m <= M; m += 2u) sum += (double)taps[M + m] * std::sin(2.0 * pi * cycles_per_row * (double)m);
    *gain = std::fabs(2.0 * sum);
    return MCRT_OK;
}

extern "C" int mcrt_psf_carrier(float freq_mhz, uint32_t res_um, double *cycles_per_row)
{
    if (!cycles_per_row) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_psf_carrier: null cycles_per_row");
    const double c = (double)freq_mhz * ((double)res_um / 1000.0);
    *cycles_per_row = std::fabs(c - std::rint(c));
    return MCRT_OK;
}

// ---- transducer<N>::transducer (transducer.h:24-62) -------------------------------------------
namespace {
struct F3 { float x, y, z; };
inline F3 rot(F3 v, F3 ax, float ang)   // btVector3::rotate
{
    const float d = ax.x * v.x + ax.y * v.y + ax.z * v.z;
    const F3 o{ ax.x * d, ax.y * d, ax.z * d };
    const F3 xx{ v.x - o.x, v.y - o.y, v.z - o.z };
    const F3 yy{ ax.y * v.z - ax.z * v.y, ax.z * v.x - ax.x * v.z, ax.x * v.y - ax.y * v.x };
    const float c = std::cos(ang), s = std::sin(ang);
    return F3{ o.x + xx.x * c + yy.x * s, o.y + xx.y * c + yy.y * s, o.z + xx.z * c + yy.z * s };
}
}  // namespace

// transducer.h:24-62; steer (mcrt_transducer_steered) tilts the directions alone: the beams pivot on their elements; tilt (mcrt_transducer_swept)
// turns the whole array about the line parallel to x through (0, pivot_cm, 0) of the probe-local frame.  At most one of the two is non-zero
static void transducer_tables(uint32_t n, double radius_cm, double sep_mm, const float position[3], const float angles_deg[3], float steer, float *pos, float *dir,
                              float tilt = 0.0f, float pivot_cm = 0.0f)
{
    const double pi = 3.14159265358979323846264338327950288419716939937510;   // units.h:360
    const double xa = (angles_deg[0] * pi * 1.0) / 180.0, ya = (angles_deg[1] * pi * 1.0) / 180.0, za = (angles_deg[2] * pi * 1.0) / 180.0;
    const float amp = (float)(((sep_mm / radius_cm) * 1.0) / 10.0);   // mm/cm -> scalar
    const double amplitude = amp;
    double angle = -(amplitude * (double)n / 2.0) + amplitude / 2.0;
    const float rf = (float)radius_cm;
    for (uint32_t t = 0; t < n; t++) {
        const float a = (float)angle;
        if (tilt != 0.0f) {
            const float s = std::sin(a), c = std::cos(a), ct = std::cos(tilt), st = std::sin(tilt), yp = pivot_cm;
            F3 d{ s, c * ct, c * st }, q{ rf * s, yp + (rf * c - yp) * ct, (rf * c - yp) * st };
            d = rot(d, F3{ 0, 0, 1 }, (float)za); q = rot(q, F3{ 0, 0, 1 }, (float)za);
            d = rot(d, F3{ 1, 0, 0 }, (float)xa); q = rot(q, F3{ 1, 0, 0 }, (float)xa);
            d = rot(d, F3{ 0, 1, 0 }, (float)ya); q = rot(q, F3{ 0, 1, 0 }, (float)ya);
            pos[3 * t] = position[0] + q.x; pos[3 * t + 1] = position[1] + q.y; pos[3 * t + 2] = position[2] + q.z;
            dir[3 * t] = d.x; dir[3 * t + 1] = d.y; dir[3 * t + 2] = d.z;
            angle = angle + amplitude;
            continue;
        }
        F3 d{ std::sin(a), std::cos(a), 0.f };
        d = rot(d, F3{ 0, 0, 1 }, (float)za);
        d = rot(d, F3{ 1, 0, 0 }, (float)xa);
        d = rot(d, F3{ 0, 1, 0 }, (float)ya);
        pos[3 * t] = position[0] + rf * d.x; pos[3 * t + 1] = position[1] + rf * d.y; pos[3 * t + 2] = position[2] + rf * d.z;
        if (steer != 0.0f) {
            const float as = (float)(angle + (double)steer);
            d = F3{ std::sin(as), std::cos(as), 0.f };
            d = rot(d, F3{ 0, 0, 1 }, (float)za);
            d = rot(d, F3{ 1, 0, 0 }, (float)xa);
            d = rot(d, F3{ 0, 1, 0 }, (float)ya);
        }
        dir[3 * t] = d.x; dir[3 * t + 1] = d.y; dir[3 * t + 2] = d.z;
        angle = angle + amplitude;
    }
}

extern "C" int mcrt_transducer_elements(uint32_t n, double radius_cm, double sep_mm, const float position[3], const float angles_deg[3], float *pos, float *dir)
{
    if (!pos || !dir || !position || !angles_deg || n == 0) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_transducer_elements: bad arguments");
    transducer_tables(n, radius_cm, sep_mm, position, angles_deg, 0.0f, pos, dir);
    return MCRT_OK;
}

// ---- spatial compounding (the contracts are in include/mcrt.h) ----------------------------------
static bool steer_ok(float s) { return std::isfinite(s) && std::fabs((double)s) < 1.57079632679489661923; }

extern "C" int mcrt_transducer_steered(uint32_t n, double radius_cm, double sep_mm, const float position[3], const float angles_deg[3], float steer_rad,
                                       float *pos, float *dir)
{
    if (!pos || !dir || !position || !angles_deg || n == 0) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_transducer_steered: bad arguments");
    if (!steer_ok(steer_rad)) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_transducer_steered: steer_rad must be finite and |steer| < pi/2 (%g)", (double)steer_rad);
    transducer_tables(n, radius_cm, sep_mm, position, angles_deg, steer_rad, pos, dir);
    return MCRT_OK;
}

// the weight view `steer_rad` contributes with at every pixel (include/mcrt.h): k_compound's own float expression -- the coverage rule on the
// floors of the maps, the lateral ramp of the column map, the view weight -- over mcrt_compound_maps' maps
extern "C" int mcrt_compound_weights(uint32_t E, uint32_t R, double radius_mm, double total_angle, uint32_t max_travel_us, uint32_t speed_of_sound,
                                     uint32_t orows, uint32_t ocols, float steer_rad, float view_weight, float feather_lines, float *w)
{
    if (!w) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_compound_weights: null w");
    if (!(std::isfinite(view_weight) && view_weight >= 0.0f)) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_compound_weights: view_weight must be finite and >= 0 (%g)", (double)view_weight);
    if (!(std::isfinite(feather_lines) && feather_lines >= 0.0f)) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_compound_weights: feather_lines must be finite and >= 0 (%g)", (double)feather_lines);
    if (E == 0 || R == 0 || orows == 0 || ocols == 0) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_compound_weights: bad arguments");
    const size_t n = (size_t)orows * ocols;
    std::vector<float> mr(n), mc(n);
    const int rc = mcrt_compound_maps(E, R, radius_mm, total_angle, max_travel_us, speed_of_sound, orows, ocols, steer_rad, mr.data(), mc.data());
    if (rc != MCRT_OK) return rc;
    const float last_line = (float)(E - 1u);
    for (size_t i = 0; i < n; i++) {
        const float mx = mc[i], my = mr[i];
        const float fx = std::floor(mx), fy = std::floor(my);           // (compared as floats: the kernel's integer comparisons without the conversion)
        const bool covered = (mx == mx) && (my == my) && fx >= -1.0f && (double)fx < (double)E && fy >= -1.0f && (double)fy < (double)R;
        const float a = feather_lines > 0.0f ? std::fmin(std::fmax(std::fmin(mx, last_line - mx) / feather_lines, 0.0f), 1.0f) : 1.0f;
        const float wt = view_weight * a;
        w[i] = covered && wt > 0.0f ? wt : 0.0f;
    }
    return MCRT_OK;
}

// ---- slice thickness (psf.h:16-18,42,77; the contracts are in include/mcrt.h) -------------------
// the probe's elevation direction: (0,0,1) through the rotations mcrt_transducer_elements applies to an element's direction
extern "C" int mcrt_transducer_elevation_axis(const float angles_deg[3], float axis[3])
{
    if (!angles_deg || !axis) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_transducer_elevation_axis: null %s", angles_deg ? "axis" : "angles");
    const double pi = 3.14159265358979323846264338327950288419716939937510;   // units.h:360
    const double xa = (angles_deg[0] * pi * 1.0) / 180.0, ya = (angles_deg[1] * pi * 1.0) / 180.0, za = (angles_deg[2] * pi * 1.0) / 180.0;
    F3 d{ 0.f, 0.f, 1.f };
    d = rot(d, F3{ 0, 0, 1 }, (float)za);
    d = rot(d, F3{ 1, 0, 0 }, (float)xa);
    d = rot(d, F3{ 0, 1, 0 }, (float)ya);
    axis[0] = d.x; axis[1] = d.y; axis[2] = d.z;
    return MCRT_OK;
}

namespace {
inline float plane_z_mm(uint32_t k, uint32_t K, uint32_t pitch_um)   // centred: plane (K-1)/2 lies in the probe's own plane
{
    return (float)(((double)k - (double)((K - 1u) / 2u)) * (double)pitch_um / 1000.0);
}
}  // namespace

extern "C" int mcrt_elevation_planes(const float *pos, const float *dir, uint32_t n, const float axis[3], uint32_t K, uint32_t pitch_um,
                                     float *pos_out, float *dir_out, float *z_mm_out)
{
    if (!pos || !dir || !axis || !pos_out || !dir_out) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_elevation_planes: null pointer");
    if (n == 0) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_elevation_planes: no elements");
    if (K == 0 || K > 32) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_elevation_planes: n_planes must be 1..32 (%u)", K);
    if (pitch_um == 0) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_elevation_planes: pitch_um must be > 0");
    if (!(std::isfinite(axis[0]) && std::isfinite(axis[1]) && std::isfinite(axis[2]))) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_elevation_planes: the axis must be finite");
    const float ax[3] = { axis[0], axis[1], axis[2] };                    // (axis may alias an output)
    for (uint32_t k = 0; k < K; k++) {
        const float z = plane_z_mm(k, K, pitch_um);
        const float o = (float)((double)z / 10.0);                        // mm -> scene units (cm)
        if (z_mm_out) z_mm_out[k] = z;
        for (uint32_t e = 0; e < n; e++)
            for (int c = 0; c < 3; c++) {
                const size_t i = 3 * (size_t)e + (size_t)c, j = 3 * ((size_t)k * n + e) + (size_t)c;
                const float shift = o * ax[c];
                pos_out[j] = pos[i] + shift;
                dir_out[j] = dir[i];
            }
    }
    return MCRT_OK;
}

// mcrt_psf_focus_kernels' depth model with var_z, evaluated at the plane positions of mcrt_elevation_planes
extern "C" int mcrt_psf_elevation_kernels(float var_z, uint32_t pitch_um, const mcrt_focus *f, uint32_t n_rows, double row_mm, int normalize,
                                          float *w_rows, uint32_t K)
{
    if (!w_rows) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_psf_elevation_kernels: null w_rows");
    if (K == 0 || K > 32) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_psf_elevation_kernels: n_planes must be 1..32 (%u)", K);
    if (pitch_um == 0) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_psf_elevation_kernels: pitch_um must be > 0");
    if (!(std::isfinite(var_z) && var_z > 0.0f)) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_psf_elevation_kernels: var_z must be finite and > 0");
    if (!(std::isfinite(row_mm) && row_mm > 0.0)) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_psf_elevation_kernels: row_mm must be finite and > 0");
    const uint32_t n_focus = f ? f->n_focus : 0u;
    if (n_focus > 8) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_psf_elevation_kernels: at most 8 foci (%u)", n_focus);
    for (uint32_t j = 0; j < n_focus; j++) {
        if (!(std::isfinite(f->focus_mm[j]) && f->focus_mm[j] >= 0.0f)) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_psf_elevation_kernels: focus_mm[%u] must be finite and >= 0", j);
        if (j > 0 && !(f->focus_mm[j] > f->focus_mm[j - 1])) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_psf_elevation_kernels: foci must be strictly ascending");
    }
    if (n_focus > 0 && !(std::isfinite(f->focal_range_mm) && f->focal_range_mm > 0.0f))
        return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_psf_elevation_kernels: focal_range_mm must be finite and > 0");
    if (n_rows > MCRT_MAX_ROWS) return mcrt::set_error(MCRT_ERR_LIMIT, "mcrt_psf_elevation_kernels: at most %d rows", MCRT_MAX_ROWS);
    double z2[32];
    for (uint32_t k = 0; k < K; k++) { const float z = plane_z_mm(k, K, pitch_um); z2[k] = (double)z * (double)z; }
    for (uint32_t r = 0; r < n_rows; r++) {
        const double z = (double)r * row_mm;
        double var = (double)var_z, g = 1.0;
        if (n_focus > 0) {
            uint32_t best = 0;
            for (uint32_t j = 1; j < n_focus; j++)             // strictly nearer only: a tie keeps the shallower focus
                if (std::fabs(z - (double)f->focus_mm[j]) < std::fabs(z - (double)f->focus_mm[best])) best = j;
            const double q = (z - (double)f->focus_mm[best]) / (double)f->focal_range_mm;
            var = (double)var_z * (1.0 + q * q);
            g = std::sqrt((double)var_z / var);
        }
        double v[32], sum = 0.0;
        for (uint32_t k = 0; k < K; k++) { v[k] = g * std::exp(-0.5 * (z2[k] / var)); sum += v[k]; }
        for (uint32_t k = 0; k < K; k++) w_rows[(size_t)r * K + k] = normalize ? (float)(v[k] / sum) : (float)v[k];
    }
    return MCRT_OK;
}

// rfimage.h:183-215 create_mapping, evaluated once per geometry on the host (as the reference does in its constructor).
// Operand types as C++ gives them to the reference's statements (pinned by tests/golden/ref_probe.json "scan_maps_*": the same
// statements evaluated with the reference's own unit types, compiled from its units.h):
//   :186 ratio: `max_travel_time * speed_of_sound * 0.001f` is an unsigned product times a float = FLOAT (150.0f for 100 us x 1500);
//        `+ radius` stays float; `- radius * cos(angle_f / 2.0)` is double; `/ rows` double; rounded once to float
//   :189 shift_y: millimeter_t (double) * cosf(angle_f / 2.0f)
//   :201-205 fi, fj, r: float throughout            :208 angle: atan2f, widened
//   :211 map_x (row coordinate): float throughout, the divisor the same float depth as in :186
//   :212 map_y (column coordinate): radian_t arithmetic in double, * (float)rf_width, rounded once
// (Rounds 1-3 held the depth as a double -- 150.0000071 -- and divided in double: ratio 0.385048121 instead of 0.385048091.)
extern "C" int mcrt_scan_maps(uint32_t E, uint32_t R, double radius_mm, double total_angle, uint32_t max_travel_us, uint32_t speed_of_sound,
                              uint32_t orows, uint32_t ocols, float *map_row, float *map_col)
{
    if (!map_row || !map_col || E == 0 || R == 0 || orows == 0 || ocols == 0 || !(total_angle > 0.0)) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_scan_maps: bad arguments");
    const float radius_f = (float)radius_mm, ta_f = (float)total_angle;
    const float depth_mm_f = (float)(uint32_t)(max_travel_us * speed_of_sound) * 0.001f;
    const float ratio = (float)(((double)(depth_mm_f + radius_f) - (double)radius_f * std::cos((double)ta_f / 2.0)) / (double)(int)orows);
    const double shift_y = radius_mm * (double)std::cos(ta_f / 2.0f);
    const float half_width = (float)(int)ocols / 2.0f;
    for (uint32_t j = 0; j < ocols; j++)
        for (uint32_t i = 0; i < orows; i++) {
            const float fi = (float)(int)i + (float)shift_y / ratio;
            const float fj = (float)(int)j - half_width;
            const float r = std::sqrt(fi * fi + fj * fj);
            const double angle = (double)std::atan2(fj, fi);
            map_row[(size_t)i * ocols + j] = (r * ratio - radius_f) / depth_mm_f * (float)R;
            map_col[(size_t)i * ocols + j] = (float)(((angle - (-total_angle / 2)) / total_angle) * (double)(float)E);
        }
    return MCRT_OK;
}

// mcrt_scan_maps for a view whose beams are tilted by steer_rad (include/mcrt.h): the pixel grid is mcrt_scan_maps' own floats, the
// inverse of P = radius u(phi) + t u(phi + steer) is evaluated in double and rounded once
extern "C" int mcrt_compound_maps(uint32_t E, uint32_t R, double radius_mm, double total_angle, uint32_t max_travel_us, uint32_t speed_of_sound,
                                  uint32_t orows, uint32_t ocols, float steer_rad, float *map_row, float *map_col)
{
    if (!map_row || !map_col || E == 0 || R == 0 || orows == 0 || ocols == 0 || !(total_angle > 0.0)) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_compound_maps: bad arguments");
    if (!steer_ok(steer_rad)) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_compound_maps: steer_rad must be finite and |steer| < pi/2 (%g)", (double)steer_rad);
    if (steer_rad == 0.0f) return mcrt_scan_maps(E, R, radius_mm, total_angle, max_travel_us, speed_of_sound, orows, ocols, map_row, map_col);
    const float radius_f = (float)radius_mm, ta_f = (float)total_angle;
    const float depth_mm_f = (float)(uint32_t)(max_travel_us * speed_of_sound) * 0.001f;
    const float ratio = (float)(((double)(depth_mm_f + radius_f) - (double)radius_f * std::cos((double)ta_f / 2.0)) / (double)(int)orows);
    const double shift_y = radius_mm * (double)std::cos(ta_f / 2.0f);
    const float half_width = (float)(int)ocols / 2.0f;
    const double steer = (double)steer_rad, q = radius_mm * std::sin(steer), along = radius_mm * std::cos(steer);
    const float nan = std::numeric_limits<float>::quiet_NaN();
    for (uint32_t j = 0; j < ocols; j++)
        for (uint32_t i = 0; i < orows; i++) {
            const float fi = (float)(int)i + (float)shift_y / ratio;
            const float fj = (float)(int)j - half_width;
            const double x = (double)fj * (double)ratio, y = (double)fi * (double)ratio;
            const double rho = std::sqrt(x * x + y * y), alpha = std::atan2(x, y);
            const size_t o = (size_t)i * ocols + j;
            if (rho < std::fabs(q)) { map_row[o] = nan; map_col[o] = nan; continue; }   // no beam of this view passes the pixel
            const double phi = alpha - steer + std::asin(q / rho);
            const double t = std::sqrt(rho * rho - q * q) - along;
            map_row[o] = (float)(t / (double)depth_mm_f * (double)R);
            map_col[o] = (float)((phi + total_angle / 2) / total_angle * (double)(float)E);
        }
    return MCRT_OK;
}

// ---- volume imaging (the contracts are in include/mcrt.h) ---------------------------------------
extern "C" int mcrt_transducer_swept(uint32_t n, double radius_cm, double sep_mm, const float position[3], const float angles_deg[3], float tilt_rad,
                                     float pivot_mm, float *pos, float *dir)
{
    if (!pos || !dir || !position || !angles_deg || n == 0) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_transducer_swept: bad arguments");
    if (!steer_ok(tilt_rad)) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_transducer_swept: tilt_rad must be finite and |tilt| < pi/2 (%g)", (double)tilt_rad);
    if (!std::isfinite(pivot_mm)) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_transducer_swept: pivot_mm must be finite");
    transducer_tables(n, radius_cm, sep_mm, position, angles_deg, 0.0f, pos, dir, tilt_rad, (float)(pivot_mm / 10.0));
    return MCRT_OK;
}

// what every volume call checks of its sweep and grid (fn: the caller's name, for the message)
int mcrt::volume_check(const char *fn, const mcrt_sweep *sw, const mcrt_volume_grid *g)
{
    if (!sw || !g) return mcrt::set_error(MCRT_ERR_INVALID, "%s: null %s", fn, sw ? "grid" : "sweep");
    if (sw->n_planes == 0 || sw->n_planes > 256) return mcrt::set_error(MCRT_ERR_INVALID, "%s: n_planes must be 1..256 (%u)", fn, sw->n_planes);
    if (!(std::isfinite(sw->step_rad) && sw->step_rad > 0.0f && (double)(sw->n_planes - 1u) / 2.0 * (double)sw->step_rad < 1.57079632679489661923))
        return mcrt::set_error(MCRT_ERR_INVALID, "%s: step_rad must be finite, > 0 and keep every plane's tilt below pi/2 (%g x %u planes)", fn, (double)sw->step_rad, sw->n_planes);
    if (!std::isfinite(sw->pivot_mm)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: pivot_mm must be finite", fn);
    if (g->nu == 0 || g->nv == 0 || g->nw == 0) return mcrt::set_error(MCRT_ERR_INVALID, "%s: zero grid size (%u x %u x %u)", fn, g->nu, g->nv, g->nw);
    for (int i = 0; i < 3; i++)
        if (!(std::isfinite(g->origin_mm[i]) && std::isfinite(g->du_mm[i]) && std::isfinite(g->dv_mm[i]) && std::isfinite(g->dw_mm[i])))
            return mcrt::set_error(MCRT_ERR_INVALID, "%s: the grid has an entry that is not finite (component %d)", fn, i);
    if ((double)g->nu * (double)g->nv * (double)g->nw >= 0x1p31) return mcrt::set_error(MCRT_ERR_LIMIT, "%s: 2^31 output points or more (%u x %u x %u)", fn, g->nu, g->nv, g->nw);
    return MCRT_OK;
}

// the inverse of the swept probe's forward geometry at every grid point, in double, rounded once
extern "C" int mcrt_volume_maps(uint32_t E, uint32_t R, double radius_mm, double total_angle, uint32_t max_travel_us, uint32_t speed_of_sound,
                                const mcrt_sweep *sw, const mcrt_volume_grid *g, float *map_plane, float *map_row, float *map_col)
{
    if (!map_plane || !map_row || !map_col || E == 0 || R == 0 || !(total_angle > 0.0)) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_volume_maps: bad arguments");
    { const int rc = mcrt::volume_check("mcrt_volume_maps", sw, g); if (rc != MCRT_OK) return rc; }
    const float depth_mm_f = (float)(uint32_t)(max_travel_us * speed_of_sound) * 0.001f;
    const double pivot = (double)sw->pivot_mm, step = (double)sw->step_rad, mid = (double)(sw->n_planes - 1u) / 2.0;
    size_t o = 0;
    for (uint32_t l = 0; l < g->nw; l++)
        for (uint32_t j = 0; j < g->nv; j++)
            for (uint32_t i = 0; i < g->nu; i++, o++) {
                double P[3];
                for (int k = 0; k < 3; k++) P[k] = ((g->origin_mm[k] + (double)i * g->du_mm[k]) + (double)j * g->dv_mm[k]) + (double)l * g->dw_mm[k];
                const double yr = P[1] - pivot;
                const double h = std::sqrt(yr * yr + P[2] * P[2]), theta = std::atan2(P[2], yr);
                const double y = pivot + h;
                const double rho = std::sqrt(P[0] * P[0] + y * y), alpha = std::atan2(P[0], y);
                map_plane[o] = (float)(theta / step + mid);
                map_row[o] = (float)((rho - radius_mm) / (double)depth_mm_f * (double)R);
                map_col[o] = (float)((alpha + total_angle / 2) / total_angle * (double)(float)E);
            }
    return MCRT_OK;
}

// ---- speckle reduction (the contract is in include/mcrt.h) ---------------------------------------
extern "C" int mcrt_default_speckle_opts(mcrt_speckle_opts *o)
{
    if (!o) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_default_speckle_opts: null options");
    o->n_iter = 20u; o->q0 = 0.5227232f; o->rho = (float)(1.0 / 6.0); o->lambda = 0.5f;
    return MCRT_OK;
}

// what mcrt_speckle_tables and mcrt_speckle3d_tables check of n_iter, q0, rho and lambda, and the tables [n_iter] and 0.25 * lambda they share:
// in double, each float rounded once, into a, b and l4 (the caller's own: nothing of the user's is written here)
static int speckle_tables_checked(const char *fn, uint32_t n_iter, float q0, float rho, float lambda, const float *q0sq, const float *kq, float a[256], float b[256], float *l4)
{
    if (n_iter > 256u) return mcrt::set_error(MCRT_ERR_LIMIT, "%s: n_iter must be 0..256 (%u)", fn, n_iter);
    if (n_iter && (!q0sq || !kq)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: null %s", fn, q0sq ? "kq" : "q0sq");
    if (!(std::isfinite(q0) && q0 > 0.0f)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: q0 must be finite and > 0 (%g)", fn, (double)q0);
    if (!(std::isfinite(rho) && rho >= 0.0f)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: rho must be finite and >= 0 (%g)", fn, (double)rho);
    if (!(lambda > 0.0f && lambda <= 1.0f)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: lambda must be in (0,1] (%g)", fn, (double)lambda);
    *l4 = (float)(0.25 * (double)lambda);
    if (!(std::isfinite(*l4) && *l4 != 0.0f)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: lambda is too small, 0.25 * lambda is no float above 0 (%g)", fn, (double)lambda);
    for (uint32_t t = 0; t < n_iter; t++) {
        const double q = (double)q0 * std::exp(-(double)rho * (double)t), q2 = q * q;
        a[t] = (float)q2; b[t] = (float)(1.0 / (q2 * (1.0 + q2)));
        if (!(std::isfinite(a[t]) && a[t] != 0.0f && std::isfinite(b[t]) && b[t] != 0.0f))
            return mcrt::set_error(MCRT_ERR_INVALID, "%s: q0, rho: the speckle scale of iteration %u has no finite non-zero tables (q_t^2 %g)", fn, t, q2);
    }
    return MCRT_OK;
}

extern "C" int mcrt_speckle_tables(const mcrt_speckle_opts *o, float *q0sq, float *kq, float *lam4)
{
    static const char fn[] = "mcrt_speckle_tables";
    if (!o || !lam4) return mcrt::set_error(MCRT_ERR_INVALID, "%s: null %s", fn, o ? "lam4" : "options");
    float a[256], b[256], l4 = 0.0f;
    if (const int rc = speckle_tables_checked(fn, o->n_iter, o->q0, o->rho, o->lambda, q0sq, kq, a, b, &l4)) return rc;
    for (uint32_t t = 0; t < o->n_iter; t++) { q0sq[t] = a[t]; kq[t] = b[t]; }
    *lam4 = l4;
    return MCRT_OK;
}

// ---- 3-D speckle reduction over voxel blocks (the contract is in include/mcrt.h) ---------------------------------------
extern "C" int mcrt_default_speckle3d_opts(mcrt_speckle3d_opts *o)
{
    if (!o) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_default_speckle3d_opts: null options");
    o->n_iter = 20u; o->q0 = 0.5227232f; o->rho = (float)(1.0 / 6.0); o->lambda = 0.5f;
    o->weight[0] = o->weight[1] = o->weight[2] = 1.0f;
    return MCRT_OK;
}

// (h_min / h_a)^2 per axis that has more than one voxel; everything is checked before anything is written
extern "C" int mcrt_speckle3d_weights(const mcrt_volume_grid *g, float weight[3])
{
    static const char fn[] = "mcrt_speckle3d_weights";
    if (!g || !weight) return mcrt::set_error(MCRT_ERR_INVALID, "%s: null %s", fn, g ? "weight" : "grid");
    if (g->nu == 0 || g->nv == 0 || g->nw == 0) return mcrt::set_error(MCRT_ERR_INVALID, "%s: grid: zero size (%u x %u x %u)", fn, g->nu, g->nv, g->nw);
    for (int i = 0; i < 3; i++)
        if (!(std::isfinite(g->origin_mm[i]) && std::isfinite(g->du_mm[i]) && std::isfinite(g->dv_mm[i]) && std::isfinite(g->dw_mm[i])))
            return mcrt::set_error(MCRT_ERR_INVALID, "%s: grid: an entry is not finite (component %d)", fn, i);
    const double *axis[3] = { g->du_mm, g->dv_mm, g->dw_mm };
    const uint32_t count[3] = { g->nu, g->nv, g->nw };
    static const char *const name[3] = { "du_mm", "dv_mm", "dw_mm" };
    if (count[0] == 1u && count[1] == 1u && count[2] == 1u) return mcrt::set_error(MCRT_ERR_INVALID, "%s: grid: nu, nv and nw are all 1: a single voxel has no neighbours", fn);
    double h[3], h_min = HUGE_VAL;
    for (int k = 0; k < 3; k++) {
        h[k] = std::sqrt(axis[k][0] * axis[k][0] + axis[k][1] * axis[k][1] + axis[k][2] * axis[k][2]);
        if (count[k] == 1u) continue;
        if (!(std::isfinite(h[k]) && h[k] > 0.0)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: grid: %s has length %g on an axis of %u voxels", fn, name[k], h[k], count[k]);
        h_min = std::min(h_min, h[k]);
    }
    float w[3];
    for (int k = 0; k < 3; k++) {
        const double q = h_min / h[k];
        w[k] = count[k] == 1u ? 0.0f : (float)(q * q);
        if (!std::isfinite(w[k])) return mcrt::set_error(MCRT_ERR_INVALID, "%s: grid: the weight of %s is not finite", fn, name[k]);
    }
    for (int k = 0; k < 3; k++) weight[k] = w[k];
    return MCRT_OK;
}

// in double, each float rounded once; everything is checked before anything is written
extern "C" int mcrt_speckle3d_tables(const mcrt_speckle3d_opts *o, float *q0sq, float *kq, float k[4])
{
    static const char fn[] = "mcrt_speckle3d_tables";
    if (!o || !k) return mcrt::set_error(MCRT_ERR_INVALID, "%s: null %s", fn, o ? "k" : "options");
    float a[256], b[256], l4 = 0.0f;
    if (const int rc = speckle_tables_checked(fn, o->n_iter, o->q0, o->rho, o->lambda, q0sq, kq, a, b, &l4)) return rc;
    for (int i = 0; i < 3; i++)
        if (!(std::isfinite(o->weight[i]) && o->weight[i] >= 0.0f)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: weight[%d] must be finite and >= 0 (%g)", fn, i, (double)o->weight[i]);
    const double sw = ((double)o->weight[0] + (double)o->weight[1]) + (double)o->weight[2];
    if (!(sw > 0.0)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: weight: the sum of the weights must be > 0 (%g)", fn, sw);
    const float c[4] = { (float)(1.0 / sw), (float)(1.0 / (4.0 * sw * sw)), (float)(1.0 / (2.0 * sw)), (float)((double)o->lambda / (2.0 * sw)) };
    static const char *const name[4] = { "a = 1 / sw", "b = 1 / (4 sw^2)", "hs = 1 / (2 sw)", "lamw = lambda / (2 sw)" };
    for (int i = 0; i < 4; i++)
        if (!(std::isfinite(c[i]) && c[i] != 0.0f)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: weight, lambda: %s is no finite float above 0 (sum of the weights %g)", fn, name[i], sw);
    for (uint32_t t = 0; t < o->n_iter; t++) { q0sq[t] = a[t]; kq[t] = b[t]; }
    for (int i = 0; i < 4; i++) k[i] = c[i];
    return MCRT_OK;
}

// ---- freehand 3-D reconstruction (the contract is in include/mcrt.h) ---------------------------------------
extern "C" int mcrt_default_recon_opts(mcrt_recon_opts *o)
{
    if (!o) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_default_recon_opts: null options");
    o->mode = MCRT_RECON_MEAN; o->value_max = 1024.0f; o->fill_radius = 1u; o->fill_min = 1u; o->empty = 0.0f;
    return MCRT_OK;
}

// world millimetres -> voxel index, as floats that take scene units: in double, each float rounded once; checked before anything is written
extern "C" int mcrt_recon_transform(const mcrt_volume_grid *g, double unit_mm, float A[9], float b[3])
{
    static const char fn[] = "mcrt_recon_transform";
    if (!g || !A || !b) return mcrt::set_error(MCRT_ERR_INVALID, "%s: null %s", fn, !g ? "grid" : !A ? "A" : "b");
    if (!(std::isfinite(unit_mm) && unit_mm > 0.0)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: unit_mm must be finite and > 0 (%g)", fn, unit_mm);
    if (g->nu == 0 || g->nv == 0 || g->nw == 0) return mcrt::set_error(MCRT_ERR_INVALID, "%s: grid: zero size (%u x %u x %u)", fn, g->nu, g->nv, g->nw);
    for (int i = 0; i < 3; i++)
        if (!(std::isfinite(g->origin_mm[i]) && std::isfinite(g->du_mm[i]) && std::isfinite(g->dv_mm[i]) && std::isfinite(g->dw_mm[i])))
            return mcrt::set_error(MCRT_ERR_INVALID, "%s: grid: an entry is not finite (component %d)", fn, i);
    auto norm = [](const double v[3]) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); };
    auto cross = [](const double x[3], const double y[3], double o[3]) { o[0] = x[1] * y[2] - x[2] * y[1]; o[1] = x[2] * y[0] - x[0] * y[2]; o[2] = x[0] * y[1] - x[1] * y[0]; };
    const double *du = g->du_mm, *dv = g->dv_mm, *dw = g->dw_mm, *org = g->origin_mm;
    double r[3][3];
    cross(dv, dw, r[0]); cross(dw, du, r[1]); cross(du, dv, r[2]);
    const double det = du[0] * r[0][0] + du[1] * r[0][1] + du[2] * r[0][2];
    if (!(std::isfinite(det) && std::fabs(det) > 1e-12 * norm(du) * norm(dv) * norm(dw)))
        return mcrt::set_error(MCRT_ERR_INVALID, "%s: grid: the axes du_mm, dv_mm, dw_mm do not span space", fn);
    float fa[9], fb[3];
    for (int c = 0; c < 3; c++) {
        double m[3];
        for (int k = 0; k < 3; k++) { m[k] = r[c][k] / det; fa[3 * c + k] = (float)(m[k] * unit_mm); }
        fb[c] = (float)(-((m[0] * org[0] + m[1] * org[1]) + m[2] * org[2]));
    }
    for (int i = 0; i < 9; i++)
        if (!std::isfinite(fa[i])) return mcrt::set_error(MCRT_ERR_INVALID, "%s: grid: entry %d of A is no finite float (%g)", fn, i, (double)fa[i]);
    for (int i = 0; i < 3; i++)
        if (!std::isfinite(fb[i])) return mcrt::set_error(MCRT_ERR_INVALID, "%s: grid: entry %d of b is no finite float (%g)", fn, i, (double)fb[i]);
    for (int i = 0; i < 9; i++) A[i] = fa[i];
    for (int i = 0; i < 3; i++) b[i] = fb[i];
    return MCRT_OK;
}

// ---- acoustic ground truth (the contract is in include/mcrt.h): the defaults, and the boundary rule k_transmit applies (mcrt_transmit.h) ----
extern "C" int mcrt_default_transmit_opts(mcrt_transmit_opts *o)
{
    if (!o) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_default_transmit_opts: null options");
    o->mode = MCRT_TRANSMIT_TOTAL; o->rule = MCRT_LABEL_TRACED; o->start_offset = -1.0f;
    return MCRT_OK;
}

extern "C" int mcrt_transmit_boundary(float z_before, float z_after, float inc, float intensity, float *i_refl, float *i_refr)
{
    if (!i_refl || !i_refr) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_transmit_boundary: null %s", i_refl ? "i_refr" : "i_refl");
    mcrt::transmit_boundary(z_before, z_after, inc, intensity, *i_refl, *i_refr);
    return MCRT_OK;
}

extern "C" int mcrt_default_recon_label_opts(mcrt_recon_label_opts *o, uint32_t n_labels)
{
    if (!o) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_default_recon_label_opts: null options");
    o->n_labels = n_labels; o->fill_radius = 1u; o->fill_min = 1u;       // (mcrt_default_recon_opts' own: the two volumes fill the same holes)
    return MCRT_OK;
}

// ---- receiver noise (the contract is in include/mcrt.h) ---------------------------------------
extern "C" int mcrt_default_noise_opts(mcrt_noise_opts *o)
{
    if (!o) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_default_noise_opts: null options");
    o->mode = MCRT_NOISE_SNR_DB; o->snr_db = 50.0f; o->sigma = 0.0f; o->seed = 0x4E4F4953u;
    return MCRT_OK;
}

// Philox4x32-10 on the host, as mcrt_detmath.h has it on the device (Salmon, Moraes, Dror, Shaw, SC'11)
static void host_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4])
{
    for (int i = 0; i < 10; i++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// the draws k_noise makes for one image, [E][R]
extern "C" int mcrt_noise_draws(uint32_t seed, uint32_t image_id, uint32_t n_elements, uint32_t n_rows, int32_t *d)
{
    static const char fn[] = "mcrt_noise_draws";
    if (!d) return mcrt::set_error(MCRT_ERR_INVALID, "%s: null d", fn);
    if (n_elements == 0 || n_rows == 0) return mcrt::set_error(MCRT_ERR_INVALID, "%s: zero sizes (n_elements %u, n_rows %u)", fn, n_elements, n_rows);
    if (n_rows > 2048u) return mcrt::set_error(MCRT_ERR_LIMIT, "%s: n_rows: at most 2048 rows (%u)", fn, n_rows);
    for (uint32_t e = 0; e < n_elements; e++)
        for (uint32_t r = 0; r < n_rows; r++) {
            uint32_t o[4], s = 0;
            host_philox4x32_10(e, r, 0x4E4F4953u, 0u, seed, image_id, o);
            for (int k = 0; k < 4; k++) s += (o[k] & 0xffffu) + (o[k] >> 16);
            d[(size_t)e * n_rows + r] = (int32_t)s - 262140;
        }
    return MCRT_OK;
}

// ---- colour Doppler (the contracts are in include/mcrt.h) ---------------------------------------
extern "C" int mcrt_default_flow_opts(mcrt_flow_opts *o)
{
    if (!o) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_default_flow_opts: null options");
    o->n_packets = 8u; o->wall = MCRT_FLOW_WALL_MEAN; o->avg_rows = 2u; o->avg_lines = 1u;
    o->prf_hz = 4000.0f; o->freq_mhz = 0.0f; o->sigma = 0.0f; o->seed = 0x464C4F57u;
    return MCRT_OK;
}

int mcrt::flow_check(const char *fn, const mcrt_flow_opts *o)
{
    if (o->n_packets < 2u || o->n_packets > 16u) return set_error(MCRT_ERR_INVALID, "%s: n_packets must be 2 .. 16 (%u)", fn, o->n_packets);
    if (o->wall > MCRT_FLOW_WALL_LINEAR) return set_error(MCRT_ERR_INVALID, "%s: unknown wall filter %u", fn, o->wall);
    if (o->avg_rows > 8u) return set_error(MCRT_ERR_INVALID, "%s: avg_rows must be 0 .. 8 (%u)", fn, o->avg_rows);
    if (o->avg_lines > 4u) return set_error(MCRT_ERR_INVALID, "%s: avg_lines must be 0 .. 4 (%u)", fn, o->avg_lines);
    if (!(std::isfinite(o->prf_hz) && o->prf_hz > 0.0f)) return set_error(MCRT_ERR_INVALID, "%s: prf_hz must be finite and > 0 (%g)", fn, (double)o->prf_hz);
    if (!std::isfinite(o->freq_mhz)) return set_error(MCRT_ERR_INVALID, "%s: freq_mhz must be finite (%g)", fn, (double)o->freq_mhz);
    if (!(std::isfinite(o->sigma) && o->sigma >= 0.0f)) return set_error(MCRT_ERR_INVALID, "%s: sigma must be finite and >= 0 (%g)", fn, (double)o->sigma);
    return MCRT_OK;
}

extern "C" int mcrt_flow_nyquist(const mcrt_flow_opts *o, double freq_mhz, double speed_of_sound, double *v_nyq_mm_s)
{
    static const char fn[] = "mcrt_flow_nyquist";
    if (!o || !v_nyq_mm_s) return mcrt::set_error(MCRT_ERR_INVALID, "%s: null %s", fn, o ? "v_nyq_mm_s" : "options");
    if (const int rc = mcrt::flow_check(fn, o)) return rc;
    const double f = o->freq_mhz > 0.0f ? (double)o->freq_mhz : freq_mhz;
    if (!(std::isfinite(f) && f > 0.0)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: the frequency must be finite and > 0 (%g)", fn, f);
    if (!(std::isfinite(speed_of_sound) && speed_of_sound > 0.0)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: speed_of_sound must be finite and > 0 (%g)", fn, speed_of_sound);
    *v_nyq_mm_s = (speed_of_sound * 1000.0 * (double)o->prf_hz) / (4.0 * (f * 1.0e6));
    return MCRT_OK;
}

extern "C" int mcrt_flow_phasors(double v_nyq_mm_s, const float *vel_mm_s, const float *dir, uint32_t n_labels, uint32_t n_elements, float *phasor, float *truth)
{
    static const char fn[] = "mcrt_flow_phasors";
    if (!vel_mm_s || !dir || !phasor || !truth) return mcrt::set_error(MCRT_ERR_INVALID, "%s: null pointer", fn);
    if (n_labels == 0 || n_elements == 0) return mcrt::set_error(MCRT_ERR_INVALID, "%s: zero sizes (n_labels %u, n_elements %u)", fn, n_labels, n_elements);
    if (n_labels > 254u) return mcrt::set_error(MCRT_ERR_LIMIT, "%s: at most 254 labels (%u)", fn, n_labels);
    if (!(std::isfinite(v_nyq_mm_s) && v_nyq_mm_s > 0.0)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: v_nyq_mm_s must be finite and > 0 (%g)", fn, v_nyq_mm_s);
    for (size_t i = 0; i < (size_t)n_labels * 3u; i++)
        if (!std::isfinite(vel_mm_s[i])) return mcrt::set_error(MCRT_ERR_INVALID, "%s: vel_mm_s[%zu][%zu] is not finite", fn, i / 3u, i % 3u);
    for (size_t i = 0; i < (size_t)n_elements * 3u; i++)
        if (!std::isfinite(dir[i])) return mcrt::set_error(MCRT_ERR_INVALID, "%s: dir[%zu][%zu] is not finite", fn, i / 3u, i % 3u);
    const double pi = 3.141592653589793;
    for (uint32_t l = 0; l < n_labels; l++) {
        const double vx = vel_mm_s[3u * l], vy = vel_mm_s[3u * l + 1u], vz = vel_mm_s[3u * l + 2u];
        const bool rest = vx == 0.0 && vy == 0.0 && vz == 0.0;
        for (uint32_t e = 0; e < n_elements; e++) {
            const size_t i = (size_t)l * n_elements + e;
            if (rest) { truth[i] = 0.0f; phasor[2u * i] = 1.0f; phasor[2u * i + 1u] = 0.0f; continue; }
            const double dx = dir[3u * e], dy = dir[3u * e + 1u], dz = dir[3u * e + 2u];
            const double v_t = 0.0 - ((vx * dx + vy * dy) + vz * dz);
            const double phi = pi * v_t / v_nyq_mm_s;
            truth[i] = (float)v_t; phasor[2u * i] = (float)std::cos(phi); phasor[2u * i + 1u] = (float)std::sin(phi);
        }
    }
    return MCRT_OK;
}

// the draws k_flow makes for one image's ensemble, [N][E][R][2]
extern "C" int mcrt_flow_draws(uint32_t seed, uint32_t image_id, uint32_t n_elements, uint32_t n_rows, uint32_t n_packets, int32_t *d)
{
    static const char fn[] = "mcrt_flow_draws";
    if (!d) return mcrt::set_error(MCRT_ERR_INVALID, "%s: null d", fn);
    if (n_elements == 0 || n_rows == 0) return mcrt::set_error(MCRT_ERR_INVALID, "%s: zero sizes (n_elements %u, n_rows %u)", fn, n_elements, n_rows);
    if (n_packets < 2u || n_packets > 16u) return mcrt::set_error(MCRT_ERR_INVALID, "%s: n_packets must be 2 .. 16 (%u)", fn, n_packets);
    if (n_rows > 2048u) return mcrt::set_error(MCRT_ERR_LIMIT, "%s: n_rows: at most 2048 rows (%u)", fn, n_rows);
    for (uint32_t n = 0; n < n_packets; n++)
        for (uint32_t e = 0; e < n_elements; e++)
            for (uint32_t r = 0; r < n_rows; r++) {
                uint32_t o[4];
                host_philox4x32_10(e, r, 0x464C4F57u, n, seed, image_id, o);
                int32_t *p = d + 2u * (((size_t)n * n_elements + e) * n_rows + r);
                p[0] = (int32_t)((o[0] & 0xffffu) + (o[0] >> 16) + (o[1] & 0xffffu) + (o[1] >> 16)) - 131070;
                p[1] = (int32_t)((o[2] & 0xffffu) + (o[2] >> 16) + (o[3] & 0xffffu) + (o[3] >> 16)) - 131070;
            }
    return MCRT_OK;
}

extern "C" int mcrt_colour_map(uint32_t kind, uint8_t *lut)
{
    static const char fn[] = "mcrt_colour_map";
    if (!lut) return mcrt::set_error(MCRT_ERR_INVALID, "%s: null lut", fn);
    if (kind != 0u) return mcrt::set_error(MCRT_ERR_INVALID, "%s: unknown kind %u", fn, kind);
    for (uint32_t i = 1; i < 256u; i++) {
        const uint32_t k = i >= 128u ? i - 128u : 128u - i;
        const uint32_t strong = k == 0u ? 0u : 128u + k, g = k <= 64u ? 0u : (k - 64u) * 4u;
        lut[3u * i] = (uint8_t)(i > 128u ? strong : 0u); lut[3u * i + 1u] = (uint8_t)g; lut[3u * i + 2u] = (uint8_t)(i < 128u ? strong : 0u);
    }
    lut[0] = lut[3]; lut[1] = lut[4]; lut[2] = lut[5];
    return MCRT_OK;
}

extern "C" int mcrt_default_colour_opts(mcrt_colour_opts *o)
{
    if (!o) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_default_colour_opts: null options");
    o->power_thr = 0.0f; o->vel_thr_mm_s = 0.0f; o->grey_max = 255u;
    return MCRT_OK;
}

// ---- spectral Doppler (the contracts are in include/mcrt.h) ---------------------------------------
extern "C" int mcrt_default_spectral_opts(mcrt_spectral_opts *o)
{
    if (!o) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_default_spectral_opts: null options");
    o->n_pulses = 2048u; o->gate_rows = 8u; o->n_fft = 128u; o->hop = 32u; o->wall = MCRT_SPECTRAL_WALL_MEAN; o->wall_bins = 2u;
    o->sigma = 0.0f; o->seed = 0x53504543u;
    return MCRT_OK;
}

extern "C" int mcrt_default_sonogram_opts(mcrt_sonogram_opts *o)
{
    if (!o) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_default_sonogram_opts: null options");
    o->dynamic_range_db = 40.0f; o->gain_db = 0.0f; o->ref = 0.0f;
    return MCRT_OK;
}

static bool spectral_fft_size(uint32_t N) { return N == 32u || N == 64u || N == 128u || N == 256u || N == 512u; }

int mcrt::spectral_check(const char *fn, const mcrt_spectral_opts *o)
{
    if (o->n_pulses < 1u || o->n_pulses > 16384u) return set_error(MCRT_ERR_INVALID, "%s: n_pulses must be 1 .. 16384 (%u)", fn, o->n_pulses);
    if (o->gate_rows < 1u || o->gate_rows > 64u) return set_error(MCRT_ERR_INVALID, "%s: gate_rows must be 1 .. 64 (%u)", fn, o->gate_rows);
    if (!spectral_fft_size(o->n_fft)) return set_error(MCRT_ERR_INVALID, "%s: n_fft must be 32, 64, 128, 256 or 512 (%u)", fn, o->n_fft);
    if (o->hop < 1u || o->hop > o->n_fft) return set_error(MCRT_ERR_INVALID, "%s: hop must be 1 .. n_fft (%u)", fn, o->hop);
    if (o->wall > MCRT_SPECTRAL_WALL_MEAN) return set_error(MCRT_ERR_INVALID, "%s: unknown wall filter %u", fn, o->wall);
    if (o->wall_bins > o->n_fft / 4u) return set_error(MCRT_ERR_INVALID, "%s: wall_bins must be 0 .. n_fft / 4 (%u)", fn, o->wall_bins);
    if (!(std::isfinite(o->sigma) && o->sigma >= 0.0f)) return set_error(MCRT_ERR_INVALID, "%s: sigma must be finite and >= 0 (%g)", fn, (double)o->sigma);
    return MCRT_OK;
}

extern "C" int mcrt_spectral_rotor(float *lut)
{
    if (!lut) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_spectral_rotor: null lut");
    for (uint32_t i = 0; i < 4096u; i++) {
        const double a = 6.283185307179586 * i / 4096.0;
        lut[2u * i] = (float)std::cos(a); lut[2u * i + 1u] = (float)std::sin(a);
    }
    return MCRT_OK;
}

extern "C" int mcrt_spectral_phase(double v_nyq_mm_s, const float *speed_mm_s, uint32_t T, int64_t *phase)
{
    static const char fn[] = "mcrt_spectral_phase";
    if (!speed_mm_s || !phase) return mcrt::set_error(MCRT_ERR_INVALID, "%s: null pointer", fn);
    if (T == 0) return mcrt::set_error(MCRT_ERR_INVALID, "%s: n_pulses is zero", fn);
    if (T > 16384u) return mcrt::set_error(MCRT_ERR_LIMIT, "%s: at most 16384 pulses (%u)", fn, T);
    if (!(std::isfinite(v_nyq_mm_s) && v_nyq_mm_s > 0.0)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: v_nyq_mm_s must be finite and > 0 (%g)", fn, v_nyq_mm_s);
    for (uint32_t t = 0; t < T; t++) {
        if (!std::isfinite(speed_mm_s[t])) return mcrt::set_error(MCRT_ERR_INVALID, "%s: speed_mm_s[%u] is not finite", fn, t);
        if (std::fabs((double)speed_mm_s[t] / v_nyq_mm_s * 2147483648.0) > 4294967296.5)
            return mcrt::set_error(MCRT_ERR_LIMIT, "%s: speed_mm_s[%u] = %g is more than twice the Nyquist velocity %g", fn, t, (double)speed_mm_s[t], v_nyq_mm_s);
    }
    std::vector<int64_t> step(T);
    for (uint32_t t = 0; t < T; t++) {
        step[t] = (int64_t)std::llrint((double)speed_mm_s[t] / v_nyq_mm_s * 2147483648.0);
        if (step[t] > 4294967296ll || step[t] < -4294967296ll)
            return mcrt::set_error(MCRT_ERR_LIMIT, "%s: speed_mm_s[%u] = %g is more than twice the Nyquist velocity %g", fn, t, (double)speed_mm_s[t], v_nyq_mm_s);
    }
    int64_t p = 0;
    for (uint32_t t = 0; t < T; t++) { phase[t] = p; p += step[t]; }
    return MCRT_OK;
}

extern "C" int mcrt_spectral_profile(const uint8_t *tissue_line, uint32_t R, uint32_t row0, uint32_t G, const uint8_t *moving, uint32_t n_labels, double exponent,
                                     float *frac)
{
    static const char fn[] = "mcrt_spectral_profile";
    if (!tissue_line || !moving || !frac) return mcrt::set_error(MCRT_ERR_INVALID, "%s: null pointer", fn);
    if (R == 0 || G == 0 || n_labels == 0) return mcrt::set_error(MCRT_ERR_INVALID, "%s: zero sizes (n_rows %u, gate_rows %u, n_labels %u)", fn, R, G, n_labels);
    if (G > 64u) return mcrt::set_error(MCRT_ERR_LIMIT, "%s: at most 64 gate rows (%u)", fn, G);
    if (n_labels > 254u) return mcrt::set_error(MCRT_ERR_LIMIT, "%s: at most 254 labels (%u)", fn, n_labels);
    if ((uint64_t)row0 + G > R) return mcrt::set_error(MCRT_ERR_INVALID, "%s: the gate's rows %u .. %llu pass the scan-line's %u", fn, row0, (unsigned long long)row0 + G - 1u, R);
    if (!(std::isfinite(exponent) && (exponent == 0.0 || exponent >= 1.0))) return mcrt::set_error(MCRT_ERR_INVALID, "%s: exponent must be 0 or >= 1 (%g)", fn, exponent);
    for (uint32_t i = 0; i < G; i++) {
        const uint32_t r = row0 + i, l = tissue_line[r];
        if (l >= n_labels || moving[l] == 0) { frac[i] = 0.0f; continue; }
        uint32_t a = r, b = r;
        while (a > 0u && tissue_line[a - 1u] == l) a--;
        while (b + 1u < R && tissue_line[b + 1u] == l) b++;
        const double x = ((double)r - ((double)a + (double)b) / 2.0) / (((double)b - (double)a + 1.0) / 2.0);
        frac[i] = exponent == 0.0 ? 1.0f : (float)(1.0 - std::pow(std::fabs(x), exponent));
    }
    return MCRT_OK;
}

extern "C" int mcrt_spectral_rates(const float *frac, uint32_t G, double axial, int32_t *rate)
{
    static const char fn[] = "mcrt_spectral_rates";
    if (!frac || !rate) return mcrt::set_error(MCRT_ERR_INVALID, "%s: null pointer", fn);
    if (G == 0) return mcrt::set_error(MCRT_ERR_INVALID, "%s: gate_rows is zero", fn);
    if (G > 64u) return mcrt::set_error(MCRT_ERR_LIMIT, "%s: at most 64 gate rows (%u)", fn, G);
    if (!(axial >= -1.0 && axial <= 1.0)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: axial must be in [-1, 1] (%g)", fn, axial);
    for (uint32_t i = 0; i < G; i++)
        if (!(frac[i] >= 0.0f && frac[i] <= 1.0f)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: frac[%u] must be in [0, 1] (%g)", fn, i, (double)frac[i]);
    for (uint32_t i = 0; i < G; i++) rate[i] = (int32_t)std::llrint(65536.0 * (double)frac[i] * axial);
    return MCRT_OK;
}

extern "C" int mcrt_spectral_window(uint32_t kind, uint32_t N, float *h)
{
    static const char fn[] = "mcrt_spectral_window";
    if (!h) return mcrt::set_error(MCRT_ERR_INVALID, "%s: null h", fn);
    if (kind > 1u) return mcrt::set_error(MCRT_ERR_INVALID, "%s: unknown kind %u", fn, kind);
    if (!spectral_fft_size(N)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: n_fft must be 32, 64, 128, 256 or 512 (%u)", fn, N);
    for (uint32_t n = 0; n < N; n++) h[n] = kind == 0u ? 1.0f : (float)(0.5 - 0.5 * std::cos(6.283185307179586 * n / N));
    return MCRT_OK;
}

extern "C" int mcrt_spectral_twiddles(uint32_t N, float *tw)
{
    static const char fn[] = "mcrt_spectral_twiddles";
    if (!tw) return mcrt::set_error(MCRT_ERR_INVALID, "%s: null tw", fn);
    if (!spectral_fft_size(N)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: n_fft must be 32, 64, 128, 256 or 512 (%u)", fn, N);
    for (uint32_t k = 0; k < N / 2u; k++) {
        const double a = 6.283185307179586 * k / N;
        tw[2u * k] = (float)std::cos(a); tw[2u * k + 1u] = (float)(0.0 - std::sin(a));
    }
    return MCRT_OK;
}

// the draws k_gate_series makes for one gate's series, [T][2]
extern "C" int mcrt_spectral_draws(uint32_t seed, uint32_t image_id, uint32_t line, uint32_t row0, uint32_t T, int32_t *d)
{
    static const char fn[] = "mcrt_spectral_draws";
    if (!d) return mcrt::set_error(MCRT_ERR_INVALID, "%s: null d", fn);
    if (T == 0) return mcrt::set_error(MCRT_ERR_INVALID, "%s: n_pulses is zero", fn);
    if (T > 16384u) return mcrt::set_error(MCRT_ERR_LIMIT, "%s: at most 16384 pulses (%u)", fn, T);
    for (uint32_t t = 0; t < T; t++) {
        uint32_t o[4];
        host_philox4x32_10(line, row0, 0x53504543u, t, seed, image_id, o);
        d[2u * t] = (int32_t)((o[0] & 0xffffu) + (o[0] >> 16) + (o[1] & 0xffffu) + (o[1] >> 16)) - 131070;
        d[2u * t + 1u] = (int32_t)((o[2] & 0xffffu) + (o[2] >> 16) + (o[3] & 0xffffu) + (o[3] >> 16)) - 131070;
    }
    return MCRT_OK;
}

extern "C" int mcrt_pulse_waveform(double prf_hz, double beats_per_min, double v_peak, double v_min, uint32_t T, float *speed)
{
    static const char fn[] = "mcrt_pulse_waveform";
    if (!speed) return mcrt::set_error(MCRT_ERR_INVALID, "%s: null speed_mm_s", fn);
    if (T == 0) return mcrt::set_error(MCRT_ERR_INVALID, "%s: n_pulses is zero", fn);
    if (T > 16384u) return mcrt::set_error(MCRT_ERR_LIMIT, "%s: at most 16384 pulses (%u)", fn, T);
    if (!(std::isfinite(prf_hz) && prf_hz > 0.0) || !(std::isfinite(beats_per_min) && beats_per_min > 0.0))
        return mcrt::set_error(MCRT_ERR_INVALID, "%s: prf_hz and beats_per_min must be finite and > 0 (%g, %g)", fn, prf_hz, beats_per_min);
    if (!std::isfinite(v_peak) || !std::isfinite(v_min)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: the speeds must be finite (%g, %g)", fn, v_peak, v_min);
    for (uint32_t t = 0; t < T; t++) {
        const double u = t * beats_per_min / (60.0 * prf_hz), x = u - std::floor(u), s = std::sin(3.141592653589793 * x / 0.3);
        speed[t] = (float)(v_min + (v_peak - v_min) * (x < 0.3 ? s * s : 0.0));
    }
    return MCRT_OK;
}

// ---- strain elastography (the contracts are in include/mcrt.h) ---------------------------------------
extern "C" int mcrt_default_strain_opts(mcrt_strain_opts *o)
{
    if (!o) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_default_strain_opts: null options");
    o->window_rows = 16u; o->search_rows = 8u; o->lsq_rows = 12u; o->sigma = 0.0f; o->seed = 0x5354524Eu;
    return MCRT_OK;
}

extern "C" int mcrt_default_elastogram_opts(mcrt_elastogram_opts *o)
{
    if (!o) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_default_elastogram_opts: null options");
    o->ref_strain = 0.01f; o->rho_min = 0.7f; o->grey_min = 0u; o->alpha = 160u;
    return MCRT_OK;
}

int mcrt::strain_check(const char *fn, const mcrt_strain_opts *o)
{
    if (o->window_rows > 32u) return set_error(MCRT_ERR_INVALID, "%s: window_rows must be 0 .. 32 (%u)", fn, o->window_rows);
    if (o->search_rows > 16u) return set_error(MCRT_ERR_INVALID, "%s: search_rows must be 0 .. 16 (%u)", fn, o->search_rows);
    if (o->lsq_rows < 1u || o->lsq_rows > 32u) return set_error(MCRT_ERR_INVALID, "%s: lsq_rows must be 1 .. 32 (%u)", fn, o->lsq_rows);
    if (!(std::isfinite(o->sigma) && o->sigma >= 0.0f)) return set_error(MCRT_ERR_INVALID, "%s: sigma must be finite and >= 0 (%g)", fn, (double)o->sigma);
    return MCRT_OK;
}

extern "C" int mcrt_strain_table(const double *modulus, uint32_t n_labels, double applied, double ref_modulus, int32_t *eps_q24)
{
    static const char fn[] = "mcrt_strain_table";
    if (!modulus || !eps_q24) return mcrt::set_error(MCRT_ERR_INVALID, "%s: null pointer", fn);
    if (n_labels == 0) return mcrt::set_error(MCRT_ERR_INVALID, "%s: n_labels is zero", fn);
    if (n_labels > 254u) return mcrt::set_error(MCRT_ERR_LIMIT, "%s: at most 254 labels (%u)", fn, n_labels);
    if (!std::isfinite(applied)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: applied must be finite (%g)", fn, applied);
    if (!(std::isfinite(ref_modulus) && ref_modulus > 0.0)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: ref_modulus must be finite and > 0 (%g)", fn, ref_modulus);
    for (uint32_t l = 0; l < n_labels; l++) {
        if (!(std::isfinite(modulus[l]) && modulus[l] >= 0.0)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: modulus[%u] must be finite and >= 0 (%g)", fn, l, modulus[l]);
        if (modulus[l] != 0.0 && !(std::fabs(applied * ref_modulus / modulus[l] * 16777216.0) <= 524288.5))
            return mcrt::set_error(MCRT_ERR_INVALID, "%s: the strain of label %u, %g, is above 1/32", fn, l, applied * ref_modulus / modulus[l]);
    }
    std::vector<int32_t> eps(n_labels);
    for (uint32_t l = 0; l < n_labels; l++) {
        const long long q = modulus[l] == 0.0 ? 0ll : std::llrint(applied * ref_modulus / modulus[l] * 16777216.0);
        if (q > 524288ll || q < -524288ll) return mcrt::set_error(MCRT_ERR_INVALID, "%s: the strain of label %u, %g, is above 1/32", fn, l, applied * ref_modulus / modulus[l]);
        eps[l] = (int32_t)q;
    }
    memcpy(eps_q24, eps.data(), 4 * (size_t)n_labels);
    return MCRT_OK;
}

// the draws k_strain_warp makes for one image, [E][R][2]
extern "C" int mcrt_strain_draws(uint32_t seed, uint32_t image_id, uint32_t n_elements, uint32_t n_rows, int32_t *d)
{
    static const char fn[] = "mcrt_strain_draws";
    if (!d) return mcrt::set_error(MCRT_ERR_INVALID, "%s: null d", fn);
    if (n_elements == 0 || n_rows == 0) return mcrt::set_error(MCRT_ERR_INVALID, "%s: zero sizes (n_elements %u, n_rows %u)", fn, n_elements, n_rows);
    if (n_rows > 2048u) return mcrt::set_error(MCRT_ERR_LIMIT, "%s: n_rows: at most 2048 rows (%u)", fn, n_rows);
    for (uint32_t e = 0; e < n_elements; e++)
        for (uint32_t r = 0; r < n_rows; r++) {
            uint32_t o[4];
            host_philox4x32_10(e, r, 0x5354524Eu, 0u, seed, image_id, o);
            int32_t *p = d + 2u * ((size_t)e * n_rows + r);
            p[0] = (int32_t)((o[0] & 0xffffu) + (o[0] >> 16) + (o[1] & 0xffffu) + (o[1] >> 16)) - 131070;
            p[1] = (int32_t)((o[2] & 0xffffu) + (o[2] >> 16) + (o[3] & 0xffffu) + (o[3] >> 16)) - 131070;
        }
    return MCRT_OK;
}

// kind 0 of mcrt_strain_map and of mcrt_shear_map: blue at 0 through green at 128 to red, in integer arithmetic
static void blue_green_red(uint8_t *lut)
{
    for (uint32_t i = 0; i < 256u; i++) {
        const uint32_t u = i <= 128u ? (2u * i > 255u ? 255u : 2u * i) : 2u * (i - 128u);
        lut[3u * i] = (uint8_t)(i <= 128u ? 0u : u); lut[3u * i + 1u] = (uint8_t)(i <= 128u ? u : 255u - u); lut[3u * i + 2u] = (uint8_t)(i <= 128u ? 255u - u : 0u);
    }
}

extern "C" int mcrt_strain_map(uint32_t kind, uint8_t *lut)
{
    static const char fn[] = "mcrt_strain_map";
    if (!lut) return mcrt::set_error(MCRT_ERR_INVALID, "%s: null lut", fn);
    if (kind != 0u) return mcrt::set_error(MCRT_ERR_INVALID, "%s: unknown kind %u", fn, kind);
    blue_green_red(lut);
    return MCRT_OK;
}

// ---- shear-wave elastography (the contracts are in include/mcrt.h) ---------------------------------------
extern "C" int mcrt_default_shear_opts(mcrt_shear_opts *o)
{
    if (!o) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_default_shear_opts: null options");
    o->n_pulses = 64u; o->window_rows = 8u; o->prf_hz = 10000.0f; o->sigma = 0.0f; o->seed = 0x53484552u;
    o->push_line = 0u; o->push_row0 = 0u; o->push_rows = 0u; o->peak_q24 = 1677722; o->speed_lines = 4u; o->avg_rows = 2u; o->density = 1.0f;
    return MCRT_OK;
}

int mcrt::shear_check(const char *fn, const mcrt_shear_opts *o, uint32_t E, uint32_t R)
{
    if (o->n_pulses < 4u || o->n_pulses > 256u) return set_error(MCRT_ERR_INVALID, "%s: n_pulses must be 4 .. 256 (%u)", fn, o->n_pulses);
    if (o->window_rows > 16u) return set_error(MCRT_ERR_INVALID, "%s: window_rows must be 0 .. 16 (%u)", fn, o->window_rows);
    if (!(std::isfinite(o->prf_hz) && o->prf_hz > 0.0f)) return set_error(MCRT_ERR_INVALID, "%s: prf_hz must be finite and > 0 (%g)", fn, (double)o->prf_hz);
    if (!(std::isfinite(o->sigma) && o->sigma >= 0.0f)) return set_error(MCRT_ERR_INVALID, "%s: sigma must be finite and >= 0 (%g)", fn, (double)o->sigma);
    if (o->peak_q24 > 8388608 || o->peak_q24 < -8388608) return set_error(MCRT_ERR_INVALID, "%s: peak_q24 must be within +-2^23 (%d)", fn, o->peak_q24);
    if (o->push_line >= E) return set_error(MCRT_ERR_INVALID, "%s: push_line %u is not one of the %u scan-lines", fn, o->push_line, E);
    if (o->push_row0 >= R || (uint64_t)o->push_row0 + o->push_rows > R)
        return set_error(MCRT_ERR_INVALID, "%s: the pushed rows %u + %u pass the scan-line's %u", fn, o->push_row0, o->push_rows, R);
    if (o->speed_lines < 1u || o->speed_lines > 16u) return set_error(MCRT_ERR_INVALID, "%s: speed_lines must be 1 .. 16 (%u)", fn, o->speed_lines);
    if (o->avg_rows > 16u) return set_error(MCRT_ERR_INVALID, "%s: avg_rows must be 0 .. 16 (%u)", fn, o->avg_rows);
    if (!(std::isfinite(o->density) && o->density > 0.0f)) return set_error(MCRT_ERR_INVALID, "%s: density must be finite and > 0 (%g)", fn, (double)o->density);
    return MCRT_OK;
}

extern "C" int mcrt_shear_table(const double *speed_m_s, uint32_t n_labels, double prf_hz, int64_t *slow_q16, float *speed_f)
{
    static const char fn[] = "mcrt_shear_table";
    if (!speed_m_s || !slow_q16 || !speed_f) return mcrt::set_error(MCRT_ERR_INVALID, "%s: null pointer", fn);
    if (n_labels == 0) return mcrt::set_error(MCRT_ERR_INVALID, "%s: n_labels is zero", fn);
    if (n_labels > 254u) return mcrt::set_error(MCRT_ERR_LIMIT, "%s: at most 254 labels (%u)", fn, n_labels);
    if (!(std::isfinite(prf_hz) && prf_hz > 0.0)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: prf_hz must be finite and > 0 (%g)", fn, prf_hz);
    std::vector<int64_t> slow(n_labels);
    for (uint32_t l = 0; l < n_labels; l++) {
        const double c = speed_m_s[l];
        if (!(std::isfinite(c) && c >= 0.0)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: speed_m_s[%u] must be finite and >= 0 (%g)", fn, l, c);
        slow[l] = 0;
        if (c == 0.0) continue;
        const double s = 65536.0 * 65536.0 * prf_hz / (c * 1e6);
        if (!(s >= 0.5 && s <= 274877906944.0)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: the slowness of label %u (%g m/s at %g Hz) is outside [1, 2^38] ticks per um in Q16", fn, l, c, prf_hz);
        slow[l] = (int64_t)std::llrint(s);
        if (slow[l] < 1) return mcrt::set_error(MCRT_ERR_INVALID, "%s: the slowness of label %u (%g m/s at %g Hz) is outside [1, 2^38] ticks per um in Q16", fn, l, c, prf_hz);
    }
    memcpy(slow_q16, slow.data(), 8 * (size_t)n_labels);
    for (uint32_t l = 0; l < n_labels; l++) speed_f[l] = (float)speed_m_s[l];
    return MCRT_OK;
}

extern "C" int mcrt_shear_pitch(uint32_t E, uint32_t R, double radius_mm, double total_angle, uint32_t max_travel_us, uint32_t speed_of_sound,
                                uint32_t *pitch_q8, float *pitch_mm)
{
    static const char fn[] = "mcrt_shear_pitch";
    if (!pitch_q8 && !pitch_mm) return mcrt::set_error(MCRT_ERR_INVALID, "%s: no output is given", fn);
    if (E == 0 || R == 0) return mcrt::set_error(MCRT_ERR_INVALID, "%s: zero sizes (n_elements %u, n_rows %u)", fn, E, R);
    if (!(std::isfinite(radius_mm) && radius_mm >= 0.0)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: radius_mm must be finite and >= 0 (%g)", fn, radius_mm);
    if (!(std::isfinite(total_angle) && total_angle > 0.0)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: total_angle_rad must be finite and > 0 (%g)", fn, total_angle);
    if ((uint32_t)(max_travel_us * speed_of_sound) == 0u) return mcrt::set_error(MCRT_ERR_INVALID, "%s: max_travel_us * speed_of_sound is zero", fn);
    if (R > 2048u) return mcrt::set_error(MCRT_ERR_LIMIT, "%s: n_rows: at most 2048 rows (%u)", fn, R);
    const double depth_mm = (double)(uint32_t)(max_travel_us * speed_of_sound) * 0.001;
    std::vector<double> um(R);
    for (uint32_t r = 0; r < R; r++) {
        um[r] = 1000.0 * (radius_mm + (double)r * depth_mm / (double)R) * total_angle / (double)E;
        if (!(256.0 * um[r] >= 0.5 && 256.0 * um[r] < 16777215.5)) return mcrt::set_error(MCRT_ERR_LIMIT, "%s: the pitch of row %u, %g um, is outside (0, 65536)", fn, r, um[r]);
    }
    for (uint32_t r = 0; r < R; r++) {
        if (pitch_q8) pitch_q8[r] = (uint32_t)std::llrint(256.0 * um[r]);
        if (pitch_mm) pitch_mm[r] = (float)(um[r] * 0.001);
    }
    return MCRT_OK;
}

extern "C" int mcrt_shear_shape(uint32_t width_pulses, uint32_t *shape_q16)
{
    static const char fn[] = "mcrt_shear_shape";
    if (!shape_q16) return mcrt::set_error(MCRT_ERR_INVALID, "%s: null table", fn);
    if (width_pulses == 0) return mcrt::set_error(MCRT_ERR_INVALID, "%s: width_pulses is zero", fn);
    if (width_pulses > 256u) return mcrt::set_error(MCRT_ERR_LIMIT, "%s: at most 256 pulses (%u)", fn, width_pulses);
    const uint32_t n = 64u * width_pulses;
    for (uint32_t i = 0; i < n; i++) shape_q16[i] = (uint32_t)std::llrint(65536.0 * (0.5 - 0.5 * std::cos(6.283185307179586 * ((double)i + 0.5) / (double)n)));
    return MCRT_OK;
}

extern "C" int mcrt_shear_decay(uint32_t n, double d0_lines, uint32_t *amp_q16)
{
    static const char fn[] = "mcrt_shear_decay";
    if (!amp_q16) return mcrt::set_error(MCRT_ERR_INVALID, "%s: null table", fn);
    if (n == 0) return mcrt::set_error(MCRT_ERR_INVALID, "%s: n is zero", fn);
    if (!(std::isfinite(d0_lines) && d0_lines > 0.0)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: d0_lines must be finite and > 0 (%g)", fn, d0_lines);
    for (uint32_t d = 0; d < n; d++) amp_q16[d] = (uint32_t)std::llrint(65536.0 / std::sqrt(1.0 + (double)d / d0_lines));
    return MCRT_OK;
}

// the draws k_shear_track makes for one tracking pulse of one image, [E][R][2]
extern "C" int mcrt_shear_draws(uint32_t seed, uint32_t image_id, uint32_t n_elements, uint32_t n_rows, uint32_t pulse, int32_t *d)
{
    static const char fn[] = "mcrt_shear_draws";
    if (!d) return mcrt::set_error(MCRT_ERR_INVALID, "%s: null d", fn);
    if (n_elements == 0 || n_rows == 0) return mcrt::set_error(MCRT_ERR_INVALID, "%s: zero sizes (n_elements %u, n_rows %u)", fn, n_elements, n_rows);
    if (n_rows > 2048u) return mcrt::set_error(MCRT_ERR_LIMIT, "%s: n_rows: at most 2048 rows (%u)", fn, n_rows);
    if (pulse >= 256u) return mcrt::set_error(MCRT_ERR_LIMIT, "%s: pulse: at most 256 pulses (%u)", fn, pulse);
    for (uint32_t e = 0; e < n_elements; e++)
        for (uint32_t r = 0; r < n_rows; r++) {
            uint32_t o[4];
            host_philox4x32_10(e, r, 0x53484552u, pulse, seed, image_id, o);
            int32_t *p = d + 2u * ((size_t)e * n_rows + r);
            p[0] = (int32_t)((o[0] & 0xffffu) + (o[0] >> 16) + (o[1] & 0xffffu) + (o[1] >> 16)) - 131070;
            p[1] = (int32_t)((o[2] & 0xffffu) + (o[2] >> 16) + (o[3] & 0xffffu) + (o[3] >> 16)) - 131070;
        }
    return MCRT_OK;
}

// (mcrt_strain_map's table: the index is the modulus over the reference, so blue is soft here where it is stiff there)
extern "C" int mcrt_shear_map(uint32_t kind, uint8_t *lut)
{
    static const char fn[] = "mcrt_shear_map";
    if (!lut) return mcrt::set_error(MCRT_ERR_INVALID, "%s: null lut", fn);
    if (kind != 0u) return mcrt::set_error(MCRT_ERR_INVALID, "%s: unknown kind %u", fn, kind);
    blue_green_red(lut);
    return MCRT_OK;
}

// ---- M-mode (the contracts are in include/mcrt.h) ---------------------------------------
extern "C" int mcrt_default_mmode_opts(mcrt_mmode_opts *o)
{
    if (!o) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_default_mmode_opts: null options");
    o->n_pulses = 1024u; o->sigma = 0.0f; o->seed = 0x4D4D4F44u;
    return MCRT_OK;
}

extern "C" int mcrt_default_mmode_display_opts(mcrt_mmode_display_opts *o)
{
    if (!o) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_default_mmode_display_opts: null options");
    o->hop = 4u; o->height = 400u; o->row_lo = 0u; o->row_hi = 0u; o->dynamic_range_db = 60.0f; o->gain_db = 0.0f; o->ref = 0.0f;
    return MCRT_OK;
}

int mcrt::mmode_check(const char *fn, const mcrt_mmode_opts *o)
{
    if (o->n_pulses < 1u || o->n_pulses > 16384u) return set_error(MCRT_ERR_INVALID, "%s: n_pulses must be 1 .. 16384 (%u)", fn, o->n_pulses);
    if (!(std::isfinite(o->sigma) && o->sigma >= 0.0f)) return set_error(MCRT_ERR_INVALID, "%s: sigma must be finite and >= 0 (%g)", fn, (double)o->sigma);
    return MCRT_OK;
}

int mcrt::mmode_display_check(const char *fn, const mcrt_mmode_display_opts *o, uint32_t T, uint32_t R)
{
    if (o->hop == 0u) return set_error(MCRT_ERR_INVALID, "%s: hop is zero", fn);
    if (o->hop > T) return set_error(MCRT_ERR_INVALID, "%s: a hop of %u pulses leaves no column of %u pulses", fn, o->hop, T);
    if (o->height < 1u || o->height > 4096u) return set_error(MCRT_ERR_INVALID, "%s: height must be 1 .. 4096 (%u)", fn, o->height);
    const uint32_t hi = o->row_hi ? o->row_hi : R;
    if (o->row_lo >= hi || hi > R) return set_error(MCRT_ERR_INVALID, "%s: the rows [%u, %u) are not rows of a line of %u", fn, o->row_lo, hi, R);
    if (!(std::isfinite(o->dynamic_range_db) && o->dynamic_range_db > 0.0f)) return set_error(MCRT_ERR_INVALID, "%s: dynamic_range_db must be finite and > 0 (%g)", fn, (double)o->dynamic_range_db);
    if (!std::isfinite(o->gain_db) || !std::isfinite(o->ref)) return set_error(MCRT_ERR_INVALID, "%s: gain_db and ref must be finite (%g, %g)", fn, (double)o->gain_db, (double)o->ref);
    return MCRT_OK;
}

extern "C" int mcrt_mmode_table(const double *dilation, uint32_t n_labels, int32_t *dil_q24)
{
    static const char fn[] = "mcrt_mmode_table";
    if (!dilation || !dil_q24) return mcrt::set_error(MCRT_ERR_INVALID, "%s: null pointer", fn);
    if (n_labels == 0) return mcrt::set_error(MCRT_ERR_INVALID, "%s: n_labels is zero", fn);
    if (n_labels > 254u) return mcrt::set_error(MCRT_ERR_LIMIT, "%s: at most 254 labels (%u)", fn, n_labels);
    for (uint32_t l = 0; l < n_labels; l++)
        if (!(std::fabs(dilation[l] * 16777216.0) <= 4194304.5))      // (a NaN and an infinity fail here too)
            return mcrt::set_error(MCRT_ERR_INVALID, "%s: the dilation of label %u, %g, is not finite or is above 25 %%", fn, l, dilation[l]);
    std::vector<int32_t> dil(n_labels);
    for (uint32_t l = 0; l < n_labels; l++) {
        const long long q = std::llrint(dilation[l] * 16777216.0);
        if (q > 4194304ll || q < -4194304ll) return mcrt::set_error(MCRT_ERR_INVALID, "%s: the dilation of label %u, %g, is above 25 %%", fn, l, dilation[l]);
        dil[l] = (int32_t)q;
    }
    memcpy(dil_q24, dil.data(), 4 * (size_t)n_labels);
    return MCRT_OK;
}

// the pulses of a slow-time table: mcrt_mmode_waveform's and mcrt_mmode_bulk's common refusals
static int mmode_pulses(const char *fn, const void *table, uint32_t T, double prf_hz)
{
    if (!table) return mcrt::set_error(MCRT_ERR_INVALID, "%s: null table", fn);
    if (T == 0) return mcrt::set_error(MCRT_ERR_INVALID, "%s: n_pulses is zero", fn);
    if (T > 16384u) return mcrt::set_error(MCRT_ERR_LIMIT, "%s: at most 16384 pulses (%u)", fn, T);
    if (!(std::isfinite(prf_hz) && prf_hz > 0.0)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: prf_hz must be finite and > 0 (%g)", fn, prf_hz);
    return MCRT_OK;
}

extern "C" int mcrt_mmode_waveform(double prf_hz, double beats_per_min, uint32_t T, int32_t *w_q16)
{
    static const char fn[] = "mcrt_mmode_waveform";
    if (const int rc = mmode_pulses(fn, w_q16, T, prf_hz)) return rc;
    if (!(std::isfinite(beats_per_min) && beats_per_min > 0.0)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: beats_per_min must be finite and > 0 (%g)", fn, beats_per_min);
    for (uint32_t t = 0; t < T; t++) {
        const double u = t * beats_per_min / (60.0 * prf_hz), x = u - std::floor(u), s = std::sin(3.141592653589793 * x / 0.3);
        w_q16[t] = (int32_t)std::llrint(65536.0 * (x < 0.3 ? s * s : 0.0));
    }
    return MCRT_OK;
}

extern "C" int mcrt_mmode_bulk(double prf_hz, double cycles_per_min, double amplitude_rows, uint32_t T, int32_t *bulk_q24)
{
    static const char fn[] = "mcrt_mmode_bulk";
    if (const int rc = mmode_pulses(fn, bulk_q24, T, prf_hz)) return rc;
    if (!std::isfinite(cycles_per_min)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: cycles_per_min must be finite (%g)", fn, cycles_per_min);
    if (!(std::fabs(amplitude_rows) <= 32.0)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: amplitude_rows must be finite and at most 32 rows (%g)", fn, amplitude_rows);
    for (uint32_t t = 0; t < T; t++)
        bulk_q24[t] = (int32_t)std::llrint(amplitude_rows * 16777216.0 * std::sin(6.283185307179586 * t * cycles_per_min / (60.0 * prf_hz)));
    return MCRT_OK;
}

// the draws k_mmode_lines makes for one M-line, [T][R][2]
extern "C" int mcrt_mmode_draws(uint32_t seed, uint32_t image_id, uint32_t line, uint32_t n_rows, uint32_t T, int32_t *d)
{
    static const char fn[] = "mcrt_mmode_draws";
    if (!d) return mcrt::set_error(MCRT_ERR_INVALID, "%s: null d", fn);
    if (n_rows == 0 || T == 0) return mcrt::set_error(MCRT_ERR_INVALID, "%s: zero sizes (n_rows %u, n_pulses %u)", fn, n_rows, T);
    if (n_rows > 2048u) return mcrt::set_error(MCRT_ERR_LIMIT, "%s: n_rows: at most 2048 rows (%u)", fn, n_rows);
    if (T > 16384u) return mcrt::set_error(MCRT_ERR_LIMIT, "%s: at most 16384 pulses (%u)", fn, T);
    for (uint32_t t = 0; t < T; t++)
        for (uint32_t r = 0; r < n_rows; r++) {
            uint32_t o[4];
            host_philox4x32_10(line, r, 0x4D4D4F44u, t, seed, image_id, o);
            int32_t *p = d + 2u * ((size_t)t * n_rows + r);
            p[0] = (int32_t)((o[0] & 0xffffu) + (o[0] >> 16) + (o[1] & 0xffffu) + (o[1] >> 16)) - 131070;
            p[1] = (int32_t)((o[2] & 0xffffu) + (o[2] >> 16) + (o[3] & 0xffffu) + (o[3] >> 16)) - 131070;
        }
    return MCRT_OK;
}

extern "C" int mcrt_mmode_rows(uint32_t row_lo, uint32_t row_hi, uint32_t H, uint32_t *idx, float *wt)
{
    static const char fn[] = "mcrt_mmode_rows";
    if (!idx || !wt) return mcrt::set_error(MCRT_ERR_INVALID, "%s: null table", fn);
    if (H == 0 || H > 4096u) return mcrt::set_error(MCRT_ERR_INVALID, "%s: height must be 1 .. 4096 (%u)", fn, H);
    if (row_lo >= row_hi) return mcrt::set_error(MCRT_ERR_INVALID, "%s: the rows [%u, %u) are empty", fn, row_lo, row_hi);
    if (row_hi > 2048u) return mcrt::set_error(MCRT_ERR_LIMIT, "%s: at most 2048 rows (%u)", fn, row_hi);
    for (uint32_t y = 0; y < H; y++) {
        const double p = (double)row_lo + (y + 0.5) * (double)(row_hi - row_lo) / (double)H - 0.5, f = std::floor(p);
        if (f < (double)row_lo) { idx[y] = row_lo; wt[y] = 0.0f; }
        else if (f > (double)(row_hi - 1u)) { idx[y] = row_hi - 1u; wt[y] = 0.0f; }
        else {
            const float w = (float)(p - f);
            idx[y] = (uint32_t)f; wt[y] = w < 0.0f ? 0.0f : w > 1.0f ? 1.0f : w;
        }
    }
    return MCRT_OK;
}

// ---- automatic gain (the contract is in include/mcrt.h) ---------------------------------------
extern "C" int mcrt_default_autogain_opts(mcrt_autogain_opts *o)
{
    if (!o) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_default_autogain_opts: null options");
    o->band_rows = 16u; o->min_permille = 250u; o->floor = 0.0f; o->floor_scale = 3.0f; o->max_gain = 1000.0f; o->apply = 1u;
    return MCRT_OK;
}

int mcrt::autogain_check(const char *fn, const mcrt_autogain_opts *o)
{
    if (o->band_rows < 4u || o->band_rows > 256u) return set_error(MCRT_ERR_INVALID, "%s: band_rows must be 4 .. 256 (%u)", fn, o->band_rows);
    if (o->min_permille > 1000u) return set_error(MCRT_ERR_INVALID, "%s: min_permille must be 0 .. 1000 (%u)", fn, o->min_permille);
    if (!(std::isfinite(o->floor) && o->floor >= 0.0f)) return set_error(MCRT_ERR_INVALID, "%s: floor must be finite and >= 0 (%g)", fn, (double)o->floor);
    if (!(std::isfinite(o->floor_scale) && o->floor_scale >= 0.0f)) return set_error(MCRT_ERR_INVALID, "%s: floor_scale must be finite and >= 0 (%g)", fn, (double)o->floor_scale);
    if (!(std::isfinite(o->max_gain) && o->max_gain >= 1.0f)) return set_error(MCRT_ERR_INVALID, "%s: max_gain must be finite and >= 1 (%g)", fn, (double)o->max_gain);
    return MCRT_OK;
}

// steps 3 to 8 of the contract for one frame, as k_autogain_curve (mcrt_autogain.hip) does them; this file is compiled -ffp-contract=off
extern "C" int mcrt_autogain_curve(const uint32_t *hist, uint32_t n_lines, uint32_t R, float floor_f, const mcrt_autogain_opts *o, float *k,
                                   int32_t *band_bin, uint32_t *pen)
{
    static const char fn[] = "mcrt_autogain_curve";
    if (!hist) return mcrt::set_error(MCRT_ERR_INVALID, "%s: null hist", fn);
    if (n_lines == 0 || R == 0) return mcrt::set_error(MCRT_ERR_INVALID, "%s: zero sizes (n_lines %u, n_rows %u)", fn, n_lines, R);
    if (!(std::isfinite(floor_f) && floor_f >= 0.0f)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: floor_f must be finite and >= 0 (%g)", fn, (double)floor_f);
    mcrt_autogain_opts d;
    if (!o) { mcrt_default_autogain_opts(&d); o = &d; }
    if (const int rc = mcrt::autogain_check(fn, o)) return rc;
    if (R > MCRT_MAX_ROWS) return mcrt::set_error(MCRT_ERR_LIMIT, "%s: n_rows: at most %d rows (%u)", fn, MCRT_MAX_ROWS, R);
    auto bits_of = [](float x) { uint32_t u; memcpy(&u, &x, 4); return u; };
    auto centre = [](int32_t bin) { const uint32_t u = ((uint32_t)bin << 20) | (1u << 19); float x; memcpy(&x, &u, 4); return x; };
    const uint32_t B = o->band_rows, nB = (R + B - 1u) / B;
    const float thr = floor_f * o->floor_scale;
    const uint32_t thr_bin = (std::isfinite(thr) && thr > 0.0f) ? bits_of(thr) >> 20 : 0u;
    std::vector<int32_t> m(nB, -1);
    std::vector<int32_t> sorted;
    int32_t first = -1, last = -1;
    for (uint32_t b = 0; b < nB; b++) {
        const uint32_t *h = hist + (size_t)b * 2048u;
        uint64_t n_t = 0;
        for (uint32_t i = thr_bin + 1u; i < 2048u; i++) n_t += h[i];
        const uint64_t n_s = (uint64_t)n_lines * std::min(B, R - b * B);
        if (n_t == 0 || n_t * 1000ull < (uint64_t)o->min_permille * n_s) continue;
        uint64_t c = 0;
        for (uint32_t i = thr_bin + 1u; i < 2048u; i++) { c += h[i]; if (2ull * c >= n_t) { m[b] = (int32_t)i; break; } }
        sorted.push_back(m[b]);
        if (first < 0) first = (int32_t)b;
        last = (int32_t)b;
    }
    std::vector<float> kb(nB, 1.0f);
    if (!sorted.empty()) {
        std::sort(sorted.begin(), sorted.end());
        const float ct = centre(sorted[(sorted.size() - 1u) / 2u]), inv_max = 1.0f / o->max_gain;
        int32_t src = first;
        for (uint32_t b = 0; b < nB; b++) {
            if (m[b] >= 0) src = (int32_t)b;
            kb[b] = std::fmin(std::fmax(ct / centre(m[src]), inv_max), o->max_gain);
        }
    }
    if (k) {
        const int32_t two_b = 2 * (int32_t)B;
        for (uint32_t r = 0; r < R; r++) {
            const int32_t n = 2 * (int32_t)r - ((int32_t)B - 1);
            if (n <= 0) { k[r] = kb[0]; continue; }
            const int32_t b = n / two_b;
            if (b >= (int32_t)nB - 1) { k[r] = kb[nB - 1u]; continue; }
            const float t = (float)(n - two_b * b) / (float)two_b;
            const float dk = kb[b + 1] - kb[b], p = dk * t;
            k[r] = kb[b] + p;
        }
    }
    if (band_bin) for (uint32_t b = 0; b < nB; b++) band_bin[b] = m[b];
    if (pen) *pen = last < 0 ? 0u : std::min(R, ((uint32_t)last + 1u) * B);
    return MCRT_OK;
}

// ---- volume rendering (the contract is in include/mcrt.h) ---------------------------------------
extern "C" int mcrt_default_render_opts(mcrt_render_opts *o, int in_u8)
{
    if (!o) return mcrt::set_error(MCRT_ERR_INVALID, "mcrt_default_render_opts: null options");
    o->mode = MCRT_RENDER_SURFACE; o->lo = 0.0f; o->hi = in_u8 ? 255.0f : 1.0f;
    o->threshold = 0.25f; o->ramp = 0.25f; o->opacity = 1.0f; o->depth_cue = 0.5f; o->t_cut = 0.0f;
    return MCRT_OK;
}

// an orthographic camera on a grid's block, in double; the twelve floats are rounded once at the end
extern "C" int mcrt_render_view_for_grid(const mcrt_volume_grid *g, const double dir_mm[3], const double up_mm[3], double pixel_mm, double step_mm,
                                         uint32_t nx, uint32_t ny, mcrt_render_view *out)
{
    static const char fn[] = "mcrt_render_view_for_grid";
    if (!g || !dir_mm || !up_mm || !out) return mcrt::set_error(MCRT_ERR_INVALID, "%s: null %s", fn, !g ? "grid" : !dir_mm ? "dir_mm" : !up_mm ? "up_mm" : "out");
    if (nx == 0 || ny == 0) return mcrt::set_error(MCRT_ERR_INVALID, "%s: zero picture size (nx %u, ny %u)", fn, nx, ny);
    if (g->nu == 0 || g->nv == 0 || g->nw == 0) return mcrt::set_error(MCRT_ERR_INVALID, "%s: zero grid size (%u x %u x %u)", fn, g->nu, g->nv, g->nw);
    for (int i = 0; i < 3; i++)
        if (!(std::isfinite(g->origin_mm[i]) && std::isfinite(g->du_mm[i]) && std::isfinite(g->dv_mm[i]) && std::isfinite(g->dw_mm[i])))
            return mcrt::set_error(MCRT_ERR_INVALID, "%s: the grid has an entry that is not finite (component %d)", fn, i);
    if (!(std::isfinite(pixel_mm) && pixel_mm > 0.0)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: pixel_mm must be finite and > 0 (%g)", fn, pixel_mm);
    if (!(std::isfinite(step_mm) && step_mm > 0.0)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: step_mm must be finite and > 0 (%g)", fn, step_mm);
    auto norm = [](const double v[3]) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); };
    auto cross = [](const double a[3], const double b[3], double o[3]) { o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0]; };
    const double nd = norm(dir_mm), nup = norm(up_mm);
    if (!(std::isfinite(nd) && nd > 0.0)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: dir_mm must be finite and not zero", fn);
    if (!(std::isfinite(nup) && nup > 0.0)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: up_mm must be finite and not zero", fn);
    double dn[3], right[3], down[3];
    for (int i = 0; i < 3; i++) dn[i] = dir_mm[i] / nd;
    cross(dn, up_mm, right);
    const double nr = norm(right);
    if (!(nr > 1e-12 * nup)) return mcrt::set_error(MCRT_ERR_INVALID, "%s: up_mm is parallel to dir_mm", fn);
    for (int i = 0; i < 3; i++) right[i] /= nr;
    cross(right, dn, down);
    for (int i = 0; i < 3; i++) down[i] = -down[i];
    // M^-1 by cofactors: row r of the inverse is (the cross product of the other two columns) / det
    const double *du = g->du_mm, *dv = g->dv_mm, *dw = g->dw_mm;
    double r0[3], r1[3], r2[3];
    cross(dv, dw, r0); cross(dw, du, r1); cross(du, dv, r2);
    const double det = du[0] * r0[0] + du[1] * r0[1] + du[2] * r0[2];
    if (!(std::isfinite(det) && std::fabs(det) > 1e-12 * norm(du) * norm(dv) * norm(dw)))
        return mcrt::set_error(MCRT_ERR_INVALID, "%s: the grid's axes du_mm, dv_mm, dw_mm do not span space (a cut cannot be rendered)", fn);
    auto to_index = [&](const double v[3], float o[3]) {
        o[0] = (float)((r0[0] * v[0] + r0[1] * v[1] + r0[2] * v[2]) / det);
        o[1] = (float)((r1[0] * v[0] + r1[1] * v[1] + r1[2] * v[2]) / det);
        o[2] = (float)((r2[0] * v[0] + r2[1] * v[1] + r2[2] * v[2]) / det);
    };
    const double eu = (double)(g->nu - 1u), ev = (double)(g->nv - 1u), ew = (double)(g->nw - 1u);
    double L = 0.0;
    for (int sv = -1; sv <= 1; sv += 2)
        for (int sw = -1; sw <= 1; sw += 2) {
            double d[3];
            for (int i = 0; i < 3; i++) d[i] = eu * du[i] + sv * ev * dv[i] + sw * ew * dw[i];
            L = std::max(L, norm(d) / 2.0);
        }
    const double steps = std::floor(2.0 * L / step_mm) + 1.0;
    if (!(steps <= 4096.0)) return mcrt::set_error(MCRT_ERR_LIMIT, "%s: n_steps must be 1..4096 (the diagonal %g mm at step_mm %g)", fn, 2.0 * L, step_mm);
    double P0[3], vi[3], vj[3], vs[3];
    const double hx = (double)(nx - 1u) / 2.0 * pixel_mm, hy = (double)(ny - 1u) / 2.0 * pixel_mm;
    for (int i = 0; i < 3; i++) {
        const double centre = eu / 2.0 * du[i] + ev / 2.0 * dv[i] + ew / 2.0 * dw[i];         // C - g->origin_mm
        P0[i] = centre - L * dn[i] - hx * right[i] - hy * down[i];
        vi[i] = pixel_mm * right[i]; vj[i] = pixel_mm * down[i]; vs[i] = step_mm * dn[i];
    }
    mcrt_render_view v;
    memset(&v, 0, sizeof v);
    to_index(P0, v.origin); to_index(vi, v.di); to_index(vj, v.dj); to_index(vs, v.ds);
    v.nx = nx; v.ny = ny; v.n_steps = (uint32_t)steps;
    for (int i = 0; i < 3; i++)
        if (!(std::isfinite(v.origin[i]) && std::isfinite(v.di[i]) && std::isfinite(v.dj[i]) && std::isfinite(v.ds[i])))
            return mcrt::set_error(MCRT_ERR_INVALID, "%s: the view does not fit a float (component %d)", fn, i);
    *out = v;
    return MCRT_OK;
}
