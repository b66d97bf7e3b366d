// mcrt_api.cpp -- the C-ABI of include/mcrt.h: the context, its params, stream, scene, texture and transducer, device memory, instrumentation.
// Host C++ only; the traced pass is mcrt_trace.cpp, the image stages mcrt_image.cpp, the context itself mcrt_ctx.h; kernels live in the
// mcrt_*.hip files (map: mcrt_kernels.h), the owners of the HIP resources in mcrt_hip.h.  No CPU fallback exists: every compute entry point
// needs the GPU context.
#include "mcrt_ctx.h"
#include "mcrt_kernels.h"
#include "mcrt_lbvh.h"

#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <algorithm>
#include <memory>
#include <utility>

using mcrt::set_error;

static Consts derive_consts(const mcrt_params &p)
{
    Consts c;
    c.axial_res_f = 1.45f / p.frequency;                               // main.cpp:25
    c.axial_res_mm = (double)c.axial_res_f;
    c.axial_res_um = (uint32_t)(c.axial_res_f * 1000.0f);              // main.cpp:36
    c.time_step_us = (c.axial_res_mm * 1000.0) / (double)p.speed_of_sound;   // main.cpp:118 (mm -> um is *1000, units.h:1365)
    c.row_dt_us = (double)c.axial_res_um / (double)p.speed_of_sound;   // rfimage.h:35
    c.max_travel_us = (p.depth_cm / (double)p.speed_of_sound) * 10000.0;     // main.cpp:31 (cm s/m -> us)
    c.max_rows = (uint32_t)((p.speed_of_sound * (uint32_t)c.max_travel_us) / c.axial_res_um);   // rfimage.h:180
    return c;
}

static Knobs read_knobs()
{
    using mcrt::tuning_env;
    Knobs k;
    if (const char *e = tuning_env("MCRT_KSPLIT_LIMIT")) { long v = atol(e); if (v >= 0 && v <= MCRT_KSPLIT_MAX) k.ksplit_limit = (uint32_t)v; }   // 0 = off
    if (const char *e = tuning_env("MCRT_TRACE_BLOCKS")) { int v = atoi(e); if (v >= 1) k.trace_blocks = (uint32_t)v; }
    if (const char *e = tuning_env("MCRT_TRACE_BLOCKS_WIDE")) { int v = atoi(e); if (v >= 1) k.trace_blocks_wide = (uint32_t)v; }
    if (const char *e = tuning_env("MCRT_WIDE_MAX_TREE_MB")) { long long v = atoll(e); if (v >= 0 && v <= 0xffffffffll) k.wide_max_tree_mb = (uint32_t)v; }
    if (const char *e = tuning_env("MCRT_WIDE_FROM")) { long long v = atoll(e); if (v >= 1 && v <= 0xffffffffll) k.wide_from = (uint32_t)v; }   // rays in a launch from which the walk takes its five-wavefront form (1: always; 4294967295: never)
    if (const char *e = tuning_env("MCRT_GROUPS")) { int v = atoi(e); if (v >= 1 && v <= 16) k.groups = (uint32_t)v; }
    if (const char *e = tuning_env("MCRT_PACKET_BOUNCES")) { long v = strtol(e, nullptr, 0); if (v >= 0) k.packet_mask = (uint32_t)v; }
    if (const char *e = tuning_env("MCRT_PATH_GROUPS")) { int v = atoi(e); if (v >= 1 && v <= 16) k.path_groups = (uint32_t)v; }
    if (const char *e = tuning_env("MCRT_PATH_MAX")) { long long v = atoll(e); if (v >= 0 && v <= 0xffffffffll) k.path_max = (uint32_t)v; }
    if (const char *e = tuning_env("MCRT_PACKET_FROM")) { long long v = atoll(e); if (v >= 0 && v <= 0xffffffffll) k.packet_from = (uint32_t)v; }
    if (const char *e = tuning_env("MCRT_MARCH_STREAMS")) { int v = atoi(e); if (v >= 1 && v <= MCRT_SIDE_STREAMS) k.march_streams = (uint32_t)v; }
    if (const char *e = tuning_env("MCRT_MARCH_BLOCKS")) { int v = atoi(e); if (v >= 1) k.march_blocks = (uint32_t)v; }
    k.no_overlap = tuning_env("MCRT_NO_OVERLAP") != nullptr; k.no_priority = tuning_env("MCRT_NO_PRIORITY") != nullptr;
    k.no_fast_div = tuning_env("MCRT_NO_FAST_DIV") != nullptr; k.no_lean = tuning_env("MCRT_NO_LEAN") != nullptr;
    k.test_hooks = tuning_env("MCRT_TEST_HOOKS") != nullptr;
    if (const char *e = tuning_env("MCRT_RETIRE_LATE")) k.retire_late = atoi(e) != 0;
    if (const char *e = tuning_env("MCRT_FOLD_B0")) k.fold_b0 = atoi(e) != 0;
    if (const char *e = tuning_env("MCRT_BEAM_B1")) { int v = atoi(e); if (v >= 0 && v <= 2) k.beam_b1 = (uint32_t)v; }
    if (const char *e = tuning_env("MCRT_BEAM_FROM")) { long long v = atoll(e); if (v >= 0 && v <= 0xffffffffll) k.beam_from = (uint32_t)v; }
    if (const char *e = tuning_env("MCRT_BEAM_LAST")) { int v = atoi(e); if (v >= 1 && v < MCRT_MAX_BOUNCES) k.beam_last = (uint32_t)v; }
    if (const char *e = tuning_env("MCRT_BEAM_DEEP_FROM")) { long long v = atoll(e); if (v >= 0 && v <= 0xffffffffll) k.beam_deep_from = (uint32_t)v; }
    if (const char *e = tuning_env("MCRT_BEAM_B4_FROM")) { long long v = atoll(e); if (v >= 0 && v <= 0xffffffffll) k.beam_b4_from = (uint32_t)v; }
    if (const char *e = tuning_env("MCRT_BEAM_GROUPS")) { long long v = atoll(e); if (v >= 1 && v <= (1 << 20)) k.beam_groups = (uint32_t)v; }
    if (const char *e = tuning_env("MCRT_BEAM_CAP")) { int v = atoi(e); if (v >= 1 && v <= (int)MCRT_BEAM_CAP_MAX) k.beam_cap = (uint32_t)v; }
    if (const char *e = tuning_env("MCRT_BEAM_NEAR")) { int v = atoi(e); if (v >= 1) k.beam_near = (uint32_t)v; }
    if (const char *e = tuning_env("MCRT_BEAM_ORDER")) { long v = strtol(e, nullptr, 0); if (v >= 0 && v < (1l << MCRT_MAX_BOUNCES)) k.beam_order = (uint32_t)v; }
    if (const char *e = tuning_env("MCRT_BEAM_PAIRS")) k.beam_pairs = atoi(e) != 0;
    if (const char *e = tuning_env("MCRT_RENDER_ROW_TILE")) k.render_row_tile = atoi(e) != 0;
    if (const char *e = tuning_env("MCRT_SPECKLE_FUSE")) { int v = atoi(e); if (v == 2 || v == 4) k.speckle_fuse = (uint32_t)v; }
    if (const char *e = tuning_env("MCRT_AUTOGAIN_COPIES")) { int v = atoi(e); if (v == 1 || v == 4) k.autogain_copies = (uint32_t)v; }
    if (const char *e = tuning_env("MCRT_AUTOGAIN_HIST_KB")) { int v = atoi(e); if (v >= 8 && v <= 32768) k.autogain_hist_words = (uint32_t)v * 256u; }
    return k;
}

static int prepare_tables(mcrt_ctx *c)
{
    if (c->tab.thr_rows != c->p.n_rows || c->tab.thr_dt != c->c.row_dt_us || !c->tab.d_row_thr) {
        std::vector<double> thr((size_t)c->p.n_rows + 1);
        MCRT_TRY(mcrt_row_thresholds(c->c.row_dt_us, c->p.n_rows, thr.data()));
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->tab.thr_rows = 0;
        HIP_TRY(c->tab.d_row_thr.alloc(thr.size()));
        HIP_TRY(hipMemcpy(c->tab.d_row_thr, thr.data(), thr.size() * 8, hipMemcpyHostToDevice));
        c->tab.thr_rows = c->p.n_rows; c->tab.thr_dt = c->c.row_dt_us; c->tab.thr_end = thr.back();
    }
    if (c->tab.verified_res != c->p.tex_res) {
        // the GPU checks, exhaustively, that its fma-corrected reciprocal multiply IS IEEE division by tex_res
        Buf<unsigned long long> d_bad; unsigned long long bad = 1;
        HIP_TRY(d_bad.alloc(1));
        HIP_TRY(hipMemsetAsync(d_bad, 0, 8, c->stream));
        HIP_TRY(mcrt::launch_verify_div(c->p.tex_res, 1.0f / c->p.tex_res, d_bad, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipMemcpy(&bad, d_bad, 8, hipMemcpyDeviceToHost));
        c->tab.fast_div = (bad == 0) && !c->knobs.no_fast_div;
        c->tab.fast_div_all = c->tab.fast_div && c->p.tex_res > 1e-16f && !c->knobs.no_lean;
        c->tab.verified_res = c->p.tex_res;
    }
    if (c->scene.have && (!c->tab.mtab_valid || c->tab.mtab_key[0] != c->c.axial_res_f || c->tab.mtab_key[1] != c->p.frequency)) {
        c->tab.mtab_valid = false;
        if (c->tab.d_mtab.cap < c->scene.n_mat) {
            HIP_TRY(hipStreamSynchronize(c->stream));
            HIP_TRY(c->tab.d_mtab.alloc(c->scene.n_mat));
        }
        HIP_TRY(mcrt::launch_material_table(c->scene.d_mats, c->scene.n_mat, c->c.axial_res_f, c->p.frequency, c->tab.d_mtab, c->stream));
        c->tab.mtab_key[0] = c->c.axial_res_f; c->tab.mtab_key[1] = c->p.frequency; c->tab.mtab_valid = true;
    }
    return MCRT_OK;
}

extern "C" int mcrt_version(void) { return MCRT_VERSION; }
extern "C" int mcrt_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int mcrt_default_params(mcrt_params *p)
{
    if (!p) return set_error(MCRT_ERR_INVALID, "null params");
    memset(p, 0, sizeof *p);
    p->n_elements = 512; p->n_samples = 5; p->max_depth = 10; p->n_rows = 465;
    p->frequency = 4.5f; p->intensity_epsilon = 1e-10f; p->initial_intensity = 1.0f; p->ray_start_offset = 0.1f;
    p->speed_of_sound = 1500; p->depth_cm = 15.0; p->seed = 0x5EED; p->sanitize_tir = 0; p->tex_n = 256; p->tex_res = 0.145f;
    return MCRT_OK;
}

extern "C" int mcrt_create(int device, mcrt_ctx **out)
{
    if (!out) return set_error(MCRT_ERR_INVALID, "null out pointer");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return set_error(MCRT_ERR_NO_DEVICE, "no HIP device visible: libmcrt_hip has no CPU fallback");
    if (device < 0 || device >= n) return set_error(MCRT_ERR_INVALID, "device %d out of range (0..%d)", device, n - 1);
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (!strstr(prop.gcnArchName, "gfx950"))
        return set_error(MCRT_ERR_NO_DEVICE, "device %d is %s; this library carries gfx950 (MI355X) code only", device, prop.gcnArchName);
    std::unique_ptr<mcrt_ctx> c(new (std::nothrow) mcrt_ctx());   // (a failure below releases whatever was made)
    if (!c) return set_error(MCRT_ERR_NOMEM, "out of host memory");
    c->device = device;
    c->knobs = read_knobs();
    if (prop.multiProcessorCount > 0) c->n_cu = (uint32_t)prop.multiProcessorCount;
    HIP_TRY(hipStreamCreateWithFlags(&c->own_stream.h, hipStreamNonBlocking));
    c->stream = c->own_stream;
    HIP_TRY(ensure_event(c->ev_start));
    c->work.reserve(16);   // pointers into this vector are held across get_work() calls; never more than 16 groups
    mcrt_default_params(&c->p);
    c->c = derive_consts(c->p);
    HIP_TRY(c->ins.d_stats.alloc(MCRT_STATS_WORDS));
    HIP_TRY(hipMemsetAsync(c->ins.d_stats, 0, MCRT_STATS_WORDS * sizeof(unsigned long long), c->stream));
    HIP_TRY(c->d_error.alloc(1));
    HIP_TRY(hipMemsetAsync(c->d_error, 0, 4, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    MCRT_TRY(prepare_tables(c.get()));
    *out = c.release();
    return MCRT_OK;
}

// the walk's view of the tree: child-transposed half-float nodes, rebuilt whenever d_nodes changes.  The buffer is kept while the
// node count stays (a refit -- the per-frame path of a deforming scene -- then costs one kernel on the context's stream and no
// allocation HERE; mcrt_refit_triangles itself still frees its staging copy of the vertices, which synchronises the device).
// Nothing here waits: the rebuild is ordered on the stream it was issued on, and an event recorded behind it orders a trace that
// is issued on ANOTHER stream after mcrt_set_stream (enqueue_pass waits for it).
static int refresh_soa(mcrt_ctx *c)
{
    c->scene.walked_stale = true;
    if (c->scene.bvh4.n_nodes == 0) { c->scene.d_nodes_walk.reset(); return MCRT_OK; }
    if (c->scene.d_nodes_walk.cap != 4 * (size_t)c->scene.bvh4.n_nodes) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(c->scene.d_nodes_walk.alloc(4 * (size_t)c->scene.bvh4.n_nodes));
    }
    HIP_TRY(mcrt::launch_nodes_walk(c->scene.d_nodes, c->scene.bvh4.n_nodes, c->scene.d_nodes_walk, c->stream));
    if (c->scene.d_tris_id.cap != MCRT_TRI_PIECES * (size_t)c->scene.bvh.n_tri) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(c->scene.d_tris_id.alloc(MCRT_TRI_PIECES * (size_t)c->scene.bvh.n_tri));
    }
    HIP_TRY(mcrt::launch_tris_by_id((const float4 *)c->scene.d_tris, c->scene.bvh.n_tri, c->scene.d_tris_id, c->stream));
    HIP_TRY(ensure_event(c->scene.ev_update));
    HIP_TRY(hipEventRecord(c->scene.ev_update, c->stream));
    c->scene.update_stream = c->stream; c->scene.update_pending = true;
    return MCRT_OK;
}

extern "C" int mcrt_destroy(mcrt_ctx *c)
{
    if (!c) return MCRT_OK;
    hipSetDevice(c->device);
    hipDeviceSynchronize();
    delete c;
    return MCRT_OK;
}

namespace mcrt { hipStream_t ctx_stream(mcrt_ctx *c) { return c->stream; } }   // (mcrt_group.cpp: the root context's stream)
extern "C" int mcrt_set_stream(mcrt_ctx *c, void *s) { CTX_TRY(c); c->stream = s ? (hipStream_t)s : c->own_stream; return MCRT_OK; }
int mcrt::check_device_error(mcrt_ctx *c)
{
    uint32_t e = 0;
    HIP_TRY(hipMemcpy(&e, c->d_error, 4, hipMemcpyDeviceToHost));
    if (e) { HIP_TRY(hipMemsetAsync(c->d_error, 0, 4, c->stream)); HIP_TRY(hipStreamSynchronize(c->stream)); return set_error(MCRT_ERR_LIMIT, "device error flag 0x%x:%s%s", e, (e & 1u) ? " BVH traversal stack overflow" : "", (e & 2u) ? " kernel watchdog expired (a persistent kernel ran for more than its time limit and was abandoned)" : ""); }
    return MCRT_OK;
}
extern "C" int mcrt_synchronize(mcrt_ctx *c) { CTX_TRY(c); HIP_TRY(hipStreamSynchronize(c->stream)); return mcrt::check_device_error(c); }

extern "C" int mcrt_set_params(mcrt_ctx *c, const mcrt_params *p)
{
    CTX_TRY(c);
    if (!p) return set_error(MCRT_ERR_INVALID, "null params");
    if (p->n_elements == 0 || p->n_samples == 0) return set_error(MCRT_ERR_INVALID, "n_elements and n_samples must be positive");
    if (p->max_depth == 0 || p->max_depth > MCRT_MAX_BOUNCES) return set_error(MCRT_ERR_LIMIT, "max_depth must be 1..%d", MCRT_MAX_BOUNCES);
    if (p->n_rows == 0 || p->n_rows > MCRT_MAX_ROWS) return set_error(MCRT_ERR_LIMIT, "n_rows must be 1..%d", MCRT_MAX_ROWS);
    if (!(p->frequency > 0.f) || p->speed_of_sound == 0 || !(p->depth_cm > 0.0)) return set_error(MCRT_ERR_INVALID, "frequency, speed_of_sound and depth must be positive");
    if (p->tex_n == 0 || !(p->tex_res > 0.f)) return set_error(MCRT_ERR_INVALID, "texture size/resolution must be positive");
    Consts k = derive_consts(*p);
    if (k.axial_res_um == 0) return set_error(MCRT_ERR_INVALID, "axial resolution rounds to 0 um at %g MHz", (double)p->frequency);
    c->p = *p; c->c = k;
    return prepare_tables(c);
}

extern "C" int mcrt_get_params(mcrt_ctx *c, mcrt_params *out)
{
    if (!c || !out) return set_error(MCRT_ERR_INVALID, "null argument");
    *out = c->p;
    return MCRT_OK;
}

// a deep copy of a host-built tree (the context frees its trees with mcrt_free_bvh / mcrt_free_bvh4: malloc'ed arrays)
static int copy_tree(const mcrt::HostTree &src, mcrt_bvh *bvh, mcrt_bvh4 *bvh4)
{
    *bvh = *src.bvh; *bvh4 = *src.bvh4;
    bvh->nodes = nullptr; bvh->tri = nullptr; bvh4->nodes = nullptr;
    const size_t nb = sizeof(mcrt_bvh_node) * (size_t)src.bvh->n_nodes, tb = 48 * (size_t)src.bvh->n_tri, n4 = sizeof(mcrt_bvh4_node) * (size_t)src.bvh4->n_nodes;
    bvh->nodes = (mcrt_bvh_node *)malloc(nb ? nb : 1); bvh->tri = (float *)malloc(tb ? tb : 1); bvh4->nodes = (mcrt_bvh4_node *)malloc(n4 ? n4 : 1);
    if (!bvh->nodes || !bvh->tri || !bvh4->nodes) { mcrt_free_bvh(bvh); mcrt_free_bvh4(bvh4); return set_error(MCRT_ERR_NOMEM, "out of host memory"); }
    memcpy(bvh->nodes, src.bvh->nodes, nb); memcpy(bvh->tri, src.bvh->tri, tb); memcpy(bvh4->nodes, src.bvh4->nodes, n4);
    return MCRT_OK;
}

// builds the BVH over tri[n_tri][9] (host or device pointer) with the context's builder and installs it on the device.
// pre: a tree the HOST builder has already made of exactly these triangles (mcrt_group builds once for all its ranks); ignored by the
// device builder, which needs no host work
static int index_triangles(mcrt_ctx *c, const float *tri, uint32_t n_tri, const mcrt::HostTree *pre = nullptr)
{
    // k_trace addresses nodes (64 B as walked) and triangle records (64 B) with 32-bit byte offsets
    if (n_tri >= (1u << 25)) return set_error(MCRT_ERR_LIMIT, "%u triangles: the walk addresses at most 2^25 (32-bit byte offsets into 64-byte nodes and records)", n_tri);
    c->scene.d_nodes.reset(); c->scene.d_tris.reset(); c->scene.d_tri_slot.reset();
    mcrt_free_bvh(&c->scene.bvh); mcrt_free_bvh4(&c->scene.bvh4);
    c->scene.host_bvh_stale = false;
    const bool on_device = c->scene.builder == MCRT_BVH_DEVICE_LBVH;
    Buf<float4> leaf;                                   // the builder's 48-byte leaf-order triangle array, on the device
    if (on_device) {
        mcrt::LbvhResult r;
        {
            Buf<float> d_tri; Buf<uint32_t> d_mesh;
            HIP_TRY(d_tri.alloc(9 * (size_t)n_tri));
            HIP_TRY(d_mesh.alloc(n_tri));
            if (hipMemcpyAsync(d_tri, tri, 36 * (size_t)n_tri, hipMemcpyDefault, c->stream) != hipSuccess ||
                hipMemcpyAsync(d_mesh, c->scene.tri_mesh.data(), 4 * (size_t)n_tri, hipMemcpyHostToDevice, c->stream) != hipSuccess)
                return set_error(MCRT_ERR_HIP, "triangle upload failed");
            MCRT_TRY(mcrt::lbvh_build(d_tri, d_mesh, n_tri, c->stream, &r));
        }
        c->scene.d_nodes = std::move(r.nodes); c->scene.d_tri_slot = std::move(r.tri_slot); leaf = std::move(r.tris);
        c->scene.bvh.n_nodes = 0; c->scene.bvh.n_tri = n_tri; c->scene.bvh.max_depth = r.max_depth; c->scene.bvh.pad_abs = r.pad_abs; c->scene.bvh.nodes = nullptr; c->scene.bvh.tri = nullptr;
        c->scene.bvh4.n_nodes = r.n_nodes4; c->scene.bvh4.max_stack = r.max_stack; c->scene.bvh4.nodes = nullptr;
        c->scene.host_bvh_stale = true;
        for (int i = 0; i < 3; i++) { c->scene.lo[i] = r.lo[i]; c->scene.hi[i] = r.hi[i]; }
    } else if (pre) {
        if (pre->bvh->n_tri != n_tri) return set_error(MCRT_ERR_INVALID, "prebuilt tree has %u triangles, the scene %u", pre->bvh->n_tri, n_tri);
        MCRT_TRY(copy_tree(*pre, &c->scene.bvh, &c->scene.bvh4));
    } else {
        std::vector<float> host_copy;
        if (is_device_pointer(tri)) {   // the host builder reads host memory
            host_copy.resize((size_t)n_tri * 9);
            HIP_TRY(hipMemcpy(host_copy.data(), tri, 36 * (size_t)n_tri, hipMemcpyDeviceToHost));
            tri = host_copy.data();
        }
        MCRT_TRY(mcrt_build_bvh(tri, c->scene.tri_mesh.data(), n_tri, &c->scene.bvh));
        MCRT_TRY(mcrt_build_bvh4(&c->scene.bvh, &c->scene.bvh4));
    }
    if (c->scene.bvh4.max_stack > MCRT_STACK)
        return set_error(MCRT_ERR_LIMIT, "%sBVH4 needs a %u-entry traversal stack, the kernel has %d", on_device ? "device-built " : "", c->scene.bvh4.max_stack, MCRT_STACK);
    if (c->scene.bvh4.n_nodes >= (1u << 25)) return set_error(MCRT_ERR_LIMIT, "%u BVH4 nodes: the walk addresses at most 2^25", c->scene.bvh4.n_nodes);
    if (!on_device) {   // the host-built tree: its bounds, and its arrays go to the device
        for (int i = 0; i < 3; i++) { c->scene.lo[i] = INFINITY; c->scene.hi[i] = -INFINITY; }
        for (int k = 0; k < 4; k++) {
            const mcrt_bvh4_child &ch = c->scene.bvh4.nodes[0].c[k];
            if (ch.ref == MCRT_BVH4_EMPTY) continue;
            const float hi[3] = { ch.hi_x, ch.hi_y, ch.hi_z };
            for (int i = 0; i < 3; i++) { c->scene.lo[i] = std::min(c->scene.lo[i], ch.lo[i]); c->scene.hi[i] = std::max(c->scene.hi[i], hi[i]); }
        }
        HIP_TRY(c->scene.d_nodes.alloc(sizeof(mcrt_bvh4_node) / 16 * (size_t)c->scene.bvh4.n_nodes));
        HIP_TRY(hipMemcpy(c->scene.d_nodes, c->scene.bvh4.nodes, sizeof(mcrt_bvh4_node) * (size_t)c->scene.bvh4.n_nodes, hipMemcpyHostToDevice));
        HIP_TRY(leaf.alloc(3 * (size_t)n_tri));
        HIP_TRY(hipMemcpy(leaf, c->scene.bvh.tri, 48 * (size_t)n_tri, hipMemcpyHostToDevice));
        // triangle id -> leaf-order slot (k_shade re-derives the winning triangle's normal from its vertices)
        std::vector<uint32_t> slot(n_tri);
        for (uint32_t k = 0; k < n_tri; k++) { uint32_t id; memcpy(&id, &c->scene.bvh.tri[(size_t)k * 12 + 3], 4); slot[id] = k; }
        HIP_TRY(c->scene.d_tri_slot.alloc(n_tri));
        HIP_TRY(hipMemcpy(c->scene.d_tri_slot, slot.data(), 4 * (size_t)n_tri, hipMemcpyHostToDevice));
    }
    // the walk's 64-byte records from the builder's 48-byte leaf-order array
    HIP_TRY(c->scene.d_tris.alloc(MCRT_TRI_PIECES * (size_t)n_tri));
    HIP_TRY(mcrt::launch_expand_tris(leaf, n_tri, c->scene.d_tris, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MCRT_OK;
}

// host copies of a device-built tree, for mcrt_get_bvh / mcrt_get_bvh4
static int download_bvh(mcrt_ctx *c)
{
    if (!c->scene.host_bvh_stale) return MCRT_OK;
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->scene.bvh.tri = (float *)malloc(48 * (size_t)c->scene.bvh.n_tri);
    c->scene.bvh4.nodes = (mcrt_bvh4_node *)malloc(sizeof(mcrt_bvh4_node) * (size_t)c->scene.bvh4.n_nodes);
    if (!c->scene.bvh.tri || !c->scene.bvh4.nodes) return set_error(MCRT_ERR_NOMEM, "out of memory");
    {   // back from the walk's records to the ABI's 48-byte layout (v0|id, v1|mesh, v2|0)
        const size_t W = 4 * MCRT_TRI_PIECES;      // floats per record
        std::vector<float> rec((size_t)c->scene.bvh.n_tri * W);
        HIP_TRY(hipMemcpy(rec.data(), c->scene.d_tris, 4 * W * (size_t)c->scene.bvh.n_tri, hipMemcpyDeviceToHost));
        for (size_t t = 0; t < c->scene.bvh.n_tri; t++) {
            const float *r = &rec[t * W]; float *o = &c->scene.bvh.tri[t * 12];
            memcpy(o, r, 32);                                          // v0 | id, v1 | mesh
            o[8] = r[8]; o[9] = r[9]; o[10] = r[10]; o[11] = 0.0f;      // v2 | 0 (the record keeps the edge tolerance there)
        }
    }
    HIP_TRY(hipMemcpy(c->scene.bvh4.nodes, c->scene.d_nodes, sizeof(mcrt_bvh4_node) * (size_t)c->scene.bvh4.n_nodes, hipMemcpyDeviceToHost));
    c->scene.host_bvh_stale = false;
    return MCRT_OK;
}

extern "C" int mcrt_set_bvh_builder(mcrt_ctx *c, int builder)
{
    CTX_TRY(c);
    if (builder != MCRT_BVH_HOST_SAH && builder != MCRT_BVH_DEVICE_LBVH) return set_error(MCRT_ERR_INVALID, "unknown BVH builder %d", builder);
    c->scene.builder = builder;
    return MCRT_OK;
}

// what mcrt_update_triangles and mcrt_refit_triangles ask alike: new positions for exactly the uploaded triangles, and an idle stream
static int check_new_positions(mcrt_ctx *c, const float *tri, uint32_t n_tri)
{
    CTX_TRY(c);
    if (!c->scene.have) return set_error(MCRT_ERR_INVALID, "no scene uploaded");
    if (!tri) return set_error(MCRT_ERR_INVALID, "null triangles");
    if (n_tri != c->scene.bvh.n_tri || n_tri == 0) return set_error(MCRT_ERR_INVALID, "the scene has %u triangles, the update has %u", c->scene.bvh.n_tri, n_tri);
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MCRT_OK;
}

static int update_triangles(mcrt_ctx *c, const float *tri, uint32_t n_tri, const mcrt::HostTree *pre)
{
    MCRT_TRY(check_new_positions(c, tri, n_tri));
    c->scene.have = false;                           // a failed rebuild leaves no scene
    MCRT_TRY(index_triangles(c, tri, n_tri, pre));
    MCRT_TRY(refresh_soa(c));
    c->scene.have = true;
    return MCRT_OK;
}
extern "C" int mcrt_update_triangles(mcrt_ctx *c, const float *tri, uint32_t n_tri) { return update_triangles(c, tri, n_tri, nullptr); }

extern "C" int mcrt_refit_triangles(mcrt_ctx *c, const float *tri, uint32_t n_tri)
{
    MCRT_TRY(check_new_positions(c, tri, n_tri));
    Buf<float> d_tri;
    HIP_TRY(d_tri.alloc(9 * (size_t)n_tri));
    int rc = MCRT_OK;
    if (hipMemcpyAsync(d_tri, tri, 36 * (size_t)n_tri, hipMemcpyDefault, c->stream) != hipSuccess) rc = set_error(MCRT_ERR_HIP, "triangle upload failed");
    float pad = 0.0f, lo[3], hi[3];
    if (!rc) rc = mcrt::bvh_refit(d_tri, n_tri, c->scene.d_nodes, c->scene.bvh4.n_nodes, c->scene.d_tris, c->stream, &pad, lo, hi);
    d_tri.reset();
    if (!rc) rc = refresh_soa(c);
    if (rc) { c->scene.have = false; return rc; }           // a failed refit leaves no scene
    c->scene.bvh.pad_abs = pad;
    for (int i = 0; i < 3; i++) { c->scene.lo[i] = lo[i]; c->scene.hi[i] = hi[i]; }
    // the host copies (and the host builder's BVH2, which has no refitted counterpart) are out of date: downloaded on demand
    free(c->scene.bvh.nodes); c->scene.bvh.nodes = nullptr; c->scene.bvh.n_nodes = 0;
    free(c->scene.bvh.tri); c->scene.bvh.tri = nullptr;
    free(c->scene.bvh4.nodes); c->scene.bvh4.nodes = nullptr;
    c->scene.host_bvh_stale = true;
    return MCRT_OK;
}

static int upload_scene(mcrt_ctx *c, const float *tri, const uint32_t *tri_mesh, uint32_t n_tri,
                        const mcrt_mesh *meshes, uint32_t n_mesh, const float *mats, uint32_t n_mat,
                        uint32_t start_mat, const float spacing[3], const mcrt::HostTree *pre)
{
    CTX_TRY(c);
    if (!meshes || !mats || n_mesh == 0 || n_mat == 0 || !spacing) return set_error(MCRT_ERR_INVALID, "mcrt_upload_scene: missing tables");
    if (n_tri && (!tri || !tri_mesh)) return set_error(MCRT_ERR_INVALID, "mcrt_upload_scene: missing triangles");
    if (start_mat >= n_mat) return set_error(MCRT_ERR_INVALID, "startingMaterial index %u out of range", start_mat);
    for (uint32_t i = 0; i < n_mesh; i++)
        if (meshes[i].mat_inside >= n_mat || meshes[i].mat_outside >= n_mat) return set_error(MCRT_ERR_INVALID, "mesh %u references a material out of range", i);
    for (uint32_t i = 0; i < n_tri; i++)
        if (tri_mesh[i] >= n_mesh) return set_error(MCRT_ERR_INVALID, "triangle %u references mesh %u out of range", i, tri_mesh[i]);
    HIP_TRY(hipStreamSynchronize(c->stream));
    free(c->scene.walked_nodes); c->scene.walked_nodes = nullptr; c->scene.walked_stale = true;
    mcrt_free_bvh(&c->scene.bvh); mcrt_free_bvh4(&c->scene.bvh4);
    c->scene.have = false;
    if (n_tri) {
        c->scene.tri_mesh.assign(tri_mesh, tri_mesh + n_tri);
        MCRT_TRY(index_triangles(c, tri, n_tri, pre));
        MCRT_TRY(refresh_soa(c));
    } else {
        c->scene.d_nodes.reset(); c->scene.d_tris.reset(); c->scene.d_tri_slot.reset(); c->scene.d_nodes_walk.reset(); c->scene.d_tris_id.reset();
    }
    HIP_TRY(c->scene.d_mats.alloc(2 * (size_t)n_mat));
    HIP_TRY(hipMemcpy(c->scene.d_mats, mats, 32 * (size_t)n_mat, hipMemcpyHostToDevice));
    HIP_TRY(c->scene.d_meshes.alloc(n_mesh));
    HIP_TRY(hipMemcpy(c->scene.d_meshes, meshes, sizeof(mcrt_mesh) * (size_t)n_mesh, hipMemcpyHostToDevice));
    c->scene.n_mesh = n_mesh; c->scene.n_mat = n_mat; c->scene.start_mat = start_mat;
    c->scene.start_silent = mats[8 * (size_t)start_mat + 2] == 0.0f && mats[8 * (size_t)start_mat + 4] == 0.0f;
    for (int i = 0; i < 3; i++) c->scene.spacing[i] = spacing[i];
    c->scene.have = true; c->tab.mtab_valid = false;
    return prepare_tables(c);
}
extern "C" int mcrt_upload_scene(mcrt_ctx *c, const float *tri, const uint32_t *tri_mesh, uint32_t n_tri,
                                 const mcrt_mesh *meshes, uint32_t n_mesh, const float *mats, uint32_t n_mat,
                                 uint32_t start_mat, const float spacing[3])
{
    return upload_scene(c, tri, tri_mesh, n_tri, meshes, n_mesh, mats, n_mat, start_mat, spacing, nullptr);
}
// for mcrt_group.cpp: the same calls with a tree the host builder has already made (see index_triangles)
namespace mcrt {
int ctx_bvh_builder(const mcrt_ctx *c) { return c ? c->scene.builder : MCRT_BVH_HOST_SAH; }
int upload_scene_with_tree(mcrt_ctx *c, const float *tri, const uint32_t *tri_mesh, uint32_t n_tri, const mcrt_mesh *meshes, uint32_t n_mesh,
                           const float *mats, uint32_t n_mat, uint32_t start_mat, const float spacing[3], const HostTree *pre)
{
    return upload_scene(c, tri, tri_mesh, n_tri, meshes, n_mesh, mats, n_mat, start_mat, spacing, pre);
}
int update_triangles_with_tree(mcrt_ctx *c, const float *tri, uint32_t n_tri, const HostTree *pre) { return update_triangles(c, tri, n_tri, pre); }
}

extern "C" int mcrt_get_bvh(mcrt_ctx *c, mcrt_bvh *out)
{
    if (!c || !out) return set_error(MCRT_ERR_INVALID, "null argument");
    if (!c->scene.have) return set_error(MCRT_ERR_INVALID, "no scene uploaded");
    MCRT_TRY(download_bvh(c));
    *out = c->scene.bvh;
    return MCRT_OK;
}

extern "C" int mcrt_get_bvh4(mcrt_ctx *c, mcrt_bvh4 *out)
{
    if (!c || !out) return set_error(MCRT_ERR_INVALID, "null argument");
    if (!c->scene.have) return set_error(MCRT_ERR_INVALID, "no scene uploaded");
    HIP_TRY(hipSetDevice(c->device));
    if (c->scene.d_nodes_walk) {
        // the tree AS WALKED: the lane-per-ray walk reads half-float boxes rounded outwards; decoded back into the builders' layout
        if (c->scene.walked_stale || !c->scene.walked_nodes) {
            const size_t bytes = sizeof(mcrt_bvh4_node) * (size_t)c->scene.bvh4.n_nodes;
            Buf<float4> d_tmp;
            HIP_TRY(d_tmp.alloc(bytes / 16));
            hipError_t e = mcrt::launch_nodes_walk_decode(c->scene.d_nodes_walk, c->scene.bvh4.n_nodes, d_tmp, c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            free(c->scene.walked_nodes);
            c->scene.walked_nodes = (mcrt_bvh4_node *)malloc(bytes);
            if (e == hipSuccess && c->scene.walked_nodes) e = hipMemcpy(c->scene.walked_nodes, d_tmp, bytes, hipMemcpyDeviceToHost);
            d_tmp.reset();
            if (!c->scene.walked_nodes) return set_error(MCRT_ERR_NOMEM, "out of memory");
            if (e != hipSuccess) return set_error(MCRT_ERR_HIP, "mcrt_get_bvh4: %s", hipGetErrorString(e));
            c->scene.walked_stale = false;
        }
        out->n_nodes = c->scene.bvh4.n_nodes; out->max_stack = c->scene.bvh4.max_stack; out->nodes = c->scene.walked_nodes;
        return MCRT_OK;
    }
    MCRT_TRY(download_bvh(c));
    *out = c->scene.bvh4;
    return MCRT_OK;
}

extern "C" int mcrt_upload_texture(mcrt_ctx *c, const float *vox, uint32_t n)
{
    CTX_TRY(c);
    if (n == 0) return set_error(MCRT_ERR_INVALID, "texture size 0");
    const size_t total = (size_t)n * n * n;
    std::vector<float> gen;
    bool finite = true;
    if (!vox) {
        gen.resize(total * 2);
        MCRT_TRY(mcrt_generate_texture(gen.data(), n));
        vox = gen.data();
    } else {
        for (size_t i = 0; i < total * 2; i++) if (!std::isfinite(vox[i])) { finite = false; break; }
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->tex_n = 0;
    HIP_TRY(c->d_tex.alloc(total));
    HIP_TRY(hipMemcpy(c->d_tex, vox, total * 8, hipMemcpyHostToDevice));
    c->tex_n = n; c->tex_finite = finite;
    return MCRT_OK;
}

extern "C" int mcrt_set_transducer(mcrt_ctx *c, const float *pos, const float *dir, uint32_t n)
{
    CTX_TRY(c);
    if (!pos || !dir || n == 0) return set_error(MCRT_ERR_INVALID, "mcrt_set_transducer: bad arguments");
    if (n != c->n_el) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->n_el = 0;                                   // (set again once both tables are held)
        HIP_TRY(c->d_pos.alloc(3 * (size_t)n));
        HIP_TRY(c->d_dir.alloc(3 * (size_t)n));
        c->n_el = n;
    }
    HIP_TRY(hipMemcpyAsync(c->d_pos, pos, 12 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_dir, dir, 12 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));   // pos/dir may be pageable host memory owned by the caller
    return MCRT_OK;
}

extern "C" int mcrt_alloc(mcrt_ctx *c, size_t bytes, void **dev)
{
    CTX_TRY(c);
    if (!dev) return set_error(MCRT_ERR_INVALID, "null out pointer");
    HIP_TRY(hipMalloc(dev, bytes ? bytes : 1));
    return MCRT_OK;
}
extern "C" int mcrt_free(mcrt_ctx *c, void *dev) { CTX_TRY(c); HIP_TRY(hipStreamSynchronize(c->stream)); HIP_TRY(hipFree(dev)); return MCRT_OK; }
extern "C" int mcrt_memcpy_d2h(mcrt_ctx *c, void *host, const void *dev, size_t bytes)
{
    CTX_TRY(c);
    HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MCRT_OK;
}
extern "C" int mcrt_memcpy_h2d(mcrt_ctx *c, void *dev, const void *host, size_t bytes)
{
    CTX_TRY(c);
    HIP_TRY(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MCRT_OK;
}

extern "C" int mcrt_enable_stats(mcrt_ctx *c, int on) { CTX_TRY(c); c->ins.stats_on = on != 0; return MCRT_OK; }
// words [first, first + n) of the context's counter block, once the stream is idle; zeroed afterwards on request
static int read_stats(mcrt_ctx *c, size_t first, size_t n, void *out, int reset)
{
    CTX_TRY(c);
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out, c->ins.d_stats + first, n * 8, hipMemcpyDeviceToHost));
    if (reset) { HIP_TRY(hipMemsetAsync(c->ins.d_stats + first, 0, n * 8, c->stream)); HIP_TRY(hipStreamSynchronize(c->stream)); }
    return MCRT_OK;
}
extern "C" int mcrt_get_stats(mcrt_ctx *c, mcrt_stats *out, int reset)
{
    unsigned long long v[6];
    MCRT_TRY(read_stats(c, 0, 6, v, reset));
    if (out) { out->queries = v[0]; out->nodes_visited = v[1]; out->tris_tested = v[2]; out->segments = v[3]; out->rf_steps = v[4]; out->hits = v[5]; }
    return MCRT_OK;
}

// diagnostic builds (-DMCRT_STAMP): per-phase cycle sums of k_trace [0,16) and its per-bounce launch timeline [16,120), k_march's sections [120,130) (the timeline alone: -DMCRT_STAMP_LITE); zeros otherwise
extern "C" int mcrt_debug_stamps(mcrt_ctx *c, uint64_t out[200], int reset) { return read_stats(c, 8, 200, out, reset); }

extern "C" int mcrt_debug_tail_histograms(mcrt_ctx *c, uint64_t out[2560], int reset)
{
    CTX_TRY(c);
    if (!out) return set_error(MCRT_ERR_INVALID, "null out pointer");
    return read_stats(c, 256, 2560, out, reset);
}

extern "C" int mcrt_debug_fast_paths(mcrt_ctx *c, uint32_t out[4])
{
    CTX_TRY(c);
    if (!out) return set_error(MCRT_ERR_INVALID, "null out pointer");
    out[0] = c->tab.fast_div ? 1u : 0u; out[1] = c->ins.last_lean_bound > 0.0f ? 1u : 0u; out[2] = c->ins.last_march_rows; out[3] = 0u;
    return MCRT_OK;
}

// what bounce b by beams did in the last traced pass (work set 0): whether it ran, rays its lists decided, leftover rays walked, beams incomplete, beams refused,
// beams in use, sampled rays whose group found no slot, slots claimed
static int debug_beam(mcrt_ctx *c, uint32_t b, uint32_t out[8])
{
    for (int k = 0; k < 8; k++) out[k] = 0u;
    if (b >= MCRT_MAX_BOUNCES || !((c->ins.last_beam_mask >> b) & 1u) || c->work.empty()) return MCRT_OK;
    const Work &w = c->work[0];
    uint32_t lc[MCRT_BEAM_COUNTERS] = {}, n = 0;
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(lc, w.beam.lcount.p + (size_t)b * MCRT_BEAM_COUNTERS, sizeof lc, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&n, w.b.counts.p + b, 4, hipMemcpyDeviceToHost));
    const uint32_t walked = lc[c->ins.last_beam_far ? 1 : 0];
    out[0] = 1u; out[1] = n - walked; out[2] = walked; out[3] = lc[2]; out[4] = lc[3]; out[5] = lc[4]; out[6] = lc[6]; out[7] = lc[7];
    return MCRT_OK;
}
extern "C" int mcrt_debug_beam(mcrt_ctx *c, uint32_t out[6])
{
    CTX_TRY(c);
    if (!out) return set_error(MCRT_ERR_INVALID, "null out pointer");
    uint32_t o[8];
    MCRT_TRY(debug_beam(c, 1u, o));
    for (int k = 0; k < 6; k++) out[k] = o[k];
    return MCRT_OK;
}
extern "C" int mcrt_debug_beam_bounce(mcrt_ctx *c, uint32_t b, uint32_t out[8])
{
    CTX_TRY(c);
    if (!out) return set_error(MCRT_ERR_INVALID, "null out pointer");
    return debug_beam(c, b, out);
}

// the beam order of bounce b in the last traced pass (work set 0): whether the bounce was ordered, rays placed, segments (beams with rays, the pseudo-beam of
// the rays without a beam among them), pad lanes, and the (wavefront, beam) pairs the first pass of k_beam_test met -- counted only in a context created with
// MCRT_BEAM_PAIRS=1, ordered or not; 0 otherwise
extern "C" int mcrt_debug_beam_order(mcrt_ctx *c, uint32_t b, uint32_t out[5])
{
    CTX_TRY(c);
    if (!out) return set_error(MCRT_ERR_INVALID, "null out pointer");
    for (int k = 0; k < 5; k++) out[k] = 0u;
    if (b >= MCRT_MAX_BOUNCES || !((c->ins.last_beam_mask >> b) & 1u) || c->work.empty()) return MCRT_OK;
    uint32_t lc[MCRT_BEAM_COUNTERS] = {};
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(lc, c->work[0].beam.lcount.p + (size_t)b * MCRT_BEAM_COUNTERS, sizeof lc, hipMemcpyDeviceToHost));
    out[0] = (c->ins.last_beam_order >> b) & 1u; out[1] = lc[8]; out[2] = lc[9]; out[3] = lc[10]; out[4] = lc[11];
    return MCRT_OK;
}

// the records, lists and group keys bounce b by beams left in the last traced pass (work set 0).  The buffers are shared by the pass's beamed bounces (stream order):
// what they hold is the LAST beamed bounce's, and only that bounce is answered
extern "C" int mcrt_debug_beam_records(mcrt_ctx *c, uint32_t b, uint32_t info[5], uint32_t *records, uint32_t *lists, uint64_t *keys)
{
    CTX_TRY(c);
    if (!info) return set_error(MCRT_ERR_INVALID, "null info pointer");
    for (int k = 0; k < 5; k++) info[k] = 0u;
    const uint32_t mask = c->ins.last_beam_depth >= 32u ? c->ins.last_beam_mask : c->ins.last_beam_mask & ((1u << c->ins.last_beam_depth) - 1u);
    if (b >= MCRT_MAX_BOUNCES || !((mask >> b) & 1u) || c->work.empty()) return set_error(MCRT_ERR_INVALID, "bounce %u did not run by beams in the last traced pass", b);
    if ((mask >> b) != 1u) return set_error(MCRT_ERR_INVALID, "bounce %u was not the last bounce by beams of the last traced pass: its records and lists have been overwritten", b);
    const BeamBufs &w = c->work[0].beam;
    const uint32_t groups = b == 1u ? 0u : c->ins.last_beam_groups, cap = c->ins.last_beam_cap;
    const uint32_t n_beams = b == 1u ? c->ins.last_beam_b1 : groups * 6u, n_lists = b == 1u ? c->ins.last_beam_b1 : groups * MCRT_BEAM_LISTS_PER_GROUP;
    if (n_beams > w.beams || n_lists > w.lists || groups > w.groups || cap != w.cap) return set_error(MCRT_ERR_INVALID, "the beam buffers of the last traced pass are gone");
    info[0] = n_beams; info[1] = cap; info[2] = c->ins.last_beam_near; info[3] = groups; info[4] = n_lists;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (records) HIP_TRY(hipMemcpy(records, w.rec.p, (size_t)n_beams * MCRT_BEAM_REC * 4, hipMemcpyDeviceToHost));
    if (lists) HIP_TRY(hipMemcpy(lists, w.list.p, (size_t)n_lists * cap * 64, hipMemcpyDeviceToHost));
    if (keys && groups) HIP_TRY(hipMemcpy(keys, w.gkey.p, (size_t)groups * 8, hipMemcpyDeviceToHost));
    return MCRT_OK;
}

// the hot parts of the same lists (BeamBufs::hot: plane | padded lo, begin | padded hi, id): the ten words of plane and bounds, and apart from them the two
// words k_beam_test reads there in place of the list's own (begin depth, id)
extern "C" int mcrt_debug_beam_entries(mcrt_ctx *c, uint32_t b, uint32_t info[5], uint32_t *entries, uint32_t *begin_id)
{
    MCRT_TRY(mcrt_debug_beam_records(c, b, info, nullptr, nullptr, nullptr));
    if (!entries && !begin_id) return MCRT_OK;
    const size_t n = (size_t)info[4] * info[1];
    std::vector<uint32_t> hot;
    try { hot.resize(n * MCRT_BEAM_HOT); } catch (const std::bad_alloc &) { return set_error(MCRT_ERR_NOMEM, "no memory for %zu list entries", n); }
    HIP_TRY(hipMemcpy(hot.data(), c->work[0].beam.hot.p, hot.size() * 4, hipMemcpyDeviceToHost));
    for (size_t e = 0; e < n; e++) {
        const uint32_t *h = hot.data() + e * MCRT_BEAM_HOT;
        if (entries) {
            uint32_t *o = entries + e * MCRT_DEBUG_BEAM_ENTRY;
            for (int k = 0; k < 7; k++) o[k] = h[k];
            for (int k = 0; k < 3; k++) o[7 + k] = h[8 + k];
        }
        if (begin_id) { begin_id[2 * e] = h[7]; begin_id[2 * e + 1] = h[11]; }
    }
    return MCRT_OK;
}

// k_beam_scan's arithmetic on the host (no context, no device): the segment bases of n counters -- the last is the pseudo-beam's --, and rays placed, segments,
// pad lanes and the order's length
extern "C" int mcrt_debug_beam_layout(const uint32_t *counts, uint32_t n, uint32_t *bases, uint32_t out[4])
{
    if ((!counts || !bases) && n) return set_error(MCRT_ERR_INVALID, "null pointer");
    if (!out) return set_error(MCRT_ERR_INVALID, "null out pointer");
    uint64_t at = 0, placed = 0;
    uint32_t segments = 0;
    for (uint32_t k = 0; k < n; k++) {
        if (at > 0xffffffffull) return set_error(MCRT_ERR_LIMIT, "the beam order is longer than 2^32 words");
        bases[k] = (uint32_t)at;
        at += mcrt::beam_segment(counts[k]); placed += counts[k]; segments += counts[k] != 0u ? 1u : 0u;
    }
    if (at > 0xffffffffull) return set_error(MCRT_ERR_LIMIT, "the beam order is longer than 2^32 words");
    out[0] = (uint32_t)placed; out[1] = segments; out[2] = (uint32_t)(at - placed); out[3] = (uint32_t)at;
    return MCRT_OK;
}

// k_beam_scan alone (mcrt_beam.hip) on `counts` as the beams' counters, in buffers of its own: the bases, the four totals and the order buffer, which is filled
// with a sentinel before -- what the kernel wrote there are the pads
extern "C" int mcrt_debug_beam_scan(mcrt_ctx *c, const uint32_t *counts, uint32_t n, uint32_t *bases, uint32_t out[4], uint32_t *order_words)
{
    CTX_TRY(c);
    if (!counts || !bases || !out) return set_error(MCRT_ERR_INVALID, "null pointer");
    if (n == 0u) return set_error(MCRT_ERR_INVALID, "a beam order has at least the pseudo-beam's counter");
    std::vector<uint32_t> host_bases(n);
    uint32_t lay[4];
    MCRT_TRY(mcrt_debug_beam_layout(counts, n, host_bases.data(), lay));      // (the length: the order buffer's size, checked against 2^32)
    const size_t len = lay[3];
    Buf<uint32_t> ocount, obase, order, lcount;
    HIP_TRY(ocount.alloc(n)); HIP_TRY(obase.alloc(n)); HIP_TRY(order.alloc(len + 64)); HIP_TRY(lcount.alloc(MCRT_BEAM_COUNTERS));
    std::vector<uint32_t> fill(len + 64, MCRT_DEBUG_BEAM_SENTINEL);      // (64 guard words past the length)
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(ocount, counts, (size_t)n * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(order, fill.data(), (len + 64) * 4, hipMemcpyHostToDevice));
    // (on the context's stream: a memset of device memory on the null stream does not wait for the host, and the context's stream does
    // not wait for the null stream -- the counters were once cleared after the kernel had written them)
    HIP_TRY(hipMemsetAsync(obase, 0xff, (size_t)n * 4, c->stream)); HIP_TRY(hipMemsetAsync(lcount, 0, MCRT_BEAM_COUNTERS * 4, c->stream));
    mcrt::BeamArgs g = {};
    g.n_beams = n - 1u; g.ocount = ocount; g.obase = obase; g.order = order; g.lcount = lcount; g.ordered = 1u;
    HIP_TRY(mcrt::launch_beam_scan(g, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    uint32_t lc[MCRT_BEAM_COUNTERS] = {};
    HIP_TRY(hipMemcpy(lc, lcount, sizeof lc, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(bases, obase, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (order_words) HIP_TRY(hipMemcpy(order_words, order, (len + 64) * 4, hipMemcpyDeviceToHost));
    out[0] = lc[8]; out[1] = lc[9]; out[2] = lc[10]; out[3] = lc[12];
    return MCRT_OK;
}

extern "C" int mcrt_debug_set_error(mcrt_ctx *c, uint32_t bits)
{
    CTX_TRY(c);
    if (!c->knobs.test_hooks) return set_error(MCRT_ERR_INVALID, "mcrt_debug_set_error is a test hook: create the context with MCRT_TEST_HOOKS set in the environment");
    uint32_t e = 0;
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(&e, c->d_error, 4, hipMemcpyDeviceToHost));
    e |= bits;
    HIP_TRY(hipMemcpy(c->d_error, &e, 4, hipMemcpyHostToDevice));
    return MCRT_OK;
}

extern "C" int mcrt_enable_timing(mcrt_ctx *c, int on) { CTX_TRY(c); c->ins.timing_on = on != 0; c->ins.timing_level = on; return MCRT_OK; }
extern "C" int mcrt_get_kernel_times(mcrt_ctx *c, double avg_ms[3], uint32_t n[3], int reset)
{
    CTX_TRY(c);
    // each recorded pair is waited for by itself: the pairs live on the streams their launches ran on (the groups' own, the side streams), not
    // only on the one current now -- and a caller polling the walk's time does not stall on other contexts of the device
    double sum[3] = { 0, 0, 0 }; uint32_t cnt[3] = { 0, 0, 0 };
    for (size_t i = 0; i < c->ins.ev_used; i++) {
        const TimedLaunch &t = c->ins.ev[i];
        float ms = 0;
        HIP_TRY(hipEventSynchronize(t.end));
        HIP_TRY(hipEventElapsedTime(&ms, t.start, t.end));
        sum[t.kind] += ms; cnt[t.kind]++;
    }
    for (int k = 0; k < 3; k++) { if (avg_ms) avg_ms[k] = cnt[k] ? sum[k] / (double)cnt[k] : 0.0; if (n) n[k] = cnt[k]; }
    if (reset) c->ins.ev_used = 0;
    return MCRT_OK;
}
extern "C" int mcrt_get_kernel_time(mcrt_ctx *c, double *avg_ms, uint32_t *n, int reset)
{
    double a[3]; uint32_t k[3];
    MCRT_TRY(mcrt_get_kernel_times(c, a, k, reset));
    if (avg_ms) *avg_ms = a[0];
    if (n) *n = k[0];
    return MCRT_OK;
}

extern "C" int mcrt_debug_math(mcrt_ctx *c, int op, const double *x, const double *y, double *out, uint32_t n)
{
    CTX_TRY(c);
    if (!x || !out || n == 0) return set_error(MCRT_ERR_INVALID, "mcrt_debug_math: bad arguments");
    Buf<double> dx, dy, dout;
    HIP_TRY(dx.alloc(n)); HIP_TRY(dout.alloc(n));
    HIP_TRY(hipMemcpy(dx, x, 8 * (size_t)n, hipMemcpyHostToDevice));
    if (y) { HIP_TRY(dy.alloc(n)); HIP_TRY(hipMemcpy(dy, y, 8 * (size_t)n, hipMemcpyHostToDevice)); }
    HIP_TRY(mcrt::launch_math_probe(op, dx, dy, dout, n, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out, dout, 8 * (size_t)n, hipMemcpyDeviceToHost));
    return MCRT_OK;
}

extern "C" int mcrt_debug_philox(mcrt_ctx *c, const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4])
{
    CTX_TRY(c);
    Buf<uint32_t> d;
    HIP_TRY(d.alloc(4));
    HIP_TRY(mcrt::launch_philox_probe(ctr, key, d, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out, d, 16, hipMemcpyDeviceToHost));
    return MCRT_OK;
}
