// mcrt_api.cpp -- the C-ABI of include/mcrt.h: context, uploads, frame orchestration.
// Host C++ only; kernels live in the mcrt_*.hip files (map: mcrt_kernels.h), the owners of the HIP resources in mcrt_hip.h.  No CPU
// fallback exists: every compute entry point needs the GPU context.
#include "../../include/mcrt.h"
#include "mcrt_internal.h"
#include "mcrt_hip.h"
#include "mcrt_kernels.h"
#include "mcrt_lbvh.h"

#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <algorithm>
#include <memory>
#include <utility>

using mcrt::set_error;

#define CTX_TRY(ctx) do { if (!(ctx)) return set_error(MCRT_ERR_INVALID, "null context"); HIP_TRY(hipSetDevice((ctx)->device)); } while (0)

struct Consts {   // main.cpp:23-37, rfimage.h:48-51,178-180 evaluated at run time
    float axial_res_f; double axial_res_mm, time_step_us, row_dt_us, max_travel_us; uint32_t axial_res_um, max_rows;
};
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

// Work set of ONE wavefront pipeline: path state, queues, rays, closest-hit words, march records (segments on request), and the
// streams it runs on (k_march of bounce b runs on a low-priority side stream beside k_trace of bounce b+1).  A context can own
// several, to trace the scan-lines of a pass as independent groups on separate streams (MCRT_GROUPS, a tuning knob: one group
// measured best).
struct PathBufs {   // sized for `paths` paths of `depth` bounces
    Buf<float4> st0, st1, st2, mrec;
    Buf<unsigned long long> key0, key1;
    Buf<uint32_t> q, counts, seg_count, cursors;
    size_t paths = 0; uint32_t depth = 0;
};
struct Work {
    Stream stream, side[MCRT_SIDE_STREAMS];   // k_march of bounce b runs on side[b % n] (n: Plan::sides)
    Event ev_bounce[MCRT_MAX_BOUNCES], ev_join[MCRT_SIDE_STREAMS], ev_done;
    Buf<int> stack_ovf;                       // traversal-stack overflow of THIS work set's walk (its launches run beside the other groups')
    Buf<mcrt_segment> segs;                   // [paths][depth], only for the callers that ask for segments
    Buf<int32_t> hits;                        // [paths][depth], only for the callers that ask for hit indices
    PathBufs b;
};

// tuning knobs from the environment, read ONCE at mcrt_create (never on the frame path) -- and only in a process started with
// MCRT_TUNING=1 (mcrt::tuning_env): linked into someone else's program the library has its defaults and nothing else.
struct Knobs {
    uint32_t ksplit_limit = MCRT_KSPLIT_DEFAULT, trace_blocks = 0, trace_blocks_wide = 0, wide_from = 0 /* 0: the kernels' own default */, wide_max_tree_mb = 128, groups = MCRT_GROUPS_DEFAULT, march_streams = MCRT_SIDE_STREAMS_DEFAULT, march_blocks = 0;   // march_blocks 0: launch_march picks
    bool no_overlap = false, no_priority = false, no_fast_div = false, no_lean = false;
    uint32_t path_groups = MCRT_PATH_GROUPS_DEFAULT;   // ... as this many scan-line groups on their own streams: a group's accumulation runs beside the other groups' last walks
    uint32_t path_max = MCRT_PATH_MAX_DEFAULT;    // passes of at most this many paths run as ONE launch that carries every path through all of its bounces (k_path: the latency form)
    uint32_t packet_mask = MCRT_PACKET_MASK_DEFAULT, packet_from = MCRT_PACKET_FROM;   // bit b: bounce b is walked by k_trace_packet (one wavefront per packet of 64 queue neighbours), in passes of at least packet_from paths
    bool retire_late = true;                   // MCRT_RETIRE_LATE=0: paths past the image are traced to their end, as before (FrameArgs::retire_late)
    bool fold_b0 = false;                      // MCRT_FOLD_B0=1: bounce 0 of a silent start medium is accumulated by k_shade itself (FrameArgs::fold_b0).  Bit-identical, one launch and
                                               // 48 B per path less, and no faster on the MI355X (profiles/retire_fold): off until a pass is found that it helps
    bool test_hooks = false;                   // MCRT_TEST_HOOKS: mcrt_debug_set_error may poison the context (tests only)
};
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
    return k;
}

// A float table [R][n] that a caller hands over as HOST memory with every call, on the device as [n][R] (n == 1: as it is), uploaded only
// when its bits or its shape differ from what is there.  put() is the whole contract: the device buffer, the pinned staging and the event
// are made on first use, all or none; the comparison is bitwise, on the caller's layout; the staging buffer is rewritten only after the
// previous copy's event; the table has no shape until its copy is enqueued; nothing else waits for the device; and the caller's array is
// free the moment put() returns.
struct StagedTable {
    Buf<float> dev; PinnedBuf<float> pin; Event ev; bool pending = false;
    std::vector<float> on_dev; uint32_t key[2] = { 0, 0 };   // what the device holds (or is about to): the caller's bits, and R, n
    int put(const float *src, uint32_t R, uint32_t n, size_t room, hipStream_t st)   // room: floats of the largest table this one may be given
    {
        if (!dev) {
            Buf<float> d; PinnedBuf<float> h; Event e;
            HIP_TRY(d.alloc(room));
            HIP_TRY(h.alloc(room));
            HIP_TRY(ensure_event(e));
            dev = std::move(d); pin = std::move(h); ev = std::move(e);
            on_dev.assign(room, 0.0f); key[0] = key[1] = 0;
        }
        const size_t len = (size_t)n * R;
        if (key[0] == R && key[1] == n && !memcmp(src, on_dev.data(), 4 * len)) return MCRT_OK;
        if (pending) HIP_TRY(hipEventSynchronize(ev));   // the staging buffer still feeds the previous table's copy
        for (uint32_t r = 0; r < R; r++)
            for (uint32_t k = 0; k < n; k++) pin[(size_t)k * R + r] = src[(size_t)r * n + k];
        key[0] = key[1] = 0;
        HIP_TRY(hipMemcpyAsync(dev, pin, 4 * len, hipMemcpyHostToDevice, st));
        HIP_TRY(hipEventRecord(ev, st));
        pending = true;
        memcpy(on_dev.data(), src, 4 * len);
        key[0] = R; key[1] = n;
        return MCRT_OK;
    }
};

// The scan-conversion maps of a geometry on the device, [N][2][n_pad]: per view the column map, then the row map; n_pad = out_rows * out_cols
// rounded up to 256 floats and zero-padded, so every map is 16-byte aligned.  Filled by ensure_maps, which owns the key.
struct MapCache {
    Buf<float> d; uint32_t key[7] = {}; double keyd[3] = {}; uint32_t steer[16] = {};
    static size_t pad(size_t n) { return (n + 255u) & ~(size_t)255u; }
};

// The maps of volume imaging (mcrt_volume_frames, mcrt_bmode_volume_frames) on the device: per grid [3][n_pad], plane, column, row, in
// MapCache's padding.  The four most recently used grids stay (a volume and three orthogonal cuts per frame); ensure_volume_maps owns the
// keys: the integers and float bits in key, the doubles in keyd, each compared bit for bit on its own.  used: the slot's last call, 0 = empty.
struct VolumeMapCache {
    struct Slot { Buf<float> d; uint32_t key[9] = {}; double keyd[15] = {}; uint64_t used = 0; };
    Slot slot[4]; uint64_t clock = 0;
};

struct TimedLaunch { Event start, end; int kind = 0; };   // kind 0: the walk (k_trace*, k_path), 1: k_shade, 2: k_march

struct mcrt_ctx {
    int device = 0;
    Knobs knobs;
    Stream own_stream; hipStream_t stream = nullptr;
    std::vector<Work> work;                               // one per concurrent scan-line group (see plan_pass); never moves once a pass holds pointers into it
    Event ev_start;
    mcrt_params p{};
    Consts c{};
    // scene
    mcrt_bvh bvh{};
    mcrt_bvh4 bvh4{};
    Buf<uint32_t> d_error;
    Buf<float4> d_nodes, d_tris, d_mats;
    mcrt_bvh4_node *walked_nodes = nullptr; bool walked_stale = true;   // host copy of the tree as the lane walk sees it (mcrt_get_bvh4)
    Buf<uint4> d_nodes_walk;                              // the walk's child-transposed half-float nodes
    Buf<uint4> d_meshes;
    Buf<uint32_t> d_tri_slot;
    Buf<float4> d_tris_id;                                // the triangle records in id order (refresh_soa)
    uint32_t n_mesh = 0, n_mat = 0, start_mat = 0, n_cu = 256;
    bool start_silent = false;                            // the start material has mu0 == sigma == 0: its segments' step echoes are +0 in a finite texture (k_march's `silent`)
    int builder = MCRT_BVH_HOST_SAH; bool host_bvh_stale = false;   // device-built tree: host copies are downloaded on demand
    std::vector<uint32_t> tri_mesh;   // per-triangle mesh index of the uploaded scene (for mcrt_update_triangles)
    float scene_lo[3] = { 0, 0, 0 }, scene_hi[3] = { 0, 0, 0 };
    float spacing[3] = { 1, 1, 1 };
    bool have_scene = false;
    // texture
    Buf<float2> d_tex; uint32_t tex_n = 0; bool tex_finite = false;
    // transducer
    Buf<float> d_pos, d_dir; uint32_t n_el = 0;
    const float *pose_pos = nullptr, *pose_dir = nullptr;      // set for the duration of mcrt_trace_frames_poses: device [F][E][3] per-frame probe poses
    Buf<float> d_pose[2];                                      // staging for pose tables handed over as host memory:
    PinnedBuf<float> h_pose[2]; Event ev_pose; bool pose_copy_pending = false;   // the caller's table is copied into pinned memory the context owns before the call returns
    Event ev_scene; hipStream_t scene_stream = nullptr; bool scene_pending = false;   // the last scene update's device work (refresh_soa), for traces issued on ANOTHER stream
    // accumulators
    Buf<long long> d_acc; Buf<uint32_t> d_flags;
    uint32_t acc_clean_ne = 0, acc_clean_rows = 0;   // bins known to be all-zero for this shape (k_finalize leaves them so)
    Buf<float> d_tmp;
    // row thresholds (exact replacement of the per-echo double division) and the verified fast division by tex_res
    Buf<double> d_row_thr; uint32_t thr_rows = 0; double thr_dt = 0.0, thr_end = 0.0;   // thr_end: the table's last entry, the first time past the image
    float verified_res = 0.0f; bool fast_div = false, fast_div_all = false;
    float last_lean_bound = 0.0f; uint32_t last_march_rows = 0;   // what the last frame's kernels were given (mcrt_debug_fast_paths)
    // per-material table of k_march (depends on the materials, the axial step and the frequency)
    Buf<float4> d_mtab; float mtab_key[2] = { 0.0f, 0.0f }; bool mtab_valid = false;
    // scan-conversion maps: of the plain geometry (mcrt_scan_convert_frames, mcrt_bmode_frames; one unsteered view) and of a steer list (spatial
    // compounding: mcrt_compound_frames, mcrt_bmode_compound_frames), each in a cache of its own so that alternating calls do not evict each other
    MapCache maps, cmaps;
    VolumeMapCache vmaps;
    // B-mode display (mcrt_bmode_frames): the peaks of a pass [65536], and the TGC factors [R] of the last curve
    Buf<float> d_disp; StagedTable tgc;
    // focal zones (mcrt_convolve_frames_depth): the lateral taps [n_lat][R], and slice thickness (mcrt_elevation_frames): the elevation weights
    // [K][R] (room for MCRT_MAX_ROWS x 32 each).  Two tables: a frame uses both in turn, and one shared buffer would upload both on every frame
    StagedTable lat_rows, elev_rows;
    // instrumentation
    Buf<unsigned long long> d_stats; bool stats_on = false;
    bool timing_on = false; int timing_level = 0;       // 1: the walk's launches are bracketed by HIP events; 2: k_shade's and k_march's too
    std::vector<TimedLaunch> ev; size_t ev_used = 0;
    ~mcrt_ctx() { free(walked_nodes); mcrt_free_bvh(&bvh); mcrt_free_bvh4(&bvh4); }   // (the HIP resources release themselves)
};


static int prepare_tables(mcrt_ctx *c)
{
    if (c->thr_rows != c->p.n_rows || c->thr_dt != c->c.row_dt_us || !c->d_row_thr) {
        std::vector<double> thr((size_t)c->p.n_rows + 1);
        MCRT_TRY(mcrt_row_thresholds(c->c.row_dt_us, c->p.n_rows, thr.data()));
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->thr_rows = 0;
        HIP_TRY(c->d_row_thr.alloc(thr.size()));
        HIP_TRY(hipMemcpy(c->d_row_thr, thr.data(), thr.size() * 8, hipMemcpyHostToDevice));
        c->thr_rows = c->p.n_rows; c->thr_dt = c->c.row_dt_us; c->thr_end = thr.back();
    }
    if (c->verified_res != c->p.tex_res) {
        // the GPU checks, exhaustively, that its fma-corrected reciprocal multiply IS IEEE division by tex_res
        Buf<unsigned long long> d_bad; unsigned long long bad = 1;
        HIP_TRY(d_bad.alloc(1));
        HIP_TRY(hipMemsetAsync(d_bad, 0, 8, c->stream));
        HIP_TRY(mcrt::launch_verify_div(c->p.tex_res, 1.0f / c->p.tex_res, d_bad, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipMemcpy(&bad, d_bad, 8, hipMemcpyDeviceToHost));
        c->fast_div = (bad == 0) && !c->knobs.no_fast_div;
        c->fast_div_all = c->fast_div && c->p.tex_res > 1e-16f && !c->knobs.no_lean;
        c->verified_res = c->p.tex_res;
    }
    if (c->have_scene && (!c->mtab_valid || c->mtab_key[0] != c->c.axial_res_f || c->mtab_key[1] != c->p.frequency)) {
        c->mtab_valid = false;
        if (c->d_mtab.cap < c->n_mat) {
            HIP_TRY(hipStreamSynchronize(c->stream));
            HIP_TRY(c->d_mtab.alloc(c->n_mat));
        }
        HIP_TRY(mcrt::launch_material_table(c->d_mats, c->n_mat, c->c.axial_res_f, c->p.frequency, c->d_mtab, c->stream));
        c->mtab_key[0] = c->c.axial_res_f; c->mtab_key[1] = c->p.frequency; c->mtab_valid = true;
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
    HIP_TRY(c->d_stats.alloc(MCRT_STATS_WORDS));
    HIP_TRY(hipMemsetAsync(c->d_stats, 0, MCRT_STATS_WORDS * sizeof(unsigned long long), c->stream));
    HIP_TRY(c->d_error.alloc(1));
    HIP_TRY(hipMemsetAsync(c->d_error, 0, 4, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    MCRT_TRY(prepare_tables(c.get()));
    *out = c.release();
    return MCRT_OK;
}

// work set g (created on first use).  Streams are created only when a pipeline asks for them (work_stream / side_stream):
// HIP multiplexes streams onto a few hardware queues, where one stream's event wait holds up whatever shares its queue, so a
// context keeps no stream it does not use.
static int get_work(mcrt_ctx *c, size_t g, Work **out)
{
    while (c->work.size() <= g) {
        Work w;
        for (Event &e : w.ev_join) HIP_TRY(ensure_event(e));
        for (Event &e : w.ev_bounce) HIP_TRY(ensure_event(e));
        HIP_TRY(ensure_event(w.ev_done));
        c->work.push_back(std::move(w));
    }
    *out = &c->work[g];
    return MCRT_OK;
}

// the stream of scan-line group g >= 1 of a pass (group 0 runs on the context's stream)
static int work_stream(Work &w, hipStream_t *out)
{
    if (!w.stream) HIP_TRY(hipStreamCreateWithFlags(&w.stream.h, hipStreamNonBlocking));
    *out = w.stream;
    return MCRT_OK;
}
// k_march runs beside the walk on a LOW-priority stream: k_trace / k_shade are the critical chain, and their workgroups must
// not queue behind k_march's (measured: k_shade took 0.4-0.7 ms instead of 0.1 ms when they did)
static int side_stream(mcrt_ctx *c, Work &w, uint32_t i, hipStream_t *out)
{
    if (!w.side[i]) {
        int prio_low = 0, prio_high = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&prio_low, &prio_high));
        if (c->knobs.no_priority) prio_low = 0;   // tuning knob
        HIP_TRY(hipStreamCreateWithPriority(&w.side[i].h, hipStreamNonBlocking, prio_low));
    }
    *out = w.side[i];
    return MCRT_OK;
}

// the walk's view of the tree: child-transposed half-float nodes, rebuilt whenever d_nodes changes.  The buffer is kept while the
// node count stays (a refit -- the per-frame path of a deforming scene -- then costs one kernel on the context's stream and no
// allocation HERE; mcrt_refit_triangles itself still frees its staging copy of the vertices, which synchronises the device).
// Nothing here waits: the rebuild is ordered on the stream it was issued on, and an event recorded behind it orders a trace that
// is issued on ANOTHER stream after mcrt_set_stream (enqueue_pass waits for it).
static int refresh_soa(mcrt_ctx *c)
{
    c->walked_stale = true;
    if (c->bvh4.n_nodes == 0) { c->d_nodes_walk.reset(); return MCRT_OK; }
    if (c->d_nodes_walk.cap != 4 * (size_t)c->bvh4.n_nodes) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(c->d_nodes_walk.alloc(4 * (size_t)c->bvh4.n_nodes));
    }
    HIP_TRY(mcrt::launch_nodes_walk(c->d_nodes, c->bvh4.n_nodes, c->d_nodes_walk, c->stream));
    if (c->d_tris_id.cap != MCRT_TRI_PIECES * (size_t)c->bvh.n_tri) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(c->d_tris_id.alloc(MCRT_TRI_PIECES * (size_t)c->bvh.n_tri));
    }
    HIP_TRY(mcrt::launch_tris_by_id((const float4 *)c->d_tris, c->bvh.n_tri, c->d_tris_id, c->stream));
    HIP_TRY(ensure_event(c->ev_scene));
    HIP_TRY(hipEventRecord(c->ev_scene, c->stream));
    c->scene_stream = c->stream; c->scene_pending = true;
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
static int check_device_error(mcrt_ctx *c)
{
    uint32_t e = 0;
    HIP_TRY(hipMemcpy(&e, c->d_error, 4, hipMemcpyDeviceToHost));
    if (e) { HIP_TRY(hipMemsetAsync(c->d_error, 0, 4, c->stream)); HIP_TRY(hipStreamSynchronize(c->stream)); return set_error(MCRT_ERR_LIMIT, "device error flag 0x%x:%s%s", e, (e & 1u) ? " BVH traversal stack overflow" : "", (e & 2u) ? " kernel watchdog expired (a persistent kernel ran for more than its time limit and was abandoned)" : ""); }
    return MCRT_OK;
}
extern "C" int mcrt_synchronize(mcrt_ctx *c) { CTX_TRY(c); HIP_TRY(hipStreamSynchronize(c->stream)); return check_device_error(c); }

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
    c->d_nodes.reset(); c->d_tris.reset(); c->d_tri_slot.reset();
    mcrt_free_bvh(&c->bvh); mcrt_free_bvh4(&c->bvh4);
    c->host_bvh_stale = false;
    const bool on_device = c->builder == MCRT_BVH_DEVICE_LBVH;
    Buf<float4> leaf;                                   // the builder's 48-byte leaf-order triangle array, on the device
    if (on_device) {
        mcrt::LbvhResult r;
        {
            Buf<float> d_tri; Buf<uint32_t> d_mesh;
            HIP_TRY(d_tri.alloc(9 * (size_t)n_tri));
            HIP_TRY(d_mesh.alloc(n_tri));
            if (hipMemcpyAsync(d_tri, tri, 36 * (size_t)n_tri, hipMemcpyDefault, c->stream) != hipSuccess ||
                hipMemcpyAsync(d_mesh, c->tri_mesh.data(), 4 * (size_t)n_tri, hipMemcpyHostToDevice, c->stream) != hipSuccess)
                return set_error(MCRT_ERR_HIP, "triangle upload failed");
            MCRT_TRY(mcrt::lbvh_build(d_tri, d_mesh, n_tri, c->stream, &r));
        }
        c->d_nodes = std::move(r.nodes); c->d_tri_slot = std::move(r.tri_slot); leaf = std::move(r.tris);
        c->bvh.n_nodes = 0; c->bvh.n_tri = n_tri; c->bvh.max_depth = r.max_depth; c->bvh.pad_abs = r.pad_abs; c->bvh.nodes = nullptr; c->bvh.tri = nullptr;
        c->bvh4.n_nodes = r.n_nodes4; c->bvh4.max_stack = r.max_stack; c->bvh4.nodes = nullptr;
        c->host_bvh_stale = true;
        for (int i = 0; i < 3; i++) { c->scene_lo[i] = r.lo[i]; c->scene_hi[i] = r.hi[i]; }
    } else if (pre) {
        if (pre->bvh->n_tri != n_tri) return set_error(MCRT_ERR_INVALID, "prebuilt tree has %u triangles, the scene %u", pre->bvh->n_tri, n_tri);
        MCRT_TRY(copy_tree(*pre, &c->bvh, &c->bvh4));
    } else {
        std::vector<float> host_copy;
        if (is_device_pointer(tri)) {   // the host builder reads host memory
            host_copy.resize((size_t)n_tri * 9);
            HIP_TRY(hipMemcpy(host_copy.data(), tri, 36 * (size_t)n_tri, hipMemcpyDeviceToHost));
            tri = host_copy.data();
        }
        MCRT_TRY(mcrt_build_bvh(tri, c->tri_mesh.data(), n_tri, &c->bvh));
        MCRT_TRY(mcrt_build_bvh4(&c->bvh, &c->bvh4));
    }
    if (c->bvh4.max_stack > MCRT_STACK)
        return set_error(MCRT_ERR_LIMIT, "%sBVH4 needs a %u-entry traversal stack, the kernel has %d", on_device ? "device-built " : "", c->bvh4.max_stack, MCRT_STACK);
    if (c->bvh4.n_nodes >= (1u << 25)) return set_error(MCRT_ERR_LIMIT, "%u BVH4 nodes: the walk addresses at most 2^25", c->bvh4.n_nodes);
    if (!on_device) {   // the host-built tree: its bounds, and its arrays go to the device
        for (int i = 0; i < 3; i++) { c->scene_lo[i] = INFINITY; c->scene_hi[i] = -INFINITY; }
        for (int k = 0; k < 4; k++) {
            const mcrt_bvh4_child &ch = c->bvh4.nodes[0].c[k];
            if (ch.ref == MCRT_BVH4_EMPTY) continue;
            const float hi[3] = { ch.hi_x, ch.hi_y, ch.hi_z };
            for (int i = 0; i < 3; i++) { c->scene_lo[i] = std::min(c->scene_lo[i], ch.lo[i]); c->scene_hi[i] = std::max(c->scene_hi[i], hi[i]); }
        }
        HIP_TRY(c->d_nodes.alloc(sizeof(mcrt_bvh4_node) / 16 * (size_t)c->bvh4.n_nodes));
        HIP_TRY(hipMemcpy(c->d_nodes, c->bvh4.nodes, sizeof(mcrt_bvh4_node) * (size_t)c->bvh4.n_nodes, hipMemcpyHostToDevice));
        HIP_TRY(leaf.alloc(3 * (size_t)n_tri));
        HIP_TRY(hipMemcpy(leaf, c->bvh.tri, 48 * (size_t)n_tri, hipMemcpyHostToDevice));
        // triangle id -> leaf-order slot (k_shade re-derives the winning triangle's normal from its vertices)
        std::vector<uint32_t> slot(n_tri);
        for (uint32_t k = 0; k < n_tri; k++) { uint32_t id; memcpy(&id, &c->bvh.tri[(size_t)k * 12 + 3], 4); slot[id] = k; }
        HIP_TRY(c->d_tri_slot.alloc(n_tri));
        HIP_TRY(hipMemcpy(c->d_tri_slot, slot.data(), 4 * (size_t)n_tri, hipMemcpyHostToDevice));
    }
    // the walk's 64-byte records from the builder's 48-byte leaf-order array
    HIP_TRY(c->d_tris.alloc(MCRT_TRI_PIECES * (size_t)n_tri));
    HIP_TRY(mcrt::launch_expand_tris(leaf, n_tri, c->d_tris, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MCRT_OK;
}

// host copies of a device-built tree, for mcrt_get_bvh / mcrt_get_bvh4
static int download_bvh(mcrt_ctx *c)
{
    if (!c->host_bvh_stale) return MCRT_OK;
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->bvh.tri = (float *)malloc(48 * (size_t)c->bvh.n_tri);
    c->bvh4.nodes = (mcrt_bvh4_node *)malloc(sizeof(mcrt_bvh4_node) * (size_t)c->bvh4.n_nodes);
    if (!c->bvh.tri || !c->bvh4.nodes) return set_error(MCRT_ERR_NOMEM, "out of memory");
    {   // back from the walk's records to the ABI's 48-byte layout (v0|id, v1|mesh, v2|0)
        const size_t W = 4 * MCRT_TRI_PIECES;      // floats per record
        std::vector<float> rec((size_t)c->bvh.n_tri * W);
        HIP_TRY(hipMemcpy(rec.data(), c->d_tris, 4 * W * (size_t)c->bvh.n_tri, hipMemcpyDeviceToHost));
        for (size_t t = 0; t < c->bvh.n_tri; t++) {
            const float *r = &rec[t * W]; float *o = &c->bvh.tri[t * 12];
            memcpy(o, r, 32);                                          // v0 | id, v1 | mesh
            o[8] = r[8]; o[9] = r[9]; o[10] = r[10]; o[11] = 0.0f;      // v2 | 0 (the record keeps the edge tolerance there)
        }
    }
    HIP_TRY(hipMemcpy(c->bvh4.nodes, c->d_nodes, sizeof(mcrt_bvh4_node) * (size_t)c->bvh4.n_nodes, hipMemcpyDeviceToHost));
    c->host_bvh_stale = false;
    return MCRT_OK;
}

extern "C" int mcrt_set_bvh_builder(mcrt_ctx *c, int builder)
{
    CTX_TRY(c);
    if (builder != MCRT_BVH_HOST_SAH && builder != MCRT_BVH_DEVICE_LBVH) return set_error(MCRT_ERR_INVALID, "unknown BVH builder %d", builder);
    c->builder = builder;
    return MCRT_OK;
}

// what mcrt_update_triangles and mcrt_refit_triangles ask alike: new positions for exactly the uploaded triangles, and an idle stream
static int check_new_positions(mcrt_ctx *c, const float *tri, uint32_t n_tri)
{
    CTX_TRY(c);
    if (!c->have_scene) return set_error(MCRT_ERR_INVALID, "no scene uploaded");
    if (!tri) return set_error(MCRT_ERR_INVALID, "null triangles");
    if (n_tri != c->bvh.n_tri || n_tri == 0) return set_error(MCRT_ERR_INVALID, "the scene has %u triangles, the update has %u", c->bvh.n_tri, n_tri);
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MCRT_OK;
}

static int update_triangles(mcrt_ctx *c, const float *tri, uint32_t n_tri, const mcrt::HostTree *pre)
{
    MCRT_TRY(check_new_positions(c, tri, n_tri));
    c->have_scene = false;                           // a failed rebuild leaves no scene
    MCRT_TRY(index_triangles(c, tri, n_tri, pre));
    MCRT_TRY(refresh_soa(c));
    c->have_scene = true;
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
    if (!rc) rc = mcrt::bvh_refit(d_tri, n_tri, c->d_nodes, c->bvh4.n_nodes, c->d_tris, c->stream, &pad, lo, hi);
    d_tri.reset();
    if (!rc) rc = refresh_soa(c);
    if (rc) { c->have_scene = false; return rc; }           // a failed refit leaves no scene
    c->bvh.pad_abs = pad;
    for (int i = 0; i < 3; i++) { c->scene_lo[i] = lo[i]; c->scene_hi[i] = hi[i]; }
    // the host copies (and the host builder's BVH2, which has no refitted counterpart) are out of date: downloaded on demand
    free(c->bvh.nodes); c->bvh.nodes = nullptr; c->bvh.n_nodes = 0;
    free(c->bvh.tri); c->bvh.tri = nullptr;
    free(c->bvh4.nodes); c->bvh4.nodes = nullptr;
    c->host_bvh_stale = true;
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
    free(c->walked_nodes); c->walked_nodes = nullptr; c->walked_stale = true;
    mcrt_free_bvh(&c->bvh); mcrt_free_bvh4(&c->bvh4);
    c->have_scene = false;
    if (n_tri) {
        c->tri_mesh.assign(tri_mesh, tri_mesh + n_tri);
        MCRT_TRY(index_triangles(c, tri, n_tri, pre));
        MCRT_TRY(refresh_soa(c));
    } else {
        c->d_nodes.reset(); c->d_tris.reset(); c->d_tri_slot.reset(); c->d_nodes_walk.reset(); c->d_tris_id.reset();
    }
    HIP_TRY(c->d_mats.alloc(2 * (size_t)n_mat));
    HIP_TRY(hipMemcpy(c->d_mats, mats, 32 * (size_t)n_mat, hipMemcpyHostToDevice));
    HIP_TRY(c->d_meshes.alloc(n_mesh));
    HIP_TRY(hipMemcpy(c->d_meshes, meshes, sizeof(mcrt_mesh) * (size_t)n_mesh, hipMemcpyHostToDevice));
    c->n_mesh = n_mesh; c->n_mat = n_mat; c->start_mat = start_mat;
    c->start_silent = mats[8 * (size_t)start_mat + 2] == 0.0f && mats[8 * (size_t)start_mat + 4] == 0.0f;
    for (int i = 0; i < 3; i++) c->spacing[i] = spacing[i];
    c->have_scene = true; c->mtab_valid = false;
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
int ctx_bvh_builder(const mcrt_ctx *c) { return c ? c->builder : MCRT_BVH_HOST_SAH; }
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
    if (!c->have_scene) return set_error(MCRT_ERR_INVALID, "no scene uploaded");
    MCRT_TRY(download_bvh(c));
    *out = c->bvh;
    return MCRT_OK;
}

extern "C" int mcrt_get_bvh4(mcrt_ctx *c, mcrt_bvh4 *out)
{
    if (!c || !out) return set_error(MCRT_ERR_INVALID, "null argument");
    if (!c->have_scene) return set_error(MCRT_ERR_INVALID, "no scene uploaded");
    HIP_TRY(hipSetDevice(c->device));
    if (c->d_nodes_walk) {
        // the tree AS WALKED: the lane-per-ray walk reads half-float boxes rounded outwards; decoded back into the builders' layout
        if (c->walked_stale || !c->walked_nodes) {
            const size_t bytes = sizeof(mcrt_bvh4_node) * (size_t)c->bvh4.n_nodes;
            Buf<float4> d_tmp;
            HIP_TRY(d_tmp.alloc(bytes / 16));
            hipError_t e = mcrt::launch_nodes_walk_decode(c->d_nodes_walk, c->bvh4.n_nodes, d_tmp, c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            free(c->walked_nodes);
            c->walked_nodes = (mcrt_bvh4_node *)malloc(bytes);
            if (e == hipSuccess && c->walked_nodes) e = hipMemcpy(c->walked_nodes, d_tmp, bytes, hipMemcpyDeviceToHost);
            d_tmp.reset();
            if (!c->walked_nodes) return set_error(MCRT_ERR_NOMEM, "out of memory");
            if (e != hipSuccess) return set_error(MCRT_ERR_HIP, "mcrt_get_bvh4: %s", hipGetErrorString(e));
            c->walked_stale = false;
        }
        out->n_nodes = c->bvh4.n_nodes; out->max_stack = c->bvh4.max_stack; out->nodes = c->walked_nodes;
        return MCRT_OK;
    }
    MCRT_TRY(download_bvh(c));
    *out = c->bvh4;
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

static int ensure_acc(mcrt_ctx *c, uint32_t ne)
{
    const size_t need = (size_t)ne * c->p.n_rows, needf = (size_t)ne * ((c->p.n_rows + 31u) >> 5);
    if (need > c->d_acc.cap || needf > c->d_flags.cap) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->acc_clean_ne = 0;
        HIP_TRY(c->d_acc.grow(need)); HIP_TRY(c->d_flags.grow(needf));
    }
    // k_finalize leaves the bins zeroed; only a shape change (or a failed frame) needs an explicit clear
    if (c->acc_clean_ne != ne || c->acc_clean_rows != c->p.n_rows) {
        HIP_TRY(hipMemsetAsync(c->d_acc, 0, need * 8, c->stream));
        HIP_TRY(hipMemsetAsync(c->d_flags, 0, needf * 4, c->stream));
    }
    c->acc_clean_ne = 0; c->acc_clean_rows = 0;   // dirty until the frame's k_finalize has been enqueued
    return MCRT_OK;
}

static int check_ready(mcrt_ctx *c, uint32_t e0, uint32_t e1)
{
    if (!c->have_scene) return set_error(MCRT_ERR_INVALID, "no scene uploaded");
    if (!c->d_tex) return set_error(MCRT_ERR_INVALID, "no texture uploaded");
    if (c->tex_n != c->p.tex_n) return set_error(MCRT_ERR_INVALID, "texture is %u^3 but params say %u^3", c->tex_n, c->p.tex_n);
    if (!c->pose_pos) {
        if (!c->d_pos) return set_error(MCRT_ERR_INVALID, "no transducer set");
        if (c->n_el != c->p.n_elements) return set_error(MCRT_ERR_INVALID, "transducer has %u elements but params say %u", c->n_el, c->p.n_elements);
    }
    if (e0 >= e1 || e1 > c->p.n_elements) return set_error(MCRT_ERR_INVALID, "scan-line range [%u,%u) invalid for %u elements", e0, e1, c->p.n_elements);
    return MCRT_OK;
}

// How one traced pass runs, decided here and nowhere else: the work sets are sized, the overflow stacks checked and the kernels
// launched from this plan, so they cannot disagree.  A pass that cannot fill the GPU runs in its LATENCY form: one launch carries every
// path through all of its bounces (k_path), one more accumulates every bounce's segments -- instead of a walk / shade launch pair per
// bounce, each as long as its slowest wavefront.  Every other pass runs STAGED: per bounce the walk and k_shade on the group's stream,
// k_march of the finished segments on a side stream beside the next bounce's walk.
struct Plan {
    bool latency = false;
    uint32_t groups = 1;                          // independent scan-line groups, each with its own work set and stream
    uint32_t trace_blocks = 0, trace_blocks_wide = 0;   // the staged walk's grids: k_trace_lane, k_trace_lane_wide (0: not taken)
    uint32_t e[17] = {};                          // group g traces scan-lines [e[g], e[g+1])
    uint32_t sides[16] = {};                      // side streams group g's accumulations rotate over (none in the latency form: its own stream)
    size_t ovf[16] = {};                          // traversal-stack overflow entries group g's work set is sized for
};

// one_group: the caller reads the per-path tables of work set 0 (mcrt_trace_frame_debug, mcrt_cast_rays)
static Plan plan_pass(const mcrt_ctx *c, uint32_t e0, uint32_t e1, uint32_t n_frames, bool one_group)
{
    Plan P;
    const uint32_t ne = e1 - e0, S = c->p.n_samples;
    P.latency = !c->stats_on && (uint64_t)ne * n_frames * S <= c->knobs.path_max;
    uint32_t groups = (one_group || c->stats_on) ? 1u : c->knobs.groups;
    if (!one_group && groups == 1u && P.latency) groups = c->knobs.path_groups;
    P.groups = std::max(1u, std::min({ groups, ne, 16u }));
    for (uint32_t g = 0; g <= P.groups; g++) P.e[g] = e0 + (uint32_t)(((uint64_t)ne * g) / P.groups);
    P.trace_blocks = c->knobs.trace_blocks ? c->knobs.trace_blocks : c->n_cu * 4u;   // persistent k_trace: 4 four-wave workgroups per CU (1024 on the MI355X's 256 CUs) of the 5 its registers and LDS allow --
                                                                                  // the fifth's registers go to a k_march wavefront beside them (since k_march's fast path: 0.446 -> 0.428 ms per frame on a 20-frame pass, 0.366 -> 0.364 at 128)
    P.trace_blocks_wide = c->knobs.trace_blocks_wide ? c->knobs.trace_blocks_wide : c->n_cu * 5u;      // k_trace_lane_wide: five workgroups per CU
    // ... while the tree is served from the caches: with 16 M triangles (460 MB of walked nodes, past the Infinity Cache) a fifth wavefront per SIMD only
    // adds misses -- 0.667 against 0.638 ms per frame -- where the 1 M-triangle scene (29 MB) gains 3-4 %; the line is drawn at half the Infinity Cache
    if ((uint64_t)c->bvh4.n_nodes * 64ull > (uint64_t)c->knobs.wide_max_tree_mb * 1048576ull) P.trace_blocks_wide = 0;
    const uint32_t lds_part = mcrt::lane_stack_entries();
    const size_t deep = c->bvh4.max_stack > lds_part ? c->bvh4.max_stack - lds_part : 0;
    for (uint32_t g = 0; g < P.groups; g++) {
        const uint64_t np = (uint64_t)(P.e[g + 1] - P.e[g]) * n_frames * S;
        // (two side streams only where the walk runs from the caches -- the five-wavefront form's own criterion --: on the 16 M-triangle streaming scene the walks
        //  are the longer chain and a second accumulation beside them costs 1.5 %: 0.607 against 0.598 ms per frame)
        if (!P.latency) P.sides[g] = c->knobs.march_streams ? c->knobs.march_streams : (P.trace_blocks_wide != 0u && np >= (uint64_t)MCRT_SIDE_STREAMS_TWO_FROM) ? 2u : 1u;
        uint32_t blocks = std::max({ c->knobs.trace_blocks, c->knobs.trace_blocks_wide, c->n_cu * 5u });   // (the larger of the walk's two forms)
        if (P.latency) blocks = std::max(blocks, mcrt::path_blocks(np));                                     // (... and k_path's grid)
        P.ovf[g] = deep * blocks * 256;
    }
    return P;
}

// out: 0 = RF image only, 1 = + hit indices, 2 = + the segment table (64 B per path and bounce: only allocated when asked for)
static int ensure_work(Work &w, size_t np, uint32_t B, size_t ovf, int out)
{
    if (out >= 2 && w.segs.cap < np * B) { HIP_TRY(hipDeviceSynchronize()); HIP_TRY(w.segs.alloc(np * B)); }
    if (out >= 1 && w.hits.cap < np * B) { HIP_TRY(hipDeviceSynchronize()); HIP_TRY(w.hits.alloc(np * B)); }
    if (ovf > w.stack_ovf.cap) { HIP_TRY(hipDeviceSynchronize()); HIP_TRY(w.stack_ovf.alloc(ovf)); }
    if (np <= w.b.paths && B <= w.b.depth) return MCRT_OK;
    HIP_TRY(hipDeviceSynchronize());
    w.b = PathBufs();                   // (the optional tables survive a re-allocation of the rest when they are large enough)
    PathBufs &b = w.b;
    HIP_TRY(b.st0.alloc(2 * np)); HIP_TRY(b.st1.alloc(2 * np)); HIP_TRY(b.st2.alloc(2 * np));   // two halves: bounce parity
    HIP_TRY(b.key0.alloc(np)); HIP_TRY(b.key1.alloc(np));
    HIP_TRY(b.q.alloc(2 * np)); HIP_TRY(b.seg_count.alloc(np));
    HIP_TRY(b.counts.alloc(MCRT_MAX_BOUNCES + 1));
    HIP_TRY(b.cursors.alloc((size_t)MCRT_MAX_BOUNCES * MCRT_XCDS * MCRT_CURSOR_STRIDE));
    HIP_TRY(b.mrec.alloc(3 * np * B));
    b.paths = np; b.depth = B;
    return MCRT_OK;
}

// the kernel arguments every group of a pass shares (acc_ne: scan-lines of the frame's RF block); fill_group adds each group's own
static void fill_pass(mcrt_ctx *c, const Plan &P, mcrt::FrameArgs &a, uint32_t frame, uint32_t acc_ne, bool accumulate, int out)
{
    memset(&a, 0, sizeof a);
    a.nodes_walk = c->d_nodes_walk; a.tris = c->d_tris; a.meshes = c->d_meshes; a.mats = c->d_mats; a.tex = c->d_tex;
    a.el_pos = c->pose_pos ? c->pose_pos : c->d_pos; a.el_dir = c->pose_pos ? c->pose_dir : c->d_dir; a.pose_stride = c->pose_pos ? c->p.n_elements : 0u;
    a.row_thr = c->d_row_thr;
    a.acc = c->d_acc; a.flags = c->d_flags; a.acc_stride = acc_ne;   // the frame block [n_frames][acc_ne][R]
    a.tri_slot = c->d_tri_slot; a.tris_id = c->d_tris_id; a.mtab = c->d_mtab;
    a.stats = c->d_stats; a.error_flag = c->d_error; a.stamps = c->d_stats + 8;
    a.n_mat = c->n_mat; a.n_mesh = c->n_mesh; a.n_nodes = c->bvh4.n_nodes; a.S = c->p.n_samples; a.B = c->p.max_depth; a.R = c->p.n_rows;
    a.ksplit_limit = c->knobs.ksplit_limit;   // bounces with fewer rays than this are cut into pieces (see k_trace)
    if (c->stats_on) a.ksplit_limit = 0;   // counting mode = one walk per ray, so the counts are those of a plain closest-hit walk
    for (int i = 0; i < 3; i++) { a.scene_lo[i] = c->scene_lo[i]; a.scene_hi[i] = c->scene_hi[i]; }
    a.trace_blocks = P.trace_blocks; a.trace_blocks_wide = P.trace_blocks_wide;
    a.wide_from = c->knobs.wide_from ? c->knobs.wide_from : mcrt::lane_wide_from();
    a.march_blocks = c->knobs.march_blocks;
    a.want_segs = out >= 2 ? 1u : 0u;
    a.frame = frame; a.seed = c->p.seed; a.start_mat = c->start_mat; a.tex_n = c->tex_n; a.tex_mask = (c->tex_n & (c->tex_n - 1u)) == 0u ? c->tex_n - 1u : 0u;
    a.sanitize = c->p.sanitize_tir; a.tex_finite = c->tex_finite ? 1u : 0u;
    a.freq = c->p.frequency; a.eps = c->p.intensity_epsilon; a.I0 = c->p.initial_intensity; a.offs = c->p.ray_start_offset;
    a.sx = c->spacing[0]; a.sy = c->spacing[1]; a.sz = c->spacing[2]; a.tex_res = c->p.tex_res; a.axial_res_f = c->c.axial_res_f; a.pad_abs = c->bvh.pad_abs; a.tex_rcp = 1.0f / c->p.tex_res; a.fast_div = c->fast_div ? 1u : 0u;
    // k_march's branch-free texture lookup: power-of-two texture, verified division, |x / res| < 2^31
    a.tex_shift = 0; while ((1u << a.tex_shift) < c->tex_n) a.tex_shift++;
    a.lean_bound = 0.0f;
    if (c->fast_div_all && a.tex_mask && a.tex_shift <= 10u) {
        const float lim = 2147483648.0f * c->p.tex_res * (1.0f - 0x1p-20f);
        a.lean_bound = lim < 1e18f ? lim : 1e18f;
        if (!(a.lean_bound > 0.0f)) a.lean_bound = 0.0f;
    }
    a.axial_res_mm = c->c.axial_res_mm; a.time_step = c->c.time_step_us; a.row_dt = c->c.row_dt_us;
    a.max_travel = c->c.max_travel_us; a.sos_d = (double)c->p.speed_of_sound; a.inv_row_dt = 1.0 / c->c.row_dt_us;
    // k_march's fast variant: the reference's 256^3 texture with the branch-free cell, and an LDS image long enough for the row
    // guess of every valid step -- t < max_travel, and rounding is monotone, so (int)(t * inv_row_dt) <= (int)(max_travel * inv_row_dt)
    a.march_rows = 0u;
    {
        const double g = a.max_travel * a.inv_row_dt;
        if (a.lean_bound > 0.0f && c->tex_n == 256u && g >= 0.0 && g < (double)(MCRT_MAX_ROWS + 1)) {
            const uint32_t gmax = (uint32_t)g;
            a.march_rows = (gmax + 2u > c->p.n_rows + 1u) ? gmax + 2u : c->p.n_rows + 1u;
        }
    }
    c->last_lean_bound = a.lean_bound; c->last_march_rows = a.march_rows;
    // Work the image does not need, left out where only the image is asked for: a counting pass and the hit / segment tables show every path to its end.
    const bool image_only = !c->stats_on && out == 0;
    a.thr_end = c->thr_end;
    a.retire_late = image_only && c->knobs.retire_late ? 1u : 0u;
    // bounce 0 folded into k_shade: the staged form, an RF block to add into, the start material silent by k_march's own test, and a workgroup
    // of k_shade(0) within one queued scan-line
    a.fold_b0 = image_only && c->knobs.fold_b0 && !P.latency && accumulate && c->tex_finite && c->start_silent && c->p.n_samples % 256u == 0u ? 1u : 0u;
}

// group g's own arguments: its scan-lines [b0,b1) of the pass's n_frames frames, its columns of the RF block (which begins at acc_e0), its work set
static void fill_group(const mcrt_ctx *c, const Work &w, mcrt::FrameArgs &a, uint32_t n_frames, uint32_t b0, uint32_t b1, uint32_t acc_e0, int out)
{
    a.stack_ovf = w.stack_ovf; a.segs = w.segs; a.hits = out >= 1 ? (int32_t *)w.hits : nullptr;
    a.st0 = w.b.st0; a.st1 = w.b.st1; a.st2 = w.b.st2; a.queue = w.b.q; a.key0 = w.b.key0; a.key1 = w.b.key1;
    a.counts = w.b.counts; a.cursors = w.b.cursors; a.mrec = w.b.mrec; a.seg_count = w.b.seg_count;
    a.acc_off = b0 - acc_e0;
    a.e_begin = b0; a.ne_frame = b1 - b0; a.ne = (b1 - b0) * n_frames;   // n_frames consecutive frame ids traced as one pass
    a.packet_mask = (c->stats_on || (uint64_t)a.ne * a.S < c->knobs.packet_from) ? 0u : c->knobs.packet_mask;   // bounces walked a wavefront per ray packet (k_trace_packet); the counting build walks ray by ray
}

// The walk kernels (k_trace_lane*, k_path) index their traversal-stack overflow with stride gridDim.x * 256 and check no bound: the
// largest grid a group's walks can take must fit its work set, or nothing is launched
static int check_overflow(const mcrt_ctx *c, const Plan &P, const mcrt::FrameArgs &a, const Work &w)
{
    const uint32_t lds_part = mcrt::lane_stack_entries();
    if (c->bvh4.max_stack <= lds_part) return MCRT_OK;
    const uint32_t blocks = P.latency ? mcrt::path_blocks((size_t)a.ne * a.S) : std::max(a.trace_blocks, a.trace_blocks_wide);
    const size_t need = (size_t)(c->bvh4.max_stack - lds_part) * blocks * 256;
    if (need > w.stack_ovf.cap) return set_error(MCRT_ERR_LIMIT, "traversal-stack overflow: %zu entries needed, the work set holds %zu", need, w.stack_ovf.cap);
    return MCRT_OK;
}

// one launch on stream st; when its kind is timed (0: the walk, 1: k_shade, 2: k_march -- see mcrt_enable_timing) bracketed by HIP events on st
template <class Launch> static int timed_launch(mcrt_ctx *c, int kind, hipStream_t st, Launch launch)
{
    if (!c->timing_on || (kind != 0 && c->timing_level < 2)) { HIP_TRY(launch()); return MCRT_OK; }
    if (c->ev_used == c->ev.size()) {
        if (c->ev.size() >= 65536) return set_error(MCRT_ERR_LIMIT, "timing buffer full: call mcrt_get_kernel_time(reset=1)");
        TimedLaunch t;
        HIP_TRY(hipEventCreate(&t.start.h)); HIP_TRY(hipEventCreate(&t.end.h));
        c->ev.push_back(std::move(t));
    }
    TimedLaunch &t = c->ev[c->ev_used];
    HIP_TRY(hipEventRecord(t.start, st));
    HIP_TRY(launch());
    HIP_TRY(hipEventRecord(t.end, st));
    t.kind = kind; c->ev_used++;
    return MCRT_OK;
}

// one bounce of one group of a staged pass: the walk + k_shade on the group's stream, k_march of the finished segments on its side stream.
// (Round 4 tried holding k_march of bounce b back until the walk of bounce b+1 had claimed its last ray -- a device word raised by the walk, waited
//  for with hipStreamWaitValue32, which the command processor releases ~1 us after the store --: 0.360 against 0.343 ms per frame at 128 frames in
//  flight, 0.414 against 0.405 on the driver's pass, and a hang under `rocprofv3 --pmc`.  Removed; DESIGN.md A.6, profiles/round4/exp_round4_kernels.txt.)
static int run_bounce(mcrt_ctx *c, Work &w, hipStream_t st, const mcrt::FrameArgs &a, uint32_t b, uint32_t sides, bool accumulate, bool overlap)
{
    MCRT_TRY(timed_launch(c, 0, st, [&] { return mcrt::launch_trace(a, b, c->stats_on, st); }));
    MCRT_TRY(timed_launch(c, 1, st, [&] { return mcrt::launch_shade(a, b, c->stats_on, st); }));
    if (!accumulate || (a.fold_b0 && b == 0u)) return MCRT_OK;      // (bounce 0 folded: k_shade has added its echoes; later bounces keep their side streams)
    hipStream_t ms = st;
    if (overlap) {   // the segments of bounce b are final: accumulate them beside the next bounce's walk
        HIP_TRY(hipEventRecord(w.ev_bounce[b], st));
        MCRT_TRY(side_stream(c, w, b % sides, &ms));
        HIP_TRY(hipStreamWaitEvent(ms, w.ev_bounce[b], 0));
    }
    return timed_launch(c, 2, ms, [&] { return mcrt::launch_march(a, b, c->stats_on, ms); });
}

static int enqueue_pass(mcrt_ctx *c, const Plan &P, const mcrt::FrameArgs *args, Work *const *ws, bool accumulate)
{
    const bool overlap = !c->knobs.no_overlap;
    hipStream_t gst[16] = { c->stream };
    for (uint32_t g = 1; g < P.groups; g++) MCRT_TRY(work_stream(*ws[g], &gst[g]));
    if (c->scene_pending && c->scene_stream != c->stream) HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_scene, 0));   // a scene update issued on another stream
    HIP_TRY(hipEventRecord(c->ev_start, c->stream));
    for (uint32_t g = 0; g < P.groups; g++) {
        if (gst[g] != c->stream) HIP_TRY(hipStreamWaitEvent(gst[g], c->ev_start, 0));
        HIP_TRY(mcrt::launch_init(args[g], gst[g]));
    }
    if (P.latency) {
        for (uint32_t g = 0; g < P.groups; g++) {          // (every group's k_path first, then the accumulations: the second group must not wait for the host to enqueue the first's k_march)
            MCRT_TRY(timed_launch(c, 0, gst[g], [&] { return mcrt::launch_path(args[g], gst[g]); }));
        }
        for (uint32_t g = 0; g < P.groups && accumulate; g++) {
            MCRT_TRY(timed_launch(c, 2, gst[g], [&] { return mcrt::launch_march(args[g], mcrt::MCRT_ALL_BOUNCES, false, gst[g]); }));
        }
    } else {
        for (uint32_t b = 0; b < c->p.max_depth; b++)
            for (uint32_t g = 0; g < P.groups; g++) {
                MCRT_TRY(run_bounce(c, *ws[g], gst[g], args[g], b, P.sides[g], accumulate, overlap));
            }
    }
    for (uint32_t g = 0; g < P.groups; g++) {
        for (uint32_t i = 0; i < P.sides[g] && accumulate && overlap; i++) {
            if (!ws[g]->side[i]) continue;
            HIP_TRY(hipEventRecord(ws[g]->ev_join[i], ws[g]->side[i]));
            HIP_TRY(hipStreamWaitEvent(gst[g], ws[g]->ev_join[i], 0));
        }
        if (gst[g] != c->stream) {
            HIP_TRY(hipEventRecord(ws[g]->ev_done, gst[g]));
            HIP_TRY(hipStreamWaitEvent(c->stream, ws[g]->ev_done, 0));
        }
    }
    return MCRT_OK;
}

// scene::cast_rays (scene.cpp:50-183) [+ the accumulation loop] for scan-lines [e0,e1) of n_frames frames, in the form and the
// scan-line groups plan_pass chooses.  Everything is ordered after what is already queued on the context's stream, and the
// context's stream waits for all of it.
static int run_pass(mcrt_ctx *c, uint32_t frame, uint32_t n_frames, uint32_t e0, uint32_t e1, bool accumulate, bool one_group, int out)
{
    const Plan P = plan_pass(c, e0, e1, n_frames, one_group);
    mcrt::FrameArgs pass, args[16];
    Work *ws[16];
    fill_pass(c, P, pass, frame, e1 - e0, accumulate, out);
    for (uint32_t g = 0; g < P.groups; g++) {
        MCRT_TRY(get_work(c, g, &ws[g]));
        MCRT_TRY(ensure_work(*ws[g], (size_t)(P.e[g + 1] - P.e[g]) * n_frames * c->p.n_samples, c->p.max_depth, P.ovf[g], out));
        args[g] = pass;
        fill_group(c, *ws[g], args[g], n_frames, P.e[g], P.e[g + 1], e0, out);
        MCRT_TRY(check_overflow(c, P, args[g], *ws[g]));
    }
    return enqueue_pass(c, P, args, ws, accumulate);
}

// the traced block's accumulators [lines][R] into rf_dev; k_finalize leaves them zeroed (ensure_acc)
static int finalize(mcrt_ctx *c, float *rf_dev, uint32_t lines)
{
    HIP_TRY(mcrt::launch_finalize(c->d_acc, c->d_flags, rf_dev, lines, c->p.n_rows, c->d_error, c->stream));
    c->acc_clean_ne = lines; c->acc_clean_rows = c->p.n_rows;
    return MCRT_OK;
}

extern "C" int mcrt_trace_frames(mcrt_ctx *c, uint32_t frame, uint32_t n_frames, uint32_t e0, uint32_t e1, float *rf_dev)
{
    CTX_TRY(c);
    MCRT_TRY(check_ready(c, e0, e1));
    if (!rf_dev) return set_error(MCRT_ERR_INVALID, "null rf_dev");
    if (n_frames == 0 || n_frames > 1024) return set_error(MCRT_ERR_LIMIT, "n_frames must be 1..1024");
    if ((uint64_t)(e1 - e0) * n_frames * c->p.n_samples > (1ull << 27))        // (~600 bytes of work buffers per path)
        return set_error(MCRT_ERR_LIMIT, "%u frames x %u scan-lines x %u samples: more than 2^27 paths in one pass", n_frames, e1 - e0, c->p.n_samples);
    const uint32_t lines = (e1 - e0) * n_frames;
    MCRT_TRY(ensure_acc(c, lines));
    MCRT_TRY(run_pass(c, frame, n_frames, e0, e1, true, false, 0));
    return finalize(c, rf_dev, lines);
}

extern "C" int mcrt_trace_frame(mcrt_ctx *c, uint32_t frame, uint32_t e0, uint32_t e1, float *rf_dev)
{
    return mcrt_trace_frames(c, frame, 1, e0, e1, rf_dev);
}

// A pass whose frames each have their own probe pose (transducer.h:82-118 update() between the frames of main.cpp:92-152): the element
// tables [n_frames][E][3] are staged in the context (host pointers are copied on the stream) and k_init reads frame f's rows.
extern "C" int mcrt_trace_frames_poses(mcrt_ctx *c, uint32_t frame, uint32_t n_frames, uint32_t e0, uint32_t e1,
                                       const float *pos, const float *dir, float *rf_dev)
{
    CTX_TRY(c);
    if (!pos || !dir) return set_error(MCRT_ERR_INVALID, "mcrt_trace_frames_poses: null pose tables");
    if (n_frames == 0 || n_frames > 1024) return set_error(MCRT_ERR_LIMIT, "n_frames must be 1..1024");
    const uint32_t E = c->p.n_elements;
    const size_t bytes = 12 * (size_t)n_frames * E;
    const float *src[2] = { pos, dir };
    const float *dev[2] = { nullptr, nullptr };
    // A table in HOST memory belongs to the caller and may be pageable: it is copied into pinned memory the context owns before this
    // call returns (the caller may free or rewrite it at once), and goes to the device from there on the stream.  The staging buffers are
    // reused: the copy of the previous call (an early node of the previous pass, not the pass) is waited for first.
    bool staged = false;
    for (int k = 0; k < 2; k++) {
        if (is_device_pointer(src[k])) { dev[k] = src[k]; continue; }
        if (c->pose_copy_pending) { HIP_TRY(hipEventSynchronize(c->ev_pose)); c->pose_copy_pending = false; }
        if (c->d_pose[k].cap < bytes / 4 || c->h_pose[k].cap < bytes / 4) {
            HIP_TRY(hipStreamSynchronize(c->stream));
            HIP_TRY(c->d_pose[k].grow(bytes / 4)); HIP_TRY(c->h_pose[k].grow(bytes / 4));
        }
        memcpy(c->h_pose[k], src[k], bytes);
        HIP_TRY(hipMemcpyAsync(c->d_pose[k], c->h_pose[k], bytes, hipMemcpyHostToDevice, c->stream));
        dev[k] = c->d_pose[k]; staged = true;
    }
    if (staged) {
        HIP_TRY(ensure_event(c->ev_pose));
        HIP_TRY(hipEventRecord(c->ev_pose, c->stream));
        c->pose_copy_pending = true;
    }
    c->pose_pos = dev[0]; c->pose_dir = dev[1];
    const int rc = mcrt_trace_frames(c, frame, n_frames, e0, e1, rf_dev);
    c->pose_pos = c->pose_dir = nullptr;
    return rc;
}

// copies the per-path tables (work set 0) to the host: segs [ne][S][B], seg_count [ne][S], hits [ne][S][B] (= segment.tri, -2 beyond the path's end)
static int copy_out(mcrt_ctx *c, uint32_t ne, int32_t *hits, mcrt_segment *segs, uint32_t *seg_count)
{
    const size_t np = (size_t)ne * c->p.n_samples, B = c->p.max_depth;
    const Work &w = c->work[0];
    HIP_TRY(hipStreamSynchronize(c->stream));
    MCRT_TRY(check_device_error(c));
    std::vector<uint32_t> cnt;
    if (!seg_count && (hits || segs)) { cnt.resize(np); seg_count = cnt.data(); }
    if (seg_count) HIP_TRY(hipMemcpy(seg_count, w.b.seg_count, np * 4, hipMemcpyDeviceToHost));
    if (segs) {
        HIP_TRY(hipMemcpy(segs, w.segs, np * B * sizeof(mcrt_segment), hipMemcpyDeviceToHost));
        for (size_t p = 0; p < np; p++)                         // slots beyond a path's end are unspecified on the device
            for (size_t b = seg_count[p]; b < B; b++) memset(&segs[p * B + b], 0, sizeof(mcrt_segment));
    }
    if (hits) {
        HIP_TRY(hipMemcpy(hits, w.hits, np * B * 4, hipMemcpyDeviceToHost));
        for (size_t p = 0; p < np; p++)
            for (size_t b = seg_count[p]; b < B; b++) hits[p * B + b] = -2;
    }
    return MCRT_OK;
}

extern "C" int mcrt_trace_frame_debug(mcrt_ctx *c, uint32_t frame, uint32_t e0, uint32_t e1, float *rf_dev,
                                      int32_t *hits, mcrt_segment *segs, uint32_t *seg_count)
{
    CTX_TRY(c);
    MCRT_TRY(check_ready(c, e0, e1));
    if (!rf_dev) return set_error(MCRT_ERR_INVALID, "null rf_dev");
    MCRT_TRY(ensure_acc(c, e1 - e0));
    MCRT_TRY(run_pass(c, frame, 1, e0, e1, true, true, segs ? 2 : 1));   // one group: the per-path tables are contiguous
    MCRT_TRY(finalize(c, rf_dev, e1 - e0));
    return copy_out(c, e1 - e0, hits, segs, seg_count);
}

extern "C" int mcrt_cast_rays(mcrt_ctx *c, uint32_t frame, uint32_t e0, uint32_t e1, mcrt_segment *segs, uint32_t *seg_count, int32_t *hits)
{
    CTX_TRY(c);
    MCRT_TRY(check_ready(c, e0, e1));
    MCRT_TRY(run_pass(c, frame, 1, e0, e1, false, true, segs ? 2 : 1));
    return copy_out(c, e1 - e0, hits, segs, seg_count);
}

static bool ranges_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes)
{
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + a_bytes, b0 = (uintptr_t)b, b1 = b0 + b_bytes;
    return a0 < b1 && b0 < a1;
}

static int ensure_tmp(mcrt_ctx *c, size_t n)
{
    if (n > c->d_tmp.cap) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(c->d_tmp.alloc(n));
    }
    return MCRT_OK;
}

extern "C" int mcrt_convolve_frames(mcrt_ctx *c, float *rf_dev, uint32_t n_frames, uint32_t E, uint32_t R, const float *ax, uint32_t n_ax, const float *lat, uint32_t n_lat)
{
    CTX_TRY(c);
    if (!rf_dev || !ax || !lat || E == 0 || R == 0 || n_frames == 0) return set_error(MCRT_ERR_INVALID, "mcrt_convolve: bad arguments");
    if (n_ax == 0 || n_ax > 16 || n_lat == 0 || n_lat > 32) return set_error(MCRT_ERR_LIMIT, "kernel sizes must be 1..16 axial, 1..32 lateral");
    MCRT_TRY(ensure_tmp(c, (size_t)n_frames * E * R));
    mcrt::ConvTaps t; memset(&t, 0, sizeof t);
    memcpy(t.ax, ax, 4 * n_ax); memcpy(t.lat, lat, 4 * n_lat); t.n_ax = n_ax; t.n_lat = n_lat;
    HIP_TRY(mcrt::launch_convolve(rf_dev, c->d_tmp, n_frames, E, R, t, c->stream));
    return MCRT_OK;
}

extern "C" int mcrt_convolve(mcrt_ctx *c, float *rf_dev, uint32_t E, uint32_t R, const float *ax, uint32_t n_ax, const float *lat, uint32_t n_lat)
{
    return mcrt_convolve_frames(c, rf_dev, 1, E, R, ax, n_ax, lat, n_lat);
}

// The contract is in include/mcrt.h.  Everything is checked before anything is launched; the caller's table [R][n_lat] goes to the device
// tap-major [n_lat][R] (StagedTable).
extern "C" int mcrt_convolve_frames_depth(mcrt_ctx *c, float *rf_dev, uint32_t n_frames, uint32_t E, uint32_t R, const float *ax, uint32_t n_ax,
                                          const float *lat_rows, uint32_t n_lat)
{
    CTX_TRY(c);
    if (!rf_dev || !ax || !lat_rows || E == 0 || R == 0 || n_frames == 0) return set_error(MCRT_ERR_INVALID, "mcrt_convolve_frames_depth: bad arguments");
    if (n_ax == 0 || n_ax > 16 || n_lat == 0 || n_lat > 32) return set_error(MCRT_ERR_LIMIT, "kernel sizes must be 1..16 axial, 1..32 lateral");
    if (R > MCRT_MAX_ROWS) return set_error(MCRT_ERR_LIMIT, "mcrt_convolve_frames_depth: at most %d rows", MCRT_MAX_ROWS);
    MCRT_TRY(ensure_tmp(c, (size_t)n_frames * E * R));
    MCRT_TRY(c->lat_rows.put(lat_rows, R, n_lat, (size_t)MCRT_MAX_ROWS * 32, c->stream));
    mcrt::ConvTaps t; memset(&t, 0, sizeof t);
    memcpy(t.ax, ax, 4 * n_ax); t.n_ax = n_ax; t.n_lat = n_lat;
    HIP_TRY(mcrt::launch_convolve_depth(rf_dev, c->d_tmp, n_frames, E, R, t, c->lat_rows.dev, c->stream));
    return MCRT_OK;
}

// The contract is in include/mcrt.h.  Everything is checked before anything is launched; the caller's weights [R][K] go to the device
// tap-major [K][R] (StagedTable).
extern "C" int mcrt_elevation_frames(mcrt_ctx *c, const float *planes_dev, uint32_t n_frames, uint32_t K, uint32_t E, uint32_t R,
                                     const float *w_rows, float *rf_dev)
{
    CTX_TRY(c);
    if (!planes_dev || !rf_dev || !w_rows || n_frames == 0 || K == 0 || E == 0 || R == 0) return set_error(MCRT_ERR_INVALID, "mcrt_elevation_frames: bad arguments");
    if (K > 32) return set_error(MCRT_ERR_LIMIT, "mcrt_elevation_frames: at most 32 planes (%u)", K);
    if (R > MCRT_MAX_ROWS) return set_error(MCRT_ERR_LIMIT, "mcrt_elevation_frames: at most %d rows", MCRT_MAX_ROWS);
    if ((double)n_frames * (double)K * (double)E * (double)R >= 0x1p40) return set_error(MCRT_ERR_LIMIT, "mcrt_elevation_frames: the plane stack is too large");
    if (ranges_overlap(planes_dev, 4 * (size_t)n_frames * K * E * R, rf_dev, 4 * (size_t)n_frames * E * R)) return set_error(MCRT_ERR_INVALID, "mcrt_elevation_frames: planes_dev and rf_dev overlap");
    MCRT_TRY(c->elev_rows.put(w_rows, R, K, (size_t)MCRT_MAX_ROWS * 32, c->stream));
    HIP_TRY(mcrt::launch_elevation(planes_dev, rf_dev, n_frames, K, E, R, c->elev_rows.dev, c->stream));
    return MCRT_OK;
}

extern "C" int mcrt_envelope_frames(mcrt_ctx *c, float *rf_dev, uint32_t n_frames, uint32_t E, uint32_t R)
{
    CTX_TRY(c);
    if (!rf_dev || E == 0 || R == 0 || n_frames == 0) return set_error(MCRT_ERR_INVALID, "mcrt_envelope: bad arguments");
    if ((uint64_t)n_frames * E > 0x7fffffffull) return set_error(MCRT_ERR_LIMIT, "mcrt_envelope: too many scan-lines");
    if (R > MCRT_MAX_ROWS) return set_error(MCRT_ERR_LIMIT, "mcrt_envelope: at most %d rows", MCRT_MAX_ROWS);
    HIP_TRY(mcrt::launch_envelope(rf_dev, n_frames * E, R, c->stream));      // the scan-lines of all images are independent columns
    return MCRT_OK;
}

extern "C" int mcrt_envelope(mcrt_ctx *c, float *rf_dev, uint32_t E, uint32_t R)
{
    return mcrt_envelope_frames(c, rf_dev, 1, E, R);
}

// the scan-conversion maps of a geometry on the device, in cache m: the plain maps (cp null: mcrt_scan_maps, one view) or the N views of a steer
// list (mcrt_compound_maps).  Made on the host and uploaded when the geometry changes, reused as they are otherwise.  Every part of the key is
// compared bit for bit on its own (a key folded into one double, radius_mm * 1e6 + total_angle, made (30 mm, 1 rad) and (29.999999 mm, 2 rad)
// the same geometry)
static int ensure_maps(mcrt_ctx *c, MapCache &m, uint32_t E, uint32_t R, double radius_mm, double total_angle, uint32_t orows, uint32_t ocols, const mcrt_compound *cp = nullptr)
{
    const uint32_t N = cp ? cp->n_views : 1u;
    const uint32_t key[7] = { E, R, orows, ocols, c->p.speed_of_sound, 1u, N };
    const double keyd[3] = { radius_mm, total_angle, c->c.max_travel_us };
    uint32_t steer[16] = {};
    if (cp) memcpy(steer, cp->steer_rad, 4 * (size_t)N);
    if (!memcmp(key, m.key, sizeof key) && !memcmp(keyd, m.keyd, sizeof keyd) && !memcmp(steer, m.steer, sizeof steer)) return MCRT_OK;
    const size_t n = (size_t)orows * ocols, n_pad = MapCache::pad(n);
    std::vector<float> maps(2 * (size_t)N * n_pad, 0.0f), mr(n), mc(n);
    // (the rf_image template parameter is max_travel_time.to<unsigned int>(), main.cpp:36 -- the same truncation as max_rows uses)
    const uint32_t travel = (uint32_t)c->c.max_travel_us, sos = c->p.speed_of_sound;
    for (uint32_t v = 0; v < N; v++) {
        MCRT_TRY(cp ? mcrt_compound_maps(E, R, radius_mm, total_angle, travel, sos, orows, ocols, cp->steer_rad[v], mr.data(), mc.data())
                    : mcrt_scan_maps(E, R, radius_mm, total_angle, travel, sos, orows, ocols, mr.data(), mc.data()));
        memcpy(&maps[(size_t)(2u * v) * n_pad], mc.data(), 4 * n);
        memcpy(&maps[(size_t)(2u * v + 1u) * n_pad], mr.data(), 4 * n);
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    memset(m.key, 0, sizeof key);                       // (no geometry until the maps are on the device)
    HIP_TRY(m.d.grow(maps.size()));
    HIP_TRY(hipMemcpy(m.d, maps.data(), maps.size() * 4, hipMemcpyHostToDevice));
    memcpy(m.key, key, sizeof key); memcpy(m.keyd, keyd, sizeof keyd); memcpy(m.steer, steer, sizeof steer);
    return MCRT_OK;
}

extern "C" int mcrt_scan_convert_frames(mcrt_ctx *c, const float *rf_dev, uint32_t n_frames, uint32_t E, uint32_t R, double radius_mm, double total_angle,
                                        float *out_dev, uint32_t orows, uint32_t ocols)
{
    CTX_TRY(c);
    if (!rf_dev || !out_dev || E == 0 || R == 0 || orows == 0 || ocols == 0 || n_frames == 0) return set_error(MCRT_ERR_INVALID, "mcrt_scan_convert: bad arguments");
    if (n_frames > 65535u) return set_error(MCRT_ERR_LIMIT, "mcrt_scan_convert: at most 65535 images per call");
    MCRT_TRY(ensure_maps(c, c->maps, E, R, radius_mm, total_angle, orows, ocols));
    HIP_TRY(mcrt::launch_remap(rf_dev, n_frames, E, R, c->maps.d, c->maps.d + MapCache::pad((size_t)orows * ocols), out_dev, orows * ocols, c->stream));
    return MCRT_OK;
}

extern "C" int mcrt_scan_convert(mcrt_ctx *c, const float *rf_dev, uint32_t E, uint32_t R, double radius_mm, double total_angle,
                                 float *out_dev, uint32_t orows, uint32_t ocols)
{
    return mcrt_scan_convert_frames(c, rf_dev, 1, E, R, radius_mm, total_angle, out_dev, orows, ocols);
}

extern "C" int mcrt_default_bmode(mcrt_bmode_params *p)
{
    if (!p) return set_error(MCRT_ERR_INVALID, "null params");
    memset(p, 0, sizeof *p);
    p->mode = MCRT_BMODE_DB; p->dynamic_range_db = 60.0f; p->gain_db = 0.0f; p->ref = 0.0f; p->persistence = 0.0f; p->reset_state = 1u;
    p->out_rows = 400u; p->out_cols = 500u; p->radius_mm = 30.0; p->total_angle_rad = 1.0471975511965976;
    return MCRT_OK;
}

// what mcrt_bmode_frames and mcrt_bmode_compound_frames check alike (fn: the caller's name, for the message); k receives the TGC factors
static int bmode_check(const char *fn, const float *rf_dev, const void *out_dev, uint32_t n_frames, uint32_t E, uint32_t R, const mcrt_bmode_params *p,
                       const float *tgc_db, std::vector<float> &k)
{
    if (!p) return set_error(MCRT_ERR_INVALID, "%s: null params", fn);
    if (!rf_dev || !out_dev) return set_error(MCRT_ERR_INVALID, "%s: null %s", fn, rf_dev ? "out_dev" : "rf_dev");
    if (E == 0 || R == 0 || n_frames == 0 || p->out_rows == 0 || p->out_cols == 0) return set_error(MCRT_ERR_INVALID, "%s: zero sizes", fn);
    if (R > MCRT_MAX_ROWS) return set_error(MCRT_ERR_LIMIT, "%s: at most %d rows", fn, MCRT_MAX_ROWS);
    if (n_frames > 65535u) return set_error(MCRT_ERR_LIMIT, "%s: at most 65535 frames per call", fn);
    if ((uint64_t)p->out_rows * p->out_cols > 0x7ffffffcull) return set_error(MCRT_ERR_LIMIT, "%s: output image too large", fn);
    if (p->mode != MCRT_BMODE_DB && p->mode != MCRT_BMODE_REF_LOG) return set_error(MCRT_ERR_INVALID, "%s: unknown mode %u", fn, p->mode);
    if (!(std::isfinite(p->dynamic_range_db) && p->dynamic_range_db > 0.0f))
        return set_error(MCRT_ERR_INVALID, "%s: dynamic_range_db must be finite and > 0 (%g)", fn, (double)p->dynamic_range_db);
    if (!std::isfinite(p->gain_db)) return set_error(MCRT_ERR_INVALID, "%s: gain_db must be finite", fn);
    if (!std::isfinite(p->ref)) return set_error(MCRT_ERR_INVALID, "%s: ref must be finite", fn);
    if (!(p->persistence >= 0.0f && p->persistence < 1.0f)) return set_error(MCRT_ERR_INVALID, "%s: persistence must be in [0,1) (%g)", fn, (double)p->persistence);
    if (tgc_db) {
        k.resize(R);
        for (uint32_t r = 0; r < R; r++) {
            if (!std::isfinite(tgc_db[r])) return set_error(MCRT_ERR_INVALID, "%s: tgc_db[%u] is not finite", fn, r);
            k[r] = (float)std::pow(10.0, (double)tgc_db[r] / 20.0);
        }
    }
    return MCRT_OK;
}

// steps 1-3 of mcrt_bmode_frames on the context's stream, over n_frames images of `lines` scan-lines each (the N views of a compounded frame
// are one image of N * E scan-lines): the TGC factors (only when they differ from the ones on the device), with the automatic reference
// the peaks (memset + k_bmode_peak), the grey level of every RF tap (k_bmode_grey, into the context's scratch)
static int bmode_grey_pass(mcrt_ctx *c, const float *rf_dev, uint32_t n_frames, uint32_t lines, uint32_t R, const mcrt_bmode_params *p, const float *tgc_db,
                           const std::vector<float> &k, float *peak_dev)
{
    if (!c->d_disp) HIP_TRY(c->d_disp.alloc(65536));   // (the peaks of the largest pass: 65535 frames)
    if (tgc_db) MCRT_TRY(c->tgc.put(k.data(), R, 1, MCRT_MAX_ROWS, c->stream));
    const size_t taps = (size_t)n_frames * lines * R;
    MCRT_TRY(ensure_tmp(c, taps));     // the grey levels of the pass (the scratch mcrt_convolve uses too)
    const float *tgc = tgc_db ? c->tgc.dev.p : nullptr;
    if (p->ref > 0.0f) HIP_TRY(mcrt::launch_bmode_grey(rf_dev, n_frames, lines, R, tgc, nullptr, p->ref, peak_dev, p->mode, p->gain_db, p->dynamic_range_db, c->d_tmp, c->stream));
    else {
        float *peak = peak_dev ? peak_dev : c->d_disp.p;
        HIP_TRY(hipMemsetAsync(peak, 0, 4 * (size_t)n_frames, c->stream));
        HIP_TRY(mcrt::launch_bmode_peak(rf_dev, n_frames, lines, R, tgc, peak, c->stream));
        HIP_TRY(mcrt::launch_bmode_grey(rf_dev, n_frames, lines, R, tgc, peak, 0.0f, nullptr, p->mode, p->gain_db, p->dynamic_range_db, c->d_tmp, c->stream));
    }
    return MCRT_OK;
}

// without persistence the frames are independent: they are cut into chunks (grid.y) so that a pass has about 16384 wavefronts (the
// lanes wait for their gathers; at 400 x 500 a chunk is one frame)
static uint32_t display_frames_per_chunk(uint32_t n_frames, uint32_t n, float alpha)
{
    if (alpha != 0.0f) return n_frames;
    const uint32_t waves = (n + 255u) / 256u, chunks = std::max(1u, std::min(n_frames, (16384u + waves - 1u) / waves));
    return (n_frames + chunks - 1u) / chunks;
}

// The contract is in include/mcrt.h.  Everything is checked before anything is launched; then, on the context's stream: the TGC factors
// (only when they differ from the ones on the device), with the automatic reference the peaks (memset + k_bmode_peak), the grey level of
// every RF tap (k_bmode_grey, into the context's scratch) and their scan conversion, persistence and quantisation (k_bmode).
extern "C" int mcrt_bmode_frames(mcrt_ctx *c, const float *rf_dev, uint32_t n_frames, uint32_t E, uint32_t R, const mcrt_bmode_params *p,
                                 const float *tgc_db, float *state_dev, float *peak_dev, uint8_t *out_dev)
{
    CTX_TRY(c);
    std::vector<float> k;
    MCRT_TRY(bmode_check("mcrt_bmode_frames", rf_dev, out_dev, n_frames, E, R, p, tgc_db, k));
    MCRT_TRY(ensure_maps(c, c->maps, E, R, p->radius_mm, p->total_angle_rad, p->out_rows, p->out_cols));
    MCRT_TRY(bmode_grey_pass(c, rf_dev, n_frames, E, R, p, tgc_db, k, peak_dev));
    mcrt::BmodeArgs a;
    a.grey = c->d_tmp; a.map_col = c->maps.d; a.map_row = c->maps.d + MapCache::pad((size_t)p->out_rows * p->out_cols); a.state = state_dev; a.out = out_dev; a.alpha = p->persistence;
    a.E = E; a.R = R; a.n = p->out_rows * p->out_cols; a.F = n_frames; a.reset = p->reset_state ? 1u : 0u;
    a.frames_per_chunk = display_frames_per_chunk(n_frames, a.n, a.alpha);
    HIP_TRY(mcrt::launch_bmode(a, c->stream));
    return MCRT_OK;
}

// ---- spatial compounding (the contracts are in include/mcrt.h) ----
static int compound_check(const char *fn, const mcrt_compound *cp, uint32_t n_frames)
{
    if (!cp) return set_error(MCRT_ERR_INVALID, "%s: null mcrt_compound", fn);
    if (cp->n_views == 0 || cp->n_views > 16) return set_error(MCRT_ERR_INVALID, "%s: n_views must be 1..16 (%u)", fn, cp->n_views);
    for (uint32_t n = 0; n < cp->n_views; n++)
        if (!(std::isfinite(cp->steer_rad[n]) && std::fabs((double)cp->steer_rad[n]) < 1.57079632679489661923))
            return set_error(MCRT_ERR_INVALID, "%s: steer_rad[%u] must be finite and |steer| < pi/2 (%g)", fn, n, (double)cp->steer_rad[n]);
    if ((uint64_t)n_frames * cp->n_views > 65535ull) return set_error(MCRT_ERR_LIMIT, "%s: at most 65535 views per call (%u frames x %u)", fn, n_frames, cp->n_views);
    return MCRT_OK;
}

// the options of the two *_opts calls, checked alike (null: the defaults), turned into the kernel's mode and weights.  Defaults -- the mean,
// no feathering, every weight of the first n_views 1.0f -- are COMPOUND_PLAIN: the kernel mcrt_compound_frames has always run
static int compound_opts_check(const char *fn, const mcrt_compound_opts *o, uint32_t N, mcrt::CompoundArgs &a)
{
    a.mode = mcrt::COMPOUND_PLAIN; a.feather = 0.0f;
    for (float &w : a.weight) w = 1.0f;
    if (!o) return MCRT_OK;
    if (o->mode != MCRT_COMPOUND_MEAN && o->mode != MCRT_COMPOUND_MAX && o->mode != MCRT_COMPOUND_MEDIAN) return set_error(MCRT_ERR_INVALID, "%s: unknown mode %u", fn, o->mode);
    if (!(std::isfinite(o->feather_lines) && o->feather_lines >= 0.0f)) return set_error(MCRT_ERR_INVALID, "%s: feather_lines must be finite and >= 0 (%g)", fn, (double)o->feather_lines);
    bool ones = true, any = false;
    for (uint32_t n = 0; n < N; n++) {
        const float w = o->view_weight[n];
        if (!(std::isfinite(w) && w >= 0.0f)) return set_error(MCRT_ERR_INVALID, "%s: view_weight[%u] must be finite and >= 0 (%g)", fn, n, (double)w);
        ones = ones && w == 1.0f; any = any || w > 0.0f;
    }
    if (!any) return set_error(MCRT_ERR_INVALID, "%s: view_weight: every one of the %u views has weight 0", fn, N);
    if (o->mode == MCRT_COMPOUND_MEAN && o->feather_lines == 0.0f && ones) return MCRT_OK;
    a.mode = o->mode == MCRT_COMPOUND_MAX ? mcrt::COMPOUND_MAX : o->mode == MCRT_COMPOUND_MEDIAN ? mcrt::COMPOUND_MEDIAN : mcrt::COMPOUND_WEIGHTED;
    a.feather = o->feather_lines;
    for (uint32_t n = 0; n < N; n++) a.weight[n] = o->view_weight[n];
    return MCRT_OK;
}

extern "C" int mcrt_default_compound_opts(mcrt_compound_opts *o)
{
    if (!o) return set_error(MCRT_ERR_INVALID, "mcrt_default_compound_opts: null options");
    o->mode = MCRT_COMPOUND_MEAN; o->feather_lines = 0.0f;
    for (float &w : o->view_weight) w = 1.0f;
    return MCRT_OK;
}

extern "C" int mcrt_compound_frames_opts(mcrt_ctx *c, const float *rf_dev, uint32_t n_frames, uint32_t E, uint32_t R, double radius_mm, double total_angle,
                                         const mcrt_compound *cp, float *out_dev, uint32_t orows, uint32_t ocols, const mcrt_compound_opts *o)
{
    CTX_TRY(c);
    static const char fn[] = "mcrt_compound_frames";
    if (!rf_dev || !out_dev || E == 0 || R == 0 || orows == 0 || ocols == 0 || n_frames == 0) return set_error(MCRT_ERR_INVALID, "%s: bad arguments", fn);
    if (!(total_angle > 0.0)) return set_error(MCRT_ERR_INVALID, "%s: total_angle_rad must be > 0", fn);
    MCRT_TRY(compound_check(fn, cp, n_frames));
    if (R > MCRT_MAX_ROWS) return set_error(MCRT_ERR_LIMIT, "%s: at most %d rows", fn, MCRT_MAX_ROWS);
    if ((uint64_t)orows * ocols > 0x7ffffffcull) return set_error(MCRT_ERR_LIMIT, "%s: output image too large", fn);
    const uint32_t N = cp->n_views, n = orows * ocols;
    if (ranges_overlap(rf_dev, 4 * (size_t)n_frames * N * E * R, out_dev, 4 * (size_t)n_frames * n)) return set_error(MCRT_ERR_INVALID, "%s: rf_dev and out_dev overlap", fn);
    mcrt::CompoundArgs a;
    MCRT_TRY(compound_opts_check(fn, o, N, a));
    MCRT_TRY(ensure_maps(c, c->cmaps, E, R, radius_mm, total_angle, orows, ocols, cp));
    a.src = rf_dev; a.maps = c->cmaps.d; a.state = nullptr; a.out = out_dev; a.alpha = 0.0f;
    a.E = E; a.R = R; a.n = n; a.n_pad = (uint32_t)MapCache::pad(n); a.F = n_frames; a.N = N; a.reset = 1u;
    a.frames_per_chunk = display_frames_per_chunk(n_frames, n, 0.0f);
    HIP_TRY(mcrt::launch_compound(a, false, c->stream));
    return MCRT_OK;
}

extern "C" int mcrt_compound_frames(mcrt_ctx *c, const float *rf_dev, uint32_t n_frames, uint32_t E, uint32_t R, double radius_mm, double total_angle,
                                    const mcrt_compound *cp, float *out_dev, uint32_t orows, uint32_t ocols)
{
    return mcrt_compound_frames_opts(c, rf_dev, n_frames, E, R, radius_mm, total_angle, cp, out_dev, orows, ocols, nullptr);
}

extern "C" int mcrt_bmode_compound_frames_opts(mcrt_ctx *c, const float *rf_dev, uint32_t n_frames, uint32_t E, uint32_t R, const mcrt_bmode_params *p,
                                               const mcrt_compound *cp, const float *tgc_db, float *state_dev, float *peak_dev, uint8_t *out_dev,
                                               const mcrt_compound_opts *o)
{
    CTX_TRY(c);
    static const char fn[] = "mcrt_bmode_compound_frames";
    std::vector<float> k;
    MCRT_TRY(bmode_check(fn, rf_dev, out_dev, n_frames, E, R, p, tgc_db, k));
    if (!(p->total_angle_rad > 0.0)) return set_error(MCRT_ERR_INVALID, "%s: total_angle_rad must be > 0", fn);
    MCRT_TRY(compound_check(fn, cp, n_frames));
    const uint32_t N = cp->n_views, n = p->out_rows * p->out_cols;
    if ((uint64_t)N * E > 0xffffffffull) return set_error(MCRT_ERR_LIMIT, "%s: too many scan-lines (%u views x %u)", fn, N, E);   // (a frame is N * E scan-lines to steps 1-3)
    if (ranges_overlap(rf_dev, 4 * (size_t)n_frames * N * E * R, out_dev, (size_t)n_frames * n)) return set_error(MCRT_ERR_INVALID, "%s: rf_dev and out_dev overlap", fn);
    mcrt::CompoundArgs a;
    MCRT_TRY(compound_opts_check(fn, o, N, a));
    MCRT_TRY(ensure_maps(c, c->cmaps, E, R, p->radius_mm, p->total_angle_rad, p->out_rows, p->out_cols, cp));
    MCRT_TRY(bmode_grey_pass(c, rf_dev, n_frames, N * E, R, p, tgc_db, k, peak_dev));
    a.src = c->d_tmp; a.maps = c->cmaps.d; a.state = state_dev; a.out = out_dev; a.alpha = p->persistence;
    a.E = E; a.R = R; a.n = n; a.n_pad = (uint32_t)MapCache::pad(n); a.F = n_frames; a.N = N; a.reset = p->reset_state ? 1u : 0u;
    a.frames_per_chunk = display_frames_per_chunk(n_frames, n, a.alpha);
    HIP_TRY(mcrt::launch_compound(a, true, c->stream));
    return MCRT_OK;
}

extern "C" int mcrt_bmode_compound_frames(mcrt_ctx *c, const float *rf_dev, uint32_t n_frames, uint32_t E, uint32_t R, const mcrt_bmode_params *p,
                                          const mcrt_compound *cp, const float *tgc_db, float *state_dev, float *peak_dev, uint8_t *out_dev)
{
    return mcrt_bmode_compound_frames_opts(c, rf_dev, n_frames, E, R, p, cp, tgc_db, state_dev, peak_dev, out_dev, nullptr);
}

// ---- volume imaging (the contracts are in include/mcrt.h) ----
// the three maps of a grid on the device: the slot that holds them, or the least recently used one refilled (made on the host by
// mcrt_volume_maps and uploaded; a slot's buffer only ever grows)
static int ensure_volume_maps(mcrt_ctx *c, uint32_t E, uint32_t R, double radius_mm, double total_angle, const mcrt_sweep *sw, const mcrt_volume_grid *g, const float **maps)
{
    uint32_t key[9] = { E, R, c->p.speed_of_sound, sw->n_planes, g->nu, g->nv, g->nw, 0u, 0u };
    memcpy(&key[7], &sw->step_rad, 4); memcpy(&key[8], &sw->pivot_mm, 4);
    double keyd[15] = { radius_mm, total_angle, c->c.max_travel_us };
    memcpy(&keyd[3], g->origin_mm, 12 * sizeof(double));                     // origin_mm, du_mm, dv_mm, dw_mm are contiguous (mcrt.h gives the offsets)
    VolumeMapCache &vc = c->vmaps;
    VolumeMapCache::Slot *lru = &vc.slot[0];
    for (VolumeMapCache::Slot &s : vc.slot) {
        if (s.used && !memcmp(key, s.key, sizeof key) && !memcmp(keyd, s.keyd, sizeof keyd)) { s.used = ++vc.clock; *maps = s.d; return MCRT_OK; }
        if (s.used < lru->used) lru = &s;
    }
    const size_t n = (size_t)g->nu * g->nv * g->nw, n_pad = MapCache::pad(n);
    std::vector<float> m(3 * n_pad, 0.0f);
    MCRT_TRY(mcrt_volume_maps(E, R, radius_mm, total_angle, (uint32_t)c->c.max_travel_us, c->p.speed_of_sound, sw, g, &m[0], &m[2 * n_pad], &m[n_pad]));
    HIP_TRY(hipStreamSynchronize(c->stream));                                // (the evicted grid's last gather)
    lru->used = 0;                                                            // (no grid until the maps are on the device)
    HIP_TRY(lru->d.grow(m.size()));
    HIP_TRY(hipMemcpy(lru->d, m.data(), m.size() * 4, hipMemcpyHostToDevice));
    memcpy(lru->key, key, sizeof key); memcpy(lru->keyd, keyd, sizeof keyd); lru->used = ++vc.clock;
    *maps = lru->d;
    return MCRT_OK;
}

// what the two entry points check of the stack and the grid before anything else happens
static int volume_args_check(const char *fn, uint32_t n_frames, uint32_t E, uint32_t R, double total_angle, const mcrt_sweep *sw, const mcrt_volume_grid *g)
{
    if (E == 0 || R == 0 || n_frames == 0) return set_error(MCRT_ERR_INVALID, "%s: zero sizes", fn);
    if (!(total_angle > 0.0)) return set_error(MCRT_ERR_INVALID, "%s: total_angle_rad must be > 0", fn);
    MCRT_TRY(mcrt::volume_check(fn, sw, g));
    if (R > MCRT_MAX_ROWS) return set_error(MCRT_ERR_LIMIT, "%s: at most %d rows", fn, MCRT_MAX_ROWS);
    if ((uint64_t)n_frames * sw->n_planes > 65535ull) return set_error(MCRT_ERR_LIMIT, "%s: at most 65535 planes per call (%u frames x %u)", fn, n_frames, sw->n_planes);
    return MCRT_OK;
}

static mcrt::VolumeArgs volume_args(const float *src, const float *maps, void *out, uint32_t n_frames, uint32_t E, uint32_t R, uint32_t K, uint32_t n, bool out8)
{
    mcrt::VolumeArgs a;
    a.src = src; a.maps = maps; a.out = out; a.E = E; a.R = R; a.K = K; a.n = n; a.n_pad = (uint32_t)MapCache::pad(n); a.F = n_frames;
    a.frames_per_chunk = display_frames_per_chunk(n_frames, n, 0.0f);
    a.vec = out8 && n % 4u == 0u && (uintptr_t)out % 4u == 0u ? 1u : 0u;
    return a;
}

extern "C" int mcrt_volume_frames(mcrt_ctx *c, const float *rf_dev, uint32_t n_frames, uint32_t E, uint32_t R, double radius_mm, double total_angle,
                                  const mcrt_sweep *sw, const mcrt_volume_grid *g, float *out_dev)
{
    CTX_TRY(c);
    static const char fn[] = "mcrt_volume_frames";
    if (!rf_dev || !out_dev) return set_error(MCRT_ERR_INVALID, "%s: null %s", fn, rf_dev ? "out_dev" : "rf_dev");
    MCRT_TRY(volume_args_check(fn, n_frames, E, R, total_angle, sw, g));
    const uint32_t K = sw->n_planes, n = g->nu * g->nv * g->nw;
    if (ranges_overlap(rf_dev, 4 * (size_t)n_frames * K * E * R, out_dev, 4 * (size_t)n_frames * n)) return set_error(MCRT_ERR_INVALID, "%s: rf_dev and out_dev overlap", fn);
    const float *maps = nullptr;
    MCRT_TRY(ensure_volume_maps(c, E, R, radius_mm, total_angle, sw, g, &maps));
    HIP_TRY(mcrt::launch_volume(volume_args(rf_dev, maps, out_dev, n_frames, E, R, K, n, false), false, c->stream));
    return MCRT_OK;
}

extern "C" int mcrt_bmode_volume_frames(mcrt_ctx *c, const float *rf_dev, uint32_t n_frames, uint32_t E, uint32_t R, const mcrt_bmode_params *p,
                                        const mcrt_sweep *sw, const mcrt_volume_grid *g, const float *tgc_db, float *peak_dev, uint8_t *out_dev)
{
    CTX_TRY(c);
    static const char fn[] = "mcrt_bmode_volume_frames";
    if (!p) return set_error(MCRT_ERR_INVALID, "%s: null params", fn);
    mcrt_bmode_params q = *p;
    q.out_rows = q.out_cols = 1u;                       // the picture is the grid's: p's own size is not looked at
    std::vector<float> k;
    MCRT_TRY(bmode_check(fn, rf_dev, out_dev, n_frames, E, R, &q, tgc_db, k));
    if (p->persistence != 0.0f) return set_error(MCRT_ERR_INVALID, "%s: persistence must be 0 on a volume (%g)", fn, (double)p->persistence);
    MCRT_TRY(volume_args_check(fn, n_frames, E, R, p->total_angle_rad, sw, g));
    const uint32_t K = sw->n_planes, n = g->nu * g->nv * g->nw;
    if ((uint64_t)K * E > 0xffffffffull) return set_error(MCRT_ERR_LIMIT, "%s: too many scan-lines (%u planes x %u)", fn, K, E);   // (a frame is K * E scan-lines to steps 1-3)
    if (ranges_overlap(rf_dev, 4 * (size_t)n_frames * K * E * R, out_dev, (size_t)n_frames * n)) return set_error(MCRT_ERR_INVALID, "%s: rf_dev and out_dev overlap", fn);
    const float *maps = nullptr;
    MCRT_TRY(ensure_volume_maps(c, E, R, p->radius_mm, p->total_angle_rad, sw, g, &maps));
    MCRT_TRY(bmode_grey_pass(c, rf_dev, n_frames, K * E, R, &q, tgc_db, k, peak_dev));
    HIP_TRY(mcrt::launch_volume(volume_args(c->d_tmp, maps, out_dev, n_frames, E, R, K, n, true), true, c->stream));
    return MCRT_OK;
}

extern "C" int mcrt_export_rf(mcrt_ctx *c, const float *rf_dev, uint32_t E, uint32_t R, float *host)
{
    CTX_TRY(c);
    if (!rf_dev || !host || E == 0 || R == 0) return set_error(MCRT_ERR_INVALID, "mcrt_export_rf: bad arguments");
    MCRT_TRY(ensure_tmp(c, (size_t)E * R));
    HIP_TRY(mcrt::launch_transpose(rf_dev, c->d_tmp, E, R, c->stream));
    HIP_TRY(hipMemcpyAsync(host, c->d_tmp, (size_t)E * R * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MCRT_OK;
}

extern "C" int mcrt_import_rf(mcrt_ctx *c, const float *host, uint32_t E, uint32_t R, float *rf_dev)
{
    CTX_TRY(c);
    if (!rf_dev || !host || E == 0 || R == 0) return set_error(MCRT_ERR_INVALID, "mcrt_import_rf: bad arguments");
    MCRT_TRY(ensure_tmp(c, (size_t)E * R));
    HIP_TRY(hipMemcpyAsync(c->d_tmp, host, (size_t)E * R * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(mcrt::launch_transpose(c->d_tmp, rf_dev, R, E, c->stream));          // [R][E] -> [E][R]
    HIP_TRY(hipStreamSynchronize(c->stream));
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

extern "C" int mcrt_enable_stats(mcrt_ctx *c, int on) { CTX_TRY(c); c->stats_on = on != 0; return MCRT_OK; }
// words [first, first + n) of the context's counter block, once the stream is idle; zeroed afterwards on request
static int read_stats(mcrt_ctx *c, size_t first, size_t n, void *out, int reset)
{
    CTX_TRY(c);
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out, c->d_stats + first, n * 8, hipMemcpyDeviceToHost));
    if (reset) { HIP_TRY(hipMemsetAsync(c->d_stats + first, 0, n * 8, c->stream)); HIP_TRY(hipStreamSynchronize(c->stream)); }
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
    out[0] = c->fast_div ? 1u : 0u; out[1] = c->last_lean_bound > 0.0f ? 1u : 0u; out[2] = c->last_march_rows; out[3] = 0u;
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

extern "C" int mcrt_enable_timing(mcrt_ctx *c, int on) { CTX_TRY(c); c->timing_on = on != 0; c->timing_level = on; return MCRT_OK; }
extern "C" int mcrt_get_kernel_times(mcrt_ctx *c, double avg_ms[3], uint32_t n[3], int reset)
{
    CTX_TRY(c);
    // each recorded pair is waited for by itself: the pairs live on the streams their launches ran on (the groups' own, the side streams), not
    // only on the one current now -- and a caller polling the walk's time does not stall on other contexts of the device
    double sum[3] = { 0, 0, 0 }; uint32_t cnt[3] = { 0, 0, 0 };
    for (size_t i = 0; i < c->ev_used; i++) {
        const TimedLaunch &t = c->ev[i];
        float ms = 0;
        HIP_TRY(hipEventSynchronize(t.end));
        HIP_TRY(hipEventElapsedTime(&ms, t.start, t.end));
        sum[t.kind] += ms; cnt[t.kind]++;
    }
    for (int k = 0; k < 3; k++) { if (avg_ms) avg_ms[k] = cnt[k] ? sum[k] / (double)cnt[k] : 0.0; if (n) n[k] = cnt[k]; }
    if (reset) c->ev_used = 0;
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
