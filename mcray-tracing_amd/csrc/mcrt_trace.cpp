// mcrt_trace.cpp -- the traced pass of the C-ABI (include/mcrt.h): how a pass is planned, its work sets, its launches and their streams,
// the accumulators, and the entry points that trace (mcrt_trace_frame*, mcrt_cast_rays).  Host C++ only; the context is mcrt_ctx.h.
#include "mcrt_ctx.h"
#include "mcrt_kernels.h"

#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <vector>
#include <algorithm>
#include <utility>

using mcrt::set_error;

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

static int ensure_acc(mcrt_ctx *c, uint32_t ne)
{
    const size_t need = (size_t)ne * c->p.n_rows, needf = (size_t)ne * ((c->p.n_rows + 31u) >> 5);
    if (need > c->acc.d_acc.cap || needf > c->acc.d_flags.cap) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->acc.clean_ne = 0;
        HIP_TRY(c->acc.d_acc.grow(need)); HIP_TRY(c->acc.d_flags.grow(needf));
    }
    // k_finalize leaves the bins zeroed; only a shape change (or a failed frame) needs an explicit clear
    if (c->acc.clean_ne != ne || c->acc.clean_rows != c->p.n_rows) {
        HIP_TRY(hipMemsetAsync(c->acc.d_acc, 0, need * 8, c->stream));
        HIP_TRY(hipMemsetAsync(c->acc.d_flags, 0, needf * 4, c->stream));
    }
    c->acc.clean_ne = 0; c->acc.clean_rows = 0;   // dirty until the frame's k_finalize has been enqueued
    return MCRT_OK;
}

// pose_pos: the pass's per-frame pose tables on the device, or null (the transducer of mcrt_set_transducer)
static int check_ready(mcrt_ctx *c, uint32_t e0, uint32_t e1, const float *pose_pos = nullptr)
{
    if (!c->scene.have) return set_error(MCRT_ERR_INVALID, "no scene uploaded");
    if (!c->d_tex) return set_error(MCRT_ERR_INVALID, "no texture uploaded");
    if (c->tex_n != c->p.tex_n) return set_error(MCRT_ERR_INVALID, "texture is %u^3 but params say %u^3", c->tex_n, c->p.tex_n);
    if (!pose_pos) {
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
    P.latency = !c->ins.stats_on && (uint64_t)ne * n_frames * S <= c->knobs.path_max;
    uint32_t groups = (one_group || c->ins.stats_on) ? 1u : c->knobs.groups;
    if (!one_group && groups == 1u && P.latency) groups = c->knobs.path_groups;
    P.groups = std::max(1u, std::min({ groups, ne, 16u }));
    for (uint32_t g = 0; g <= P.groups; g++) P.e[g] = e0 + (uint32_t)(((uint64_t)ne * g) / P.groups);
    P.trace_blocks = c->knobs.trace_blocks ? c->knobs.trace_blocks : c->n_cu * 4u;   // persistent k_trace: 4 four-wave workgroups per CU (1024 on the MI355X's 256 CUs) of the 5 its registers and LDS allow --
                                                                                  // the fifth's registers go to a k_march wavefront beside them (since k_march's fast path: 0.446 -> 0.428 ms per frame on a 20-frame pass, 0.366 -> 0.364 at 128)
    P.trace_blocks_wide = c->knobs.trace_blocks_wide ? c->knobs.trace_blocks_wide : c->n_cu * 5u;      // k_trace_lane_wide: five workgroups per CU
    // ... while the tree is served from the caches: with 16 M triangles (460 MB of walked nodes, past the Infinity Cache) a fifth wavefront per SIMD only
    // adds misses -- 0.667 against 0.638 ms per frame -- where the 1 M-triangle scene (29 MB) gains 3-4 %; the line is drawn at half the Infinity Cache
    if ((uint64_t)c->scene.bvh4.n_nodes * 64ull > (uint64_t)c->knobs.wide_max_tree_mb * 1048576ull) P.trace_blocks_wide = 0;
    const uint32_t lds_part = mcrt::lane_stack_entries();
    const size_t deep = c->scene.bvh4.max_stack > lds_part ? c->scene.bvh4.max_stack - lds_part : 0;
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
    HIP_TRY(b.key0.alloc(np)); HIP_TRY(b.key1.alloc(np)); HIP_TRY(b.from_tri.alloc(2 * np));   // (from_tri: by path, and behind it the beam words by queue position)
    HIP_TRY(b.q.alloc(2 * np)); HIP_TRY(b.seg_count.alloc(np));
    HIP_TRY(b.counts.alloc(MCRT_MAX_BOUNCES + 1));
    HIP_TRY(b.cursors.alloc((size_t)MCRT_MAX_BOUNCES * MCRT_XCDS * MCRT_CURSOR_STRIDE));
    HIP_TRY(b.mrec.alloc(3 * np * B));
    b.paths = np; b.depth = B;
    return MCRT_OK;
}

// the kernel arguments every group of a pass shares (acc_ne: scan-lines of the frame's RF block); fill_group adds each group's own
static void fill_pass(mcrt_ctx *c, const Plan &P, mcrt::FrameArgs &a, uint32_t frame, uint32_t acc_ne, bool accumulate, int out, const float *pose_pos, const float *pose_dir)
{
    memset(&a, 0, sizeof a);
    a.nodes_walk = c->scene.d_nodes_walk; a.tris = c->scene.d_tris; a.meshes = c->scene.d_meshes; a.mats = c->scene.d_mats; a.tex = c->d_tex;
    a.el_pos = pose_pos ? pose_pos : c->d_pos; a.el_dir = pose_pos ? pose_dir : c->d_dir; a.pose_stride = pose_pos ? c->p.n_elements : 0u;
    a.row_thr = c->tab.d_row_thr;
    a.acc = c->acc.d_acc; a.flags = c->acc.d_flags; a.acc_stride = acc_ne;   // the frame block [n_frames][acc_ne][R]
    a.tri_slot = c->scene.d_tri_slot; a.tris_id = c->scene.d_tris_id; a.mtab = c->tab.d_mtab;
    a.stats = c->ins.d_stats; a.error_flag = c->d_error; a.stamps = c->ins.d_stats + 8;
    a.n_mat = c->scene.n_mat; a.n_mesh = c->scene.n_mesh; a.n_nodes = c->scene.bvh4.n_nodes; a.S = c->p.n_samples; a.B = c->p.max_depth; a.R = c->p.n_rows;
    a.ksplit_limit = c->knobs.ksplit_limit;   // bounces with fewer rays than this are cut into pieces (see k_trace)
    if (c->ins.stats_on) a.ksplit_limit = 0;   // counting mode = one walk per ray, so the counts are those of a plain closest-hit walk
    for (int i = 0; i < 3; i++) { a.scene_lo[i] = c->scene.lo[i]; a.scene_hi[i] = c->scene.hi[i]; }
    a.trace_blocks = P.trace_blocks; a.trace_blocks_wide = P.trace_blocks_wide;
    a.wide_from = c->knobs.wide_from ? c->knobs.wide_from : mcrt::lane_wide_from();
    a.march_blocks = c->knobs.march_blocks;
    a.want_segs = out >= 2 ? 1u : 0u;
    a.frame = frame; a.seed = c->p.seed; a.start_mat = c->scene.start_mat; a.tex_n = c->tex_n; a.tex_mask = (c->tex_n & (c->tex_n - 1u)) == 0u ? c->tex_n - 1u : 0u;
    a.sanitize = c->p.sanitize_tir; a.tex_finite = c->tex_finite ? 1u : 0u;
    a.freq = c->p.frequency; a.eps = c->p.intensity_epsilon; a.I0 = c->p.initial_intensity; a.offs = c->p.ray_start_offset;
    a.sx = c->scene.spacing[0]; a.sy = c->scene.spacing[1]; a.sz = c->scene.spacing[2]; a.tex_res = c->p.tex_res; a.axial_res_f = c->c.axial_res_f; a.pad_abs = c->scene.bvh.pad_abs; a.tex_rcp = 1.0f / c->p.tex_res; a.fast_div = c->tab.fast_div ? 1u : 0u;
    // k_march's branch-free texture lookup: power-of-two texture, verified division, |x / res| < 2^31
    a.tex_shift = 0; while ((1u << a.tex_shift) < c->tex_n) a.tex_shift++;
    a.lean_bound = 0.0f;
    if (c->tab.fast_div_all && a.tex_mask && a.tex_shift <= 10u) {
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
    c->ins.last_lean_bound = a.lean_bound; c->ins.last_march_rows = a.march_rows;
    // Work the image does not need, left out where only the image is asked for: a counting pass and the hit / segment tables show every path to its end.
    const bool image_only = !c->ins.stats_on && out == 0;
    a.thr_end = c->tab.thr_end;
    a.retire_late = image_only && c->knobs.retire_late ? 1u : 0u;
    // bounce 0 folded into k_shade: the staged form, an RF block to add into, the start material silent by k_march's own test, and a workgroup
    // of k_shade(0) within one queued scan-line
    a.fold_b0 = image_only && c->knobs.fold_b0 && !P.latency && accumulate && c->tex_finite && c->scene.start_silent && c->p.n_samples % 256u == 0u ? 1u : 0u;
}

// group g's own arguments: its scan-lines [b0,b1) of the pass's n_frames frames, its columns of the RF block (which begins at acc_e0), its work set
static void fill_group(const mcrt_ctx *c, const Work &w, mcrt::FrameArgs &a, uint32_t n_frames, uint32_t b0, uint32_t b1, uint32_t acc_e0, int out)
{
    a.stack_ovf = w.stack_ovf; a.segs = w.segs; a.hits = out >= 1 ? (int32_t *)w.hits : nullptr;
    a.st0 = w.b.st0; a.st1 = w.b.st1; a.st2 = w.b.st2; a.queue = w.b.q; a.key0 = w.b.key0; a.key1 = w.b.key1; a.from_tri = w.b.from_tri;
    a.counts = w.b.counts; a.cursors = w.b.cursors; a.mrec = w.b.mrec; a.seg_count = w.b.seg_count;
    a.acc_off = b0 - acc_e0;
    a.e_begin = b0; a.ne_frame = b1 - b0; a.ne = (b1 - b0) * n_frames;   // n_frames consecutive frame ids traced as one pass
    a.packet_mask = (c->ins.stats_on || (uint64_t)a.ne * a.S < c->knobs.packet_from) ? 0u : c->knobs.packet_mask;   // bounces walked a wavefront per ray packet (k_trace_packet); the counting build walks ray by ray
}

// Bounces by beams (mcrt_beam.hip), as a mask of bounces.  Bounce 1: where it runs as packets today and the pass has ONE probe pose -- every bounce-1 ray of a
// scan-line then starts at the same point in every frame.  Bounces 2 .. MCRT_BEAM_LAST: in passes of at least MCRT_BEAM_DEEP_FROM paths with one pose (their rays
// are grouped by the triangle they left, the same in every frame), bounces >= 4 of them in passes of at least MCRT_BEAM_B4_FROM.  Not in the latency form, a counting pass or a pass with per-frame poses; MCRT_BEAM_B1=2 takes
// all of them in every other pass, 0 none.
static uint32_t beam_wanted(const mcrt_ctx *c, const Plan &P, const mcrt::FrameArgs &a)
{
    if (P.latency || c->ins.stats_on || a.pose_stride != 0u || a.B < 2u || a.n_nodes == 0u || c->knobs.beam_b1 == 0u) return 0u;
    const bool force = c->knobs.beam_b1 == 2u;
    const uint64_t np = (uint64_t)a.ne * a.S;
    uint32_t mask = 0;
    if (force || ((a.packet_mask & 2u) != 0u && np >= c->knobs.beam_from)) mask |= 2u;
    if (force || np >= c->knobs.beam_deep_from)
        for (uint32_t b = 2; b <= c->knobs.beam_last && b < a.B; b++)
            if (force || b < 4u || np >= c->knobs.beam_b4_from) mask |= 1u << b;
    return mask;
}
// what the beamed bounces of a group share: the buffers, sized for the largest of them; beam_args makes bounce b's block of it
struct BeamPlan { mcrt::BeamArgs g = {}; uint32_t mask = 0, order = 0, beams_b1 = 0, groups = 0; };
static int fill_beam(const mcrt_ctx *c, Work &w, const mcrt::FrameArgs &a, uint32_t mask, BeamPlan &bp)
{
    const uint32_t cap = c->knobs.beam_cap;
    bp.mask = mask; bp.beams_b1 = a.ne_frame * MCRT_BEAM_SLOTS; bp.groups = 0;
    if (mask & ~2u) {      // the group table: a power of two
        const uint64_t want = c->knobs.beam_groups ? c->knobs.beam_groups : (uint64_t)a.ne_frame * MCRT_BEAM_GROUPS_PER_LINE;
        bp.groups = 1u;
        while ((uint64_t)bp.groups * 2u <= want && bp.groups < (1u << 20)) bp.groups *= 2u;
        if (!c->knobs.beam_groups && bp.groups < want) bp.groups *= 2u;
    }
    const uint32_t beams = std::max((mask & 2u) ? bp.beams_b1 : 0u, bp.groups * 6u);
    const uint32_t lists = std::max((mask & 2u) ? bp.beams_b1 : 0u, bp.groups * MCRT_BEAM_LISTS_PER_GROUP);
    BeamBufs &b = w.beam;
    if (beams > b.beams || lists > b.lists || bp.groups > b.groups || cap != b.cap) {
        HIP_TRY(hipDeviceSynchronize());
        b.beams = b.lists = b.groups = b.cap = 0;
        HIP_TRY(b.red.alloc((size_t)beams * MCRT_BEAM_REC)); HIP_TRY(b.rec.alloc((size_t)beams * MCRT_BEAM_REC)); HIP_TRY(b.list.alloc(((size_t)lists * cap + 1) * 4));
        HIP_TRY(b.hot.alloc(((size_t)lists * cap + 1) * MCRT_BEAM_HOT));      // (+ one entry, as the list: the second fetch of the last pair)
        HIP_TRY(b.gkey.alloc(std::max(bp.groups, 1u)));
        HIP_TRY(b.lcount.grow((size_t)MCRT_MAX_BOUNCES * MCRT_BEAM_COUNTERS)); HIP_TRY(b.l_counts.grow(MCRT_MAX_BOUNCES + 1)); HIP_TRY(b.l_cursors.grow((size_t)MCRT_MAX_BOUNCES * MCRT_XCDS * MCRT_CURSOR_STRIDE));
        b.beams = beams; b.lists = lists; b.groups = bp.groups; b.cap = cap;
    }
    const size_t np = (size_t)a.ne * a.S;
    bp.order = mask & c->knobs.beam_order;
    if (bp.order && (np > b.order_rays || beams > b.order_beams)) {      // the beam order: only where a bounce is ordered
        HIP_TRY(hipDeviceSynchronize());
        b.order_rays = 0; b.order_beams = 0;
        HIP_TRY(b.rbeam.alloc(np)); HIP_TRY(b.rrank.alloc(np)); HIP_TRY(b.ocount.alloc((size_t)beams + 1)); HIP_TRY(b.obase.alloc((size_t)beams + 1));
        HIP_TRY(b.order.alloc(np + 64 * ((size_t)beams + 1)));
        b.order_rays = np; b.order_beams = beams;
    }
    mcrt::BeamArgs &g = bp.g;
    g.rbeam = b.rbeam; g.rrank = b.rrank; g.ocount = b.ocount; g.obase = b.obase; g.order = b.order; g.pairs = c->knobs.beam_pairs ? 1u : 0u;
    g.red = b.red; g.rec = b.rec; g.list = b.list; g.hot = b.hot; g.gkey = b.gkey; g.lcount = b.lcount; g.l_counts = b.l_counts; g.l_cursors = b.l_cursors;
    g.cap = cap; g.near = std::min(c->knobs.beam_near, cap);
    g.stride = np >= MCRT_BEAM_SAMPLE_FROM ? MCRT_BEAM_SAMPLE_STRIDE : 1u;
    g.spread_cap = MCRT_BEAM_SPREAD;
    return MCRT_OK;
}
static mcrt::BeamArgs beam_args(const BeamPlan &bp, const mcrt::FrameArgs &a, uint32_t b)
{
    mcrt::BeamArgs g = bp.g;
    const size_t other = (b & 1u) ? 0 : (size_t)a.ne * a.S;      // the halves of the other bounce parity: dead between k_shade(b - 1) and k_shade(b)
    g.b = b; g.lcount = bp.g.lcount + (size_t)b * MCRT_BEAM_COUNTERS;
    g.lq0 = a.queue + other; g.lq1 = (uint32_t *)(a.st2 + other);
    g.groups = b == 1u ? 0u : bp.groups;
    g.n_beams = b == 1u ? bp.beams_b1 : bp.groups * 6u;
    g.n_lists = b == 1u ? bp.beams_b1 : bp.groups * MCRT_BEAM_LISTS_PER_GROUP;
    g.ordered = (bp.order >> b) & 1u;
    return g;
}

// The walk kernels (k_trace_lane*, k_path) index their traversal-stack overflow with stride gridDim.x * 256 and check no bound: the
// largest grid a group's walks can take must fit its work set, or nothing is launched
static int check_overflow(const mcrt_ctx *c, const Plan &P, const mcrt::FrameArgs &a, const Work &w)
{
    const uint32_t lds_part = mcrt::lane_stack_entries();
    if (c->scene.bvh4.max_stack <= lds_part) return MCRT_OK;
    const uint32_t blocks = P.latency ? mcrt::path_blocks((size_t)a.ne * a.S) : std::max(a.trace_blocks, a.trace_blocks_wide);
    const size_t need = (size_t)(c->scene.bvh4.max_stack - lds_part) * blocks * 256;
    if (need > w.stack_ovf.cap) return set_error(MCRT_ERR_LIMIT, "traversal-stack overflow: %zu entries needed, the work set holds %zu", need, w.stack_ovf.cap);
    return MCRT_OK;
}

// one launch on stream st; when its kind is timed (0: the walk, 1: k_shade, 2: k_march -- see mcrt_enable_timing) bracketed by HIP events on st
template <class Launch> static int timed_launch(mcrt_ctx *c, int kind, hipStream_t st, Launch launch)
{
    if (!c->ins.timing_on || (kind != 0 && c->ins.timing_level < 2)) { HIP_TRY(launch()); return MCRT_OK; }
    if (c->ins.ev_used == c->ins.ev.size()) {
        if (c->ins.ev.size() >= 65536) return set_error(MCRT_ERR_LIMIT, "timing buffer full: call mcrt_get_kernel_time(reset=1)");
        TimedLaunch t;
        HIP_TRY(hipEventCreate(&t.start.h)); HIP_TRY(hipEventCreate(&t.end.h));
        c->ins.ev.push_back(std::move(t));
    }
    TimedLaunch &t = c->ins.ev[c->ins.ev_used];
    HIP_TRY(hipEventRecord(t.start, st));
    HIP_TRY(launch());
    HIP_TRY(hipEventRecord(t.end, st));
    t.kind = kind; c->ins.ev_used++;
    return MCRT_OK;
}

// one bounce of one group of a staged pass: the walk + k_shade on the group's stream, k_march of the finished segments on its side stream.
// (Round 4 tried holding k_march of bounce b back until the walk of bounce b+1 had claimed its last ray -- a device word raised by the walk, waited
//  for with hipStreamWaitValue32, which the command processor releases ~1 us after the store --: 0.360 against 0.343 ms per frame at 128 frames in
//  flight, 0.414 against 0.405 on the driver's pass, and a hang under `rocprofv3 --pmc`.  Removed; DESIGN.md A.6, profiles/round4/exp_round4_kernels.txt.)
static int run_bounce(mcrt_ctx *c, Work &w, hipStream_t st, const mcrt::FrameArgs &a, const BeamPlan &beam, uint32_t b, uint32_t sides, bool accumulate, bool overlap)
{
    if ((beam.mask >> b) & 1u) MCRT_TRY(timed_launch(c, 0, st, [&] { return mcrt::launch_beam(a, beam_args(beam, a, b), st); }));
    else MCRT_TRY(timed_launch(c, 0, st, [&] { return mcrt::launch_trace(a, b, c->ins.stats_on, st); }));
    MCRT_TRY(timed_launch(c, 1, st, [&] { return mcrt::launch_shade(a, b, c->ins.stats_on, st); }));
    if (!accumulate || (a.fold_b0 && b == 0u)) return MCRT_OK;      // (bounce 0 folded: k_shade has added its echoes; later bounces keep their side streams)
    hipStream_t ms = st;
    if (overlap) {   // the segments of bounce b are final: accumulate them beside the next bounce's walk
        HIP_TRY(hipEventRecord(w.ev_bounce[b], st));
        MCRT_TRY(side_stream(c, w, b % sides, &ms));
        HIP_TRY(hipStreamWaitEvent(ms, w.ev_bounce[b], 0));
    }
    return timed_launch(c, 2, ms, [&] { return mcrt::launch_march(a, b, c->ins.stats_on, ms); });
}

static int enqueue_pass(mcrt_ctx *c, const Plan &P, const mcrt::FrameArgs *args, const BeamPlan *beams, Work *const *ws, bool accumulate)
{
    const bool overlap = !c->knobs.no_overlap;
    hipStream_t gst[16] = { c->stream };
    for (uint32_t g = 1; g < P.groups; g++) MCRT_TRY(work_stream(*ws[g], &gst[g]));
    if (c->scene.update_pending && c->scene.update_stream != c->stream) HIP_TRY(hipStreamWaitEvent(c->stream, c->scene.ev_update, 0));   // a scene update issued on another stream
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
                MCRT_TRY(run_bounce(c, *ws[g], gst[g], args[g], beams[g], b, P.sides[g], accumulate, overlap));
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
static int run_pass(mcrt_ctx *c, uint32_t frame, uint32_t n_frames, uint32_t e0, uint32_t e1, bool accumulate, bool one_group, int out, const float *pose_pos = nullptr, const float *pose_dir = nullptr)
{
    const Plan P = plan_pass(c, e0, e1, n_frames, one_group);
    mcrt::FrameArgs pass, args[16];
    BeamPlan beams[16];
    Work *ws[16];
    fill_pass(c, P, pass, frame, e1 - e0, accumulate, out, pose_pos, pose_dir);
    for (uint32_t g = 0; g < P.groups; g++) {
        MCRT_TRY(get_work(c, g, &ws[g]));
        MCRT_TRY(ensure_work(*ws[g], (size_t)(P.e[g + 1] - P.e[g]) * n_frames * c->p.n_samples, c->p.max_depth, P.ovf[g], out));
        args[g] = pass;
        fill_group(c, *ws[g], args[g], n_frames, P.e[g], P.e[g + 1], e0, out);
        MCRT_TRY(check_overflow(c, P, args[g], *ws[g]));
        if (const uint32_t mask = beam_wanted(c, P, args[g])) { MCRT_TRY(fill_beam(c, *ws[g], args[g], mask, beams[g])); args[g].beam_mask = mask & ~3u; args[g].order_mask = beams[g].order & ~3u; }
    }
    c->ins.last_beam_mask = beams[0].mask; c->ins.last_beam_order = beams[0].order; c->ins.last_beam_far = c->knobs.beam_near < c->knobs.beam_cap;
    c->ins.last_beam_b1 = beams[0].beams_b1; c->ins.last_beam_groups = beams[0].groups; c->ins.last_beam_cap = beams[0].g.cap; c->ins.last_beam_near = beams[0].g.near; c->ins.last_beam_depth = c->p.max_depth;
    return enqueue_pass(c, P, args, beams, ws, accumulate);
}

// the traced block's accumulators [lines][R] into rf_dev; k_finalize leaves them zeroed (ensure_acc)
static int finalize(mcrt_ctx *c, float *rf_dev, uint32_t lines)
{
    HIP_TRY(mcrt::launch_finalize(c->acc.d_acc, c->acc.d_flags, rf_dev, lines, c->p.n_rows, c->d_error, c->stream));
    c->acc.clean_ne = lines; c->acc.clean_rows = c->p.n_rows;
    return MCRT_OK;
}

// mcrt_trace_frames, with the pass's per-frame pose tables on the device [n_frames][E][3] (k_init reads frame f's rows) or null
static int trace_frames(mcrt_ctx *c, uint32_t frame, uint32_t n_frames, uint32_t e0, uint32_t e1, const float *pose_pos, const float *pose_dir, float *rf_dev)
{
    CTX_TRY(c);
    MCRT_TRY(check_ready(c, e0, e1, pose_pos));
    if (!rf_dev) return set_error(MCRT_ERR_INVALID, "null rf_dev");
    if (n_frames == 0 || n_frames > 1024) return set_error(MCRT_ERR_LIMIT, "n_frames must be 1..1024");
    if ((uint64_t)(e1 - e0) * n_frames * c->p.n_samples > (1ull << 27))        // (~600 bytes of work buffers per path)
        return set_error(MCRT_ERR_LIMIT, "%u frames x %u scan-lines x %u samples: more than 2^27 paths in one pass", n_frames, e1 - e0, c->p.n_samples);
    const uint32_t lines = (e1 - e0) * n_frames;
    MCRT_TRY(ensure_acc(c, lines));
    MCRT_TRY(run_pass(c, frame, n_frames, e0, e1, true, false, 0, pose_pos, pose_dir));
    return finalize(c, rf_dev, lines);
}

extern "C" int mcrt_trace_frames(mcrt_ctx *c, uint32_t frame, uint32_t n_frames, uint32_t e0, uint32_t e1, float *rf_dev)
{
    return trace_frames(c, frame, n_frames, e0, e1, nullptr, nullptr, rf_dev);
}

extern "C" int mcrt_trace_frame(mcrt_ctx *c, uint32_t frame, uint32_t e0, uint32_t e1, float *rf_dev)
{
    return mcrt_trace_frames(c, frame, 1, e0, e1, rf_dev);
}

// the pose tables of `lines` (frame, scan-line) entries on the device: a table in host memory is staged (see mcrt_trace_frames_poses), a
// device table is used as it is.  Two Staging begin / commit pairs on the context's stream, positions first.
int mcrt::stage_poses(mcrt_ctx *c, size_t lines, const float *dev[2])
{
    for (int k = 0; k < 2; k++) {
        if (is_device_pointer(dev[k])) continue;
        float *h = nullptr;
        MCRT_TRY(c->pose_stage[k].begin(3 * lines, c->stream, &h));
        memcpy(h, dev[k], 12 * lines);
        MCRT_TRY(c->pose_stage[k].commit(3 * lines, c->stream));
        dev[k] = c->pose_stage[k].dev;
    }
    return MCRT_OK;
}

// A pass whose frames each have their own probe pose (transducer.h:82-118 update() between the frames of main.cpp:92-152).  A table in
// HOST memory belongs to the caller and may be pageable: it is staged in the context (Staging: copied into pinned memory before this call
// returns, so that the caller may free or rewrite it at once, and to the device from there on the stream; the copy of the previous call
// -- an early node of the previous pass, not the pass -- is waited for first).
extern "C" int mcrt_trace_frames_poses(mcrt_ctx *c, uint32_t frame, uint32_t n_frames, uint32_t e0, uint32_t e1,
                                       const float *pos, const float *dir, float *rf_dev)
{
    CTX_TRY(c);
    if (!pos || !dir) return set_error(MCRT_ERR_INVALID, "mcrt_trace_frames_poses: null pose tables");
    if (n_frames == 0 || n_frames > 1024) return set_error(MCRT_ERR_LIMIT, "n_frames must be 1..1024");
    const float *dev[2] = { pos, dir };
    MCRT_TRY(mcrt::stage_poses(c, (size_t)n_frames * c->p.n_elements, dev));
    return trace_frames(c, frame, n_frames, e0, e1, dev[0], dev[1], rf_dev);
}

// copies the per-path tables (work set 0) to the host: segs [ne][S][B], seg_count [ne][S], hits [ne][S][B] (= segment.tri, -2 beyond the path's end)
static int copy_out(mcrt_ctx *c, uint32_t ne, int32_t *hits, mcrt_segment *segs, uint32_t *seg_count)
{
    const size_t np = (size_t)ne * c->p.n_samples, B = c->p.max_depth;
    const Work &w = c->work[0];
    HIP_TRY(hipStreamSynchronize(c->stream));
    MCRT_TRY(mcrt::check_device_error(c));
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

// ---- ground-truth label maps (the contract is in include/mcrt.h) ----
extern "C" int mcrt_default_label_opts(mcrt_label_opts *o)
{
    if (!o) return set_error(MCRT_ERR_INVALID, "mcrt_default_label_opts: null options");
    o->rule = MCRT_LABEL_TRACED; o->start_offset = -1.0f;
    return MCRT_OK;
}

// The two walks of the central beams (mcrt_label_frames, mcrt_transmit_frames) share their conditions and their prologue.  Everything is
// checked before anything is staged or launched.
struct BeamWalk { uint32_t n_frames, e0, e1; const float *pos, *dir; uint32_t rule; float start_offset; bool any_output; };
static int beam_walk_check(mcrt_ctx *c, const char *fn, const BeamWalk &w)
{
    if (!c->scene.have) return set_error(MCRT_ERR_INVALID, "%s: no scene uploaded", fn);
    if ((w.pos == nullptr) != (w.dir == nullptr)) return set_error(MCRT_ERR_INVALID, "%s: pos and dir go together (null %s)", fn, w.pos ? "dir" : "pos");
    if (!w.pos) {
        if (!c->d_pos) return set_error(MCRT_ERR_INVALID, "%s: no transducer set", fn);
        if (c->n_el != c->p.n_elements) return set_error(MCRT_ERR_INVALID, "%s: transducer has %u elements but params say %u", fn, c->n_el, c->p.n_elements);
        if (w.n_frames != 1) return set_error(MCRT_ERR_INVALID, "%s: the context's transducer is one pose: n_frames must be 1 (%u)", fn, w.n_frames);
    }
    if (w.e0 >= w.e1 || w.e1 > c->p.n_elements) return set_error(MCRT_ERR_INVALID, "%s: scan-line range [%u,%u) invalid for %u elements", fn, w.e0, w.e1, c->p.n_elements);
    if (!w.any_output) return set_error(MCRT_ERR_INVALID, "%s: no output asked for", fn);
    if (w.rule != MCRT_LABEL_TRACED && w.rule != MCRT_LABEL_GEOMETRIC) return set_error(MCRT_ERR_INVALID, "%s: unknown rule %u", fn, w.rule);
    if (!std::isfinite(w.start_offset) || w.start_offset == 0.0f) return set_error(MCRT_ERR_INVALID, "%s: start_offset must be finite and not 0 (%g)", fn, (double)w.start_offset);
    if (w.n_frames == 0) return set_error(MCRT_ERR_INVALID, "%s: n_frames must be 1..1024", fn);
    if (w.n_frames > 1024) return set_error(MCRT_ERR_LIMIT, "%s: n_frames must be 1..1024 (%u)", fn, w.n_frames);
    return MCRT_OK;
}
// The kernels walk with the lane walk's steps, so their traversal stack is sized as the traced pass sizes its own: lds_part entries in LDS,
// the tree's worst case beyond that in the context's overflow array (blocks workgroups of 64 lanes).  Stages the pose tables and fills what
// the kernels read of a FrameArgs (mcrt_kernels.h: LabelArgs, TransmitArgs).
static int beam_walk_args(mcrt_ctx *c, const BeamWalk &w, uint32_t blocks, uint32_t lds_part, mcrt::FrameArgs &a)
{
    const size_t ovf = c->scene.bvh4.max_stack > lds_part ? (size_t)(c->scene.bvh4.max_stack - lds_part) * blocks * 64 : 0;
    if (ovf > c->label_ovf.cap) { HIP_TRY(hipDeviceSynchronize()); HIP_TRY(c->label_ovf.alloc(ovf)); }      // (as ensure_work: an earlier pass may run on a stream the context has left)
    const float *dev[2] = { w.pos, w.dir };
    if (w.pos) MCRT_TRY(mcrt::stage_poses(c, (size_t)w.n_frames * c->p.n_elements, dev));
    if (c->scene.update_pending && c->scene.update_stream != c->stream) HIP_TRY(hipStreamWaitEvent(c->stream, c->scene.ev_update, 0));   // a scene update issued on another stream
    memset(&a, 0, sizeof a);
    a.nodes_walk = c->scene.d_nodes_walk; a.tris = c->scene.d_tris; a.tris_id = c->scene.d_tris_id; a.meshes = c->scene.d_meshes; a.mats = c->scene.d_mats; a.n_nodes = c->scene.bvh4.n_nodes;
    a.n_mat = c->scene.n_mat; a.n_mesh = c->scene.n_mesh; a.start_mat = c->scene.start_mat; a.pad_abs = c->scene.bvh.pad_abs;
    a.sx = c->scene.spacing[0]; a.sy = c->scene.spacing[1]; a.sz = c->scene.spacing[2];
    a.el_pos = w.pos ? dev[0] : c->d_pos; a.el_dir = w.pos ? dev[1] : c->d_dir; a.pose_stride = w.pos ? c->p.n_elements : 0u;
    a.e_begin = w.e0; a.ne_frame = w.e1 - w.e0; a.ne = (w.e1 - w.e0) * w.n_frames;
    a.row_thr = c->tab.d_row_thr; a.R = c->p.n_rows; a.thr_end = c->tab.thr_end; a.inv_row_dt = 1.0 / c->c.row_dt_us; a.row_dt = c->c.row_dt_us;
    a.max_travel = c->c.max_travel_us; a.sos_d = (double)c->p.speed_of_sound; a.freq = c->p.frequency;
    a.offs = w.start_offset < 0.0f ? c->p.ray_start_offset : w.start_offset;
    a.stack_ovf = c->label_ovf; a.error_flag = c->d_error;
    return MCRT_OK;
}

extern "C" int mcrt_label_frames(mcrt_ctx *c, uint32_t n_frames, uint32_t e0, uint32_t e1, const float *pos, const float *dir, const mcrt_label_opts *o,
                                 uint8_t *tissue_dev, int32_t *interface_dev, uint32_t *crossings_dev)
{
    CTX_TRY(c);
    static const char fn[] = "mcrt_label_frames";
    mcrt_label_opts d;
    mcrt_default_label_opts(&d);
    if (!o) o = &d;
    const BeamWalk w = { n_frames, e0, e1, pos, dir, o->rule, o->start_offset, tissue_dev || interface_dev || crossings_dev };
    MCRT_TRY(beam_walk_check(c, fn, w));
    if (c->scene.n_mat > 254) return set_error(MCRT_ERR_LIMIT, "%s: at most 254 materials fit a tissue byte (%u)", fn, c->scene.n_mat);
    mcrt::FrameArgs a;
    MCRT_TRY(beam_walk_args(c, w, mcrt::label_blocks((size_t)(e1 - e0) * n_frames), mcrt::label_stack_entries(), a));
    mcrt::LabelArgs l;
    l.tissue = tissue_dev; l.interface = interface_dev; l.crossings = crossings_dev; l.rule = o->rule; l.Ls = (float)(2.0 * c->p.depth_cm);
    HIP_TRY(mcrt::launch_label(a, l, c->stream));
    return MCRT_OK;
}

// ---- acoustic ground truth (the contract is in include/mcrt.h; mcrt_default_transmit_opts and mcrt_transmit_boundary are host code: mcrt_host.cpp) ----
extern "C" int mcrt_transmit_frames(mcrt_ctx *c, uint32_t n_frames, uint32_t e0, uint32_t e1, const float *pos, const float *dir, const mcrt_transmit_opts *o,
                                    float *transmit_dev, float *reflect_dev, uint32_t *crossings_dev)
{
    CTX_TRY(c);
    static const char fn[] = "mcrt_transmit_frames";
    mcrt_transmit_opts d;
    mcrt_default_transmit_opts(&d);
    if (!o) o = &d;
    const BeamWalk w = { n_frames, e0, e1, pos, dir, o->rule, o->start_offset, transmit_dev || reflect_dev || crossings_dev };
    MCRT_TRY(beam_walk_check(c, fn, w));
    if (o->mode != MCRT_TRANSMIT_TOTAL && o->mode != MCRT_TRANSMIT_BOUNDARIES) return set_error(MCRT_ERR_INVALID, "%s: unknown mode %u", fn, o->mode);
    if (((uintptr_t)transmit_dev | (uintptr_t)reflect_dev | (uintptr_t)crossings_dev) & 3u)
        return set_error(MCRT_ERR_INVALID, "%s: %s is not aligned to its 4-byte elements", fn, ((uintptr_t)transmit_dev & 3u) ? "transmit_dev" : ((uintptr_t)reflect_dev & 3u) ? "reflect_dev" : "crossings_dev");
    mcrt::FrameArgs a;
    MCRT_TRY(beam_walk_args(c, w, mcrt::transmit_blocks((size_t)(e1 - e0) * n_frames), mcrt::transmit_stack_entries(), a));
    mcrt::TransmitArgs l;
    l.transmit = transmit_dev; l.reflect = reflect_dev; l.crossings = crossings_dev; l.rule = o->rule; l.mode = o->mode; l.Ls = (float)(2.0 * c->p.depth_cm);
    HIP_TRY(mcrt::launch_transmit(a, l, c->stream));
    return MCRT_OK;
}
