// mcrt_ctx.h -- private to the host side of the C-ABI: struct mcrt_ctx, the types it is made of, and what crosses between mcrt_api.cpp
// (context, params, scene, texture, transducer, memory, instrumentation), mcrt_trace.cpp (the traced pass) and mcrt_image.cpp (the image
// stages).  The context's fields are grouped by who owns them; a function's first lines show which group it touches.
#pragma once
#include "../../include/mcrt.h"
#include "mcrt_internal.h"
#include "mcrt_hip.h"

#include <cstdlib>
#include <cstring>
#include <vector>

#define CTX_TRY(ctx) do { if (!(ctx)) return mcrt::set_error(MCRT_ERR_INVALID, "null context"); HIP_TRY(hipSetDevice((ctx)->device)); } while (0)

struct Consts {   // main.cpp:23-37, rfimage.h:48-51,178-180 evaluated at run time (derive_consts)
    float axial_res_f; double axial_res_mm, time_step_us, row_dt_us, max_travel_us; uint32_t axial_res_um, max_rows;
};

// Work set of ONE wavefront pipeline: path state, queues, rays, closest-hit words, march records (segments on request), and the
// streams it runs on (k_march of bounce b runs on a low-priority side stream beside k_trace of bounce b+1).  A context can own
// several, to trace the scan-lines of a pass as independent groups on separate streams (MCRT_GROUPS, a tuning knob: one group
// measured best).
struct PathBufs {   // sized for `paths` paths of `depth` bounces
    Buf<float4> st0, st1, st2, mrec;
    Buf<unsigned long long> key0, key1;
    Buf<uint32_t> q, counts, seg_count, cursors, from_tri;
    size_t paths = 0; uint32_t depth = 0;
};
// bounces by beams (mcrt_beam.hip; BeamArgs in mcrt_kernels.h): the beams' reduction words, records and candidate lists, the group table of the bounces >= 2,
// every bounce's counters, and the counts and cursors the leftovers are walked with.  Sized for `beams` beams, `lists` lists of `cap` candidates and `groups`
// slots; reused from bounce to bounce (stream order).  The beam order (MCRT_BEAM_ORDER; made only where a bounce is ordered): every ray's beam and rank, the beams'
// counters and segment bases (beams + 1: the pseudo-beam of the rays without a beam), and the order itself, `order_rays` rays and 64 pad words per segment.
struct BeamBufs {
    Buf<uint32_t> red, rec, lcount, l_counts, l_cursors;
    Buf<uint4> list;
    Buf<uint32_t> hot;                        // the entries' planes and padded bounds, beside `list` (BeamArgs::hot)
    Buf<unsigned long long> gkey;
    Buf<uint32_t> rbeam, rrank, ocount, obase, order;
    uint32_t beams = 0, lists = 0, groups = 0, cap = 0, order_beams = 0;
    size_t order_rays = 0;
};
struct Work {
    Stream stream, side[MCRT_SIDE_STREAMS];   // k_march of bounce b runs on side[b % n] (n: Plan::sides)
    Event ev_bounce[MCRT_MAX_BOUNCES], ev_join[MCRT_SIDE_STREAMS], ev_done;
    Buf<int> stack_ovf;                       // traversal-stack overflow of THIS work set's walk (its launches run beside the other groups')
    Buf<mcrt_segment> segs;                   // [paths][depth], only for the callers that ask for segments
    Buf<int32_t> hits;                        // [paths][depth], only for the callers that ask for hit indices
    PathBufs b;
    BeamBufs beam;
};

// tuning knobs from the environment, read ONCE at mcrt_create (never on the frame path) -- and only in a process started with
// MCRT_TUNING=1 (mcrt::tuning_env): linked into someone else's program the library has its defaults and nothing else.
#define MCRT_SPECKLE_FUSE_DEFAULT 2u
#define MCRT_AUTOGAIN_COPIES_DEFAULT 1u
#define AUTOGAIN_HIST_WORDS (2048u * 4096u)        // 32 MiB: the histograms of 4096 (frame, band) pairs -- 136 frames of 465 rows in bands of 16
struct Knobs {
    uint32_t ksplit_limit = MCRT_KSPLIT_DEFAULT, trace_blocks = 0, trace_blocks_wide = 0, wide_from = 0 /* 0: the kernels' own default */, wide_max_tree_mb = 128, groups = MCRT_GROUPS_DEFAULT, march_streams = MCRT_SIDE_STREAMS_DEFAULT, march_blocks = 0;   // march_blocks 0: launch_march picks
    bool no_overlap = false, no_priority = false, no_fast_div = false, no_lean = false;
    uint32_t path_groups = MCRT_PATH_GROUPS_DEFAULT;   // ... as this many scan-line groups on their own streams: a group's accumulation runs beside the other groups' last walks
    uint32_t path_max = MCRT_PATH_MAX_DEFAULT;    // passes of at most this many paths run as ONE launch that carries every path through all of its bounces (k_path: the latency form)
    uint32_t packet_mask = MCRT_PACKET_MASK_DEFAULT, packet_from = MCRT_PACKET_FROM;   // bit b: bounce b is walked by k_trace_packet (one wavefront per packet of 64 queue neighbours), in passes of at least packet_from paths
    bool retire_late = true;                   // MCRT_RETIRE_LATE=0: paths past the image are traced to their end, as before (FrameArgs::retire_late)
    bool fold_b0 = false;                      // MCRT_FOLD_B0=1: bounce 0 of a silent start medium is accumulated by k_shade itself (FrameArgs::fold_b0).  Bit-identical, one launch and
                                               // 48 B per path less, and no faster on the MI355X (profiles/retire_fold): off until a pass is found that it helps
    uint32_t beam_b1 = 1;                      // MCRT_BEAM_B1=0|1|2: bounce 1 of a pass with one probe pose tests each scan-line's rays against its beams' triangles (mcrt_beam.hip) -- 1: where it
                                               // would run as packets, 2: in every staged pass, 0: never
    uint32_t beam_from = MCRT_BEAM_FROM;       // MCRT_BEAM_FROM: ... in passes of at least this many paths (MCRT_BEAM_B1=1)
    uint32_t beam_last = MCRT_BEAM_LAST_DEFAULT;   // MCRT_BEAM_LAST: the last bounce run by beams (1: bounce 1 alone); the bounces 2 .. beam_last of a pass with one probe pose group their rays by the triangle they left
    uint32_t beam_deep_from = MCRT_BEAM_DEEP_FROM; // MCRT_BEAM_DEEP_FROM: ... in passes of at least this many paths (MCRT_BEAM_B1=1; 2 takes them in every staged pass, 0 in none)
    uint32_t beam_b4_from = MCRT_BEAM_B4_FROM; // MCRT_BEAM_B4_FROM: bounces >= 4 of those only in passes of at least this many paths (a threshold of their own: their tables are fuller and their queues shorter)
    uint32_t beam_groups = 0;                  // MCRT_BEAM_GROUPS: slots of the group table (rounded down to a power of two); 0: MCRT_BEAM_GROUPS_PER_LINE per scan-line
    uint32_t beam_cap = MCRT_BEAM_CAP_DEFAULT, beam_near = MCRT_BEAM_NEAR_DEFAULT;   // MCRT_BEAM_CAP, MCRT_BEAM_NEAR: candidates a beam's list holds, and how many of them the first pass tests
    uint32_t beam_order = MCRT_BEAM_ORDER_DEFAULT;   // MCRT_BEAM_ORDER: a mask of bounces -- bit b: where bounce b runs by beams, k_beam_test reads its rays through a permutation of the queue grouped by beam
    bool beam_pairs = false;                   // MCRT_BEAM_PAIRS=1: k_beam_test counts the (wavefront, beam) pairs it meets (mcrt_debug_beam_order)
    bool render_row_tile = false;              // MCRT_RENDER_ROW_TILE=1: a wavefront of k_render owns 64 pixels of one picture row in place of an 8 x 8 tile (RenderArgs::row_tile)
    uint32_t speckle_fuse = MCRT_SPECKLE_FUSE_DEFAULT;   // MCRT_SPECKLE_FUSE=2|4: iterations of mcrt_speckle_frames per launch of k_srad; 4 is faster for one frame, 2 for a stack
    uint32_t autogain_copies = MCRT_AUTOGAIN_COPIES_DEFAULT;   // MCRT_AUTOGAIN_COPIES=1|4: LDS histograms per workgroup of k_autogain_hist; 4 lost
    uint32_t autogain_hist_words = AUTOGAIN_HIST_WORDS;   // MCRT_AUTOGAIN_HIST_KB: the bound of the histogram scratch [KiB] (tests: a small one walks a small pass in chunks)
    bool test_hooks = false;                   // MCRT_TEST_HOOKS: mcrt_debug_set_error may poison the context (tests only)
};

// A float table [R][n] that a caller hands over as HOST memory with every call, on the device as [n][R] (n == 1: as it is), uploaded only
// when its bits or its shape differ from what is there.  put() is the whole contract: the device buffer, the pinned staging and the event
// are made on first use, all or none; the comparison is bitwise, on the caller's layout; the staging buffer is rewritten only after the
// previous copy's event; the table has no shape until its copy is enqueued; nothing else waits for the device; and the caller's array is
// free the moment put() returns.
// B such tables at once (the axial taps of mcrt_convolve_bands_frames): the caller's [B][R][n] on the device as [B][n][R].
struct StagedTable : Staging {
    std::vector<float> on_dev; uint32_t key[3] = { 0, 0, 0 };   // what the device holds (or is about to): the caller's bits, and R, n, B
    int put(const float *src, uint32_t R, uint32_t n, size_t room, hipStream_t st, uint32_t B = 1)   // room: floats of the largest table this one may be given
    {
        const size_t one = (size_t)n * R, len = one * B;
        if (key[0] == R && key[1] == n && key[2] == B && !memcmp(src, on_dev.data(), 4 * len)) return MCRT_OK;
        float *h = nullptr;
        MCRT_TRY(begin(room, st, &h));
        on_dev.resize(room);
        for (uint32_t b = 0; b < B; b++)
            for (uint32_t r = 0; r < R; r++)
                for (uint32_t k = 0; k < n; k++) h[b * one + (size_t)k * R + r] = src[b * one + (size_t)r * n + k];
        key[0] = key[1] = key[2] = 0;
        MCRT_TRY(commit(len, st));
        memcpy(on_dev.data(), src, 4 * len);
        key[0] = R; key[1] = n; key[2] = B;
        return MCRT_OK;
    }
};

// A host table of 32-bit words of any type (gates, integer rates, 64-bit phases as word pairs, floats) on the device as it is, under
// Staging's rules and StagedTable's comparison: uploaded only when its bits or its length differ from what is there.  The buffers only
// ever grow.
struct StagedWords : Staging {
    std::vector<uint32_t> on_dev; bool valid = false;
    int put(const void *src, size_t words, hipStream_t st)
    {
        if (valid && on_dev.size() == words && !memcmp(src, on_dev.data(), 4 * words)) return MCRT_OK;
        float *h = nullptr;
        MCRT_TRY(begin(words > dev.cap ? words : dev.cap, st, &h));
        valid = false;
        memcpy(h, src, 4 * words);
        MCRT_TRY(commit(words, st));
        on_dev.resize(words);
        memcpy(on_dev.data(), src, 4 * words);
        valid = true;
        return MCRT_OK;
    }
    template <class T> const T *as() const { return (const T *)dev.p; }
};

// Maps that a stage's kernels gather through, made on the host from a geometry and kept on the device under that geometry's key: the
// scan-conversion maps [N][2][n_pad] (per view the column map, then the row map) and the volume maps [3][n_pad] (plane, column, row),
// n_pad = the output points rounded up to 256 floats and zero-padded, so every map is 16-byte aligned.  The key is the bytes the caller
// appended, field by field (no struct padding), and is compared byte for byte: -0.0 and 0.0 are two geometries, and so are (30 mm, 1 rad)
// and (29.999999 mm, 2 rad), which a key folded into one double, radius_mm * 1e6 + total_angle, once made the same.  The most recently
// used `slots` geometries stay; a slot's buffer only ever grows.  used: the slot's last call, 0 = empty.
struct MapCache {
    struct Key {
        std::vector<unsigned char> bytes;
        template <class T> Key &add(const T &v) { return add(&v, sizeof v); }
        Key &add(const void *p, size_t n) { bytes.insert(bytes.end(), (const unsigned char *)p, (const unsigned char *)p + n); return *this; }
    };
    struct Slot { Buf<float> d; std::vector<unsigned char> key; uint64_t used = 0; };
    std::vector<Slot> slot; uint64_t clock = 0;
    explicit MapCache(size_t slots) : slot(slots) {}
    static size_t pad(size_t n) { return (n + 255u) & ~(size_t)255u; }
    // the maps of `key` on the device: the slot that holds them, or the least recently used one (the lowest of equals: empty slots are
    // taken in order) refilled with the n floats that fill(std::vector<float> &), given them zeroed, makes on the host
    template <class Fill> int get(const Key &key, size_t n, hipStream_t st, Fill fill, const float **maps)
    {
        Slot *lru = &slot[0];
        for (Slot &s : slot) {
            if (s.used && s.key == key.bytes) { s.used = ++clock; *maps = s.d; return MCRT_OK; }
            if (s.used < lru->used) lru = &s;
        }
        std::vector<float> m(n, 0.0f);
        MCRT_TRY(fill(m));                                   // (first: a failure leaves the cache as it was)
        HIP_TRY(hipStreamSynchronize(st));                   // (the evicted maps' last gather)
        lru->used = 0;                                       // (no geometry until the maps are on the device)
        HIP_TRY(lru->d.grow(n));
        HIP_TRY(hipMemcpy(lru->d, m.data(), n * 4, hipMemcpyHostToDevice));
        lru->key = key.bytes; lru->used = ++clock;
        *maps = lru->d;
        return MCRT_OK;
    }
};

struct TimedLaunch { Event start, end; int kind = 0; };   // kind 0: the walk (k_trace*, k_path), 1: k_shade, 2: k_march

// the uploaded scene: the trees, the triangles as the builder left them and as the walk reads them, the meshes and materials
struct Scene {
    bool have = false;
    mcrt_bvh bvh{};
    mcrt_bvh4 bvh4{};
    Buf<float4> d_nodes, d_tris, d_mats;
    mcrt_bvh4_node *walked_nodes = nullptr; bool walked_stale = true;   // host copy of the tree as the lane walk sees it (mcrt_get_bvh4)
    Buf<uint4> d_nodes_walk;                              // the walk's child-transposed half-float nodes
    Buf<uint4> d_meshes;
    Buf<uint32_t> d_tri_slot;
    Buf<float4> d_tris_id;                                // the triangle records in id order (refresh_soa)
    uint32_t n_mesh = 0, n_mat = 0, start_mat = 0;
    bool start_silent = false;                            // the start material has mu0 == sigma == 0: its segments' step echoes are +0 in a finite texture (k_march's `silent`)
    int builder = MCRT_BVH_HOST_SAH; bool host_bvh_stale = false;   // device-built tree: host copies are downloaded on demand
    std::vector<uint32_t> tri_mesh;   // per-triangle mesh index of the uploaded scene (for mcrt_update_triangles)
    float lo[3] = { 0, 0, 0 }, hi[3] = { 0, 0, 0 };
    float spacing[3] = { 1, 1, 1 };
    Event ev_update; hipStream_t update_stream = nullptr; bool update_pending = false;   // the last scene update's device work (refresh_soa), for traces issued on ANOTHER stream
    ~Scene() { free(walked_nodes); mcrt_free_bvh(&bvh); mcrt_free_bvh4(&bvh4); }   // (the HIP resources release themselves)
};
// what prepare_tables keeps in step with the params and the scene
struct Tables {
    // row thresholds (exact replacement of the per-echo double division) and the verified fast division by tex_res
    Buf<double> d_row_thr; uint32_t thr_rows = 0; double thr_dt = 0.0, thr_end = 0.0;   // thr_end: the table's last entry, the first time past the image
    float verified_res = 0.0f; bool fast_div = false, fast_div_all = false;
    // per-material table of k_march (depends on the materials, the axial step and the frequency)
    Buf<float4> d_mtab; float mtab_key[2] = { 0.0f, 0.0f }; bool mtab_valid = false;
};
struct Accumulators {
    Buf<long long> d_acc; Buf<uint32_t> d_flags;
    uint32_t clean_ne = 0, clean_rows = 0;   // bins known to be all-zero for this shape (k_finalize leaves them so)
};
// the image stages' state (mcrt_image.cpp, which reads nothing else of a context but its device, its stream, p.speed_of_sound and c.max_travel_us)
struct ImageStages {
    // scan-conversion maps: of the plain geometry (mcrt_scan_convert_frames, mcrt_bmode_frames; one unsteered view), of a steer list (spatial
    // compounding: mcrt_compound_frames, mcrt_bmode_compound_frames) and of the grids of volume imaging (mcrt_volume_frames,
    // mcrt_bmode_volume_frames: a volume and three orthogonal cuts per frame), each in a cache of its own so that alternating calls do not evict each other
    MapCache maps{ 1 }, cmaps{ 1 }, vmaps{ 4 };
    Buf<float> d_tmp;                          // scratch of a pass: mcrt_convolve's, the grey levels of B-mode, the transposition of export / import
    // B-mode display (mcrt_bmode_frames): the peaks of a pass [65536], and the TGC factors [R] of the last curve
    Buf<float> d_disp; StagedTable tgc;
    // focal zones (mcrt_convolve_frames_depth): the lateral taps [n_lat][R], and slice thickness (mcrt_elevation_frames): the elevation weights
    // [K][R] (room for MCRT_MAX_ROWS x 32 each).  Two tables: a frame uses both in turn, and one shared buffer would upload both on every frame
    StagedTable lat_rows, elev_rows;
    // frequency compounding (mcrt_convolve_bands_frames, mcrt_band_fold_frames): the axial taps [B][n_ax][R] (room for 8 x 16 x MCRT_MAX_ROWS) and
    // the band weights [B][R] (room for MCRT_MAX_ROWS x 8), tables of their own for the same reason
    StagedTable band_ax, band_w;
    // receiver noise (mcrt_noise_frames): the gain of every transducer element [E] of the last table (room for the largest E so far); the peaks are d_disp's
    StagedTable gain;
    // colour Doppler (mcrt_flow_frames): the phasors [n_labels][E][2] and the true velocities [n_labels][E] of the last tables, the
    // per-sample autocorrelation [F][3][E][R] of the largest call so far; (mcrt_colour_frames): the last colour table, 256 packed entries
    StagedTable flow_phasor, flow_truth, colour_lut; Buf<float> d_flow;
    // spectral Doppler: the last host tables of mcrt_spectral_series_frames (the rotor [4096][2], gates [n_gates][3], weight [G], rate
    // [n_gates][G], phase [T] as word pairs) and of mcrt_spectral_frames (window [N]; the twiddles of N = 32 << i, each made once), and
    // the gates' peaks of a mcrt_sonogram_frames without a peak_dev
    StagedWords spec_rotor, spec_gates, spec_weight, spec_rate, spec_phase, spec_window, spec_tw[5]; Buf<float> d_sono_peak;
    // strain elastography: the last strain table [n_labels] of mcrt_strain_compress_frames (its rotor is spec_rotor), the displacement
    // [F][E][R] of the largest mcrt_strain_frames so far that gave no disp_dev, and the last colour table of mcrt_elastogram_frames
    StagedWords strain_eps; Buf<float> d_strain_disp; StagedTable elasto_lut;
    // shear-wave elastography: the last host tables of mcrt_shear_wave_frames (the slownesses [n_labels] as word pairs, the true speeds
    // [n_labels], the pitches [R], the time profile [n_shape] and the decay [n_amp]; its rotor is spec_rotor) and of mcrt_shear_speed_frames
    // (the pitches in mm [R]), and the arrival ticks [F][E][R] of the largest mcrt_shear_wave_frames so far
    StagedWords shear_slow, shear_speed, shear_pitch, shear_shape, shear_amp, shear_pitch_mm; Buf<long long> d_shear_arrival;
    // M-mode: the last host tables of mcrt_mmode_lines_frames (the lines [n_lines][2], the dilations [n_labels], the waveform [T] and the
    // bulk motion [T]; its rotor is spec_rotor) and of mcrt_mmode_picture_frames (the depth table: first taps [H] and weights [H]), and
    // the lines' peaks of a mcrt_mmode_picture_frames without a peak_dev
    StagedWords mmode_lines, mmode_dil, mmode_w, mmode_bulk, mmode_idx, mmode_wt; Buf<float> d_mmode_peak;
    // automatic gain (mcrt_autogain_frames): the histograms of a chunk of frames [frames][n_bands][2048], at most AUTOGAIN_HIST_WORDS, and the row
    // gains [n_frames][R] of the largest call so far that gave no gain_dev
    Buf<uint32_t> d_aghist; Buf<float> d_aggain;
    // freehand reconstruction (mcrt_recon_frames): the accumulators of the largest grid so far, n sums (8 B each), then n counts (4 B each)
    Buf<unsigned long long> d_recon;
    // freehand label reconstruction (mcrt_recon_label_frames): the vote table of the largest call so far, voxels x n_labels words
    Buf<uint32_t> d_votes;
};
struct Instrumentation {
    Buf<unsigned long long> d_stats; bool stats_on = false;
    bool timing_on = false; int timing_level = 0;       // 1: the walk's launches are bracketed by HIP events; 2: k_shade's and k_march's too
    std::vector<TimedLaunch> ev; size_t ev_used = 0;
    uint32_t last_beam_mask = 0;                        // bit b: the last pass ran bounce b by beams (mcrt_debug_beam, mcrt_debug_beam_bounce)
    uint32_t last_beam_order = 0;                       // ... and read its rays through the beam order (mcrt_debug_beam_order)
    bool last_beam_far = false;                         // ... and its leftovers are those of the second pass over the lists
    uint32_t last_beam_b1 = 0, last_beam_groups = 0, last_beam_cap = 0, last_beam_near = 0, last_beam_depth = 0;   // ... its bounce-1 beams, the slots of its group table, its lists' capacity and first pass, the bounces it launched (mcrt_debug_beam_records)
    float last_lean_bound = 0.0f; uint32_t last_march_rows = 0;   // what the last frame's kernels were given (mcrt_debug_fast_paths)
};

struct mcrt_ctx {
    int device = 0; uint32_t n_cu = 256;
    Knobs knobs;
    Stream own_stream; hipStream_t stream = nullptr;
    std::vector<Work> work;                               // one per concurrent scan-line group (see plan_pass); never moves once a pass holds pointers into it
    Event ev_start;
    mcrt_params p{};
    Consts c{};
    Buf<uint32_t> d_error;
    Scene scene;
    Buf<float2> d_tex; uint32_t tex_n = 0; bool tex_finite = false;
    Buf<float> d_pos, d_dir; uint32_t n_el = 0;          // the transducer
    Buf<int> label_ovf;                                   // traversal-stack overflow of k_label's walk (mcrt_label_frames)
    Staging pose_stage[2];                                // per-frame probe poses handed over as host memory: positions, directions (mcrt::stage_poses)
    Tables tab;
    Accumulators acc;
    ImageStages img;
    Instrumentation ins;
};

namespace mcrt {
int check_device_error(mcrt_ctx *c);   // mcrt_api.cpp: the device's error word, read and cleared (the stream is idle)
int stage_poses(mcrt_ctx *c, size_t lines, const float *dev[2]);   // mcrt_trace.cpp: host pose tables [lines][3] through pose_stage, positions then directions; dev[k] becomes the device's
}
