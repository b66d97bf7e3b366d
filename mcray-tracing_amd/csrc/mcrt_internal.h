// mcrt_internal.h -- shared between the translation units of libmcrt_hip.so
#pragma once
#include <stdint.h>

#define MCRT_BVH_MAX_DEPTH 32      // deepest leaf the builder may emit == traversal stack entries per lane
#define MCRT_STACK 64              // BVH4 traversal stack entries per path (LDS); trees needing more are rejected at upload
#define MCRT_KSPLIT_DEFAULT 262144 // work items a small bounce of k_trace is cut into (pieces x rays); one 128 x 1024 frame at a time is cut in two
#ifndef MCRT_KSPLIT_MAX
#define MCRT_KSPLIT_MAX 1048576
#endif
#define MCRT_GROUPS_DEFAULT 1        // independent scan-line groups a frame is traced as (their kernels overlap)
#define MCRT_SIDE_STREAMS 4         // streams k_march launches rotate over
#define MCRT_SIDE_STREAMS_DEFAULT 0       // 0: by the size of the pass -- one side stream, two from MCRT_SIDE_STREAMS_TWO_FROM paths
#define MCRT_SIDE_STREAMS_TWO_FROM 5242880u   // (40 frames of 128 x 1024 paths.  One box, ms per B-mode frame with one / two side streams: 20 frames 0.338 / 0.350, 32: 0.311 / 0.314, 48: 0.306 / 0.298,
                                              //  64: 0.300 / 0.291, 96: 0.298 / 0.282, 128: 0.295 / 0.283 (three: 0.287; at 20 frames 0.446).  In a large pass the accumulations, stretched threefold beside the
                                              //  walks, are the longer chain: two of them side by side shorten it; in a small pass the second one takes the walk's tail away.)
#define MCRT_LBVH_LEAF 1             // device builder: triangles per leaf (1..4); measured best at 1, like the SAH builder's own leaves
#define MCRT_XCDS 8                   // XCDs of the MI355X = sub-queues of a bounce's ray queue (see k_trace)
#define MCRT_CURSOR_STRIDE 64         // uint32 between two queue cursors: 256 B, so they sit in different L2 lines / channels
#define MCRT_XCD_MIN_ITEMS 262144     // bounces with fewer work items use a single queue
#define MCRT_PACKET_MASK_DEFAULT 2u   // bounces (bit b) walked a wavefront per ray packet (k_trace_packet): bounce 1 -- every pass size from two frames up and every BASELINE
                                      // configuration gains 0.3-6 % (profiles/round5/exp_packet.txt); bounce 2 is a wash, later bounces lose (packet_count_*.json)
#define MCRT_PACKET_FROM 262144u      // ... in passes of at least this many paths (one 128 x 1024 frame at a time keeps the lane walk: its launches are cut into pieces, 1.624 vs 1.634 ms)
#define MCRT_BEAM_FROM 2097152u        // bounce 1 by beams (mcrt_beam.hip) in passes of at least this many paths (16 frames of 128 x 1024), where bounce 1 would run as packets: the stage has fixed parts
                                       // (one collection per beam, the bounds, seven launches) -- against packets, ms per frame at 6 / 8 / 12 / 16 / 20 / 128 frames: 0.520 / 0.446 / 0.377 / 0.341 / 0.319 / 0.252
                                       // against 0.511 / 0.441 / 0.370 / 0.341 / 0.320 / 0.272 (profiles/beam/small_pass.txt)
#define MCRT_BEAM_LAST_DEFAULT 4u       // the last bounce run by beams (mcrt_beam.hip): bounces 2 .. 4 by the triangle their rays left, tested in the beam order (MCRT_BEAM_ORDER_DEFAULT).  ms per frame of the
                                       // headline pass, min / median / max of seven alternating runs on one box (profiles/beam_order_fast/ab_configs.txt): bounces 2-3 ordered 0.2216 / 0.2245 / 0.2261,
                                       // bounces 2-4 ordered at 64 slots per scan-line 0.2103 / 0.2127 / 0.2157 -- 0.0118 lower, spreads <= 0.0054, every run below.  With bounce 2 in queue order
                                       // (MCRT_BEAM_ORDER=0x18) 0.2134 / 0.2179 / 0.2230.  (Before the order was cheap bounce 4 gained 0.0079 inside a spread of 0.0089: DESIGN.md A.12, A.13)
#define MCRT_BEAM_DEEP_FROM 4194304u   // ... in passes of at least this many paths (32 frames of 128 x 1024): ms per frame without bounces >= 2 by beams / with bounces 2-3 ordered, seven alternating runs,
                                       // at 32 frames 0.2808 / 0.2822 / 0.2831 against 0.2675 / 0.2693 / 0.2726 (0.0129 lower, spreads <= 0.0052, every run below); at 48 frames 0.2681 against 0.2478 at the
                                       // median.  A 20-frame pass lost 4-14 % with the dearer order (profiles/beam_order); nothing was measured between 20 and 32 frames
#define MCRT_BEAM_B4_FROM 16777216u    // bounces >= 4 by beams only in passes of at least this many paths (128 frames of 128 x 1024), a threshold of their own: bounces 2-3 / 2-4 ordered, 64 slots, seven
                                       // alternating runs, median ms per frame at 48 / 64 / 96 / 128 frames 0.2488 / 0.2399 / 0.2267 / 0.2227 against 0.2472 / 0.2331 / 0.2212 / 0.2127.  At 64 and 96 frames
                                       // every run with bounce 4 is below every run without, but the gains (0.0068, 0.0055) are not beyond the larger spread (0.0170, 0.0058): by the rule only 128 passes
#define MCRT_BEAM_ORDER_DEFAULT 0x1cu   // bounces whose rays k_beam_test reads through the beam order (a mask; only where the bounce runs by beams): bounces 2, 3 and 4.  Bounce 2 ordered, seven alternating
                                       // runs: 0.2276 / 0.2302 / 0.2316 -> 0.2216 / 0.2245 / 0.2261 (0.0057 lower, spreads <= 0.0044, every run below) since k_beam_rank reads k_shade's beam word and
                                       // k_beam_scan runs in workgroups of 256 (rank + scan + place 1111 -> 463 us at bounce 3).  Bounce 1 ordered (1.2 beams per wavefront) did not pay for the extra pass
                                       // over its rays: 0.2286 / 0.2301 / 0.2332 against 0.2250 / 0.2269 / 0.2282 (profiles/beam_order/ab_configs.txt; not measured again)
#define MCRT_BEAM_GROUPS_PER_LINE 64u  // slots of the group table per scan-line (rounded up to a power of two in all): the headline pass of 128 x 1024 x 128 paths claims 6 / 20 / 30 slots per
                                       // scan-line at bounces 2 / 3 / 4 with 32 (profiles/beam_deep/debug_counters.txt), and bounce 4's table was full.  64 cost bounces 2-3 nothing: 0.2216 / 0.2245 / 0.2261
                                       // at 32 against 0.2221 / 0.2227 / 0.2269 (profiles/beam_order_fast/ab_configs.txt); a group that finds no slot among MCRT_BEAM_PROBES is walked
#define MCRT_BEAM_LISTS_PER_GROUP 1u   // lists of the pool per slot of the table: nearly every group has one dominant axis and sign
#define MCRT_BEAM_CAP_DEFAULT 512u     // candidates a beam's list holds (bounce 1 by beams, mcrt_beam.hip), at most MCRT_BEAM_CAP_MAX
#define MCRT_BEAM_NEAR_DEFAULT 512u    // ... of which the first pass over all rays tests this many; fewer than the capacity: what is undecided then goes on as a compact queue through a second pass
#define MCRT_BEAM_SPREAD 0.25f         // a beam whose slopes spread further than this is refused: its rays are walked
#define MCRT_BEAM_SAMPLE_FROM 4194304u // passes of at least this many paths take every MCRT_BEAM_SAMPLE_STRIDE-th packet of the queue as the sample for the beams' bounds
#define MCRT_BEAM_SAMPLE_STRIDE 16u    // (a ray outside its beam's bounds is a leftover: the sample only has to be large, and 32 frames' worth of a scan-line still give a beam 2000 rays;
                                       //  which packet of the 16 is taken is hashed per wavefront, k_beam_bounds)
#define MCRT_PATH_MAX_DEFAULT 655360u  // passes of at most this many paths take the latency form (k_path: one launch for all bounces): five 128 x 1024 frames (ms per frame at 1 / 2 / 3 / 4 / 5 / 6 frames: 0.87 / 0.77 / 0.72 / 0.69 / 0.67 / 0.65 against the staged 1.62 / 1.12 / 0.88 / 0.76 / 0.68 / 0.60)
#define MCRT_PATH_GROUPS_DEFAULT 2u     // ... traced as this many scan-line groups on their own streams (a group's k_march runs beside the other groups' slowest wavefronts)
#define MCRT_MAX_ROWS 2048
#define MCRT_MAX_BOUNCES 16
#define MCRT_STATS_WORDS (256 + 2560)  // the context's counter block: 8 statistics, 248 stamps (mcrt_debug_stamps), 10 x 256 tail histograms (mcrt_debug_tail_histograms)

#define MCRT_TRI_PIECES 3             // 16-byte pieces of the walk's triangle record: v0|id, v1|mesh, v2|edge tolerance (48 B; the plane is rebuilt from the vertices)

namespace mcrt {
int set_error(int code, const char *fmt, ...);
// A TUNING knob from the environment: nullptr unless the process runs with MCRT_TUNING=1 (mcrt_host.cpp).  The library is meant to be
// linked into someone else's program: left alone it reads ONE environment variable, once; the knobs themselves are
// for tools/ and tests/, which set MCRT_TUNING=1 beside the knob they turn.
const char *tuning_env(const char *name);
}
#ifdef MCRT_H
// mcrt_api.cpp <-> mcrt_group.cpp (what crosses between mcrt_api.cpp, mcrt_trace.cpp and mcrt_image.cpp is in mcrt_ctx.h): a scene (or a triangle update) installed with a tree the HOST builder has already made of exactly
// these triangles -- a group builds once on the calling thread and every rank copies and uploads (the device builder ignores it)
namespace mcrt {
struct HostTree { const mcrt_bvh *bvh; const mcrt_bvh4 *bvh4; };
int ctx_bvh_builder(const mcrt_ctx *c);
int upload_scene_with_tree(mcrt_ctx *c, const float *tri, const uint32_t *tri_mesh, uint32_t n_tri, const mcrt_mesh *meshes, uint32_t n_mesh,
                           const float *mats, uint32_t n_mat, uint32_t start_mat, const float spacing[3], const HostTree *pre);
int update_triangles_with_tree(mcrt_ctx *c, const float *tri, uint32_t n_tri, const HostTree *pre);
// mcrt_host.cpp: the conditions on a sweep and a grid that mcrt_volume_maps and the two device entry points share
int volume_check(const char *fn, const mcrt_sweep *sw, const mcrt_volume_grid *g);
// mcrt_host.cpp: the ranges of mcrt_autogain_opts, which mcrt_autogain_curve and mcrt_autogain_frames share
int autogain_check(const char *fn, const mcrt_autogain_opts *o);
// mcrt_host.cpp: the ranges of mcrt_flow_opts, which mcrt_flow_nyquist and mcrt_flow_frames share
int flow_check(const char *fn, const mcrt_flow_opts *o);
// mcrt_host.cpp: the ranges of mcrt_spectral_opts, which mcrt_spectral_series_frames and mcrt_spectral_frames share
int spectral_check(const char *fn, const mcrt_spectral_opts *o);
// mcrt_host.cpp: the ranges of mcrt_strain_opts, which mcrt_strain_compress_frames and mcrt_strain_frames share
int strain_check(const char *fn, const mcrt_strain_opts *o);
// mcrt_host.cpp: the ranges of mcrt_shear_opts against a stack of E scan-lines of R rows, which mcrt_shear_wave_frames and mcrt_shear_speed_frames share
int shear_check(const char *fn, const mcrt_shear_opts *o, uint32_t E, uint32_t R);
// mcrt_host.cpp: the ranges of mcrt_mmode_opts (mcrt_mmode_lines_frames) and of mcrt_mmode_display_opts against lines of T pulses and R rows (mcrt_mmode_picture_frames)
int mmode_check(const char *fn, const mcrt_mmode_opts *o);
int mmode_display_check(const char *fn, const mcrt_mmode_display_opts *o, uint32_t T, uint32_t R);
}
#endif
