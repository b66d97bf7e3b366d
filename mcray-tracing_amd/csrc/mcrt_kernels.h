// mcrt_kernels.h -- kernel argument blocks and launchers: the interface between the host C++ (mcrt_api.cpp, mcrt_trace.cpp, mcrt_image.cpp, mcrt_group.cpp; mcrt_hip.h owns their HIP resources) and the gfx950 kernels.
//
// The hot path's kernels, one translation unit per pipeline stage, each kernel beside its launcher:
//   mcrt_walk.hip    k_trace_lane / k_trace_lane_wide (closest hit, one lane per ray), k_trace_packet (one wavefront per ray packet),
//                    k_nodes_walk / k_nodes_walk_decode (the walk's 64-byte nodes)
//   mcrt_beam.hip    k_beam_clear / bounds / rank / scan / place / collect / test / gather / scatter (bounces 1 .. MCRT_BEAM_LAST of a pass with one probe pose: the rays of a group against one beam's triangles)
//   mcrt_shade.hip   k_init (the first ray of every path), k_shade (interface physics of a bounce, survivors compacted into the next queue),
//                    k_shade_fold (k_shade of bounce 0 with the boundary echoes of a silent start medium added in the kernel)
//   mcrt_path.hip    k_path (the latency form: every bounce of every path in one launch)
//   mcrt_march.hip   k_march (RF accumulation of the segments), k_material_table
//   mcrt_post.hip    k_finalize, k_clear_flags, k_conv_* (k_conv_lateral_rows: focal zones, k_conv_axial_bands: frequency compounding), k_elevation (slice thickness, the band fold), k_envelope, k_remap, k_transpose, k_blocks_to_frames
//   mcrt_display.hip k_bmode_peak, k_bmode_grey, k_bmode (mcrt_bmode_frames: log-compressed 8-bit B-mode frames), k_compound (spatial compounding:
//                    mcrt_compound_frames, mcrt_bmode_compound_frames)
//   mcrt_volume.hip  k_volume (volume imaging: mcrt_volume_frames, mcrt_bmode_volume_frames)
//   mcrt_render.hip  k_render (volume rendering: mcrt_render_frames)
//   mcrt_speckle.hip k_srad (speckle reduction: mcrt_speckle_frames)
//   mcrt_speckle3d.hip k_srad3 (3-D speckle reduction over voxel blocks: mcrt_speckle_volume_frames)
//   mcrt_noise.hip   k_noise (receiver noise: mcrt_noise_frames; its peaks are k_bmode_peak's)
//   mcrt_detect.hip  k_detect<NT> (quadrature detection: mcrt_detect_frames; NT taps, 1..16)
//   mcrt_flow.hip    k_flow_split, k_flow<N, WALL>, k_flow_avg (colour Doppler: mcrt_flow_split_frames, mcrt_flow_frames), k_colour (mcrt_colour_frames)
//   mcrt_spectral.hip k_gate_series (spectral Doppler: mcrt_spectral_series_frames), k_spectrum<N> (mcrt_spectral_frames), k_sonogram_peak, k_sonogram (mcrt_sonogram_frames)
//   mcrt_strain.hip  k_strain_warp (strain elastography: mcrt_strain_compress_frames), k_strain_track, k_strain_slope (mcrt_strain_frames), k_elastogram (mcrt_elastogram_frames)
//   mcrt_shear.hip   k_shear_arrival, k_shear_track (shear-wave elastography: mcrt_shear_wave_frames), k_shear_speed (mcrt_shear_speed_frames); mcrt_warp.h: the line reading it shares with k_strain_warp
//   mcrt_mmode.hip   k_mmode_lines (M-mode: mcrt_mmode_lines_frames; it reads its lines through mcrt_warp.h too), k_mmode_peak, k_mmode_picture (mcrt_mmode_picture_frames)
//   mcrt_autogain.hip k_autogain_hist, k_autogain_curve, k_autogain_apply (automatic gain: mcrt_autogain_frames)
//   mcrt_recon.hip   k_recon_splat, k_recon_resolve (freehand 3-D reconstruction: mcrt_recon_frames)
//   mcrt_label.hip   k_label (ground-truth label maps: mcrt_label_frames), k_label_gather (mcrt_label_scan_convert_frames, mcrt_label_volume_frames)
//   mcrt_transmit.hip k_transmit (acoustic ground truth: mcrt_transmit_frames; the boundary rule it shares with the host is mcrt_transmit.h)
//   mcrt_label3d.hip k_recon_label_splat, k_recon_label_resolve (a freehand label volume by majority vote: mcrt_recon_label_frames),
//                    k_render_label (the label of what a rendering shows: mcrt_render_label_frames)
//   mcrt_scene.hip   k_tris_by_id, k_expand_tris; the probes k_math_probe, k_verify_div, k_philox_probe
//   mcrt_lbvh.hip    the device BVH builder (mcrt_lbvh.h)
// Shared device code: mcrt_device.h (primitives and the knobs more than one unit reads), mcrt_walk.h (the lane walk's steps, also k_path's),
// mcrt_shade.h (shade_path, also k_path's), mcrt_voxels.h (the voxel block of the 3-D stages: a sample's voxel, a wavefront's runs,
// the resolve tile, the picture tile -- included by mcrt_recon / label3d / render.hip and, for recon_tiling, mcrt_image.cpp), mcrt_pixels.h (the pixel tile of k_bmode, k_compound, k_volume and k_label_gather and the byte
// k_render writes: layout, frame chunks, persistence, quantisation, the word store -- included by mcrt_display / volume / label / render / flow / strain.hip
// only).  Everything is scalar fp32/fp64 VALU + integer work -- no dense contraction, hence no MFMA -- and the arithmetic follows the
// parity contract expression by expression (compiled -ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mcrt.h"
#include "mcrt_internal.h"

namespace mcrt {

struct FrameArgs {
    // scene (HBM-resident, read-only)
    const uint4 *nodes_walk;   // [n_nodes][4]  the walk's 64-byte nodes: child-transposed half-float boxes (rounded outwards) + refs
    int *stack_ovf;            // [max_stack - MCRT_LANE_STACK][trace_blocks * 256] traversal-stack entries beyond the LDS part (this work set's own)
    const float4 *tris;        // [T][3]         48-B triangle records, leaf order: v0|id, v1|mesh, v2|edge tolerance
    const float4 *tris_id;     // [T][3]         the same records in TRIANGLE-ID order (k_shade looks the winning triangle up by its id: one dependent load less than through tri_slot)
    const uint4 *meshes;       // [n_mesh]      mat_inside, mat_outside, vascular, -
    const float4 *mats;        // [n_mat][2]    imp, att, mu0, mu1 | sigma, spec, shine, thick
    const float2 *tex;         // [n^3]         texture_noise, scattering_probability
    const float *el_pos;       // [E][3], or [F][E][3] when the frames of a pass have their own probe poses (pose_stride = E)
    const float *el_dir;       // same shape
    const double *row_thr;     // [R+1] row thresholds (see row_of)
    // per-frame work buffers; np = ne * S paths
    float4 *st0, *st1, *st2;   // [2][np] path state in queue order, two halves by bounce parity: from, ray length factor | dir, media | distance_traveled(f64), outside, intensity
                               //         (the walk reads st0 + st1 and rebuilds the ray from them: ray_of)
    uint32_t *queue;           // [2][np] live path ids of bounce b in buffer b & 1
    unsigned long long *key0, *key1;   // [np] closest hit per ray: fraction bits << 32 | triangle id (atomicMin), ping-pong by bounce parity
    uint32_t *from_tri;        // [np] by path: the triangle its ray of the next bounce leaves; k_shade(b) writes it only where bounce b + 1 runs by beams (beam_mask).
                               // Behind it [np] by QUEUE POSITION of the next bounce: the queued ray's beam word (beam_words, beam_word_of), written only where bounce
                               // b + 1 is ordered (order_mask); k_beam_rank(b + 1) has read it before k_shade(b + 1) writes the next (stream order)
    const uint32_t *tri_slot;  // [T] triangle id -> position in the leaf-order triangle array
    uint32_t *counts;          // [MAX_BOUNCES+1] live rays per bounce
    uint32_t *cursors;         // [MAX_BOUNCES][MCRT_XCDS][MCRT_CURSOR_STRIDE] queue cursors of the persistent walk, one per XCD sub-queue
    mcrt_segment *segs;        // [np][B]   written only when want_segs (mcrt_cast_rays / mcrt_trace_frame_debug with a segment buffer)
    int32_t *hits;             // [np][B]   triangle hit at the end of each segment (-1 none); null unless the caller asked for hit indices
    float4 *mrec;              // [B][np][3] what k_march needs of a segment: from,refl | delta,intensity | t_start(f64),steps,media
    const float4 *mtab;        // [M] per material, for k_march: mu0, mu1, sigma, per-step attenuation factor
    uint32_t *seg_count;       // [np]
    long long *acc;            // [ne][R] fixed-point RF accumulators (2^-40 units)
    uint32_t *flags;           // [ne][(R+31)/32] non-finite flags
    unsigned long long *stats; // [6]
    uint32_t *error_flag;      // device word, bit 0: traversal stack overflow
    unsigned long long *stamps; // diagnostic builds only (tools/variants/round6_stamps.patch); unused by the product's kernels
    // sizes / parameters
    uint32_t n_nodes, S, B, R, e_begin, ne, ne_frame, pose_stride, acc_stride, acc_off, trace_blocks, trace_blocks_wide, wide_from, packet_mask, march_blocks, ksplit_limit, frame, seed, start_mat, tex_n, tex_mask, sanitize, tex_finite, fast_div, want_segs, tex_shift, march_rows, n_mat, n_mesh;   // march_rows: entries of k_march's padded LDS image when its fast variant applies, else 0
    float scene_lo[3], scene_hi[3];   // bounds of the whole BVH
    float freq, eps, I0, offs, sx, sy, sz, tex_res, axial_res_f, pad_abs, tex_rcp, lean_bound;
    double axial_res_mm, time_step, row_dt, max_travel, sos_d, inv_row_dt;
    double thr_end;            // row_thr[R]: the first time past the image
    uint32_t retire_late;      // shade_path ends a path whose next segment would start past max_travel and past the image (off for counting and debug passes)
    uint32_t beam_mask;        // bit b >= 2: bounce b runs by beams (mcrt_beam.hip), so k_shade(b - 1) writes from_tri
    uint32_t fold_b0;          // staged pass in a silent start medium: k_shade(b = 0) adds bounce 0's boundary echoes itself, writes no march record, no k_march(0)
    uint32_t order_mask;       // bit b >= 2: bounce b is tested in the beam order (mcrt_beam.hip), so k_shade(b - 1) writes the ray's beam word (beam_words).  (In the
                               // struct's tail padding: its size, and with it the offset of every kernel argument behind a FrameArgs, stays)
};
static_assert(sizeof(FrameArgs) % 8 == 0 && offsetof(FrameArgs, order_mask) + 4 == sizeof(FrameArgs), "order_mask fills FrameArgs' tail padding");

// k_beam_* (mcrt_beam.hip): a bounce by beams.  A beam of BOUNCE 1 is a scan-line's rays of one history (reflected or refracted at bounce 0), one dominant axis
// and one sign along it: MCRT_BEAM_SLOTS per scan-line, addressed directly, most of them empty.  A beam of a bounce b >= 2 is the rays of one GROUP -- scan-line,
// the triangle the ray left (FrameArgs::from_tri), medium -- of one dominant axis and sign: the group claims a slot of a hash table (gkey), 6 beams per slot.
// Scratch that is dead between k_shade(b - 1) and k_shade(b) -- the halves of the OTHER parity, bounce b - 1's consumed input -- carries the leftovers: lq0 is
// that half of the queue, lq1 lies in that half of st2, and their compact state is that half of st0 / st1 with its key words (launch_beam).
// THE BEAM ORDER (`ordered`): in queue order 64 neighbours hold several beams, whose lists k_beam_test runs one after the other.  k_beam_rank counts every beam's rays
// (one atomic per wavefront and beam) and gives each ray a rank, k_beam_scan lays the beams' segments out -- each padded to whole wavefronts with MCRT_BEAM_PAD,
// the rays without a beam in a pseudo-beam behind the last --, k_beam_place writes the permutation, and k_beam_test's first pass takes its rays through it: one
// beam, one list per wavefront.  Buffers of its own (BeamBufs), made only where a bounce is ordered.
#define MCRT_BEAM_SLOTS 12u
#define MCRT_BEAM_REC 16u            // words of a beam's reduction block and of its record
#define MCRT_BEAM_HOT 12u            // words of the hot part of a list entry (BeamArgs::hot)
#define MCRT_BEAM_CAP_MAX 1024u      // the largest list capacity (k_beam_collect sorts in LDS)
#define MCRT_BEAM_PROBES 4u          // slots of the group table a key is looked for in
#define MCRT_BEAM_COUNTERS 16u       // counters of one beamed bounce (0-7: mcrt_debug_beam_bounce's; 8-12: the beam order's, mcrt_debug_beam_order)
#define MCRT_BEAM_PAD 0xffffffffu    // a word of the beam order that holds no ray: the padding of a beam's segment to whole wavefronts
constexpr uint32_t beam_segment(uint32_t count) { return (count + 63u) & ~63u; }   // words of a beam's segment of the order: its rays, rounded up to whole wavefronts (k_beam_scan; mcrt_debug_beam_layout)
struct BeamArgs {
    uint32_t *red;             // [n_beams][MCRT_BEAM_REC] k_beam_bounds' minima and maxima
    uint32_t *rec;             // [n_beams][MCRT_BEAM_REC] the beams as k_beam_test reads them (k_beam_collect)
    uint4 *list;               // [n_lists][cap][4] (+ one entry of padding) 64-byte candidates, nearest first: v0 | id, v1 | depth at which the padded bounds begin, v2 | edge tolerance, -
                               // the COLD part of an entry: k_beam_test fetches it only for the edge tests; what every entry's test needs is in `hot`
    unsigned long long *gkey;  // [groups] the group that holds the slot (0: free); bounces >= 2
    uint32_t *lq0, *lq1;       // [np] leftover rays (queue positions) of the near and of the far pass
    uint32_t *lcount;          // [MCRT_BEAM_COUNTERS] of THIS bounce -- 0, 1: leftovers of the two passes; 2: beams whose list is incomplete; 3: beams refused (spread, or no list left);
                               // 4: beams with members; 5: lists handed out; 6: sampled rays whose group found no slot; 7: slots claimed
                               // 8: rays placed in the beam order; 9: its segments (beams with rays, the pseudo-beam of the rays without one included); 10: its pad lanes;
                               // 11: (wavefront, beam) pairs k_beam_test's first pass met (only with `pairs`); 12: the order's length, pads included (k_beam_test's n)
    uint32_t *l_counts, *l_cursors;   // the leftover walk's FrameArgs::counts and cursors
    uint32_t b;                // the bounce
    uint32_t groups;           // slots of the group table, a power of two; 0: bounce 1's direct addressing, a beam's list is list[beam]
    uint32_t n_beams, n_lists, cap, near, stride;   // near: entries of a list the first pass tests; stride: every stride-th packet of the queue is sampled for the bounds
    float spread_cap;          // a beam whose slopes spread further is refused
    uint32_t ordered;          // k_beam_test's first pass reads the bounce's rays through `order`: one beam per wavefront (MCRT_BEAM_ORDER)
    uint32_t pairs;            // count lcount[11] (MCRT_BEAM_PAIRS: a debug flag, off in every timed path)
    // the beam order (behind everything k_beam_collect reads: its argument offsets stay)
    uint32_t *rbeam, *rrank;   // [np] by queue position: the ray's beam (n_beams: none) and its rank among the beam's rays (k_beam_rank)
    uint32_t *ocount, *obase;  // [n_beams + 1] rays of a beam, and where its segment of the order begins (k_beam_scan); the last is the pseudo-beam of the rays without a beam
    uint32_t *order;           // [np + 64 (n_beams + 1)] queue positions grouped by beam, every segment padded to a multiple of 64 with MCRT_BEAM_PAD (k_beam_place)
    // what depends on the candidate's triangle alone, computed once per entry by k_beam_collect (behind everything else: the other beam kernels' argument offsets stay)
    uint32_t *hot;             // [n_lists][cap][MCRT_BEAM_HOT] (+ one entry of padding) 48 bytes beside every entry of `list`: tri_plane's n.x n.y n.z dot(v0, n) |
                               // tri_padded_bounds' lo.x lo.y lo.z, the depth at which they begin | hi.x hi.y hi.z, id -- bit for bit what packet_tri_test rebuilds
};

constexpr uint32_t MCRT_ALL_BOUNCES = 0xffffffffu;   // launch_march: accumulate the segments of every bounce in one launch

struct ConvTaps { float ax[16]; float lat[32]; uint32_t n_ax, n_lat; };

// What the host says about a pass over F pictures of n points (pixel_pass in mcrt_image.cpp fills it, mcrt_pixels.h reads it): n_pad is n rounded
// up to 256, the length of every map; blockIdx.y is a chunk of frames_per_chunk frames; vec: 8-bit output, n % 4 == 0 and out word-aligned
struct PixelPass { uint32_t n, n_pad, F, frames_per_chunk, vec; };

// k_bmode (mcrt_bmode_frames): the grey levels [F][E][R] of k_bmode_grey -> bytes [F][n], n = out_rows * out_cols
struct BmodeArgs {
    const float *grey;                  // [F][E][R]
    const float *map_col, *map_row;     // [n] the context's scan-conversion maps (16-byte aligned: the two halves of a [2][n_pad] buffer)
    float *state;                       // [n] persistence state, or null
    uint8_t *out;                       // [F][n]
    float alpha;
    uint32_t E, R, reset;
    PixelPass pass;
};

// k_compound (mcrt_compound_frames / mcrt_bmode_compound_frames): the views [F][N][E][R] (RF floats, or the grey levels of k_bmode_grey)
// -> floats or bytes [F][n], n = out_rows * out_cols
struct CompoundArgs {
    const float *src;                   // [F][N][E][R]
    const float *maps;                  // [N][2][n_pad] the context's compound maps: per view the column map, then the row map, zero-padded to n_pad = n rounded up to 256
    float *state;                       // [n] persistence state, or null (8-bit form only)
    void *out;                          // float or uint8_t [F][n]
    float alpha;
    uint32_t E, R;
    PixelPass pass;
    uint32_t N, reset;
    uint32_t mode;                      // COMPOUND_*: which k_compound runs
    float feather;                      // mcrt_compound_opts::feather_lines (COMPOUND_PLAIN does not read it)
    float weight[16];                   // mcrt_compound_opts::view_weight, the first N (COMPOUND_PLAIN does not read them)
};
// COMPOUND_PLAIN is the mean of mcrt_compound_frames (every weight 1, no feathering); the others are mcrt_compound_opts' modes
enum { COMPOUND_PLAIN = 0, COMPOUND_WEIGHTED = 1, COMPOUND_MAX = 2, COMPOUND_MEDIAN = 3 };

// k_volume (mcrt_volume_frames / mcrt_bmode_volume_frames): the planes [F][K][E][R] of a swept probe (RF floats, or the grey levels of
// k_bmode_grey) -> floats or bytes [F][n], n = nu * nv * nw
struct VolumeArgs {
    const float *src;                   // [F][K][E][R]
    const float *maps;                  // [3][n_pad] the grid's maps: plane, column, row; zero-padded to n_pad = n rounded up to 256
    void *out;                          // float or uint8_t [F][n]
    uint32_t E, R, K;
    PixelPass pass;
};

// what k_render and k_render_label know of a view and its block (view_args in mcrt_image.cpp fills it, mcrt_voxels.h reads it)
struct ViewArgs { float origin[3], di[3], dj[3], ds[3]; uint32_t nx, ny, n_steps, F, nu, nv, nw; };   // origin .. ds: mcrt_render_view, component order u, v, w

// k_render (mcrt_render_frames): the voxel blocks [F][nw][nv][nu] (floats or bytes) -> floats, bytes and step indices [F][ny][nx]
struct RenderArgs {
    const void *vol;                    // float or uint8_t [F][nw][nv][nu]
    float *out;                         // [F][ny][nx] or null
    uint8_t *out8;                      // same or null
    float *depth;                       // same or null
    ViewArgs view;
    uint32_t mode;                      // MCRT_RENDER_*
    uint32_t row_tile;                  // 0: a wavefront owns an 8 x 8 tile of the picture; 1: 64 pixels of one row
    float lo, inv_range, threshold, inv_ramp, opacity, depth_cue, t_cut, inv_steps;
};

// k_srad (mcrt_speckle_frames): one launch carries every frame of the stack [F][H][W] through n <= SRAD_FUSE_MAX iterations, src -> dst (two buffers)
#ifndef SRAD_TH             // (make variant DEFS=-DSRAD_TH=...: the tile is a tuning build's to change)
#define SRAD_TH 16          // a workgroup's tile: rows ...
#endif
#ifndef SRAD_TW
#define SRAD_TW 64          // ... and columns (W is contiguous)
#endif
#define SRAD_FUSE_MAX 4     // iterations per launch: k_srad<2> and <4> are built
struct SpeckleArgs {
    const float *src;                   // [F][H][W]
    float *dst;                         // [F][H][W], not src
    uint32_t H, W;
    uint32_t n;                         // iterations of this launch, 1 .. the instantiation's TT
    uint32_t first;                     // the call's first launch: step 0 of the contract (|v|, or 0 where v is not finite) is applied while staging
    uint32_t tx, ty;                    // tiles along W and H (launch_srad fills them)
    float lam4;
    float q0sq[SRAD_FUSE_MAX], kq[SRAD_FUSE_MAX];   // mcrt_speckle_tables' entries of these n iterations
};

// k_srad3 (mcrt_speckle_volume_frames): one launch carries every block of the stack [F][nw][nv][nu] through one iteration, src -> dst (two buffers)
#ifndef SRAD3_TV            // (make variant DEFS=-DSRAD3_TV=...: the tile and the chunk are a tuning build's to change)
#define SRAD3_TV 8          // a workgroup's tile: voxels along v ...
#endif
#ifndef SRAD3_TU
#define SRAD3_TU 32         // ... and along u (contiguous); 8 x 32 x 8 was the fastest of the tiles and chunks measured
#endif
#ifndef SRAD3_CW
#define SRAD3_CW 8          // the slices along w a workgroup marches its tile through
#endif
struct Speckle3Args {
    const float *src;                   // [F][nw][nv][nu]
    float *dst;                         // [F][nw][nv][nu], not src
    uint32_t nu, nv, nw;
    uint32_t first;                     // the call's first launch: step 0 of the contract (|v|, or 0 where v is not finite) is applied while staging
    uint32_t tx, ty, tc;                // tiles along u and v, chunks along w (launch_srad3 fills them)
    float wu, wv, ww;                   // the weights of the two neighbours along u, v and w
    float a, b, hs, lamw;               // mcrt_speckle3d_tables' four constants
    float q0sq, kq;                     // ... and its entries of this iteration
};

// k_recon_splat and k_recon_resolve (mcrt_recon_frames): the stack [F][E][R] binned into the accumulators of n = nu * nv * nw voxels, then the
// accumulators resolved and the holes filled into out [nw][nv][nu]
#define RECON_TU 32         // k_recon_resolve: a workgroup's tile of voxels along u (contiguous) ...
#define RECON_TV 8          // ... along v ...
#define RECON_TW 8          // ... and along w; staged in LDS with a halo of fill_radius on every side
#define RECON_MAX_FILL 3    // the largest fill_radius (the LDS image is sized per launch: 5 bytes per staged voxel)
#define RECON_MAX_TILES (1u << 24)   // a grid must need fewer resolve tiles than this: a launch holds fewer than 2^32 lanes
// what the two splats and the two resolves know of the stack's poses and of the block (recon_block in mcrt_image.cpp fills it, mcrt_voxels.h reads it)
struct ReconBlock {
    const float *pos, *dir;             // [F][E][3]
    uint32_t *stats;                    // [2] or null: samples outside the block, samples inside it that are not binned
    uint32_t R, n_samples;              // n_samples = F * E * R < 2^31
    uint32_t nu, nv, nw, fill_radius, fill_min;
    uint32_t tu, tv;                    // tiles along u and v (launch_resolve fills them)
    float A[9], b[3], row_u;            // mcrt_recon_transform; row_mm / unit_mm
};
struct ReconArgs {
    const float *stack;                 // [F][E][R]
    ReconBlock blk;                     // stats[1]: unusable samples inside the block
    unsigned long long *sum;            // [n] MEAN: the int64 sum of q;  MAX: the largest q, biased by 2^63 so that a cleared word is "none yet"
    uint32_t *count;                    // [n]
    float *out;                         // [nw][nv][nu]
    uint32_t *count_out;                // same, or null
    uint32_t mode;
    float value_max, empty;
    double qscale;
};

// k_noise (mcrt_noise_frames): the stack [F][N][E][R] in place; a wavefront owns NOISE_WAVE_ROWS consecutive rows of one scan-line
#define NOISE_LANE_ROWS 4u                          // consecutive rows of a lane: one 16-byte access where the scan-line's base allows
#define NOISE_WAVE_ROWS (64u * NOISE_LANE_ROWS)
struct NoiseArgs {
    float *rf;                          // [F][N][E][R]
    const float *peak;                  // [F]: sigma_f = peak[f] * c (MCRT_NOISE_SNR_DB), or null: sigma_f = c (MCRT_NOISE_ABS)
    const float *gain;                  // [E] or null
    float *sigma_out;                   // [F] or null: receives sigma_f
    uint32_t N, E, R;
    uint32_t lines;                     // F * N * E
    uint32_t chunks;                    // ceil(R / NOISE_WAVE_ROWS)
    uint32_t seed, first_id;            // Philox key word 0, and the id of image 0
    float c, inv_std;
};

// k_autogain_hist, k_autogain_curve, k_autogain_apply (mcrt_autogain_frames): a chunk of F frames of the stack [F][N][E][R]
#define AUTOGAIN_BINS 2048u                         // bin(a) = bits(a) >> 20
#define AUTOGAIN_MAX_BANDS 512u                     // MCRT_MAX_ROWS / the smallest band_rows
#define AUTOGAIN_WG_SAMPLES 4096u                   // samples a workgroup of k_autogain_hist reads: 16 per lane
struct AutogainArgs {
    float *rf;                          // [F][lines][R]
    uint32_t *hist;                     // [F][n_bands][AUTOGAIN_BINS], zeroed before k_autogain_hist
    const float *floor_dev;             // [F] or null: floor_f = floor
    float *gain;                        // [F][R]: the caller's gain_dev or the context's
    int32_t *band_bin;                  // [F][n_bands] or null
    uint32_t *pen;                      // [F] or null
    uint32_t lines, R;                  // lines = N * E
    uint32_t band_rows, n_bands, shares;   // shares: workgroups of k_autogain_hist per (frame, band), each a run of scan-lines
    uint32_t min_permille;
    float floor, floor_scale, max_gain, inv_max_gain;   // inv_max_gain = 1.0f / max_gain, made on the host
    uint32_t chunks;                    // k_autogain_apply: ceil(R / NOISE_WAVE_ROWS)
};

// k_label (mcrt_label_frames): beside these, a FrameArgs of which it reads the scene, the probe (el_pos, el_dir, pose_stride, e_begin, ne_frame,
// ne = ne_frame * frames), the row table (row_thr, R, inv_row_dt, thr_end, max_travel, sos_d), start_mat, offs, the spacing, pad_abs, stack_ovf
// (label_stack_entries() in LDS, the rest [..][label_blocks * 64]) and error_flag
struct LabelArgs {
    uint8_t *tissue;                    // [F][ne][R] or null
    int32_t *interface;                 // [F][ne][R] or null
    uint32_t *crossings;                // [F][ne] or null
    uint32_t rule;                      // MCRT_LABEL_TRACED / MCRT_LABEL_GEOMETRIC
    float Ls;                           // the beam's length factor: (float)(2.0 * depth_cm)
};

// k_transmit (mcrt_transmit_frames): beside these, the FrameArgs of k_label and in it the material table (mats), freq and row_dt; stack_ovf is
// sized by transmit_stack_entries() and transmit_blocks
struct TransmitArgs {
    float *transmit;                    // [F][ne][R] or null: the fraction of the emitted intensity that arrives at a row
    float *reflect;                     // [F][ne][R] or null: what the shallowest boundary of a row turns back, 0 elsewhere
    uint32_t *crossings;                // [F][ne] or null
    uint32_t rule;                      // MCRT_LABEL_TRACED / MCRT_LABEL_GEOMETRIC
    uint32_t mode;                      // MCRT_TRANSMIT_TOTAL / MCRT_TRANSMIT_BOUNDARIES
    float Ls;                           // the beam's length factor: (float)(2.0 * depth_cm)
};

// k_label_gather (mcrt_label_scan_convert_frames, mcrt_label_volume_frames): the tissue maps [F][K][E][R] -> bytes [F][n] through the float
// calls' own maps (map_plane null: one plane, K = 1)
struct LabelGatherArgs {
    const uint8_t *src;                 // [F][K][E][R]
    const float *map_plane, *map_col, *map_row;   // [n_pad] each, n_pad = n rounded up to 256
    uint8_t *out;                       // [F][n]
    uint32_t E, R, K;
    PixelPass pass;
};

// k_recon_label_splat and k_recon_label_resolve (mcrt_recon_label_frames): the tissue stack [F][E][R] voted into a table of n_vox * n_labels
// words, then the winners resolved and the holes filled into out [nw][nv][nu]; the tile and the limits are k_recon_resolve's (RECON_*)
struct ReconLabelArgs {
    const uint8_t *stack;               // [F][E][R]
    ReconBlock blk;                     // stats[1]: samples inside the block whose label is >= n_labels
    uint32_t *votes;                    // [n_vox][n_labels], cleared before the splat
    uint8_t *out;                       // [nw][nv][nu] or null
    uint32_t *count_out, *votes_out;    // same, or null: the votes of a voxel, the winner's votes
    uint32_t n_vox, n_labels;           // n_vox = nu * nv * nw;  n_vox * n_labels < 2^31
};

// k_render_label (mcrt_render_label_frames): the label blocks [F][nw][nv][nu] read at the points a depth buffer [F][ny][nx] names -> bytes [F][ny][nx]
struct RenderLabelArgs {
    const uint8_t *labels;              // [F][nw][nv][nu]
    const float *depth;                 // [F][ny][nx]: mcrt_render_frames' depth_dev
    uint8_t *out;                       // [F][ny][nx]
    ViewArgs view;
};

hipError_t launch_init(const FrameArgs &a, hipStream_t st);
hipError_t launch_trace(const FrameArgs &a, uint32_t b, bool stats, hipStream_t st);
hipError_t launch_beam_scan(const BeamArgs &g, hipStream_t st);                   // k_beam_scan alone over g.ocount[0 .. g.n_beams]: obase, the pads of g.order, lcount[8, 9, 10, 12] (launch_beam; mcrt_debug_beam_scan)
hipError_t launch_beam(const FrameArgs &a, const BeamArgs &g, hipStream_t st);   // bounce g.b's closest hits by beams, in place of launch_trace(a, g.b): the same key words
hipError_t launch_nodes_walk(const float4 *nodes, uint32_t n_nodes, uint4 *out, hipStream_t st);
hipError_t launch_nodes_walk_decode(const uint4 *walk, uint32_t n_nodes, float4 *out, hipStream_t st);
uint32_t lane_stack_entries();
uint32_t lane_wide_from();
hipError_t launch_shade(const FrameArgs &a, uint32_t b, bool stats, hipStream_t st);
uint32_t path_blocks(size_t np);                                  // workgroups of a k_path launch over np paths (sizes the overflow stacks)
hipError_t launch_path(const FrameArgs &a, hipStream_t st);      // k_path: every bounce of every path in one launch (the latency form)
hipError_t launch_march(const FrameArgs &a, uint32_t b, bool stats, hipStream_t st);
hipError_t launch_finalize(long long *acc, uint32_t *flags, float *rf, uint32_t ne, uint32_t R, const uint32_t *error_flag, hipStream_t st);
hipError_t launch_convolve(float *img, float *tmp, uint32_t n_img, uint32_t E, uint32_t R, const ConvTaps &taps, hipStream_t st);
// k_conv_axial, then k_conv_lateral_rows with the device table lat [taps.n_lat][R] (tap-major); taps.lat is not read
hipError_t launch_convolve_depth(float *img, float *tmp, uint32_t n_img, uint32_t E, uint32_t R, const ConvTaps &taps, const float *lat, hipStream_t st);
// k_conv_axial_bands (rf [F][E][R] -> tmp and bands [F][B][E][R], the device table ax [B][taps.n_ax][R] tap-major; taps.ax is not read), then the lateral pass of
// launch_convolve (lat null: taps.lat) or of launch_convolve_depth (the device table lat) over the F * B band images
hipError_t launch_convolve_bands(const float *rf, float *tmp, float *bands, uint32_t F, uint32_t B, uint32_t E, uint32_t R, const ConvTaps &taps,
                                 const float *ax, const float *lat, hipStream_t st);
// k_elevation: planes [F][K][E][R] folded into rf [F][E][R] with the device table w [K][R] (tap-major); float4 lanes where E*R and the pointers allow
hipError_t launch_elevation(const float *planes, float *rf, uint32_t F, uint32_t K, uint32_t E, uint32_t R, const float *w, hipStream_t st);
hipError_t launch_envelope(float *img, uint32_t E, uint32_t R, hipStream_t st);
// k_detect: the FIR Hilbert transformer along every scan-line of rf [lines][R]; env (may be rf) and iq are written where they are given
struct DetectArgs {
    const float *rf;                    // [lines][R]
    float *env;                         // [lines][R] or null
    float2 *iq;                         // [lines][R] (x, q) or null
    size_t lines;
    uint32_t R, nt;                     // nt: the taps at the odd offsets 1, 3, ..., 2 * nt - 1 (1..16)
    float t[16];                        // t[k]: the tap at offset 2 * k + 1
};
hipError_t launch_detect(const DetectArgs &a, hipStream_t st);
// k_flow_split (mcrt_flow_split_frames): the raw trace [F][E][R] -> out [F][2][E][R], what stands still and what moves
struct FlowSplitArgs {
    const float *rf;                    // [F][E][R]
    const uint8_t *tissue;              // [F][E][R]
    float *out;                         // [F][2][E][R]
    uint32_t plane, n;                  // E * R, F * E * R
    uint32_t moving[8];                 // bit l: label l moves (labels >= n_labels: 0)
};
hipError_t launch_flow_split(const FlowSplitArgs &a, hipStream_t st);
// k_flow<N, WALL> and k_flow_avg (mcrt_flow_frames): the ensemble, the wall filter and the autocorrelation of every sample into raw, then the
// window average and the outputs
#define FLOW_WAVE_ROWS 64u                          // a wavefront of k_flow owns 64 consecutive rows of one scan-line, a lane one of them
struct FlowArgs {
    const float2 *iq_static;            // [F][E][R] (I, Q) or null
    const float2 *iq_moving;            // [F][E][R]
    const uint8_t *tissue;              // [F][E][R]
    const float2 *phasor;               // [n_labels][E] the context's copy
    const float *truth;                 // [n_labels][E] the context's copy
    const float *sigma_dev;             // [F] or null: sigma
    float *raw;                         // [F][3][E][R] the per-sample r0, Re r1, Im r1 (the context's buffer)
    float *corr, *vel, *var, *truth_out;   // the outputs, each or null
    uint32_t F, E, R, n_labels;
    uint32_t lines, chunks;             // F * E, ceil(R / FLOW_WAVE_ROWS)
    uint32_t n_packets, wall, avg_rows, avg_lines;
    uint32_t seed, first_id;
    float sigma, inv_std, vscale;       // vscale: (float)(v_nyq / pi)
};
hipError_t launch_flow(const FlowArgs &a, hipStream_t st);       // both kernels, in stream order
// k_colour (mcrt_colour_frames): corr_img [F][3][n] and the grey bytes [F][n] -> rgb [F][n][3] and vel_img [F][n]
struct ColourArgs {
    const float *corr;                  // [F][3][n]
    const uint8_t *grey;                // [F][n]
    const float *lut;                   // [256]: (float)(r | g << 8 | b << 16), exact (the context's copy)
    uint8_t *rgb;                       // [F][n][3]
    float *vel;                         // [F][n] or null
    float power_thr, vel_thr, vscale, iscale;      // vscale: (float)(v_nyq / pi), iscale: (float)(127.0 / pi)
    uint32_t grey_max;
    PixelPass pass;
};
hipError_t launch_colour(const ColourArgs &a, hipStream_t st);
// k_gate_series (mcrt_spectral_series_frames): the detected pairs and the context's copies of the host tables -> series [n_gates][T]
struct GateSeriesArgs {
    const float2 *iq_static;            // [F][E][R] (I, Q) or null
    const float2 *iq_moving;            // [F][E][R]
    const uint32_t *gates;              // [n_gates][3]: image, line, row0
    const float *weight;                // [G]
    const int32_t *rate;                // [n_gates][G], Q16
    const long long *phase;             // [T], 2^-32 turn
    const float2 *lut;                  // [4096] the rotor
    const float *sigma_dev;             // [F] or null: sigma
    float2 *series;                     // [n_gates][T]
    uint32_t E, R, G, T, n_gates, chunks;   // chunks: ceil(T / 64)
    uint32_t seed, first_id;
    float sigma, wnorm, inv_std;
};
hipError_t launch_gate_series(const GateSeriesArgs &a, hipStream_t st);
// k_spectrum<N> (mcrt_spectral_frames): series [n_gates][T] -> power [n_gates][n_cols][N] and mean [n_gates][n_cols], each or null
struct SpectrumArgs {
    const float2 *series;
    const float *window;                // [N] the context's copy
    const float2 *tw;                   // [N / 2] the context's table of this N
    float *power, *mean;
    uint32_t n_gates, T, n_cols, N, hop, wall, wall_bins;
    float vscale;                       // (float)(2 v_nyq / N)
};
hipError_t launch_spectrum(const SpectrumArgs &a, hipStream_t st);
// k_sonogram_peak and k_sonogram (mcrt_sonogram_frames): power [n_gates][n_cols][N] -> the gates' largest finite powers and the bytes [n_gates][N][n_cols]
struct SonogramArgs {
    const float *power;
    float *peak;                        // [n_gates], zeroed before k_sonogram_peak; null: ref
    uint8_t *out;
    uint32_t n_gates, n_cols, N;
    float ref, gain, dr;
};
hipError_t launch_sonogram_peak(const SonogramArgs &a, hipStream_t st);
hipError_t launch_sonogram(const SonogramArgs &a, hipStream_t st);
// k_strain_warp (mcrt_strain_compress_frames): the detected pairs and the tissue labels -> the post-compression pairs and the true displacement and strain
struct StrainWarpArgs {
    const float2 *iq;                   // [F][E][R] (I, Q)
    const uint8_t *tissue;              // [F][E][R]
    const int32_t *eps;                 // [n_labels] Q24 strains (the context's copy)
    const float2 *lut;                  // [4096] the rotor (the context's copy)
    const float *sigma_dev;             // [F] or null: sigma
    float2 *post;                       // [F][E][R] or null
    float *truth_disp, *truth_strain;   // [F][E][R], each or null
    long long carrier_q32;              // llrint(cycles_per_row * 2^32)
    uint32_t E, R, lines, n_labels;     // lines: F * E
    uint32_t seed, first_id;
    float sigma, inv_std;
};
hipError_t launch_strain_warp(const StrainWarpArgs &a, hipStream_t st);
// k_strain_track and k_strain_slope (mcrt_strain_frames): the two stacks of pairs -> the displacement, the correlation coefficient and the strain
#define STRAIN_TILE_ROWS 64u                        // a wavefront of k_strain_track owns 64 consecutive rows of one scan-line, a lane one of them
#define STRAIN_MAX_WINDOW 32u                       // the largest window_rows and search_rows: they size the tile's LDS
#define STRAIN_MAX_SEARCH 16u
struct StrainTrackArgs {
    const float2 *pre, *post;           // [F][E][R]
    float *disp;                        // [F][E][R]: the caller's, or the context's buffer
    float *rho, *strain;                // [F][E][R], each or null
    uint32_t R, lines, chunks;          // F * E, ceil(R / STRAIN_TILE_ROWS)
    uint32_t window, search, lsq;
    float scale;                        // (float)(1.0 / (2 pi cycles_per_row))
};
hipError_t launch_strain_track(const StrainTrackArgs &a, hipStream_t st);      // both kernels, in stream order (the slope only with a strain output)
// k_elastogram (mcrt_elastogram_frames): the gathered strain and rho [F][n] and the grey bytes [F][n] -> rgb [F][n][3]
struct ElastogramArgs {
    const float *strain, *rho;          // [F][n]
    const uint8_t *grey;                // [F][n]
    const float *lut;                   // [256]: (float)(r | g << 8 | b << 16), exact (the context's copy)
    uint8_t *rgb;                       // [F][n][3]
    float ref_strain, rho_min;
    uint32_t grey_min, alpha;
    PixelPass pass;
};
hipError_t launch_elastogram(const ElastogramArgs &a, hipStream_t st);
// k_shear_arrival and k_shear_track (mcrt_shear_wave_frames): the detected pairs and the tissue labels -> the arrival ticks, the tracked displacement's
// peak and the truths
#define SHEAR_TILE_ROWS 64u                         // a wavefront of k_shear_track owns 64 consecutive rows of one scan-line, a lane one of them
#define SHEAR_MAX_WINDOW 16u                        // the largest window_rows: it sizes the tile's LDS
#define SHEAR_NEVER (1ll << 40)                     // ticks: a blocked crossing, and the arrival that never comes
#define SHEAR_SHAPE_SHIFT 10                        // ticks per entry of the shape table: 1/64 pulse
struct ShearWaveArgs {
    const float2 *iq;                   // [F][E][R] (I, Q)
    const uint8_t *tissue;              // [F][E][R]
    const long long *slow;              // [n_labels] Q16 ticks per um, 0: blocked (the context's copy, as the next four)
    const float *speed_f;               // [n_labels]
    const uint32_t *pitch;              // [R] Q8 um
    const uint32_t *shape, *amp;        // [n_shape], [n_amp] Q16
    const float2 *lut;                  // [4096] the rotor (the context's copy)
    const float *sigma_dev;             // [F] or null: sigma
    long long *arrival;                 // [F][E][R] ticks: the context's buffer
    float *peak_time, *peak_disp;       // [F][E][R], each or null
    float *disp;                        // [F][T][E][R] or null
    float *truth_arrival, *truth_speed; // [F][E][R], each or null
    long long carrier_q32;              // llrint(cycles_per_row * 2^32)
    uint32_t F, E, R, chunks, n_labels, n_shape, n_amp, T, window;   // chunks: ceil(R / SHEAR_TILE_ROWS)
    uint32_t push_line, row0, row1;     // the pushed rows [row0, row1)
    int32_t peak_q24;
    uint32_t seed, first_id;
    float sigma, inv_std, scale;        // scale: (float)(1.0 / (2 pi cycles_per_row))
};
hipError_t launch_shear_wave(const ShearWaveArgs &a, hipStream_t st);          // both kernels, in stream order (the tracker only with one of its outputs)
// k_shear_speed (mcrt_shear_speed_frames): the peak times -> the shear speed, the modulus and the quality of the fit
struct ShearSpeedArgs {
    const float *peak_time;             // [F][E][R]
    const float *pitch_mm;              // [R] (the context's copy)
    float *speed, *modulus, *quality;   // [F][E][R], each or null
    uint32_t F, E, R, chunks, push_line, lines, avg;    // lines: b, avg: v
    float kf, d3;                       // (float)(prf_hz * 0.001), 3.0f * density
};
hipError_t launch_shear_speed(const ShearSpeedArgs &a, hipStream_t st);
// k_mmode_lines (mcrt_mmode_lines_frames): the detected pairs and the tissue labels of the named scan-lines -> T moving lines of each, their envelopes and the truths
#define MMODE_PULSE_CHUNK 16u                       // a workgroup of k_mmode_lines owns one M-line and at most this many consecutive pulses
#define MMODE_THREADS 256u
struct MmodeLinesArgs {
    const float2 *iq;                   // [F][E][R] (I, Q)
    const uint8_t *tissue;              // [F][E][R]
    const uint32_t *lines;              // [n_lines][2]: image, line (the context's copy, as the next three)
    const int32_t *dil;                 // [n_labels] Q24
    const int32_t *w, *bulk;            // [T] Q16, [T] Q24
    const float2 *lut;                  // [4096] the rotor (the context's copy)
    const float *sigma_dev;             // [F] or null: sigma
    float *env;                         // [n_lines][T][R] or null
    float2 *iq_out;                     // [n_lines][T][R] or null
    float *truth_disp;                  // [n_lines][T][R] or null
    uint8_t *truth_label;               // [n_lines][T][R] or null
    long long carrier_q32;              // llrint(cycles_per_row * 2^32)
    uint32_t E, R, T, n_lines, chunks, n_labels;    // chunks: ceil(T / MMODE_PULSE_CHUNK)
    uint32_t seed, first_id;
    float sigma, inv_std;
};
hipError_t launch_mmode_lines(const MmodeLinesArgs &a, hipStream_t st);       // the instantiation: the outputs that are given
// k_mmode_peak and k_mmode_picture (mcrt_mmode_picture_frames): env [n_lines][T][R] -> the column means, the lines' peaks and the bytes [n_lines][H][W]
struct MmodePictureArgs {
    const float *env;                   // [n_lines][T][R]
    const uint8_t *truth_label;         // [n_lines][T][R] or null
    const float *truth_disp;            // [n_lines][T][R] or null
    const uint32_t *idx;                // [H] the first tap (the context's copy, as wt)
    const float *wt;                    // [H] the second tap's weight
    float *peak;                        // [n_lines], zeroed before k_mmode_peak; null in k_mmode_picture: ref
    float *mean;                        // [n_lines][W][R] or null
    uint8_t *out;                       // [n_lines][H][W]
    uint8_t *label_out;                 // [n_lines][H][W] or null
    float *disp_out;                    // [n_lines][H][W] or null
    uint32_t n_lines, T, R, W, H, hop, row_lo, row_hi;
    float ref, gain, dr;
};
hipError_t launch_mmode_peak(const MmodePictureArgs &a, hipStream_t st);
hipError_t launch_mmode_picture(const MmodePictureArgs &a, hipStream_t st);
hipError_t launch_remap(const float *img, uint32_t n_img, uint32_t E, uint32_t R, const float *map_col, const float *map_row, float *out, uint32_t n, hipStream_t st);
hipError_t launch_bmode_peak(const float *rf, uint32_t F, uint32_t E, uint32_t R, const float *tgc, float *peak, hipStream_t st);   // peak[F] zeroed before
hipError_t launch_bmode_grey(const float *rf, uint32_t F, uint32_t E, uint32_t R, const float *tgc, const float *peak /*[F] or null: ref*/, float ref,
                             float *peak_out /*[F] or null*/, uint32_t mode, float gain, float dr, float *grey, hipStream_t st);
hipError_t launch_bmode(const BmodeArgs &a, hipStream_t st);
hipError_t launch_compound(const CompoundArgs &a, bool out8, hipStream_t st);   // a.mode: the instantiation
hipError_t launch_volume(const VolumeArgs &a, bool out8, hipStream_t st);
hipError_t launch_render(const RenderArgs &a, bool in8, hipStream_t st);
hipError_t launch_srad3(Speckle3Args a, uint32_t F, hipStream_t st);                // one iteration over F blocks
hipError_t launch_srad(SpeckleArgs a, uint32_t F, uint32_t fuse, hipStream_t st);   // fuse: 2 or 4 (the instantiation); a.n <= fuse
hipError_t launch_noise(const NoiseArgs &a, hipStream_t st);
hipError_t launch_autogain_hist(const AutogainArgs &a, uint32_t F, uint32_t copies, hipStream_t st);   // copies: 1 or 4 LDS histograms per workgroup (the instantiation)
hipError_t launch_autogain_curve(const AutogainArgs &a, uint32_t F, hipStream_t st);
hipError_t launch_autogain_apply(const AutogainArgs &a, uint32_t F, hipStream_t st);
hipError_t launch_recon_splat(const ReconArgs &a, hipStream_t st);
hipError_t launch_recon_resolve(ReconArgs a, hipStream_t st);
hipError_t launch_recon_label_splat(const ReconLabelArgs &a, hipStream_t st);
hipError_t launch_recon_label_resolve(ReconLabelArgs a, hipStream_t st);
hipError_t launch_render_label(const RenderLabelArgs &a, hipStream_t st);
uint32_t label_blocks(size_t lines);                              // workgroups of a k_label launch over `lines` (frame, scan-line) beams (sizes the overflow stacks)
uint32_t label_stack_entries();
hipError_t launch_label(const FrameArgs &a, const LabelArgs &l, hipStream_t st);
hipError_t launch_label_gather(const LabelGatherArgs &a, hipStream_t st);
uint32_t transmit_blocks(size_t lines);                           // workgroups of a k_transmit launch over `lines` beams (sizes the overflow stacks)
uint32_t transmit_stack_entries();
hipError_t launch_transmit(const FrameArgs &a, const TransmitArgs &l, hipStream_t st);
hipError_t launch_blocks_to_frames(const float *blocks, float *frames, uint32_t F, uint32_t E, uint32_t R, uint32_t G, const uint32_t *off /*[G+1]*/, hipStream_t st);   // at most 64 ranks
hipError_t launch_transpose(const float *in, float *out, uint32_t E, uint32_t R, hipStream_t st);
hipError_t launch_math_probe(int op, const double *x, const double *y, double *out, uint32_t n, hipStream_t st);
hipError_t launch_verify_div(float res, float rcp, unsigned long long *bad, hipStream_t st);
hipError_t launch_tris_by_id(const float4 *tris, uint32_t n_tri, float4 *out, hipStream_t st);   // leaf-order records -> id order (record i goes to slot id(i))
hipError_t launch_expand_tris(const float4 *in48, uint32_t n_tri, float4 *out, hipStream_t st);   // (v0|id, v1|mesh, v2|-) -> the walk's records (v2.w = the edge tolerance)
hipError_t launch_material_table(const float4 *mats, uint32_t n_mat, float axial_res_f, float freq, float4 *mtab, hipStream_t st);
hipError_t launch_philox_probe(const uint32_t c[4], const uint32_t k[2], uint32_t *out, hipStream_t st);

}  // namespace mcrt
