/*
 * mcrt.h -- C-ABI of libmcrt_hip.so: the MI355X (gfx950) implementation of the Monte-Carlo
 * ultrasound ray-tracing hot path of thepochynsons/MCRay-Tracing.
 *
 * The reference has no FFI layer; its seam is C++ (paths relative to /root/reference/src):
 *   scene::scene(json, transducer&)            scene.h:24, scene.cpp:16-48   -> mcrt_upload_scene
 *   transducer<N>::element(i)                  transducer.h:64-67           -> mcrt_set_transducer
 *   volume<256,145> texture_volume             main.cpp:52, volume.h:19-35  -> mcrt_upload_texture
 *   rf_image.clear()                           main.cpp:102, rfimage.h:161  -> (inside mcrt_trace_frame)
 *   scene.cast_rays<S,E>(transducer)           main.cpp:104, scene.cpp:50   -> mcrt_trace_frame / mcrt_cast_rays
 *   accumulation loop + rf_image::add_echo     main.cpp:106-144, rfimage.h:33-40 -> (fused in mcrt_trace_frame)
 *   rf_image.convolve(psf)                     main.cpp:146, rfimage.h:93-123 -> mcrt_convolve
 *   rf_image.envelope() / postprocess()        main.cpp:147-148, rfimage.h:54-91,125-140 -> mcrt_envelope / mcrt_scan_convert
 *   transducer<N>::update() between frames     transducer.h:82-118, main.cpp:100 -> mcrt_set_transducer, mcrt_trace_frames_poses
 * A maintainer of the reference replaces main.cpp:102-148 with the calls shown in INTEGRATION.md.
 *
 * Conventions: every function returns 0 on success or a negative mcrt_status; the message is
 * available from mcrt_last_error() (thread-local).  No exceptions cross this boundary.  A
 * context belongs to one GPU and is used from one host thread at a time.  Pointers named
 * *_dev are device pointers on the context's GPU; everything else is host memory.  Uploads copy.
 * There is NO CPU fallback: without a usable GPU mcrt_create fails.
 */
#ifndef MCRT_H
#define MCRT_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCRT_VERSION 109  /* round 3: + mcrt_trace_frames_poses, mcrt_envelope_frames, mcrt_scan_convert_frames; the slab rule of the closest-hit contract is one fma per plane;
                              104: + the test hooks mcrt_debug_set_error, mcrt_debug_fast_paths; RF images are NaN while the device error word is set;
                              105 (round 4): + mcrt_group_* (several GPUs behind one call), mcrt_scan_maps; the scan-conversion maps follow the reference's float promotions;
                              106 (round 5): environment knobs are only read under MCRT_TUNING=1; the HIP-graph replay of passes (MCRT_GRAPH) is gone;
                              107: + mcrt_default_bmode, mcrt_bmode_frames (log-compressed 8-bit B-mode frames: dynamic range, gain, TGC, persistence);
                              108: + mcrt_focus, mcrt_psf_focus_kernels, mcrt_convolve_frames_depth (focal zones: a lateral PSF per RF row);
                              109: + mcrt_transducer_elevation_axis, mcrt_elevation_planes, mcrt_psf_elevation_kernels, mcrt_elevation_frames (slice thickness:
                                   elevation planes traced as one pose pass and folded with the elevation PSF);
                                   + mcrt_compound, mcrt_transducer_steered, mcrt_compound_maps, mcrt_compound_frames, mcrt_bmode_compound_frames (spatial
                                   compounding: steered views of one plane traced as one pose pass and averaged in image space);
                                   + mcrt_compound_opts, mcrt_default_compound_opts, mcrt_compound_weights, mcrt_compound_frames_opts,
                                   mcrt_bmode_compound_frames_opts (compounding modes: per-view weights, a lateral edge ramp, max, median; additive);
                                   + mcrt_sweep, mcrt_volume_grid, mcrt_transducer_swept, mcrt_volume_maps, mcrt_volume_frames, mcrt_bmode_volume_frames
                                   (volume imaging: a probe swept in elevation, 3-D scan conversion into voxels or any cut; additive);
                                   + mcrt_label_opts, mcrt_default_label_opts, mcrt_label_frames, mcrt_label_scan_convert_frames, mcrt_label_volume_frames
                                   (ground-truth label maps: tissue and interface per scan-line sample, pixel and voxel; additive);
                                   + mcrt_render_view, mcrt_render_opts, mcrt_default_render_opts, mcrt_render_view_for_grid, mcrt_render_frames
                                   (volume rendering: MIP, mean and surface views of a block of voxels seen from a direction; additive);
                                   + mcrt_speckle_opts, mcrt_default_speckle_opts, mcrt_speckle_tables, mcrt_speckle_frames
                                   (speckle reduction: speckle-reducing anisotropic diffusion over a stack of float frames; additive);
                                   + mcrt_recon_opts, mcrt_default_recon_opts, mcrt_recon_transform, mcrt_recon_frames
                                   (freehand 3-D reconstruction: tracked frames binned into voxels by their poses, with hole filling; additive);
                                   + mcrt_recon_label_opts, mcrt_default_recon_label_opts, mcrt_recon_label_frames, mcrt_render_label_frames
                                   (3-D ground truth: a freehand label volume by majority vote, the label of what a rendering shows; additive);
                                   + mcrt_debug_beam (what bounce 1 by beams did in the last pass; additive);
                                   + mcrt_debug_beam_bounce (the same for any bounce run by beams; additive);
                                   + mcrt_debug_beam_order, mcrt_debug_beam_layout (the beam order of a bounce run by beams, its layout on the host; additive);
                                   + mcrt_debug_beam_scan (the kernel that lays a beam order out, run alone on given counters; additive);
                                   + mcrt_debug_beam_records (the records, candidate lists and group keys of the last bounce a pass ran by beams; additive);
                                   + mcrt_debug_beam_entries (the planes and padded bounds stored with those lists' entries; additive);
                                   + mcrt_noise_opts, mcrt_default_noise_opts, mcrt_noise_draws, mcrt_noise_frames (receiver noise: a Gaussian noise floor
                                   from integer Philox sums and a gain per transducer element, over the RF stack in place; additive);
                                   + mcrt_transmit_opts, mcrt_default_transmit_opts, mcrt_transmit_boundary, mcrt_transmit_frames (acoustic ground truth:
                                   the intensity that arrives at every scan-line sample and what each boundary turns back; additive);
                                   + mcrt_speckle3d_opts, mcrt_default_speckle3d_opts, mcrt_speckle3d_weights, mcrt_speckle3d_tables, mcrt_speckle_volume_frames
                                   (3-D speckle reduction: the diffusion of mcrt_speckle_frames over voxel blocks, six neighbours, a weight per axis; additive);
                                   + mcrt_autogain_opts, mcrt_default_autogain_opts, mcrt_autogain_curve, mcrt_autogain_frames (automatic gain: a depth gain
                                   curve estimated from each frame's own amplitude histograms, and the frame's penetration depth; additive);
                                   + mcrt_bands, mcrt_default_bands, mcrt_psf_band_kernels, mcrt_convolve_bands_frames, mcrt_band_fold_frames
                                   (frequency compounding and the depth downshift: an axial kernel per RF row and per band; additive);
                                   + mcrt_detect_opts, mcrt_default_detect_opts, mcrt_detect_taps, mcrt_detect_gain, mcrt_psf_carrier, mcrt_detect_frames
                                   (quadrature detection: an FIR Hilbert transformer along the scan-line, the envelope and the I/Q pair; additive);
                                   + mcrt_flow_opts, mcrt_default_flow_opts, mcrt_flow_nyquist, mcrt_flow_phasors, mcrt_flow_draws, mcrt_colour_map,
                                   mcrt_flow_split_frames, mcrt_flow_frames, mcrt_colour_opts, mcrt_default_colour_opts, mcrt_colour_frames
                                   (colour Doppler: a slow-time ensemble synthesised from one traced frame, the Kasai autocorrelator, the flow overlay and
                                   the true axial velocity per sample; additive);
                                   + mcrt_spectral_opts, mcrt_default_spectral_opts, mcrt_gate, mcrt_spectral_rotor, mcrt_spectral_phase, mcrt_spectral_profile,
                                   mcrt_spectral_rates, mcrt_spectral_window, mcrt_spectral_twiddles, mcrt_spectral_draws, mcrt_pulse_waveform,
                                   mcrt_spectral_series_frames, mcrt_spectral_frames, mcrt_sonogram_opts, mcrt_default_sonogram_opts, mcrt_sonogram_frames
                                   (spectral Doppler: a sample gate's slow-time series under a pulsatile waveform and a velocity profile, its short-time
                                   FFT and the sonogram; additive);
                                   + mcrt_strain_opts, mcrt_default_strain_opts, mcrt_strain_table, mcrt_strain_draws, mcrt_strain_map,
                                   mcrt_strain_compress_frames, mcrt_strain_frames, mcrt_elastogram_opts, mcrt_default_elastogram_opts, mcrt_elastogram_frames
                                   (strain elastography: a quasi-static compression synthesised from one traced frame, speckle tracking by normalised
                                   cross-correlation, the strain, its ground truth and the elastogram; additive);
                                   + mcrt_shear_opts, mcrt_default_shear_opts, mcrt_shear_table, mcrt_shear_pitch, mcrt_shear_shape, mcrt_shear_decay,
                                   mcrt_shear_draws, mcrt_shear_map, mcrt_shear_wave_frames, mcrt_shear_speed_frames
                                   (shear-wave elastography: a push, the shear wave tracked over slow time from one traced frame, the time to peak,
                                   the shear speed, the modulus and their ground truth; additive);
                                   + mcrt_mline, mcrt_mmode_opts, mcrt_default_mmode_opts, mcrt_mmode_table, mcrt_mmode_waveform, mcrt_mmode_bulk, mcrt_mmode_draws,
                                   mcrt_mmode_display_opts, mcrt_default_mmode_display_opts, mcrt_mmode_rows, mcrt_mmode_lines_frames, mcrt_mmode_picture_frames
                                   (M-mode: tissue that moves over slow time, the pulses of one scan-line synthesised from one traced frame, the sweep
                                   display and its ground truth; additive) */

typedef enum {
    MCRT_OK = 0,
    MCRT_ERR_INVALID = -1,      /* bad argument / call order               */
    MCRT_ERR_HIP = -2,          /* HIP runtime error (message has details) */
    MCRT_ERR_NOMEM = -3,
    MCRT_ERR_NO_DEVICE = -4,
    MCRT_ERR_LIMIT = -5         /* a documented capacity was exceeded      */
} mcrt_status;

typedef struct mcrt_ctx mcrt_ctx;

/* Run-time form of the reference's compile-time constants (main.cpp:23-37, ray.h:23-24,
 * scene.h:49, scene.cpp:115).  mcrt_default_params() fills the reference values. */
typedef struct {
    uint32_t n_elements;         /* E: scan-lines = transducer elements = RF columns (512)   */
    uint32_t n_samples;          /* S: Monte-Carlo sample paths per scan-line (5)            */
    uint32_t max_depth;          /* B: ray::max_depth (10), <= 16                            */
    uint32_t n_rows;             /* R: RF rows (465 = max_rows), <= 2048                     */
    float    frequency;          /* MHz (4.5)                                                */
    float    intensity_epsilon;  /* 1e-10                                                    */
    float    initial_intensity;  /* 1.0                                                      */
    float    ray_start_offset;   /* 0.1 (scene.cpp:115)                                      */
    uint32_t speed_of_sound;     /* um/us (1500)                                             */
    double   depth_cm;           /* 15                                                       */
    uint32_t seed;               /* RNG key word 0; key word 1 is the frame id               */
    uint32_t sanitize_tir;       /* 0 = reference behaviour: NaN echo on total internal reflection */
    uint32_t tex_n;              /* texture edge in voxels (256)                             */
    float    tex_res;            /* voxel edge, scene units (0.145)                          */
} mcrt_params;

/* mesh.h:12-20 reduced to what the hot path reads */
typedef struct { uint32_t mat_inside, mat_outside, vascular, _pad; } mcrt_mesh;

/* 64-byte BVH2 node.  child >= 0: inner node index; child < 0: leaf, v = ~child,
 * first triangle = v >> 3, count = (v & 7) + 1 (positions in leaf order). */
typedef struct {
    float lo0[3]; int32_t c0;
    float hi0[3]; int32_t c1;
    float lo1[3]; uint32_t pad0;
    float hi1[3]; uint32_t pad1;
} mcrt_bvh_node;

typedef struct {
    uint32_t n_nodes, n_tri, max_depth;
    float pad_abs;           /* absolute part of the per-triangle bounds padding (4e-6 * scene scale) */
    mcrt_bvh_node *nodes;    /* [n_nodes]                                                     */
    float *tri;              /* [n_tri][12] leaf order: v0.xyz,bits(tri id) | v1.xyz,bits(mesh id) | v2.xyz,0 */
} mcrt_bvh;

/* 128-byte BVH4 node, the BUILDERS' form: four 32-byte child records with float boxes -- what mcrt_build_bvh4 and the device builder
 * emit, what a refit updates and what this ABI exports.  The GPU walk reads a 64-byte copy made from it after every build / refit
 * (child-transposed half-float boxes rounded outwards, csrc/mcrt_walk.hip k_nodes_walk); mcrt_get_bvh4 hands out that copy decoded
 * back into this form, i.e. the tree exactly as walked.  ref: >= 0 inner node; < 0 leaf (as in mcrt_bvh_node, at most 4 triangles);
 * MCRT_BVH4_EMPTY = unused slot.  Built by collapsing the SAH BVH2. */
#define MCRT_BVH4_EMPTY ((int32_t)0x80000000)
typedef struct { float lo[3]; float hi_x; float hi_y, hi_z; int32_t ref; uint32_t pad; } mcrt_bvh4_child;
typedef struct { mcrt_bvh4_child c[4]; } mcrt_bvh4_node;
typedef struct {
    uint32_t n_nodes, max_stack;   /* max_stack: worst-case traversal stack entries for this tree */
    mcrt_bvh4_node *nodes;
} mcrt_bvh4;

/* ray_physics::segment (ray.h:28-36) as a POD; media is the material INDEX in effect along it */
typedef struct {
    float from[3], to[3], dir[3];
    float reflected_intensity, initial_intensity, attenuation;
    double distance_traveled;
    int32_t media;
    int32_t tri;             /* triangle hit at the end of the segment, -1 = none */
} mcrt_segment;              /* 64 bytes */

typedef struct {
    uint64_t queries, nodes_visited, tris_tested, segments, rf_steps, hits;
} mcrt_stats;

const char *mcrt_last_error(void);
int mcrt_version(void);
int mcrt_device_count(void);

int mcrt_create(int device, mcrt_ctx **out);
int mcrt_destroy(mcrt_ctx *ctx);
/* The stream every asynchronous entry point enqueues on.  Calls are ordered on the stream they were issued on; the one cross-stream
 * guarantee: a trace issued after mcrt_set_stream waits for the device work of the last scene upload / update / refit wherever that ran.
 *  NULL = the context's own (non-blocking) stream -- NOT the legacy
 * default stream: to order the kernels with work on HIP's legacy stream pass hipStreamLegacy explicitly, and with a
 * framework's stream (torch.cuda.Stream().cuda_stream) pass that handle. */
int mcrt_set_stream(mcrt_ctx *ctx, void *hip_stream);
/* Waits for the context's stream AND reads the context's device error word: MCRT_ERR_LIMIT when a launch since the last call was
 * abandoned (a persistent kernel's watchdog expired, a traversal stack ran out).  A caller that synchronises by other means (its own
 * stream, a framework's synchronize) must still call this to learn of such a launch; until it does -- the call clears the word --
 * every RF image the context finalises is NaN throughout, so that a broken frame cannot pass for an image. */
int mcrt_synchronize(mcrt_ctx *ctx);

int mcrt_default_params(mcrt_params *p);
int mcrt_set_params(mcrt_ctx *ctx, const mcrt_params *p);
int mcrt_get_params(mcrt_ctx *ctx, mcrt_params *out);           /* the parameters in effect */

/* Which builder mcrt_upload_scene / mcrt_update_triangles use for the BVH that replaces the per-mesh
 * btBvhTriangleMeshShape of scene.cpp:306-309:
 *   MCRT_BVH_HOST_SAH     binned-SAH build on the host (default; best trees, seconds for 1 M triangles)
 *   MCRT_BVH_DEVICE_LBVH  Morton-order LBVH built on the GPU (milliseconds; for moving geometry, the interactive path
 *                         the reference prepares in inputmanager.cpp:117-121 / transducer.h:82-118).  Needs >= 8 triangles.
 * Images do not depend on the builder: the closest-hit contract is independent of the hierarchy. */
enum { MCRT_BVH_HOST_SAH = 0, MCRT_BVH_DEVICE_LBVH = 1 };
int mcrt_set_bvh_builder(mcrt_ctx *ctx, int builder);

/* Geometry in WORLD space (scene.cpp:313-324 already applied: v*scaling + deltas*scaling^2 + origin),
 * triangles in OBJ face order, meshes in scene order.  Builds the BVH (see mcrt_set_bvh_builder) and uploads it.
 * materials: [n_mat][8] = impedance, attenuation, mu0, mu1, sigma, specularity, shininess, thickness. */
int mcrt_upload_scene(mcrt_ctx *ctx, const float *tri_xyz /*[T][9]*/, const uint32_t *tri_mesh /*[T]*/, uint32_t n_tri,
                      const mcrt_mesh *meshes, uint32_t n_mesh, const float *materials, uint32_t n_mat,
                      uint32_t start_mat, const float spacing[3]);
/* New vertex positions for the uploaded scene's triangles (same count, same order, same mesh / material tables):
 * re-indexes them with the selected builder.  tri_xyz may be a host or a device pointer. */
int mcrt_update_triangles(mcrt_ctx *ctx, const float *tri_xyz /*[T][9]*/, uint32_t n_tri);
/* The same, keeping the uploaded tree: every box is refitted bottom-up on the GPU around the moved triangles (about a
 * millisecond for 1 M triangles).  Right for deformations that keep the neighbourhoods intact; frames are exact either way,
 * only the walk gets slower when the tree no longer matches the geometry.  tri_xyz may be a host or a device pointer. */
int mcrt_refit_triangles(mcrt_ctx *ctx, const float *tri_xyz /*[T][9]*/, uint32_t n_tri);
/* voxels [n^3][2] = {texture_noise, scattering_probability}; NULL => generate the reference's texture */
int mcrt_upload_texture(mcrt_ctx *ctx, const float *voxels, uint32_t n);
int mcrt_set_transducer(mcrt_ctx *ctx, const float *pos /*[E][3]*/, const float *dir /*[E][3]*/, uint32_t n_elements);

/* clear + trace + accumulate for scan-lines [e_begin, e_end).  rf_dev: device float [(e_end-e_begin)][R]
 * (scan-line-major).  Asynchronous on the context's stream. */
int mcrt_trace_frame(mcrt_ctx *ctx, uint32_t frame_id, uint32_t e_begin, uint32_t e_end, float *rf_dev);
/* n_frames consecutive frames (ids frame_id .. frame_id+n_frames-1, same scene and probe pose) traced as ONE pass: every
 * stage of the pipeline then runs over n_frames times the rays, which is what fills the GPU when a single frame is small.
 * rf_dev: device float [n_frames][(e_end-e_begin)][R].  Each image is bit-identical to the one mcrt_trace_frame produces.
 * Limits (MCRT_ERR_LIMIT beyond them): n_frames <= 1024 and n_frames x scan-lines x samples <= 2^27 paths per pass (a path takes
 * about 600 bytes of work buffers). */
int mcrt_trace_frames(mcrt_ctx *ctx, uint32_t frame_id, uint32_t n_frames, uint32_t e_begin, uint32_t e_end, float *rf_dev);
/* The same pass with a probe pose PER FRAME: pos / dir are [n_frames][E][3] tables (host or device memory), frame f of the pass is
 * traced from the elements pos[f], dir[f] -- the moving probe the reference's loop is built for (transducer<N>::update(),
 * transducer.h:82-118; inputmanager.cpp:117-121; the frame loop main.cpp:92-152 reads the transducer anew every frame).  Each image is
 * bit-identical to mcrt_set_transducer(pos[f], dir[f]) followed by mcrt_trace_frame(frame_id + f).  The context's own transducer
 * (mcrt_set_transducer) is neither needed nor changed. */
/* Lifetime: a table in HOST memory is copied before the call returns (free or rewrite it at once); a table in DEVICE memory is read by
 * the pass on the context's stream -- keep it unchanged until that work has finished. */
int mcrt_trace_frames_poses(mcrt_ctx *ctx, uint32_t frame_id, uint32_t n_frames, uint32_t e_begin, uint32_t e_end,
                            const float *pos /*[F][E][3]*/, const float *dir /*[F][E][3]*/, float *rf_dev);
/* same, and additionally returns per-path data to HOST buffers (any may be NULL); synchronous.
 * hits [ne][S][B] int32 (-1 miss, -2 not cast); segs [ne][S][B]; seg_count [ne][S]. */
int mcrt_trace_frame_debug(mcrt_ctx *ctx, uint32_t frame_id, uint32_t e_begin, uint32_t e_end, float *rf_dev,
                           int32_t *hits, mcrt_segment *segs, uint32_t *seg_count);
/* scene::cast_rays (scene.cpp:50-183) alone: segments only, no RF accumulation; synchronous */
int mcrt_cast_rays(mcrt_ctx *ctx, uint32_t frame_id, uint32_t e_begin, uint32_t e_end,
                   mcrt_segment *segs, uint32_t *seg_count, int32_t *hits);

/* rf_image::convolve (rfimage.h:93-123) in place on a device image [E][R]; tmp_dev same size or NULL */
int mcrt_convolve(mcrt_ctx *ctx, float *rf_dev, uint32_t n_elements, uint32_t n_rows,
                  const float *axial, uint32_t n_ax, const float *lateral, uint32_t n_lat);
/* the same on the n_frames images [n_frames][E][R] of an mcrt_trace_frames pass, in one launch per convolution pass */
int mcrt_convolve_frames(mcrt_ctx *ctx, float *rf_dev, uint32_t n_frames, uint32_t n_elements, uint32_t n_rows,
                         const float *axial, uint32_t n_ax, const float *lateral, uint32_t n_lat);
/* ---- focal zones: a depth-dependent lateral PSF (psf.h:17-24 plans it: "lateral and elevation ranges vary according to distance to
 * the transducer"; psf.h:34-58 builds one constant kernel).  The axial taps stay mcrt_psf_kernels' own.  RF row r lies at depth
 * z_r = r * row_mm (path length, as the reference's row index; row_mm = the context's axial resolution in mm, 0.322 at 4.5 MHz) and gets
 * its own n_lat lateral taps, at mcrt_psf_kernels' positions and spacing (res_um):
 *   z_f(r)    the focus nearest to z_r (on a tie the shallower one); none when n_focus = 0
 *   q         (z_r - z_f(r)) / focal_range_mm, in double; q = 0 when n_focus = 0
 *   var(r)    (double)var_y * (1 + q*q)
 *   g         sqrt(var_y / var(r))                         the area-preserving gain of a widening Gaussian
 *   lat[r][i] (float)(g * exp(-0.5f * (y_i^2 / var(r))))    y_i as mcrt_psf_kernels, y_i^2 in double
 * At a focal row (q = 0), and on every row when n_focus = 0, var(r) == var_y and g == 1: the row equals mcrt_psf_kernels' lateral taps
 * bit for bit.  focal_range_mm sets how fast the beam widens away from a focus; it has no default that the reference backs (a Gaussian
 * beam's Rayleigh range from var_y = 0.2 mm^2 at 4.5 MHz, about 3.8 mm, blurs nearly the whole image): the wrappers use 20 mm, a display
 * choice no measurement backs.  The elevation kernel (var_z) is modelled by the slice-thickness block below (elevation planes). */
typedef struct {
    uint32_t n_focus;            /* 0..8                                                    */
    float    focus_mm[8];        /* the first n_focus: finite, >= 0, strictly ascending      */
    float    focal_range_mm;     /* > 0 and finite when n_focus > 0                         */
} mcrt_focus;                    /* 40 bytes: n_focus at offset 0, focus_mm at 4, focal_range_mm at 36 */
/* the table lat_rows [n_rows][n_lat] (row-major) of the model above; host only, no GPU needed.  MCRT_ERR_INVALID for a null f / lat_rows,
 * n_focus > 8, foci that are not finite, negative or not strictly ascending, focal_range_mm <= 0 or not finite (when n_focus > 0), var_y
 * <= 0 or not finite, row_mm <= 0 or not finite, n_lat outside 1..32; MCRT_ERR_LIMIT for n_rows > 2048.  On an error lat_rows is untouched. */
int mcrt_psf_focus_kernels(float var_y, uint32_t res_um, const mcrt_focus *f, uint32_t n_rows, double row_mm,
                           float *lat_rows /* [n_rows][n_lat] */, uint32_t n_lat);
/* mcrt_convolve_frames with one row of lateral taps per RF row: lat_rows is host memory [n_rows][n_lat] (mcrt_psf_focus_kernels, or any
 * table).  The reference's index ranges and order of operations: the axial pass of mcrt_convolve_frames unchanged, then for output rows
 * [n_ax, R-n_ax) and columns [n_lat/2, E-n_lat)  img[col][row] = sum_k tmp[col+k][row] * lat_rows[row][k], summed in k order with one
 * rounding per multiply and per add.  A table whose rows all equal `lateral` gives mcrt_convolve_frames' image bit for bit.  Pixels
 * outside those ranges keep their bits.  Limits and errors are mcrt_convolve_frames' (taps 1..16 axial and 1..32 lateral, MCRT_ERR_LIMIT),
 * plus MCRT_ERR_INVALID for a null lat_rows and MCRT_ERR_LIMIT for n_rows > 2048; on any error nothing is launched and the image is
 * untouched.  Asynchronous on the context's stream; lat_rows may be rewritten once the call returns.  The table is copied to the device
 * only when it differs from the one there (a new table waits for the upload of the previous one); nothing is allocated once the table
 * buffer (2048 x 32 floats, made by the first call) and the scratch of mcrt_convolve exist.  Groups: call it on mcrt_group_root(). */
int mcrt_convolve_frames_depth(mcrt_ctx *ctx, float *rf_dev, uint32_t n_frames, uint32_t n_elements, uint32_t n_rows,
                               const float *axial, uint32_t n_ax, const float *lat_rows /* host [n_rows][n_lat] */, uint32_t n_lat);
/* ---- slice thickness: elevation planes and the elevation PSF (psf.h:16-18 names the elevation range, psf.h:42 takes var_z, psf.h:77
 * declares elevation_kernel; the reference never fills or applies it: its rf_image is two-dimensional, every frame the echo of an
 * infinitely thin sheet).  A frame with slice thickness is K parallel copies of the probe, spread along its elevation direction, traced
 * as ONE pose pass (mcrt_trace_frames_poses / mcrt_group_trace_frames_poses) into a stack [K][E][R] and folded into one RF image with the
 * elevation weights BEFORE mcrt_convolve*: a target beside the image plane then shows up in the picture (the partial-volume artefact).
 * The planes are parallel: the rays are not steered in elevation, the lens is modelled by the weights alone.
 *
 * The frame-id rule (applied by the wrappers: Simulator(elevation=True), rf_image::trace(frame, transducer, psf), mattausch_hip
 * --elevation): image f of a pass that starts at frame id f0 traces its plane k with frame id (f0 + f) * K + k -- every plane has its own
 * random streams (the tissue beside the plane is other tissue), and frame f is the same picture traced alone or inside a pass.  The
 * limits of mcrt_trace_frames_poses then apply to n_frames * K (1024 frames, 2^27 paths). */
/* (psf.h:16-18,42,77) the probe's elevation direction: the vector (0,0,1) taken through the three rotations of mcrt_transducer_elements,
 * in its order and float arithmetic (about z by angles_deg[2], about x by angles_deg[0], about y by angles_deg[1]).  Exactly (0,0,1) for
 * angles (0,0,a).  Host only.  MCRT_ERR_INVALID for a null pointer. */
int mcrt_transducer_elevation_axis(const float angles_deg[3], float axis[3]);
/* (psf.h:16-18,42,77) K parallel copies of an element table, plane k shifted along `axis` by
 *   z_k = (float)(((double)k - (double)((K - 1) / 2)) * (double)pitch_um / 1000.0)   [mm]   ((K - 1) / 2 an integer division: z = 0 at plane (K-1)/2)
 *   o_k = (float)((double)z_k / 10.0)                                                 scene units (cm, as the radius of transducer.h:24-62)
 *   pos_out[k][e][c] = pos[e][c] + o_k * axis[c]   one float multiply and one float add, not fused;   dir_out[k][e] = dir[e]
 * z_mm_out [K] receives z_k (may be NULL).  K = 1 is the probe's own plane: the input table bit for bit.  CENTRED positions are a deliberate
 * departure from the off-centre tap positions of psf.h:40-57 (i * res - size * res / 2): those belong to the forward-looking windows of
 * rf_image::convolve, while a plane is a place in the scene.  Host only.  MCRT_ERR_INVALID for a null pos / dir / axis / pos_out / dir_out,
 * n_elements == 0, K outside 1..32, pitch_um == 0, an axis that is not finite; on an error nothing is written. */
int mcrt_elevation_planes(const float *pos /*[E][3]*/, const float *dir /*[E][3]*/, uint32_t n_elements, const float axis[3], uint32_t n_planes,
                          uint32_t pitch_um, float *pos_out /*[K][E][3]*/, float *dir_out /*[K][E][3]*/, float *z_mm_out /*[K] or NULL*/);
/* (psf.h:16-18,42,77) the elevation weights w_rows [n_rows][K] (row-major), one row per RF row: the depth model of mcrt_psf_focus_kernels
 * (z_r = r * row_mm, the nearest focus, q, var(r) = var_z (1 + q*q), g = sqrt(var_z / var(r)), all in double; f == NULL or n_focus == 0:
 * q = 0 on every row -- an acoustic lens has one fixed elevation focus, so n_focus is normally 0 or 1) at the plane positions z_k of
 * mcrt_elevation_planes:
 *   v[r][k] = g * exp(-0.5 * (z_k^2 / var(r)))      in double, z_k^2 in double from the float z_k
 *   w[r][k] = (float)v[r][k]                        normalize == 0: as the reference leaves its lateral taps; the centre weight is exactly 1 without foci
 *   w[r][k] = (float)(v[r][k] / (v[r][0] + v[r][1] + ...))   normalize != 0: the sum in k order and the division in double, one rounding;
 *                                                   tissue that does not vary across the slice keeps its brightness
 * Rows are symmetric bit for bit for odd K.  Host only.  MCRT_ERR_INVALID for a null w_rows, K outside 1..32, pitch_um == 0, var_z <= 0 or not
 * finite, row_mm <= 0 or not finite, and mcrt_psf_focus_kernels' conditions on *f when it is given; MCRT_ERR_LIMIT for n_rows > 2048.  On an
 * error w_rows is untouched. */
int mcrt_psf_elevation_kernels(float var_z, uint32_t pitch_um, const mcrt_focus *f /* or NULL */, uint32_t n_rows, double row_mm, int normalize,
                               float *w_rows /* [n_rows][K] */, uint32_t n_planes);
/* (psf.h:16-18,42,77) folds the K plane images of every frame:
 *   rf[f][e][r] = sum over k = 0..K-1 of planes[f][k][e][r] * w_rows[r][k]
 * summed in k order starting from 0.0f, one float rounding per multiply and per add, no fma (the rule of mcrt_convolve_frames_depth).
 * So a NaN or an infinity in any plane reaches the output even under a zero weight (a scan-line the reference turns NaN by total internal
 * reflection stays NaN), and K = 1 with weight 1 copies the image (a -0.0 becomes +0.0).  Every (f, e, r) is written: there are no borders.
 * planes_dev [n_frames][K][E][R] and rf_dev [n_frames][E][R] are device memory and must not overlap (MCRT_ERR_INVALID); w_rows is host
 * memory (mcrt_psf_elevation_kernels, or any table) and may be rewritten once the call returns.  Asynchronous on the context's stream.
 * MCRT_ERR_INVALID for null pointers and zero sizes, MCRT_ERR_LIMIT for K > 32, n_rows > 2048 or a stack of 2^40 floats or more; on an
 * error nothing is launched and rf_dev is untouched.  The table lives on the device (tap-major, a buffer of its own beside the focal zones'
 * so that a frame using both uploads neither) and is copied only when it differs from the one there (a new table waits for the upload of
 * the previous one); nothing is allocated after the first call.  Groups: call it on mcrt_group_root() after mcrt_group_trace_frames_poses. */
int mcrt_elevation_frames(mcrt_ctx *ctx, const float *planes_dev /* [n_frames][K][E][R] */, uint32_t n_frames, uint32_t n_planes,
                          uint32_t n_elements, uint32_t n_rows, const float *w_rows /* host [n_rows][K] */, float *rf_dev /* [n_frames][E][R] */);
/* ---- frequency compounding and the depth downshift: an axial kernel per RF row and per band (psf.h:34-58 builds one axial kernel, the
 * same at every depth).  The received band is split into B sub-bands; the RF stack of a traced pass is convolved with each band's pulse
 * (mcrt_convolve_bands_frames), every band image is detected on its own (mcrt_envelope_frames over the F * B images) and the detected
 * images are averaged (mcrt_band_fold_frames): speckle decorrelates between bands and falls, at the price of axial resolution.  No second
 * trace is needed.  Folding the band images WITHOUT the envelope between is a coherent sum: linear, the same as one convolution with the
 * weighted sum of the pulses, and it reduces no speckle.
 *
 * RF row r lies at depth z_r = (double)r * row_mm (the rule of mcrt_psf_focus_kernels).  Band b at row r has, in double, the centre frequency
 *   f(b, r)        = max((double)min_mhz, (double)band_mhz[b] - (double)downshift_mhz_per_mm * z_r)
 *   ax_rows[b][r][i] = (float)(exp(-0.5f * (x_i^2 / (double)var_x)) * cos(2 * 3.14159 * f(b, r) * (double)x_i))
 * mcrt_psf_kernels' axial expression -- its x_i, half_ax, 3.14159 and order of operations -- with f(b, r) in the place of (double)freq: a
 * band at freq with downshift 0 and min_mhz <= freq equals mcrt_psf_kernels(freq, var_x, ...)'s axial taps bit for bit on every row.  The
 * formula multiplies MHz by mm as the reference's does; a band is what the formula gives, not a calibrated spectrum.
 *   w_rows[r][b]   = (float)((double)band_weight[b] / S),   S the double sum of the weights in b order
 * the same on every row (the table has the shape mcrt_elevation_frames takes: a caller may hand mcrt_band_fold_frames a depth-dependent blend
 * of their own).  downshift_mhz_per_mm has no default that the reference backs: the wrappers use 0 and a value is the caller's choice. */
typedef struct {
    uint32_t n_bands;               /* 1..8 */
    float    band_mhz[8];           /* centre frequency of band b at the probe's face: finite, > 0 (any order) */
    float    band_weight[8];        /* finite, >= 0, their sum > 0 */
    float    var_x;                 /* mm^2, axial variance of every band's pulse: finite, > 0 */
    float    downshift_mhz_per_mm;  /* finite, >= 0: how fast the centre frequency falls with depth */
    float    min_mhz;               /* finite, >= 0: the frequency stops falling here */
} mcrt_bands;                       /* 80 bytes: n_bands 0, band_mhz 4, band_weight 36, var_x 68, downshift 72, min_mhz 76 */
/* one band at freq, weight 1, no downshift, min_mhz 0 (the other entries 0).  MCRT_ERR_INVALID for a null b. */
int mcrt_default_bands(mcrt_bands *b, float freq, float var_x);
/* the tables of the model above; host only, no GPU needed.  w_rows may be NULL.  MCRT_ERR_INVALID for a null b / ax_rows, n_bands outside
 * 1..8, any field outside the ranges above, res_um == 0, row_mm <= 0 or not finite, n_ax outside 1..16; MCRT_ERR_LIMIT for n_rows > 2048.
 * On an error nothing is written. */
int mcrt_psf_band_kernels(const mcrt_bands *b, uint32_t res_um, uint32_t n_rows, double row_mm,
                          float *ax_rows /* [B][n_rows][n_ax] */, uint32_t n_ax, float *w_rows /* [n_rows][B] or NULL */);
/* bands_dev[f][b] is the image that mcrt_convolve_frames (lateral given) or mcrt_convolve_frames_depth (lat_rows given) leaves from
 * rf_dev[f], with row r's own axial taps:  tmp[e][r] = sum_k rf[e][r+k] * ax_rows[b][r][k]  for r in [n_ax, R-n_ax), summed in k order from
 * 0.0f, one rounding per multiply and per add, no fma; the lateral pass is unchanged.  Pixels outside the convolved windows hold rf_dev's own
 * bits (NaN and -0.0 included).  When the rows of ax_rows[b] all equal one `axial`, bands_dev[f][b] equals the existing call's image bit for
 * bit at every pixel.  rf_dev [F][E][R] is read only; bands_dev [F][B][E][R] must not overlap it (MCRT_ERR_INVALID).  Exactly one of
 * lateral [n_lat] / lat_rows [R][n_lat] is non-null (MCRT_ERR_INVALID otherwise).  Limits and errors are mcrt_convolve_frames_depth's, plus
 * MCRT_ERR_INVALID for n_bands outside 1..8, and MCRT_ERR_LIMIT for a band stack of 2^40 floats or more; on any error nothing is launched and
 * nothing is written.  Asynchronous on the context's stream; the caller may rewrite its tables as soon as the call returns.  The tables live on
 * the device tap-major -- the axial table [B][n_ax][R] in a buffer of its own (8 x 16 x 2048 floats, made by the first call), lat_rows in
 * mcrt_convolve_frames_depth's -- and are copied only when they differ from the ones there; nothing is allocated once the table buffers and
 * the scratch (F * B * E * R floats) exist.  Groups: call it on mcrt_group_root(). */
int mcrt_convolve_bands_frames(mcrt_ctx *ctx, const float *rf_dev /* [F][E][R] */, uint32_t n_frames, uint32_t n_elements, uint32_t n_rows,
                               uint32_t n_bands, const float *ax_rows /* host [B][R][n_ax] */, uint32_t n_ax,
                               const float *lateral /* host [n_lat] or NULL */, const float *lat_rows /* host [R][n_lat] or NULL */, uint32_t n_lat,
                               float *bands_dev /* [F][B][E][R] */);
/* folds the B band images of every frame:  rf[f][e][r] = sum over b of bands[f][b][e][r] * w_rows[r][b].  The contract is
 * mcrt_elevation_frames' word for word with K = B (the sum in b order from 0.0f, one rounding per multiply and per add; a NaN reaches the
 * output under a zero weight; B = 1 with weight 1 copies, a -0.0 becomes +0.0; no borders; the buffers must not overlap), except that
 * n_bands is 1..8 (MCRT_ERR_INVALID outside).  The weights have a device table of their own beside the elevation weights', so that a frame
 * with slice thickness and bands uploads neither twice. */
int mcrt_band_fold_frames(mcrt_ctx *ctx, const float *bands_dev /* [F][B][E][R] */, uint32_t n_frames, uint32_t n_bands,
                          uint32_t n_elements, uint32_t n_rows, const float *w_rows /* host [R][B] */, float *rf_dev /* [F][E][R] */);
/* rf_image::envelope (rfimage.h:54-91) in place on a device image [E][R].  n_rows <= 2048 (MCRT_ERR_LIMIT beyond: a wavefront holds
 * its scan-line in LDS) -- the limit mcrt_params.n_rows has anyway; an image brought in through mcrt_import_rf is bound by it too.
 * An image of n_rows < 2 has no peak to find and is left unchanged. */
int mcrt_envelope(mcrt_ctx *ctx, float *rf_dev, uint32_t n_elements, uint32_t n_rows);
/* the same on the n_frames images [n_frames][E][R] of a pass (main.cpp:147 once per frame), one launch */
int mcrt_envelope_frames(mcrt_ctx *ctx, float *rf_dev, uint32_t n_frames, uint32_t n_elements, uint32_t n_rows);
/* ---- quadrature detection: an FIR Hilbert transformer along the scan-line, the envelope and the I/Q pair.  rf_image::envelope calls itself
 * "a fast approximation of the hilbert transform": it joins the local maxima of the SAMPLES by straight lines.  The axial pulse of
 * mcrt_psf_kernels has its taps one RF row apart, so its carrier is freq * res_um / 1000 cycles per row -- 0.6525 at 4.5 MHz and 145 um, which
 * aliases to 0.3475: fewer than three rows per cycle.  The maxima of such samples beat against the carrier, and a reflector of constant
 * brightness is read as anything between half and all of it (DESIGN.md 5.19 has the table).  A scanner detects in quadrature: the RF line x
 * and its Hilbert transform q form the analytic signal, whose magnitude is the envelope and whose two parts are the I/Q data.  An opt-in
 * stage in the place of mcrt_envelope_frames; without it no call and no bit changes.
 *
 * The transformer is a type-III FIR (antisymmetric, odd length) under a Hamming window.  With M = (n_taps - 1) / 2, for odd m in 1..M, in
 * double with pi = 3.141592653589793:
 *   t_m = (float)((2.0 / (pi * m)) * (0.54 + 0.46 * cos(pi * m / (M + 1))))
 *   taps[M + m] = t_m,  taps[M - m] = -t_m;  every even offset, the centre included, is exactly +0.0f
 * Its magnitude response at f cycles per row is G(f) = |2 * sum over odd m of t_m * sin(2 pi f m)|: a line cos(w r) gives q = G sin(w r), and
 * the envelope sqrt(cos^2 + G^2 sin^2) stays within |G - 1| of 1.  At 31 taps G is within 1 % of 1 from 0.05 to 0.45 cycles per row, at 15
 * taps from 0.10 to 0.40.  THE LIMIT OF THE MODEL: G falls to 0 at 0 and at 0.5 (Nyquist), where a real line has no separable envelope at
 * all -- the 3.5 MHz band of three bands spanning 2 MHz about 4.5 has the carrier 0.4925 and G = 0.26 at 31 taps, and comes out darker
 * under this detector.  mcrt_psf_carrier and mcrt_detect_gain let a caller see that; the library does not refuse it. */
typedef struct { uint32_t n_taps; } mcrt_detect_opts;          /* 3, 7, 11, ..., 63 (n_taps % 4 == 3); default 31 */
/* n_taps = 31.  MCRT_ERR_INVALID for a null o.  Host only. */
int mcrt_default_detect_opts(mcrt_detect_opts *o);
/* the taps above; host only, no GPU needed.  MCRT_ERR_INVALID for a null pointer or an n_taps outside the set; on an error nothing is written. */
int mcrt_detect_taps(const mcrt_detect_opts *o, float *taps /* [n_taps] */);
/* *gain = G(cycles_per_row) of the taps given, in double: the sum over odd m in ascending order of (double)taps[M + m] * sin(2 pi f m), doubled,
 * its absolute value.  Host only.  MCRT_ERR_INVALID for a null pointer or an n_taps outside the set. */
int mcrt_detect_gain(const float *taps, uint32_t n_taps, double cycles_per_row, double *gain);
/* the digital carrier of mcrt_psf_kernels' axial pulse at freq_mhz, and of a band of mcrt_psf_band_kernels at the probe's face: with
 * c = (double)freq_mhz * ((double)res_um / 1000.0),  *cycles_per_row = |c - rint(c)|, in 0..0.5.  Host only.  MCRT_ERR_INVALID for a null pointer. */
int mcrt_psf_carrier(float freq_mhz, uint32_t res_um, double *cycles_per_row);
/* Per scan-line x[0..R) of the stack, with xz[i] = x[i] for 0 <= i < R and +0.0f outside:
 *   q[r]   = sum over m = 1, 3, 5, ... <= M, in ascending order, starting from 0.0f, of  (xz[r - m] - xz[r + m]) * t_m
 *   env[r] = sqrtf(x[r] * x[r] + q[r] * q[r])
 * the difference, every multiply and every add rounded once, no fma; the two squares and their sum rounded once each; the square root
 * correctly rounded.  env_dev[f][e][r] = env[r]; iq_dev[f][e][r][0] holds x[r]'s own bits and iq_dev[f][e][r][1] = q[r]: the analytic pair
 * at the RF rate, neither mixed to baseband nor decimated.  A NaN or an infinity at row r reaches the rows r +- m for odd m <= M (and, in
 * env and in I, row r itself) and no others; a scan-line that is NaN throughout -- the reference's total internal reflection -- stays NaN.
 * Every (f, e, r) is written: there are no borders, and any R >= 1 is allowed, R <= M included (rows near an end see the zeros of xz).
 * rf_dev [F][E][R] is device memory; env_dev may EQUAL rf_dev (detection in place, as mcrt_envelope_frames) and rf_dev is otherwise read
 * only; any other overlap between the three buffers is MCRT_ERR_INVALID.  At least one of env_dev and iq_dev must be given.
 * Asynchronous on the context's stream.  MCRT_ERR_INVALID for a null ctx, rf_dev or o, zero sizes, an n_taps outside the set, both outputs
 * null; MCRT_ERR_LIMIT for n_rows > 2048 (a wavefront holds its scan-line in LDS) or a stack of 2^40 floats or more; on any error nothing
 * is launched and nothing is written.  Nothing is allocated or uploaded by the call: the 16 distinct taps at most travel as kernel
 * arguments.  Groups: call it on mcrt_group_root(). */
int mcrt_detect_frames(mcrt_ctx *ctx, const float *rf_dev /* [F][E][R] */, uint32_t n_frames, uint32_t n_elements, uint32_t n_rows,
                       const mcrt_detect_opts *o, float *env_dev /* [F][E][R] or NULL */, float *iq_dev /* [F][E][R][2] or NULL */);
/* rf_image::postprocess scan conversion (rfimage.h:125-140,183-215), exact bilinear;
 * out_dev float [out_rows][out_cols] */
int mcrt_scan_convert(mcrt_ctx *ctx, const float *rf_dev, uint32_t n_elements, uint32_t n_rows,
                      double radius_mm, double total_angle_rad, float *out_dev, uint32_t out_rows, uint32_t out_cols);
/* rf_image::create_mapping (rfimage.h:183-215) alone, on the host (no GPU needed): map_row = the reference's map_x (ROW coordinate
 * in the RF image), map_col = its map_y (COLUMN coordinate), each [out_rows][out_cols] row-major -- what mcrt_scan_convert gathers
 * with.  max_travel_us / speed_of_sound are rf_image's unsigned template parameters (100, 1500; main.cpp:36). */
int mcrt_scan_maps(uint32_t n_elements, uint32_t n_rows, double radius_mm, double total_angle_rad, uint32_t max_travel_us,
                   uint32_t speed_of_sound, uint32_t out_rows, uint32_t out_cols, float *map_row, float *map_col);
/* the same on the n_frames images of a pass (main.cpp:148 once per frame), one launch; out_dev float [n_frames][out_rows][out_cols] */
int mcrt_scan_convert_frames(mcrt_ctx *ctx, const float *rf_dev, uint32_t n_frames, uint32_t n_elements, uint32_t n_rows,
                             double radius_mm, double total_angle_rad, float *out_dev, uint32_t out_rows, uint32_t out_cols);

/* ---- the displayed picture: log-compressed 8-bit B-mode frames (rfimage.h:131-136 planned it and left it commented out; rfimage.h:142-147
 * saves 8-bit grey).  An opt-in stage after mcrt_convolve_frames / mcrt_envelope_frames, in place of mcrt_scan_convert_frames. */
enum { MCRT_BMODE_DB = 0,        /* decibels below a reference amplitude: the clinical display                  */
       MCRT_BMODE_REF_LOG = 1 }; /* log10(a+1)/log10(ref+1): the reference's commented-out rfimage.h:131-136     */
typedef struct {
    uint32_t mode;               /* MCRT_BMODE_*                                                  (DB)       */
    float    dynamic_range_db;   /* DB: grey 0 at -DR dB below ref, > 0 and finite                (60)       */
    float    gain_db;            /* DB: added before the range is applied, finite                 (0)        */
    float    ref;                /* reference amplitude; <= 0: each frame's own peak (auto)       (0)        */
    float    persistence;        /* alpha in [0,1): temporal smoothing across frames              (0)        */
    uint32_t reset_state;        /* 1: the first frame of this call starts the smoothing afresh   (1)        */
    uint32_t out_rows, out_cols; /* scan-converted size                                           (400, 500) */
    double   radius_mm, total_angle_rad;  /* as mcrt_scan_convert                                (30, pi/3) */
} mcrt_bmode_params;             /* 48 bytes; the doubles at offsets 32 and 40 */
/* the defaults above; host only, no GPU needed */
int mcrt_default_bmode(mcrt_bmode_params *p);
/* rf_dev: device float [n_frames][n_elements][n_rows] (any image; normally enveloped) -> out_dev: device bytes [n_frames][out_rows][out_cols],
 * the row-major layout of mcrt_scan_convert_frames with one byte per pixel.  Asynchronous on the context's stream; every launch covers all the
 * frames (the grey level of each RF tap, then their scan conversion; the peaks first with the automatic reference).  For each frame f and
 * each RF tap v at (scan-line e, row r):
 *   1. amplitude   a = |v| * k[r], k[r] = (float)pow(10.0, tgc_db[r] / 20.0) computed in double on the host (1 without tgc_db); a NaN or
 *                  infinite a counts as no echo, a = 0 (the reference's NaN scan-lines, sanitize_tir = 0, neither blank a frame nor set its peak)
 *   2. reference   ref_f = p->ref if p->ref > 0, else the largest a of the frame (exact; order-independent).  ref_f == 0: the frame is black.
 *                  peak_dev[f] = ref_f when peak_dev is given.
 *   3. grey level  per tap, in float:  DB       g = a > 0 ? clamp((20.0f * log10f(a / ref_f) + gain_db + DR) / DR, 0, 1) : 0
 *                                      REF_LOG  g = clamp(log10f(a + 1.0f) / log10f(ref_f + 1.0f), 0, 1)
 *                  (clamp = fminf(fmaxf(x, 0), 1): a NaN quotient is 0)
 *   4. scan conversion of g: mcrt_scan_convert's bilinear expression, masks and maps (mcrt_scan_maps); taps outside the sector are 0.
 *                  Compression runs before interpolation, as on a scanner.
 *   5. persistence y_f = fmaf(alpha, y_{f-1}, (1 - alpha) * s_f), s_f = step 4's value; y_{-1} = state_dev unless reset_state is set or
 *                  state_dev is NULL, then y_{-1} = s_0.  state_dev (float [out_rows][out_cols], values in [0,1]) receives y_{n_frames-1}: two
 *                  calls of 2 frames equal one call of 4.  alpha = 0: y_f = s_f and the state is not read.
 *   6. quantisation out = (uint8_t)(y * 255.0f + 0.5f).
 * The log10f of the device may differ from a correctly rounded one in the last place: a grey level can then differ by one.
 * Limits: n_rows <= 2048 and n_frames <= 65535 (MCRT_ERR_LIMIT).  MCRT_ERR_INVALID, with a message, for a null rf_dev / out_dev / p, zero sizes,
 * an unknown mode, a dynamic range <= 0 or not finite, a gain or ref that is not finite, persistence outside [0,1), a non-finite tgc_db
 * entry, bad scan geometry.  On any error nothing is launched and out_dev, state_dev and peak_dev are untouched.
 * tgc_db is host memory [n_rows] and may be rewritten once the call returns; the factors live on the device until they change (a new
 * curve waits for the upload of the previous one).  The grey levels of a pass live in the context's scratch (the one mcrt_convolve uses,
 * grown to the largest pass); nothing is allocated once that and the maps of a geometry (shared with mcrt_scan_convert_frames) exist. */
int mcrt_bmode_frames(mcrt_ctx *ctx, const float *rf_dev, uint32_t n_frames, uint32_t n_elements, uint32_t n_rows,
                      const mcrt_bmode_params *p, const float *tgc_db /* host [n_rows] dB per RF row, or NULL */,
                      float *state_dev /* [out_rows][out_cols] smoothing state, or NULL */,
                      float *peak_dev  /* [n_frames]: the ref each frame used, or NULL */,
                      uint8_t *out_dev /* [n_frames][out_rows][out_cols] */);

/* ---- spatial compounding: the same plane insonified from several in-plane steering angles and the views averaged in image space, as every
 * current scanner does (speckle decorrelates between the looks, shadows narrow, oblique interfaces light up).  The reference has one look
 * direction: its beams leave the arc along its normals (transducer.h:24-62) and create_mapping (rfimage.h:183-215) knows only those.  A
 * compounded frame is N steered copies of the probe traced as ONE pose pass (mcrt_trace_frames_poses / mcrt_group_trace_frames_poses) into
 * a stack [N][E][R]; convolution and envelope run over the N views as over N frames; the views then meet in one gather through N map pairs.
 *
 * The frame-id rule (applied by the wrappers: Simulator(compound=...), rf_image::trace(frame, transducer, steers), mattausch_hip --compound):
 * view n of image f of a pass that starts at frame id f0 is traced with frame id (f0 + f) * N + n -- every look has its own random streams.
 * With elevation planes the views are outer: ((f0 + f) * N + n) * K + k; the fold then sees F * N frames and writes the [F][N][E][R] stack. */
typedef struct { uint32_t n_views;      /* 1..16 */
                 float    steer_rad[16];/* the first n_views: finite, |steer| < pi/2; any order, duplicates allowed */
} mcrt_compound;                        /* 68 bytes: n_views at offset 0, steer_rad at 4 */
/* mcrt_transducer_elements with every beam tilted in the image plane by steer_rad: the statements of mcrt_transducer_elements, except that
 * the DIRECTION is built from as = (float)(angle + (double)steer_rad) -- (sin(as), cos(as), 0) through the same three rotations -- while the
 * POSITION still uses a = (float)angle.  The beams pivot on their elements; a positive steer tilts towards higher element numbers.
 * steer_rad == 0 gives mcrt_transducer_elements' tables bit for bit.  Host only.  Errors: mcrt_transducer_elements' own, plus
 * MCRT_ERR_INVALID for a steer that is not finite or has |steer| >= pi/2; on an error nothing is written. */
int mcrt_transducer_steered(uint32_t n_elements, double radius_cm, double separation_mm, const float position[3], const float angles_deg[3],
                            float steer_rad, float *pos, float *dir);
/* the scan-conversion maps of a steered view (layout and arguments of mcrt_scan_maps).  steer_rad == 0 CALLS mcrt_scan_maps: the unsteered
 * maps bit for bit.  Otherwise ratio, shift_y, half_width, fi, fj, radius_f and depth_mm_f are mcrt_scan_maps' own floats; everything else
 * is double, rounded once to float at the end:
 *   x = (double)fj * ratio,  y = (double)fi * ratio           the pixel, mm from the arc's centre
 *   rho = sqrt(x*x + y*y),   alpha = atan2(x, y),   q = radius_mm * sin(steer)
 *   phi = alpha - steer + asin(q / rho)                       arc angle of the element whose steered beam passes the pixel
 *   t   = sqrt(rho*rho - q*q) - radius_mm * cos(steer)        path length along that beam, mm
 *   map_row = (float)(t / depth_mm_f * R),   map_col = (float)((phi + total_angle/2) / total_angle * (double)(float)E)
 * (P = radius u(phi) + t u(phi + steer); crossing with u(phi + steer): rho sin(phi + steer - alpha) = radius sin(steer); the principal
 * branch is the forward beam.)  Where rho < |q| no beam passes the pixel: both maps are NaN, which the gather treats as unmapped.  The
 * half-scan-line offset of the reference's column convention (rfimage.h:212) is kept.  Host only.  MCRT_ERR_INVALID for mcrt_scan_maps'
 * conditions and a steer that is not finite or has |steer| >= pi/2; on an error nothing is written. */
int mcrt_compound_maps(uint32_t n_elements, uint32_t n_rows, double radius_mm, double total_angle_rad, uint32_t max_travel_us,
                       uint32_t speed_of_sound, uint32_t out_rows, uint32_t out_cols, float steer_rad, float *map_row, float *map_col);
/* The N views of every frame gathered through their N map pairs into one float image.  rf_dev: device float [n_frames][N][E][R];
 * out_dev: device float [n_frames][out_rows][out_cols].  Asynchronous on the context's stream, one launch.  Per frame f and output pixel:
 *   sum = 0.0f; cnt = 0
 *   for n = 0..N-1:  p = the pixel's point in view n's maps (mcrt_scan_convert's floor and fractions)
 *                    covered = both maps not NaN && p.x0 >= -1 && p.x0 < E && p.y0 >= -1 && p.y0 < R        (at least one tap inside)
 *                    if covered: sum = sum + (mcrt_scan_convert's bilinear expression on view n of frame f);  cnt++
 *   out = cnt ? sum / (float)cnt : 0.0f
 * in n order, one rounding per operation, no fma.  A NaN tap reaches its pixel, as in mcrt_scan_convert.  N = 1 with steer 0 equals
 * mcrt_scan_convert_frames bit for bit, except that a -0.0 becomes +0.0.  Per-view weights, a lateral edge ramp, max and median compounding:
 * mcrt_compound_frames_opts below; this call is that one with the default options.
 * MCRT_ERR_INVALID for null pointers, zero sizes, n_views outside 1..16, a steer that is not finite or has |steer| >= pi/2, bad scan
 * geometry, rf_dev overlapping out_dev; MCRT_ERR_LIMIT for n_rows > 2048 or n_frames * N > 65535.  On any error nothing is launched and
 * out_dev is untouched.  The N map pairs live on the device in a buffer of their own beside the plain maps (alternating this call with
 * mcrt_scan_convert_frames uploads neither), keyed like those plus N and the steer bits, every double and float compared on its own;
 * nothing is allocated once the maps of a geometry exist.  Groups: call it on mcrt_group_root() after mcrt_group_trace_frames_poses. */
int mcrt_compound_frames(mcrt_ctx *ctx, const float *rf_dev /* [n_frames][N][E][R] */, uint32_t n_frames, uint32_t n_elements, uint32_t n_rows,
                         double radius_mm, double total_angle_rad, const mcrt_compound *cp, float *out_dev /* [n_frames][out_rows][out_cols] */,
                         uint32_t out_rows, uint32_t out_cols);
/* mcrt_bmode_frames over compounded views: rf_dev is [n_frames][N][E][R].  Steps 1-3 run over the N views of a frame TOGETHER: the
 * automatic reference, and peak_dev[f], is the largest amplitude over all N views of frame f.  Step 4 is mcrt_compound_frames' expression
 * applied to the grey levels; steps 5-6 are unchanged (two calls of 2 frames equal one call of 4).  N = 1 with steer 0 gives
 * mcrt_bmode_frames' bytes bit for bit.  Errors and limits: mcrt_bmode_frames' and mcrt_compound_frames' (n_frames * N <= 65535), and
 * MCRT_ERR_LIMIT for N * n_elements >= 2^32; on any error nothing is launched and out_dev, state_dev and peak_dev are untouched. */
int mcrt_bmode_compound_frames(mcrt_ctx *ctx, const float *rf_dev /* [n_frames][N][E][R] */, uint32_t n_frames, uint32_t n_elements, uint32_t n_rows,
                               const mcrt_bmode_params *p, const mcrt_compound *cp, const float *tgc_db /* host [n_rows] or NULL */,
                               float *state_dev /* [out_rows][out_cols] or NULL */, float *peak_dev /* [n_frames] or NULL */,
                               uint8_t *out_dev /* [n_frames][out_rows][out_cols] */);

/* ---- compounding modes: per-view weights, a lateral edge ramp (apodisation) that hides where a steered view's coverage ends, and the
 * maximum or the median of the looks in place of their mean (the maximum keeps oblique interfaces bright, the median rejects a look that is
 * an outlier, such as a reverberation seen from one angle only). */
enum { MCRT_COMPOUND_MEAN = 0, MCRT_COMPOUND_MAX = 1, MCRT_COMPOUND_MEDIAN = 2 };
typedef struct { uint32_t mode;            /* MCRT_COMPOUND_*                                   (MEAN) */
                 float    feather_lines;   /* lateral edge ramp in scan-lines, 0 = off          (0)    */
                 float    view_weight[16]; /* the first n_views are read                        (1)    */
} mcrt_compound_opts;                      /* 72 bytes: mode at 0, feather_lines at 4, view_weight at 8 */
int mcrt_default_compound_opts(mcrt_compound_opts *o);                       /* host only */
/* mcrt_compound_frames with options (o == NULL: the defaults).  Per frame, output pixel and view n: the point p, the four taps, the blend s
 * and `covered` are mcrt_compound_frames' own, and mx is view n's column map at the pixel.  Then, in float, one rounding per operation, no fma:
 *   a = feather_lines > 0 ? fminf(fmaxf(fminf(mx, (float)(E - 1) - mx) / feather_lines, 0), 1) : 1
 *   w = view_weight[n] * a
 *   contributes = covered && w > 0
 *   MEAN    sum = sum + w * s;  wsum = wsum + w        (the contributing views, in n order from 0.0f)
 *           out = wsum > 0 ? sum / wsum : 0.0f
 *   MAX     m = the first contributing s, then s > m ? s : m   (in n order)
 *           out = m + 0.0f
 *   MEDIAN  the contributing s ordered by <; c of them
 *           out = (c odd ? v[(c-1)/2] : (v[c/2-1] + v[c/2]) * 0.5f) + 0.0f
 *   MAX, MEDIAN: any contributing s that is NaN -> out is NaN.  No contributing view: out = +0.0f.
 * In MAX and MEDIAN the weights only gate (a view with w > 0 counts fully).  With feathering on, the ramp removes the half-covered rim:
 * mx <= 0 or mx >= E-1 gives a = 0, so a view contributes only where both its neighbouring scan-lines exist, and n_elements == 1 with
 * feathering on is a black picture.  The ramp is lateral only: the picture's bottom edge, where a steered view ends a few pixels above the
 * unsteered one, is not feathered.
 * Defaults -- o == NULL, or MEAN with feather_lines 0 and every one of the first n_views weights equal to 1.0f -- give mcrt_compound_frames
 * bit for bit (w * s == s, wsum is the count) and run its kernel.  Errors: mcrt_compound_frames' own, and MCRT_ERR_INVALID, the message
 * naming the field, for an unknown mode, a feather_lines that is negative or not finite, a weight among the first n_views that is negative
 * or not finite, and all of those weights being zero.  On any error nothing is launched and out_dev is untouched.  Nothing new is uploaded:
 * the weights are made in the kernel from the maps of mcrt_compound_frames. */
int mcrt_compound_frames_opts(mcrt_ctx *ctx, const float *rf_dev /* [n_frames][N][E][R] */, uint32_t n_frames, uint32_t n_elements, uint32_t n_rows,
                              double radius_mm, double total_angle_rad, const mcrt_compound *cp, float *out_dev /* [n_frames][out_rows][out_cols] */,
                              uint32_t out_rows, uint32_t out_cols, const mcrt_compound_opts *o /* NULL = defaults */);
/* mcrt_bmode_compound_frames with options: the rule above applied to the grey levels in place of step 4; steps 1-3 and 5-6 are unchanged, the
 * persistence state carries across calls as before.  Defaults give mcrt_bmode_compound_frames' bytes.  Errors: that call's own and the four
 * above; on any error nothing is launched and out_dev, state_dev and peak_dev are untouched. */
int mcrt_bmode_compound_frames_opts(mcrt_ctx *ctx, const float *rf_dev /* [n_frames][N][E][R] */, uint32_t n_frames, uint32_t n_elements, uint32_t n_rows,
                                    const mcrt_bmode_params *p, const mcrt_compound *cp, const float *tgc_db /* host [n_rows] or NULL */,
                                    float *state_dev /* [out_rows][out_cols] or NULL */, float *peak_dev /* [n_frames] or NULL */,
                                    uint8_t *out_dev /* [n_frames][out_rows][out_cols] */, const mcrt_compound_opts *o /* NULL = defaults */);
/* what one view contributes with, per pixel: w [out_rows][out_cols] = contributes ? w : 0 of the rule above, the same float expression
 * the kernel evaluates, over mcrt_compound_maps' maps of the view (its arguments, then the view's weight and feather_lines).  Host only.
 * MCRT_ERR_INVALID for mcrt_compound_maps' conditions, a null w, a view_weight or feather_lines that is negative or not finite; on an error
 * nothing is written. */
int mcrt_compound_weights(uint32_t n_elements, uint32_t n_rows, double radius_mm, double total_angle_rad, uint32_t max_travel_us,
                          uint32_t speed_of_sound, uint32_t out_rows, uint32_t out_cols, float steer_rad, float view_weight, float feather_lines,
                          float *w /* [out_rows][out_cols] */);

/* ---- volume imaging: the curved array that wobbles in elevation (the "4D" abdominal or obstetric probe) and the pictures no 2-D probe can
 * show: the C-plane (a cut at constant depth), the sagittal cut, any oblique cut, or a whole block of voxels.  The reference has one plane.
 * A volume is K tilted copies of the probe traced as ONE pose pass (mcrt_trace_frames_poses / mcrt_group_trace_frames_poses) into a stack
 * [K][E][R]; convolution and envelope run over the K planes as over K frames; then every output point is gathered from the stack through
 * three maps (plane, row, column): a trilinear scan conversion.  Parallel planes need nothing of this: mcrt_elevation_planes followed by
 * mcrt_scan_convert_frames already is that volume.
 *
 * The probe-local frame: millimetres, origin at the arc's centre, x lateral (the direction of growing element number), y the arc's axis
 * (element angle 0), z elevation -- the frame BEFORE mcrt_transducer_elements' three rotations and `position`.
 * A sweep has K planes; plane k is the array tilted about the line parallel to x through (0, pivot_mm, 0) by
 *   theta_k = (k - (K-1)/2.0) * step_rad
 * The centring is real-valued: an even K has no plane at tilt 0 (K = 2: -step/2 and +step/2).
 * Forward geometry, the specification of everything below: the point at path length t on the beam of the element at arc angle phi in a
 * plane tilted by theta is, with a = radius + t,
 *   P = ( a sin(phi),   pivot + (a cos(phi) - pivot) cos(theta),   (a cos(phi) - pivot) sin(theta) )
 *
 * The frame-id rule (applied by the wrappers: Simulator(sweep=...), rf_image::trace(frame, transducer, sweep), mattausch_hip --sweep): plane k
 * of volume f of a pass that starts at frame id f0 is traced with frame id (f0 + f) * K + k. */
typedef struct { uint32_t n_planes;     /* K, 1..256 */
                 float    step_rad;     /* finite, > 0, and (K-1)/2 * step_rad < pi/2 */
                 float    pivot_mm;     /* finite; where on the arc's axis the wobble's axis crosses (0: the arc's centre, radius_mm: the apex) */
} mcrt_sweep;                           /* 12 bytes: n_planes 0, step_rad 4, pivot_mm 8 */
/* the output points, in the probe-local frame: point (i, j, l) = ((origin + i*du) + j*dv) + l*dw per component, evaluated in double in
 * exactly that order; i < nu, j < nv, l < nw.  The output layout is [nw][nv][nu], u fastest.  nw = 1 is a cut -- any plane in any
 * orientation; a volume and a cut are the same call.  Every entry must be finite; the axes need be neither orthogonal nor of equal length. */
typedef struct { double origin_mm[3], du_mm[3], dv_mm[3], dw_mm[3];
                 uint32_t nu, nv, nw, _pad;
} mcrt_volume_grid;                     /* 112 bytes: origin_mm 0, du_mm 24, dv_mm 48, dw_mm 72, nu 96, nv 100, nw 104 */
/* mcrt_transducer_elements with the array tilted by tilt_rad about the sweep's axis.  tilt_rad == 0 takes mcrt_transducer_elements' path:
 * its tables bit for bit.  Otherwise, with mcrt_transducer_elements' own `angle` and rf = (float)radius_cm:
 *   a = (float)angle,  s = sinf(a),  c = cosf(a),  ct = cosf(tilt_rad),  st = sinf(tilt_rad),  yp = (float)(pivot_mm / 10.0)       [cm]
 *   local direction (s, c*ct, c*st);   local position (rf*s, yp + (rf*c - yp)*ct, (rf*c - yp)*st)
 * one float rounding per operation, each through the same three rotations, pos = position + rot(local position).  Host only.
 * MCRT_ERR_INVALID for null pointers, n_elements == 0, a tilt that is not finite or has |tilt| >= pi/2, a pivot that is not finite; on an
 * error nothing is written. */
int mcrt_transducer_swept(uint32_t n_elements, double radius_cm, double separation_mm, const float position[3], const float angles_deg[3],
                          float tilt_rad, float pivot_mm, float *pos, float *dir);
/* the three maps of a grid, each [nw][nv][nu]: where in the stack [K][E][R] an output point (X, Y, Z) lies.  depth_mm_f is mcrt_scan_maps'
 * own float; everything else is double, rounded once to float at the end:
 *   h = sqrt((Y-pivot)^2 + Z^2),   theta = atan2(Z, Y-pivot),   y = pivot + h,   rho = sqrt(X^2 + y^2),   alpha = atan2(X, y)
 *   map_plane = (float)(theta / step + (K-1)/2.0)
 *   map_row   = (float)((rho - radius_mm) / depth_mm_f * R)
 *   map_col   = (float)((alpha + total_angle/2) / total_angle * (double)(float)E)
 * (the inverse of the forward geometry above; the column convention is mcrt_compound_maps', half-scan-line offset kept).  A point behind
 * the pivot or beside the sweep gets a map_plane outside [0, K-1], which the gather treats plane by plane.  Host only.  MCRT_ERR_INVALID
 * for mcrt_scan_maps' conditions (null maps, zero n_elements / n_rows, total_angle_rad not > 0), a null sweep or grid, a sweep outside the
 * conditions of mcrt_sweep, a zero nu, nv or nw, a grid entry that is not finite; MCRT_ERR_LIMIT for nu*nv*nw >= 2^31.  On an error
 * nothing is written. */
int mcrt_volume_maps(uint32_t n_elements, uint32_t n_rows, double radius_mm, double total_angle_rad, uint32_t max_travel_us, uint32_t speed_of_sound,
                     const mcrt_sweep *sweep, const mcrt_volume_grid *grid, float *map_plane, float *map_row, float *map_col);
/* The K planes of every frame gathered into the grid's points.  rf_dev: device float [n_frames][K][E][R]; out_dev: device float
 * [n_frames][nw][nv][nu].  Asynchronous on the context's stream, one launch.  Per frame and output point, with p, the four taps and the
 * blend mcrt_scan_convert's own (floor and fractions of map_col and map_row):
 *   mapped = none of the three maps is NaN
 *   fz = floorf(map_plane);  az = map_plane - fz;  z0 = (long long)fz
 *   v[d] = (mapped && 0 <= z0+d < K) ? (mcrt_scan_convert's bilinear expression at p on plane z0+d of the frame) : 0.0f        d = 0, 1
 *   out  = v[0] * (1.0f - az) + v[1] * az
 * one rounding per operation, no fma.  A plane outside the sweep is not read.  A NaN tap of a plane inside the sweep reaches its point even
 * under weight 0, as in mcrt_scan_convert.  The maps are mcrt_volume_maps' with the context's max_travel_time and speed of sound.
 * MCRT_ERR_INVALID for null pointers, zero sizes, a bad sweep, a bad grid or bad scan geometry, rf_dev overlapping out_dev; MCRT_ERR_LIMIT
 * for n_rows > 2048, n_frames * K > 65535, or 2^31 points and more.  On any error nothing is launched and out_dev is untouched.
 * The maps live on the device, [3][n_pad] per grid, keyed by the scan geometry, the sweep and the grid -- every double, float and integer
 * compared on its own.  The context keeps the four most recently used grids: a volume and three orthogonal cuts per frame upload nothing
 * after the first round, and nothing is allocated once a grid's maps exist.  Groups: call it on mcrt_group_root() after
 * mcrt_group_trace_frames_poses. */
int mcrt_volume_frames(mcrt_ctx *ctx, const float *rf_dev /* [n_frames][K][E][R] */, uint32_t n_frames, uint32_t n_elements, uint32_t n_rows,
                       double radius_mm, double total_angle_rad, const mcrt_sweep *sweep, const mcrt_volume_grid *grid,
                       float *out_dev /* [n_frames][nw][nv][nu] */);
/* mcrt_bmode_frames over a swept volume: rf_dev is [n_frames][K][E][R].  Steps 1-3 run over the K planes of a frame TOGETHER (the stack is
 * n_frames images of K * E scan-lines): the automatic reference, and peak_dev[f], is the largest amplitude over the whole sweep of frame f.
 * Step 4 is mcrt_volume_frames' expression applied to the grey levels; step 6 is unchanged.  p->persistence must be 0 (MCRT_ERR_INVALID
 * otherwise: a volume-sized state is out of scope), and p->reset_state is not read.  The picture is the grid's: p->out_rows and p->out_cols
 * are ignored (they may be 0); p->radius_mm and p->total_angle_rad describe the probe and are used.  Errors and limits: mcrt_bmode_frames'
 * and mcrt_volume_frames', and MCRT_ERR_LIMIT for K * n_elements >= 2^32; on any error nothing is launched and out_dev and peak_dev are
 * untouched. */
int mcrt_bmode_volume_frames(mcrt_ctx *ctx, const float *rf_dev /* [n_frames][K][E][R] */, uint32_t n_frames, uint32_t n_elements, uint32_t n_rows,
                             const mcrt_bmode_params *p, const mcrt_sweep *sweep, const mcrt_volume_grid *grid,
                             const float *tgc_db /* host [n_rows] or NULL */, float *peak_dev /* [n_frames] or NULL */,
                             uint8_t *out_dev /* [n_frames][nw][nv][nu] */);

/* ---- volume rendering: the block of voxels seen from a direction -- the maximum-intensity view of a vessel tree, the mean ("X-ray") view,
 * the surface picture of a fetal face.  The reference has one plane and draws none of this.  The input is a voxel block on the device,
 * [n_frames][nw][nv][nu] with u fastest: exactly what mcrt_volume_frames (float) or mcrt_bmode_volume_frames (uint8) wrote.  The renderer works
 * in the block's INDEX SPACE (u, v, w): a ray per pixel, orthographic, n_steps samples along it, each a trilinear blend of 8 voxels.  The
 * kernel needs no geometry beyond the twelve floats of the view; mcrt_render_view_for_grid makes them from a direction in millimetres.
 *
 * Derived floats, computed on the host:
 *   inv_range = (float)(1.0 / ((double)hi - (double)lo)),   inv_ramp = (float)(1.0 / (double)ramp),
 *   inv_steps = n_steps > 1 ? (float)(1.0 / (double)(n_steps - 1)) : 0.0f
 * The rule, per frame and pixel (i, j), i < nx, j < ny; everything in float, every operation rounded once, no fma:
 *   m = 0, arg = -1;  sum = 0, cnt = 0;  C = 0, T = 1, depth = -1
 *   for s = 0 .. n_steps-1:
 *       p_c = ((origin_c + (float)i * di_c) + (float)j * dj_c) + (float)s * ds_c              c = u, v, w   (not a running sum)
 *       f_c = floorf(p_c);  a_c = p_c - f_c
 *       covered = no p_c is NaN  &&  -1 <= f_c < n_c for every c        (compared in float; at least one tap can lie inside)
 *       if !covered: continue                                           (the step neither contributes nor counts, in every mode)
 *       t[dw][dv][du] = the voxel at (f_u+du, f_v+dv, f_w+dw) where that index is inside the block, else 0.0f and not read;
 *                       a uint8 voxel b is (float)b
 *       c[dw][dv] = t[dw][dv][0] * (1 - a_u) + t[dw][dv][1] * a_u
 *       e[dw]     = c[dw][0] * (1 - a_v) + c[dw][1] * a_v
 *       v         = e[0] * (1 - a_w) + e[1] * a_w;      v = (v == v) ? v : 0.0f        (a NaN sample is no echo, as step 1 of mcrt_bmode_frames)
 *       x = fminf(fmaxf((v - lo) * inv_range, 0), 1)
 *       MIP      if x > m: m = x, arg = s
 *       MEAN     sum = sum + x;  cnt++
 *       SURFACE  a = fminf(fmaxf((x - threshold) * inv_ramp, 0), 1) * opacity
 *                shade = 1.0f - depth_cue * ((float)s * inv_steps)
 *                C = C + (T * a) * (x * shade);   T = T * (1.0f - a)
 *                if depth < 0 && T <= 0.5f: depth = (float)s
 *                if T < t_cut: break
 *   out   = MIP: m      MEAN: cnt ? sum / (float)cnt : 0.0f      SURFACE: C
 *   depth = MIP: (float)arg      MEAN: -1.0f      SURFACE: depth          (the step index of what is seen; -1: nothing)
 *   out8  = (uint8_t)(fminf(fmaxf(out, 0), 1) * 255.0f + 0.5f)
 * Every pixel of every requested output is written.  SURFACE is front-to-back compositing: a sample's opacity rises from 0 at x = threshold
 * to `opacity` at x = threshold + ramp, its brightness falls with depth by depth_cue; the early stop (t_cut) is part of the contract because
 * it is visible in the bits.  `depth` is what a caller needs to shade the surface from the depth buffer's gradient, or to ask a label block
 * what tissue the surface belongs to.
 * The defaults of threshold, ramp, opacity and depth_cue are display choices that no measurement backs (as focal_range_mm's 20 mm). */
enum { MCRT_RENDER_MIP = 0, MCRT_RENDER_MEAN = 1, MCRT_RENDER_SURFACE = 2 };
typedef struct { float origin[3], di[3], dj[3], ds[3];   /* index units; component order u, v, w; all finite */
                 uint32_t nx, ny, n_steps, _pad;          /* the picture [ny][nx]; n_steps 1..4096 */
} mcrt_render_view;                                       /* 64 bytes: origin 0, di 12, dj 24, ds 36, nx 48, ny 52, n_steps 56 */
typedef struct { uint32_t mode;       /* MCRT_RENDER_*                                                       (SURFACE) */
                 float lo, hi;        /* window: finite, hi > lo               (float input 0, 1; uint8 input 0, 255) */
                 float threshold;     /* SURFACE: opacity starts at x = threshold, in [0,1)   (0.25) */
                 float ramp;          /* SURFACE: width of the opacity ramp in x, in (0,1]    (0.25) */
                 float opacity;       /* SURFACE: in (0,1]                                    (1)    */
                 float depth_cue;     /* SURFACE: in [0,1]                                    (0.5)  */
                 float t_cut;         /* SURFACE: in [0,1); 0 = never stop early              (0)    */
} mcrt_render_opts;                   /* 32 bytes: mode 0, lo 4, hi 8, threshold 12, ramp 16, opacity 20, depth_cue 24, t_cut 28 */
/* the defaults above (in_u8 != 0: the window of a uint8 block); host only.  MCRT_ERR_INVALID for a null o */
int mcrt_default_render_opts(mcrt_render_opts *o, int in_u8);
/* An orthographic camera in the probe-local mm frame of mcrt_volume_grid, looking along dir_mm at the block's centre; nx x ny pixels pixel_mm
 * apart, samples step_mm apart along the whole of the block's longest diagonal.  Everything in double, the twelve floats rounded once at the end:
 *   dn = dir/|dir|;   right = normalize(dn x up);   down = -(right x dn)          (picture rows run against `up`)
 *   C  = the grid point at index ((nu-1)/2, (nv-1)/2, (nw-1)/2)
 *   L  = half the longest of the block's four space diagonals |(nu-1) du +- (nv-1) dv +- (nw-1) dw|
 *   n_steps = floor(2L / step_mm) + 1
 *   P0 = C - L dn - (nx-1)/2 pixel_mm right - (ny-1)/2 pixel_mm down
 *   origin = M^-1 (P0 - g->origin_mm),   di = M^-1 (pixel_mm right),   dj = M^-1 (pixel_mm down),   ds = M^-1 (step_mm dn)
 *   M  = the matrix with the columns du, dv, dw
 * Picture columns run along the viewer's right, dn x up: looking along +dw with up = dv in a right-handed grid that is -du, di = (-1, 0, 0);
 * picture rows run against up.  The view is only a way to make the floats: a caller may fill mcrt_render_view by hand.  Host only.  MCRT_ERR_INVALID for null pointers, a
 * zero nx, ny, nu, nv or nw, a grid entry that is not finite, a dir that is zero or not finite, an up that is not finite or parallel to dir,
 * pixel_mm or step_mm not > 0 and finite, a grid whose three axes do not span space (a cut has dw = 0 and cannot be rendered);
 * MCRT_ERR_LIMIT for n_steps > 4096.  On an error *out is untouched. */
int mcrt_render_view_for_grid(const mcrt_volume_grid *g, const double dir_mm[3], const double up_mm[3], double pixel_mm, double step_mm,
                              uint32_t nx, uint32_t ny, mcrt_render_view *out);
/* The rule above over n_frames blocks: vol_dev is float (in_u8 == 0) or uint8 (in_u8 != 0) [n_frames][nw][nv][nu]; each output is a device
 * pointer [n_frames][ny][nx] or NULL.  Asynchronous on the context's stream, one launch; uploads nothing and allocates nothing.
 * MCRT_ERR_INVALID, the message naming the field: null ctx / vol_dev / view, all three outputs NULL, a zero n_frames, nu, nv, nw, nx or ny, a
 * view entry that is not finite, an unknown mode, a window that is not finite or has hi <= lo, threshold, ramp, opacity, depth_cue or t_cut
 * outside the ranges above, a window or a ramp so narrow that inv_range or inv_ramp is no finite float (a subnormal width), an output
 * overlapping the block.  MCRT_ERR_LIMIT: n_steps outside 1..4096, nu, nv or nw >= 2^24, nu*nv*nw or
 * nx*ny >= 2^31, n_frames > 65535.  On any error nothing is launched and nothing is written.  Groups: call it on mcrt_group_root(). */
int mcrt_render_frames(mcrt_ctx *ctx, const void *vol_dev, int in_u8, uint32_t n_frames, uint32_t nu, uint32_t nv, uint32_t nw,
                       const mcrt_render_view *view, const mcrt_render_opts *o /* NULL = defaults for in_u8 */,
                       float *out_dev /* [F][ny][nx] or NULL */, uint8_t *out8_dev /* same or NULL */, float *depth_dev /* same or NULL */);

/* ---- speckle reduction: the despeckle filter every scanner has ("SRI", "XRES").  The reference has none.  The algorithm is Yu & Acton's
 * speckle-reducing anisotropic diffusion (SRAD, IEEE Trans. Image Processing 11(11), 2002) in its usual conservative 4-neighbour
 * discretisation.  The input is a stack [n_frames][height][width] of floats on the device, width contiguous: the enveloped RF stack
 * (height = E scan-lines, width = R rows) or a scan-converted float stack alike -- the filter works in index space and knows no geometry.
 *
 * Host tables, computed in double and rounded once (mcrt_speckle_tables):
 *   q_t = q0 * exp(-rho * t),   q0sq[t] = (float)(q_t*q_t),   kq[t] = (float)(1 / (q_t*q_t * (1 + q_t*q_t))),   t = 0 .. n_iter-1
 *   lam4 = (float)(0.25 * lambda)
 * Options of which a table entry is not finite or is 0 (a q_t that has decayed to nothing) are refused: MCRT_ERR_INVALID.
 * The rule, per frame; everything in float, every multiply, add and divide rounded once, no fma:
 *   0. X = |v| where v is finite, else 0        (step 1 of mcrt_bmode_frames: a NaN scan-line is no echo -- and does not spread 2 pixels per iteration)
 *   1. for t = 0 .. n_iter-1, over the whole frame, iteration t reading only iteration t-1's X; neighbour indices are clamped,
 *      iN = max(i-1, 0), iS = min(i+1, H-1), jW = max(j-1, 0), jE = min(j+1, W-1):
 *        dN = X[iN][j] - X[i][j],  dS = X[iS][j] - X[i][j],  dW = X[i][jW] - X[i][j],  dE = X[i][jE] - X[i][j]
 *        S1 = ((dN + dS) + dW) + dE
 *        S2 = ((dN*dN + dS*dS) + dW*dW) + dE*dE
 *        m  = X[i][j] + 0.25f*S1                                  (the neighbours' mean: the rule never divides by the pixel itself)
 *        q2 = (0.5f*S2 - 0.0625f*(S1*S1)) / (m*m)
 *        c[i][j] = fminf(fmaxf(1.0f / (1.0f + (q2 - q0sq[t]) * kq[t]), 0.0f), 1.0f)
 *            0/0 (a flat zero patch): NaN, which fmaxf turns into c = 0 -- moot, every d there is 0;  x/0, x > 0 (an isolated spike): q2 = inf,
 *            c = 0;  S2 overflowing: c = 0
 *        D = ((c[i][j]*dN + c[iS][j]*dS) + c[i][j]*dW) + c[i][jE]*dE
 *        X'[i][j] = X[i][j] + lam4 * D
 * What follows: the flux across every interior edge is antisymmetric, so a frame's sum is kept up to rounding; with lambda <= 1 and c in
 * [0,1] every X' is a convex combination of X and its neighbours; a constant frame keeps its bits; scaling the input by a power of two
 * scales the output exactly (while nothing overflows or goes subnormal).  n_iter = 0: out = in bit for bit (step 0 is not applied).
 * q0 is the coefficient of variation of fully developed speckle of a Rayleigh amplitude and rho the paper's decay; n_iter and lambda are
 * display choices that no measurement backs (a CPU prototype on synthetic speckle, where the effect saturates near 20 iterations). */
typedef struct { uint32_t n_iter;   /* 0..256; 0: out = in bit for bit                                            (20)        */
                 float q0;          /* speckle scale at t = 0, > 0, finite                 (0.5227232 = sqrt(4/pi - 1))       */
                 float rho;         /* decay of the scale per iteration, >= 0, finite                             (1/6)       */
                 float lambda;      /* time step, in (0, 1]                                                       (0.5)       */
} mcrt_speckle_opts;                /* 16 bytes: n_iter 0, q0 4, rho 8, lambda 12 */
/* the defaults above; host only.  MCRT_ERR_INVALID for a null o */
int mcrt_default_speckle_opts(mcrt_speckle_opts *o);
/* the tables above; host only.  q0sq and kq may be null when n_iter == 0.  MCRT_ERR_INVALID: null o, q0sq, kq or lam4, q0 not > 0 and finite, rho
 * not >= 0 and finite, lambda outside (0, 1], a table entry that is not finite or is 0;  MCRT_ERR_LIMIT: n_iter > 256.  On an error nothing is written */
int mcrt_speckle_tables(const mcrt_speckle_opts *o, float *q0sq /* [n_iter] */, float *kq /* [n_iter] */, float *lam4 /* [1] */);
/* The rule above over n_frames frames: in_dev -> out_dev, both [n_frames][height][width] on the device.  out_dev == in_dev (in place) is
 * allowed; any other overlap is MCRT_ERR_INVALID.  o: NULL = the defaults.  Asynchronous on the context's stream: ceil(n_iter / T) launches
 * of T fused iterations, the last one running the remainder, ping-ponging between out_dev and the context's scratch (the one mcrt_convolve
 * uses, grown to the largest stack: nothing is allocated once it exists) so that the last launch lands in out_dev; in place with an odd
 * number of launches the stack is first copied into the scratch.  The per-iteration floats are kernel arguments.  n_iter == 0: a device copy when the buffers differ,
 * nothing otherwise.  MCRT_ERR_INVALID: null ctx, in_dev or out_dev, a zero n_frames, height or width, options that mcrt_speckle_tables
 * refuses, buffers that overlap without being the same;  MCRT_ERR_LIMIT: n_iter > 256, a stack of 2^31 floats or more.  On an error nothing is
 * launched and out_dev is untouched.  Groups: call it on mcrt_group_root(). */
int mcrt_speckle_frames(mcrt_ctx *ctx, const float *in_dev, uint32_t n_frames, uint32_t height, uint32_t width,
                        const mcrt_speckle_opts *o /* NULL = defaults */, float *out_dev);

/* ---- 3-D speckle reduction: the rule above with six neighbours, over voxel blocks.  A surface rendering's rays cross the slices of a
 * block, and a 2-D filter -- over the RF stack before the gather, or over the block as nw frames -- leaves the speckle between slices as it
 * is; scanners smooth the block before they render it.  The input is a stack [n_frames][nw][nv][nu] of floats on the device, u contiguous:
 * what mcrt_volume_frames and mcrt_recon_frames write and mcrt_render_frames (in_u8 = 0) reads.  The filter works in index space; the
 * geometry enters only through one weight per axis, w_a = (h_min / h_a)^2 for voxel pitches h_a (mcrt_speckle3d_weights): the weight of
 * a finite-difference second derivative along an axis of another pitch, scaled so that the finest axis has weight 1.
 *
 * Host tables, computed in double and rounded once (mcrt_speckle3d_tables): q0sq[t] and kq[t] are mcrt_speckle_tables' (the same floats for
 * the same q0, rho and n_iter), and with sw = (double)wu + wv + ww
 *   a = (float)(1 / sw),   b = (float)(1 / (4 sw^2)),   hs = (float)(1 / (2 sw)),   lamw = (float)(lambda / (2 sw))
 * The rule, per block; everything in float, every multiply, add and divide rounded once, no fma:
 *   0. X = |v| where v is finite, else 0
 *   1. for t = 0 .. n_iter-1, over the whole block, iteration t reading only iteration t-1's X; neighbour indices are clamped against
 *      the block (a clamped neighbour is the voxel itself), with X = X[l][j][i]:
 *        dN = X[l][j-1][i] - X,  dS = X[l][j+1][i] - X,  dW = X[l][j][i-1] - X,  dE = X[l][j][i+1] - X,  dD = X[l-1][j][i] - X,  dU = X[l+1][j][i] - X
 *        gN = wv*dN,  gS = wv*dS,  gW = wu*dW,  gE = wu*dE,  gD = ww*dD,  gU = ww*dU
 *        S1 = ((((gN + gS) + gW) + gE) + gD) + gU
 *        S2 = ((((gN*dN + gS*dS) + gW*dW) + gE*dE) + gD*dD) + gU*dU
 *        m  = X + hs*S1                                           (the neighbours' weighted mean)
 *        q2 = (a*S2 - b*(S1*S1)) / (m*m)
 *        c  = fminf(fmaxf(1.0f / (1.0f + (q2 - q0sq[t]) * kq[t]), 0.0f), 1.0f)
 *        D  = ((((c*gN + c[S]*gS) + c*gW) + c[E]*gE) + c*gD) + c[U]*gU      (c[S], c[E], c[U]: c at the clamped higher neighbour along v, u, w)
 *        X' = X + lamw * D
 * What follows: the flux across every interior face is antisymmetric (face (l, j, i) | (l, j+1, i) carries wv * c[l][j+1][i] * d one way and
 * the same product of the negated d the other), so a block's sum is kept up to rounding; lamw * (sum of c*w over the six faces) <= lambda
 * <= 1, so every X' is a convex combination of X and its neighbours; a constant block keeps its bits; scaling the input by a power of two
 * scales the output exactly (while nothing overflows or goes subnormal); n_iter = 0: out = in bit for bit (step 0 is not applied).
 * With weight = (1, 1, 0) the constants are exactly 0.5, 0.0625, 0.25 and 0.25 * lambda, every gD and gU is 0, and the block equals
 * mcrt_speckle_frames over it as nw frames of [nv][nu] bit for bit -- NaN, +-inf, -0.0 and zero patches in the input included, while no
 * difference of two voxels overflows.  The summation order above is what that property rests on.
 * The axes are treated as orthogonal: the weights know the axes' lengths only.  No measurement backs the filter on a skewed grid, whose
 * Laplacian has cross terms that this rule leaves out. */
typedef struct { uint32_t n_iter;   /* 0..256; 0: out = in bit for bit                                            (20)        */
                 float q0, rho, lambda;   /* as mcrt_speckle_opts, same ranges and defaults */
                 float weight[3];   /* per axis u, v, w: each finite and >= 0, their sum > 0                      (1, 1, 1)   */
} mcrt_speckle3d_opts;              /* 28 bytes: n_iter 0, q0 4, rho 8, lambda 12, weight 16 */
/* the defaults above; host only.  MCRT_ERR_INVALID for a null o */
int mcrt_default_speckle3d_opts(mcrt_speckle3d_opts *o);
/* the weights of a grid; host only.  h_a is the length of du_mm, dv_mm, dw_mm.  An axis with a count of 1 gets weight 0 and takes no part in
 * the minimum; every other axis gets (float)((h_min / h_a)^2), h_min the smallest of the remaining lengths (nw = 1, a cut: (.., .., 0), the
 * 2-D filter).  MCRT_ERR_INVALID: null g or weight, a zero count, an entry of the grid that is not finite, a zero-length axis with a count
 * above 1, all three counts 1.  On an error nothing is written */
int mcrt_speckle3d_weights(const mcrt_volume_grid *g, float weight[3]);
/* the tables above; host only.  q0sq and kq may be null when n_iter == 0.  MCRT_ERR_INVALID: null o, q0sq, kq or k, what mcrt_speckle_tables
 * refuses of q0, rho and lambda, a weight that is negative or not finite, a sum of weights that is not > 0, one of the four constants
 * not finite or 0;  MCRT_ERR_LIMIT: n_iter > 256.  On an error nothing is written */
int mcrt_speckle3d_tables(const mcrt_speckle3d_opts *o, float *q0sq /* [n_iter] */, float *kq /* [n_iter] */, float k[4] /* a, b, hs, lamw */);
/* The rule above over n_frames blocks: in_dev -> out_dev, both [n_frames][nw][nv][nu] on the device.  out_dev == in_dev (in place) is
 * allowed; any other overlap is MCRT_ERR_INVALID.  o: NULL = the defaults.  Asynchronous on the context's stream: n_iter launches of one
 * iteration, ping-ponging between out_dev and the context's scratch (the one mcrt_convolve and mcrt_speckle_frames use, grown to the
 * largest stack: nothing is allocated once it exists) so that the last launch lands in out_dev; in place with an odd number of launches
 * the stack is first copied into the scratch.  The weights, the constants and the iteration's floats are kernel arguments.  n_iter == 0:
 * a device copy when the buffers differ, nothing otherwise.  MCRT_ERR_INVALID: null ctx, in_dev or out_dev, a zero n_frames, nu, nv or nw,
 * options that mcrt_speckle3d_tables refuses, buffers that overlap without being the same;  MCRT_ERR_LIMIT: n_iter > 256, nu, nv or nw >=
 * 2^24, a stack of 2^31 floats or more.  On an error nothing is launched and out_dev is untouched.  Groups: call it on mcrt_group_root(). */
int mcrt_speckle_volume_frames(mcrt_ctx *ctx, const float *in_dev, uint32_t n_frames, uint32_t nu, uint32_t nv, uint32_t nw,
                               const mcrt_speckle3d_opts *o /* NULL = defaults */, float *out_dev);

/* ---- receiver noise: the noise floor of the receive chain and the gain of every transducer element.  The reference has neither: its RF
 * images hold echoes and exact zeros, so no gain finds a penetration depth (mcrt_autogain_frames, below, finds the floor's) and no element is weak or dead.  The stage works on the RF stack
 * [n_frames][n_images][E][R] that a traced pass left on the device (n_images: the N views of a compounded frame, the K planes of a sweep, or 1),
 * in place.  It sits after the lateral PSF and before the envelope: receive noise is uncorrelated between scan-lines.  That is a modelling
 * choice that no measurement backs.
 *
 * The draw; integers only.  Image j = f * n_images + i of the stack has the id first_image_id + j.  For scan-line e and row r of it:
 *   o[0..3] = philox4x32_10(ctr = (e, r, 0x4E4F4953, 0), key = (seed, id))
 *   S = the sum of the eight 16-bit halves of o[0..3],   d = S - 262140
 * an Irwin-Hall sum of 8: the mean is exactly 0, the variance exactly 2863311530 = 8 * (65536^2 - 1) / 12, and |d| <= 262140, which is 4.9
 * standard deviations (excess kurtosis -0.15).  The counter's third word is no bounce number (max_depth <= 16), so a noise stream cannot
 * coincide with a tracer stream even under equal key words.  mcrt_noise_draws returns exactly these d, on the host.
 * The rule, per frame f; everything in float, every operation rounded once, no fma:
 *   a(v)    = |v| where v is finite, else 0                          (step 1 of mcrt_bmode_frames without TGC)
 *   peak_f  = the largest a over the frame's n_images * E * R INPUT values (exact, independent of the order, taken before the gain)
 *   sigma_f = sigma (MCRT_NOISE_ABS), or peak_f * c with c = (float)pow(10.0, -(double)snr_db / 20.0) made on the host (MCRT_NOISE_SNR_DB)
 *   k_f     = sigma_f * inv_std,   inv_std = (float)(1.0 / sqrt(2863311530.0))
 *   u       = element_gain ? v * element_gain[e] : v
 *   out     = (k_f == 0.0f) ? u : u + (float)d * k_f
 * What follows: a NaN or an infinity stays what it is; a frame of zeros in SNR_DB mode only gets its gain; ABS with sigma == 0 and no gain
 * launches nothing (sigma_dev, when given, is cleared) and the stack keeps its bits, a -0.0 included; the views or planes of one frame share one receiver, hence one peak (the
 * joint reference of mcrt_bmode_compound_frames).  sigma_dev[f], when given, receives sigma_f.
 * The ids (applied by the wrappers: Simulator(noise=...), rf_image::add_noise, mattausch_hip --noise-db / --noise-sigma): first_image_id is
 * the frame id the stack's first image was traced with, by the frame-id rules above ((f0 + f) * N + n, (f0 + f) * K + k) -- a frame carries
 * the same noise traced alone or inside a pass. */
enum { MCRT_NOISE_SNR_DB = 0,   /* sigma_f = the frame's own peak * 10^(-snr_db/20) */
       MCRT_NOISE_ABS    = 1 }; /* sigma_f = sigma */
typedef struct { uint32_t mode;     /* MCRT_NOISE_*                                   (SNR_DB)     */
                 float    snr_db;   /* SNR_DB: finite                                 (50)         */
                 float    sigma;    /* ABS: finite, >= 0                              (0)          */
                 uint32_t seed;     /* Philox key word 0 of the noise streams         (0x4E4F4953) */
} mcrt_noise_opts;                  /* 16 bytes: mode 0, snr_db 4, sigma 8, seed 12 */
/* the defaults above; host only.  MCRT_ERR_INVALID for a null o */
int mcrt_default_noise_opts(mcrt_noise_opts *o);                                              /* host only */
/* the draws d of one image; host only.  MCRT_ERR_INVALID: a null d, a zero n_elements or n_rows;  MCRT_ERR_LIMIT: n_rows > 2048.  On an error
 * nothing is written */
int mcrt_noise_draws(uint32_t seed, uint32_t image_id, uint32_t n_elements, uint32_t n_rows,
                     int32_t *d /* [E][R] */);                                                /* host only */
/* The rule above over the stack, in place.  Asynchronous on the context's stream: in SNR_DB mode a clear of the context's peaks and one
 * launch of k_bmode_peak (each frame's n_images * E scan-lines as one image), then one launch of k_noise.  element_gain is a HOST table [E],
 * free the moment the call returns; it lives on the device in a buffer of the context's and is copied only when it differs from what is
 * there (as tgc_db is).  Nothing is allocated after the first call at a size.
 * MCRT_ERR_INVALID: null ctx or rf_dev, a zero n_frames, n_images, n_elements or n_rows, an unknown mode, snr_db not finite (SNR_DB),
 * sigma negative or not finite (ABS), an element_gain entry that is not finite;  MCRT_ERR_LIMIT: n_rows > 2048, n_frames * n_images >
 * 65535, first_image_id + n_frames * n_images > 2^32, a stack of 2^31 samples or more.  On an error nothing is launched and rf_dev and
 * sigma_dev are untouched.  Groups: call it on mcrt_group_root(). */
int mcrt_noise_frames(mcrt_ctx *ctx, float *rf_dev /* [n_frames][n_images][E][R], in place */, uint32_t n_frames,
                      uint32_t n_images, uint32_t n_elements, uint32_t n_rows, uint32_t first_image_id,
                      const mcrt_noise_opts *o /* NULL = defaults */, const float *element_gain /* host [E] or NULL */,
                      float *sigma_dev /* [n_frames] or NULL */);

/* ---- automatic gain: the "auto-optimise" key of a scanner.  A depth gain curve is estimated from each frame itself: it flattens the tissue
 * brightness over depth and stops amplifying where only noise is left, which is the frame's penetration depth.  The reference has no gain at
 * all, and mcrt_bmode_params::tgc_db is a curve that only a caller can write.  The stage works on a float stack [n_frames][n_images][E][R] on the
 * device, normally enveloped (it goes after mcrt_envelope_frames and mcrt_speckle_frames and before whatever gathers a picture); n_images is
 * the N views of a compounded frame, the K planes of a sweep, or 1: they share one receiver, hence one curve, as in mcrt_noise_frames.
 * Integers decide, and the few float operations are rounded once each (no fma, no transcendental, the divisions correctly rounded), so a
 * numpy reading of this text equals the device bit for bit.
 *
 * The rule, per frame f:
 *   1. amplitude   a(v) = |v| where v is finite, else 0.  bin(a) = bits(a) >> 20: 0 .. 2047, eight bins per octave.  Bin 0 (zeros and the
 *                  smallest denormals) counts as "no echo".
 *   2. bands       band b holds the rows [b * band_rows, min((b + 1) * band_rows, R)), n_bands = ceil(R / band_rows).  hist[f][b][bin] is the
 *                  number of samples of the band, over all n_images * E scan-lines, whose amplitude falls into the bin: integer counts,
 *                  independent of the order of addition.
 *   3. floor       thr = floor_f * floor_scale, one float multiply; floor_f = floor_dev[f] when floor_dev is given (a device pointer: the
 *                  sigma_dev of mcrt_noise_frames), else opts.floor.  thr_bin = bin(thr) when thr is finite and > 0, else 0.  A sample is
 *                  TISSUE when its bin is greater than thr_bin.  floor_scale = 3 by default: a modelling choice that no measurement backs.
 *   4. band level  n_t[b] = the tissue samples of the band, n_s[b] = all its samples = n_images * E * (rows of the band).  The band is VALID
 *                  when n_t * 1000 >= min_permille * n_s (in 64 bits) and n_t > 0.  m[b] = the lower median bin of the tissue samples: the
 *                  smallest bin whose cumulative tissue count c satisfies 2 * c >= n_t.
 *   5. target      m* = the lower median of the valid bands' m[b]: element (V - 1) / 2 of the V values sorted.  With no valid band every gain
 *                  is 1 and the penetration is 0.
 *   6. band gain   centre(bin) = the float whose bits are (bin << 20) | (1 << 19).  A valid band has
 *                  k_b = fminf(fmaxf(centre(m*) / centre(m[b]), 1.0f / max_gain), max_gain); an invalid band has the gain of the nearest valid
 *                  band shallower than it -- noise past the penetration depth and anechoic spans are not amplified further --, and with none
 *                  shallower the first valid band's gain.
 *   7. row gain    linear between the band centres.  With n = 2 * r - (band_rows - 1) (signed): n <= 0: k[r] = k_0; else b = n / (2 * band_rows);
 *                  b >= n_bands - 1: k[r] = k_last; else t = (float)(n - 2 * band_rows * b) / (float)(2 * band_rows) and
 *                  k[r] = k_b + (k_{b+1} - k_b) * t: a subtraction, a multiplication, an addition.
 *   8. penetration pen[f] = min(R, (last valid band + 1) * band_rows) rows, or 0 with no valid band.
 *   9. apply       (opts.apply != 0) out = v * k[f][r], one multiply; a NaN or an infinity stays what it is.  With apply == 0 the stack keeps
 *                  its bits and only gain_dev, band_bin_dev and pen_dev are written. */
typedef struct { uint32_t band_rows;     /* rows of a band: 4 .. 256                                     (16)   */
                 uint32_t min_permille;  /* tissue samples a valid band needs, per mille: 0 .. 1000      (250)  */
                 float    floor;         /* floor_f where no floor_dev is given: finite, >= 0            (0)    */
                 float    floor_scale;   /* thr = floor_f * floor_scale: finite, >= 0                    (3)    */
                 float    max_gain;      /* a band's gain stays in [1 / max_gain, max_gain]: finite, >= 1 (1000: 60 dB) */
                 uint32_t apply;         /* 0: estimate only, the stack keeps its bits                   (1)    */
} mcrt_autogain_opts;                    /* 24 bytes: band_rows 0, min_permille 4, floor 8, floor_scale 12, max_gain 16, apply 20 */
/* the defaults above; host only.  MCRT_ERR_INVALID for a null o */
int mcrt_default_autogain_opts(mcrt_autogain_opts *o);                                        /* host only */
/* Steps 3 to 8 for one frame, on the host; no GPU is needed, and k_autogain_curve equals it bit for bit.  hist holds the counts of step 2,
 * n_lines is n_images * E (n_s[b] = n_lines * the rows of band b, whatever hist adds up to), band_bin[b] receives m[b], or -1 for an
 * invalid band.  k, band_bin and pen may each be null.  MCRT_ERR_INVALID: a null hist, a zero n_lines or n_rows, floor_f negative or not
 * finite, an option outside its range (the message names the field);  MCRT_ERR_LIMIT: n_rows > 2048.  On an error nothing is written */
int mcrt_autogain_curve(const uint32_t *hist /* [n_bands][2048] */, uint32_t n_lines, uint32_t n_rows, float floor_f,
                        const mcrt_autogain_opts *o /* NULL = defaults */, float *k /* [n_rows] */, int32_t *band_bin /* [n_bands] */,
                        uint32_t *pen);                                                       /* host only */
/* The rule above over the stack, in place.  Asynchronous on the context's stream; per chunk of frames a clear of the context's histograms,
 * k_autogain_hist (one read of the chunk), k_autogain_curve (one workgroup per frame) and, with apply, k_autogain_apply.  The histograms
 * [frames][n_bands][2048] belong to the context and stay bounded (32 MiB): a pass that needs more is walked in chunks of frames, with the
 * same result.  The gains of a call without gain_dev live in the context too.  Nothing is allocated after the first call at a size.
 * floor_dev is read on the device when the kernels run (a NaN, an infinity or a value <= 0 there gives thr_bin = 0).
 * MCRT_ERR_INVALID: null ctx or rf_dev, a zero n_frames, n_images, n_elements or n_rows, band_rows outside 4 .. 256, min_permille > 1000,
 * floor or floor_scale negative or not finite, max_gain not finite or < 1 (the message names the field);  MCRT_ERR_LIMIT: n_rows > 2048,
 * n_frames * n_images > 65535, a stack of 2^31 samples or more.  On an error nothing is launched and nothing is written.  Groups: call it on
 * mcrt_group_root(). */
int mcrt_autogain_frames(mcrt_ctx *ctx, float *rf_dev /* [n_frames][n_images][E][R], in place */, uint32_t n_frames, uint32_t n_images,
                         uint32_t n_elements, uint32_t n_rows, const mcrt_autogain_opts *o /* NULL = defaults */,
                         const float *floor_dev /* [n_frames] or NULL */, float *gain_dev /* [n_frames][R] or NULL */,
                         int32_t *band_bin_dev /* [n_frames][n_bands] or NULL */, uint32_t *pen_dev /* [n_frames] or NULL */);

/* ---- freehand 3-D reconstruction: a tracked 2-D probe moved by hand over the patient, its frames binned into voxels from their poses --
 * pixel-nearest-neighbour binning with hole filling (Rohling, Gee, Berman: "A comparison of freehand three-dimensional ultrasound
 * reconstruction techniques", Medical Image Analysis 3(4), 1999; the default of PLUS / 3D Slicer).  The reference has one plane.  The input
 * is the stack [F][E][R] that mcrt_trace_frames_poses left on the device (convolved, enveloped, despeckled or not) and the very pose
 * tables [F][E][3] it was traced with; the output is a voxel block [nw][nv][nu], u fastest, as mcrt_render_frames and (slice by slice)
 * mcrt_speckle_frames take it.  The grid is an mcrt_volume_grid read in the WORLD frame, in millimetres: voxel (i, j, l) has its centre
 * at origin + i*du + j*dv + l*dw.  unit_mm is the length of a scene unit in millimetres (10: the tables are in cm).  Row r of a scan-line
 * lies at path length r * row_mm from the element's position; the wrappers pass depth_mm_f / R, the convention of mcrt_volume_maps'
 * map_row, so that a reconstruction of a swept pass lies where mcrt_volume_frames puts it.
 *
 * Host floats (mcrt_recon_transform), computed in double and rounded once.  M has the columns du, dv, dw; its inverse by cofactors:
 *   r_u = dv x dw,  r_v = dw x du,  r_w = du x dv,  det = du . r_u,  Minv[c][k] = r_c[k] / det
 *   A[c][k] = (float)(Minv[c][k] * unit_mm),   b[c] = (float)(-((Minv[c][0]*o_x + Minv[c][1]*o_y) + Minv[c][2]*o_z)),   o = origin_mm
 *   row_u = (float)(row_mm / unit_mm),   qscale = 2^31 / (double)value_max   (a double)
 * The rule per sample (f, e, r) with value v; everything in float, one rounding per operation, no fma:
 *   t   = (float)r * row_u
 *   P_k = pos[f][e][k] + dir[f][e][k] * t                                k = x, y, z
 *   x_c = ((b[c] + P_x*A[c][0]) + P_y*A[c][1]) + P_z*A[c][2]             c = u, v, w
 *   i_c = floorf(x_c + 0.5f)
 *   inside = 0 <= i_c < n_c for every c            (compared in float; a NaN is not inside)
 *   usable = v is finite && fabsf(v) < value_max
 *   if !inside: stats[0]++          else if !usable: stats[1]++
 *   else: q = (long long)((double)v * qscale)      (truncation)
 *         count[voxel]++;   MEAN: sum[voxel] += q;   MAX: qmax[voxel] = max(qmax[voxel], q)
 * F*E*R < 2^31 and |q| < 2^31, so neither sum (int64) nor count (uint32) can overflow; integer sums commute, so the result does not
 * depend on the order in which the device adds.
 * Resolve: a voxel with count > 0 is (float)((double)sum / ((double)count * qscale)) in MEAN mode, (float)((double)qmax / qscale) in MAX mode.
 * Hole filling, for a voxel with count == 0 when fill_radius H > 0:
 *   for h = 1..H:
 *       s = 0.0f, n = 0
 *       over dw, dv, du in [-h, h]   (w outermost, u innermost, ascending):
 *           if the neighbour is inside the block and its count > 0:  s = s + its resolved value;  n++
 *       if n >= fill_min: value = s / (float)n;  stop
 *   if no h succeeded (or H == 0): value = empty
 * Only sampled voxels are read, never filled ones: the result does not depend on any order.  count_dev gets the sample counts; a filled
 * hole keeps 0.  stats_dev[0] counts the samples outside the block, stats_dev[1] the unusable ones inside it.  Every voxel of every
 * requested output is written.
 * value_max bounds what is binned and fixes the fixed-point step (value_max * 2^-31); fill_radius and fill_min are display choices. */
enum { MCRT_RECON_MEAN = 0, MCRT_RECON_MAX = 1 };
typedef struct { uint32_t mode;        /* MCRT_RECON_*                                          (MEAN) */
                 float    value_max;   /* finite, > 0: a sample with |v| >= value_max is skipped (1024) */
                 uint32_t fill_radius; /* H, 0..3: 0 = no hole filling                           (1)    */
                 uint32_t fill_min;    /* >= 1: sampled neighbours a hole needs                  (1)    */
                 float    empty;       /* finite: the value of a voxel nothing reached           (0)    */
} mcrt_recon_opts;                     /* 20 bytes: mode 0, value_max 4, fill_radius 8, fill_min 12, empty 16 */
/* the defaults above; host only.  MCRT_ERR_INVALID for a null o */
int mcrt_default_recon_opts(mcrt_recon_opts *o);
/* A [3][3] (row c = u, v, w) and b [3] above; host only.  MCRT_ERR_INVALID: a null pointer, a grid entry that is not finite, a zero nu, nv
 * or nw, a unit_mm that is not finite or not > 0, axes that do not span space (|det| <= 1e-12 |du| |dv| |dw|), an A or b entry that is no
 * finite float.  On an error nothing is written */
int mcrt_recon_transform(const mcrt_volume_grid *grid_world_mm, double unit_mm, float A[9], float b[3]);
/* The rule above.  stack_dev: device float [F][E][R]; pos, dir: [F][E][3], host or device, with the lifetime rule of
 * mcrt_trace_frames_poses; out_dev: device float [nw][nv][nu]; count_dev: device uint32, same shape, or NULL; stats_dev: device uint32 [2]
 * or NULL.  Asynchronous on the context's stream: a clear of the accumulators, k_recon_splat, k_recon_resolve.  The accumulators (12 bytes
 * per voxel) are a scratch buffer of the context that grows to the largest grid: nothing is allocated on a repeat.  Everything is checked
 * before anything is launched.  MCRT_ERR_INVALID, the message naming the field: a null ctx, stack_dev, pos, dir, grid or out_dev; a zero
 * n_frames, n_elements or n_rows; row_mm or unit_mm not finite or not > 0; an unknown mode, a value_max that is not finite and > 0, a
 * fill_radius above 3, a fill_min of 0, an empty that is not finite; a grid that mcrt_recon_transform refuses; an output that overlaps the
 * stack or another output.  MCRT_ERR_LIMIT: n_rows > 2048, n_frames > 65535, F*E*R >= 2^31, nu*nv*nw >= 2^31, and a block so
 * thin that ceil(nu/32) * ceil(nv/8) * ceil(nw/8) >= 2^24 (1 x 1 x N from N = 2^27).  On any error nothing is
 * written.  Groups: call it on mcrt_group_root(). */
int mcrt_recon_frames(mcrt_ctx *ctx, const float *stack_dev /* [F][E][R] */, uint32_t n_frames, uint32_t n_elements, uint32_t n_rows,
                      const float *pos /* [F][E][3] host or device */, const float *dir /* same */, double row_mm, double unit_mm,
                      const mcrt_volume_grid *grid /* WORLD frame, mm */, const mcrt_recon_opts *o /* NULL = defaults */,
                      float *out_dev /* [nw][nv][nu] */, uint32_t *count_dev /* same or NULL */, uint32_t *stats_dev /* [2] or NULL */);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Ground-truth label maps: what is in the picture.  The tracer knows the anatomy exactly; these calls hand it out aligned with every
 * image the library makes -- sample by sample along each scan-line (mcrt_label_frames), pixel by pixel in the sector
 * (mcrt_label_scan_convert_frames), voxel by voxel in a swept volume (mcrt_label_volume_frames).  The reference draws pictures only:
 * ray.cpp:13-47 decides the medium behind a boundary, rfimage.h:33-40 the row of an echo, rfimage.h:183-215 the sector's maps,
 * scene.cpp:115 the start offset of a ray; it keeps no map of what it drew.
 *
 * mcrt_label_frames walks the CENTRAL BEAM of every scan-line -- the straight line along the element's direction, which is bounce 0 of
 * every sample path -- deterministically: it does not depend on n_samples, the seed, the frame id or the texture.  Per scan-line, every
 * float operation rounded on its own (no fma), spacing the scene's, R = n_rows:
 *   state   from = el_pos, dir = el_dir, dist = 0.0 (double), b_prev = 0, k = 0;
 *           TRACED: media = start_mat, outside = none;   GEOMETRIC: an empty stack of mesh ids (capacity 16), media = start_mat
 *   loop    1. Ls = (float)(2.0 * depth_cm);  to = from + Ls * (spacing * dir);  f2 = from + offs * dir      [per component: the tracer's
 *              own segment arithmetic; offs = start_offset, or the context's ray_start_offset]
 *           2. when k == MCRT_LABEL_MAX_CROSSINGS stop (no further query is made; bit 31 of crossings is set).  Take the closest hit of
 *              the segment (f2, to) under the closest-hit contract; on a miss stop
 *           3. p = (1-frac)*f2 + frac*to, the contract's own hit point
 *           4. mm = distance_in_mm(from, p) = sqrt(xd^2 + yd^2 + zd^2) * 10 in double, xd = |from.x - p.x| * spacing.x in float (travel,
 *              ray.cpp:99-103);  dist += mm
 *           5. t = ((dist * 1000.0) / 1.0) / (double)speed_of_sound
 *           6. stop when !(t < max_travel_us)
 *           7. b = the row of t by add_echo's rule, (int)(t / row_dt) (rfimage.h:33-40, through mcrt_row_thresholds); stop when it is not < R
 *           8. rows [b_prev, b) get media;  interface[b] gets the hit triangle's mesh id if it still holds -1 (the shallowest boundary of a
 *              row wins);  the medium is updated (below);  b_prev = b, from = p, k++
 *   after   rows [b_prev, R) get media;  crossings = k, bit 31 set when the walk stopped at the cap or (GEOMETRIC) the stack overflowed
 * Row ownership: the row that contains a boundary belongs to the medium BEHIND the boundary; a layer thinner than a row owns no row and
 * shows in `interface` only.  The tracer deposits a boundary's own echo up to one row EARLIER, at t_start + time_step * (steps - 1): the
 * last whole axial step before the boundary, not the boundary's own time.  And where the material behind a boundary has a non-zero
 * thickness, the tracer's path length runs to the hit point plus a random penetration along the ray (scene.cpp:132-139), so its later
 * boundaries' echoes lie that much deeper than the rows given here, which are measured to the hit points themselves.
 * The medium update.  MCRT_LABEL_TRACED: exactly the four branches of hit_boundary that make the medium and the vascular memory of the
 * refracted ray (ray.cpp:13-47), quirk 1 included -- leaving a non-vascular mesh keeps its mat_inside.  This map explains the picture the
 * tracer draws.  MCRT_LABEL_GEOMETRIC: if the hit mesh is on the stack it is removed (the beam leaves it), else pushed (it enters);
 * media = stack empty ? start_mat : mat_inside(top).  This is the anatomy, for closed, nested meshes whatever their orientation.  On
 * overflow the entry is dropped and bit 31 of crossings is set.
 * A start_offset larger than a wall's thickness skips the far wall in either rule -- the tracer's own behaviour at its 0.1 --: GEOMETRIC
 * callers should pass a small offset such as 1e-3.
 * pos == NULL means the context's transducer (mcrt_set_transducer), and then n_frames must be 1; otherwise pos and dir are pose tables
 * [n_frames][n_elements][3], host or device, with the lifetime rules of mcrt_trace_frames_poses.  Outputs, each a device pointer or
 * NULL, ne = e_end - e_begin: tissue_dev uint8 [n_frames][ne][R] material indices; interface_dev int32 [n_frames][ne][R] mesh ids, -1
 * where no boundary falls; crossings_dev uint32 [n_frames][ne].  Asynchronous on the context's stream, one launch; nothing is allocated
 * after the first call of a size.
 * MCRT_ERR_INVALID: a null context, no scene, no transducer (pos NULL), e_begin >= e_end or e_end > n_elements, only one of pos / dir, all
 * three outputs NULL, an unknown rule, a start_offset that is not finite or is 0, n_frames != 1 with pos NULL, n_frames == 0.
 * MCRT_ERR_LIMIT: more than 254 materials (255 is MCRT_LABEL_NONE), n_frames > 1024.  On an error nothing is launched and nothing is
 * written.  The traversal stack is sized from the tree as in the traced pass; a walk that runs away sets the context's error word.
 * Groups: there is no group call -- the root context has no scene.  Take labels on mcrt_group_member(grp, 0), which shares the root's GPU,
 * and mcrt_synchronize it before the root reads them. */
enum { MCRT_LABEL_TRACED = 0, MCRT_LABEL_GEOMETRIC = 1 };
#define MCRT_LABEL_NONE 255u          /* tissue value of "no data" (outside the sector / sweep) */
#define MCRT_LABEL_MAX_CROSSINGS 64u
typedef struct { uint32_t rule;          /* MCRT_LABEL_*                                                  (TRACED) */
                 float    start_offset;  /* scene units; < 0: the context's ray_start_offset              (-1)     */
} mcrt_label_opts;                       /* 8 bytes: rule at 0, start_offset at 4 */
int mcrt_default_label_opts(mcrt_label_opts *o);                             /* host only */
int mcrt_label_frames(mcrt_ctx *ctx, uint32_t n_frames, uint32_t e_begin, uint32_t e_end,
                      const float *pos /* [n_frames][E][3] host or device, or NULL */, const float *dir /* same */,
                      const mcrt_label_opts *o /* NULL = defaults */,
                      uint8_t *tissue_dev /* [n_frames][ne][R] or NULL */, int32_t *interface_dev /* [n_frames][ne][R] or NULL */,
                      uint32_t *crossings_dev /* [n_frames][ne] or NULL */);
/* Labels as pictures: a NEAREST-NEIGHBOUR gather (labels cannot be interpolated) of tissue maps through the cached maps of
 * mcrt_scan_convert_frames / mcrt_volume_frames -- the same device buffers under the same keys, so alternating a picture and its labels
 * uploads nothing.  Per map coordinate m of an output point, in float:
 *   f = floorf(m);  a = m - f;  i = (long long)f + (a >= 0.5f);   inside when 0 <= i < extent      [extents: E, R and, for the volume, K]
 * out = every coordinate inside ? tissue[..][i_col][i_row] : MCRT_LABEL_NONE; a NaN map value is outside.  Every output element is written.
 * Errors and limits are those of the float calls they mirror (tissue_dev in rf_dev's place).  Interface maps are NOT scan-converted: a
 * one-row arc does not survive a nearest gather at the display's pixel pitch. */
int mcrt_label_scan_convert_frames(mcrt_ctx *ctx, const uint8_t *tissue_dev /* [n_frames][E][R] */, uint32_t n_frames, uint32_t n_elements, uint32_t n_rows,
                                   double radius_mm, double total_angle_rad, uint8_t *out_dev /* [n_frames][out_rows][out_cols] */, uint32_t out_rows, uint32_t out_cols);
int mcrt_label_volume_frames(mcrt_ctx *ctx, const uint8_t *tissue_dev /* [n_frames][K][E][R] */, uint32_t n_frames, uint32_t n_elements, uint32_t n_rows,
                             double radius_mm, double total_angle_rad, const mcrt_sweep *sweep, const mcrt_volume_grid *grid,
                             uint8_t *out_dev /* [n_frames][nw][nv][nu] */);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Acoustic ground truth: how much sound gets there.  The label maps say what tissue a sample shows; these say what fraction of the emitted
 * intensity ARRIVES at it (`transmit`: the shadow behind bone and gas, the enhancement behind fluid) and what fraction each boundary turns
 * back (`reflect`).  It is the quantity the tracer carries along every path (scene.cpp:122-165, ray.cpp:11-97: the attenuation of a segment,
 * the impedance rule at its end) and loses in the Monte-Carlo sum, here carried along the label walk's deterministic central beam: it
 * depends on neither seed, samples, frame id nor texture.  Both maps are float stacks [F][E][R]: mcrt_scan_convert_frames,
 * mcrt_volume_frames, mcrt_recon_frames and mcrt_render_frames take them as they are, so they are registered to every picture with no
 * gather of their own.
 *
 * THE WALK is mcrt_label_frames' own, steps 1-8 of its comment, unchanged -- the segment arithmetic, the closest hit, the hit point, dist,
 * t and the stop conditions, the row b, MCRT_LABEL_MAX_CROSSINGS, the medium update of `rule` --, so crossings equals mcrt_label_frames'
 * bit for bit under the same rule and start_offset.  On top of it the beam carries I (float, 1.0f at the start) and t_prev (double, 0.0);
 * every float operation is rounded on its own (no fma), expf is the contract's (det_expf), freq is the context's frequency, sos its speed
 * of sound as a double, imp(m) / att(m) the impedance and the attenuation of material m (in MCRT_TRANSMIT_BOUNDARIES att(m) is 0.0f):
 *   rows    a row r of [b_prev, b), m the medium the segment runs in:
 *               dt = (double)r * row_dt_us - t_prev;  if (!(dt > 0.0)) dt = 0.0;   mm_r = (dt * sos) / 1000.0
 *               transmit[r] = I * expf(-att(m) * ((float)mm_r * 0.01f) * freq)
 *           -- the tracer's own attenuation with the distance to the row's start in place of the distance to the boundary.  The row that
 *           holds the previous boundary takes the value just behind it (dt clamps to 0); row 0 is exactly 1.0f
 *   at the boundary (mm: step 4's double, m: the medium BEFORE the update, m2: the medium after it)
 *               Ia = I * expf(-att(m) * ((float)mm * 0.01f) * freq)
 *               nn = normalized(cross(v1 - v0, v2 - v0)) of the hit triangle;  inc = dot(dir, -nn);  if (inc < 0) inc = dot(dir, nn)
 *               (i_refl, i_refr) = mcrt_transmit_boundary(imp(m), imp(m2), inc, Ia)
 *               reflect[b] = i_refl if no boundary has written row b yet (the shallowest boundary of a row wins, as for `interface`)
 *               I = i_refr > 0 ? i_refr : 0.0f;   t_prev = t, b_prev = b, from = p
 *           A NaN or a negative remainder ends the energy, not the walk: the walk goes on (crossings stays the label walk's), every later
 *           row is 0 * ...
 *   after   rows [b_prev, R) are filled from the last segment by the same rule;  reflect is 0.0f wherever no boundary falls
 * mcrt_transmit_boundary is the tracer's impedance rule (in ray.cpp:11-97), host only, no GPU:
 *               rr = z_before / z_after;  refa = 1 - rr * rr * (1 - inc * inc)
 *               refa < 0 (total internal reflection):  i_refl = intensity, i_refr = 0
 *               else  refa = sqrtf(refa);  num = z_before * inc - z_after * refa;  den = z_before * inc + z_after * refa;  qq = num / den
 *                     i_refl = (float)((double)intensity * ((double)qq * (double)qq));  i_refr = intensity - i_refl
 * THIS IS THE ENERGY THE GEOMETRY ALLOWS, NOT ONE SAMPLE'S FATE: no random perturbation of the normal, no thickness penetration, no
 * intensity_epsilon cut, the beam stays straight (no refraction), and the way back to the probe is not attenuated.  A thresholded shadow
 * mask is a caller's one comparison; `reflect` is not made into a picture (a one-row arc does not survive scan conversion).
 * pos, dir, e_begin, e_end, n_frames: as mcrt_label_frames.  Outputs, each a device pointer or NULL, ne = e_end - e_begin: transmit_dev and
 * reflect_dev float [n_frames][ne][R], crossings_dev uint32 [n_frames][ne]; every element of every non-NULL output is written, whatever
 * the pointers' alignment beyond a float's.  Asynchronous on the context's stream, one launch; nothing is allocated after the first call
 * of a size.  Errors and limits: mcrt_label_frames' with these three outputs in its outputs' place, without the limit of 254 materials,
 * and MCRT_ERR_INVALID for an unknown mode.  On an error nothing is launched and nothing is written.  Groups: as mcrt_label_frames -- take
 * the maps on mcrt_group_member(grp, 0). */
enum { MCRT_TRANSMIT_TOTAL = 0,        /* attenuation along the beam and the loss at every boundary */
       MCRT_TRANSMIT_BOUNDARIES = 1 }; /* the boundaries alone: every attenuation taken as 0.0f (piecewise constant) */
typedef struct { uint32_t mode;         /* MCRT_TRANSMIT_*                                   (TOTAL)  */
                 uint32_t rule;         /* MCRT_LABEL_TRACED / MCRT_LABEL_GEOMETRIC          (TRACED) */
                 float    start_offset; /* as mcrt_label_opts                                (-1)     */
} mcrt_transmit_opts;                   /* 12 bytes */
int mcrt_default_transmit_opts(mcrt_transmit_opts *o);                                   /* host only */
/* the boundary rule alone, on the host (no GPU): what one crossing does to an intensity.  MCRT_ERR_INVALID for a null i_refl or i_refr */
int mcrt_transmit_boundary(float z_before, float z_after, float inc, float intensity, float *i_refl, float *i_refr);
int mcrt_transmit_frames(mcrt_ctx *ctx, uint32_t n_frames, uint32_t e_begin, uint32_t e_end,
                         const float *pos, const float *dir,              /* as mcrt_label_frames */
                         const mcrt_transmit_opts *o /* NULL = defaults */,
                         float *transmit_dev  /* [n_frames][ne][R] or NULL */,
                         float *reflect_dev   /* [n_frames][ne][R] or NULL */,
                         uint32_t *crossings_dev /* [n_frames][ne] or NULL */);

/* Labels in 3-D, I: a freehand label volume -- the ground truth of mcrt_recon_frames' voxels -- by MAJORITY VOTE.  The input is the tissue
 * stack uint8 [F][E][R] that mcrt_label_frames wrote for the pose tables [F][E][3], those tables, and row_mm, unit_mm and the WORLD-frame
 * grid exactly as mcrt_recon_frames takes them.  The position of sample (f, e, r) is mcrt_recon_frames' contract word for word: t, P_k, x_c,
 * i_c = floorf(x_c + 0.5f) and `inside`, with A and b from mcrt_recon_transform and row_u = (float)(row_mm / unit_mm).
 * The vote, per sample with label l = stack[f][e][r]:
 *   if !inside: stats[0]++          else if l >= n_labels: stats[1]++     (MCRT_LABEL_NONE and anything else out of range)
 *   else: votes[voxel][l]++
 * Resolve: count = the sum of votes[voxel][l] over l.  A voxel with count > 0 gets the label with the most votes, on a tie the SMALLEST such
 * label; votes_dev gets the winner's votes (the purity of a voxel is votes / count), count_dev gets count.
 * Hole filling, for a voxel with count == 0 when fill_radius H > 0 -- the structure of mcrt_recon_frames' rule:
 *   for h = 1..H:
 *       tally[l] = 0 for every l;  n = 0
 *       over the cube [-h, h]^3: every neighbour inside the block with count > 0 adds ONE to tally[its winning label];  n++
 *       if n >= fill_min: label = the label of the largest tally, on a tie the smallest;  stop
 *   if no h succeeded (or H == 0): MCRT_LABEL_NONE
 * A filled hole keeps count = 0 and votes = 0.  Only sampled voxels are read, never filled ones, and every sum is an integer: neither the
 * order in which the device adds nor its tiling shows in the result.  Every voxel of every requested output is written.
 * What follows: where every float sample is usable (mcrt_recon_frames) and every label is below n_labels, count_dev equals
 * mcrt_recon_frames' count_dev for the same poses and grid, and a voxel is MCRT_LABEL_NONE exactly where the float volume is `empty` -- the
 * defaults of fill_radius and fill_min are mcrt_recon_opts' own on purpose, so that the two volumes fill the same holes. */
typedef struct { uint32_t n_labels;    /* 1..254: labels at or above it do not vote; the scene's material count   (no default) */
                 uint32_t fill_radius; /* H, 0..3: 0 = no hole filling                                             (1)          */
                 uint32_t fill_min;    /* >= 1: sampled neighbours a hole needs                                    (1)          */
} mcrt_recon_label_opts;               /* 12 bytes: n_labels 0, fill_radius 4, fill_min 8 */
/* n_labels as given, the defaults above; host only.  MCRT_ERR_INVALID for a null o */
int mcrt_default_recon_label_opts(mcrt_recon_label_opts *o, uint32_t n_labels);
/* The rule above.  stack_dev: device uint8 [F][E][R]; pos, dir: [F][E][3], host or device, with the lifetime rule of
 * mcrt_trace_frames_poses.  Outputs, each a device pointer or NULL, at least one given: out_dev uint8 [nw][nv][nu]; count_dev and votes_dev
 * uint32 of the same shape; stats_dev uint32 [2].  Asynchronous on the context's stream: a clear of the vote table, k_recon_label_splat,
 * k_recon_label_resolve.  The vote table (n_labels * nu*nv*nw * 4 bytes) is a scratch buffer of the context that grows to the largest call:
 * nothing is allocated on a repeat.  Everything is checked before anything is enqueued.  MCRT_ERR_INVALID, the message naming the field: a
 * null ctx, stack_dev, pos, dir, grid or o (n_labels has no default); all four outputs NULL; a zero n_frames, n_elements or n_rows; row_mm or
 * unit_mm not finite or not > 0; n_labels outside 1..254, a fill_radius above 3, a fill_min of 0; a grid that mcrt_recon_transform refuses;
 * an output that overlaps the stack or another output.  MCRT_ERR_LIMIT: those of mcrt_recon_frames (n_rows > 2048, n_frames > 65535,
 * F*E*R >= 2^31, nu*nv*nw >= 2^31, the thin-block tile limit), and nu*nv*nw * n_labels >= 2^31.  On any error nothing is written.
 * Groups: call it on mcrt_group_root(), with the labels taken on mcrt_group_member(grp, 0) as above. */
int mcrt_recon_label_frames(mcrt_ctx *ctx, const uint8_t *stack_dev /* [F][E][R] */, uint32_t n_frames, uint32_t n_elements, uint32_t n_rows,
                            const float *pos /* [F][E][3] host or device */, const float *dir /* same */, double row_mm, double unit_mm,
                            const mcrt_volume_grid *grid /* WORLD frame, mm */, const mcrt_recon_label_opts *o,
                            uint8_t *out_dev /* [nw][nv][nu] or NULL */, uint32_t *count_dev /* same or NULL */, uint32_t *votes_dev /* same or NULL */,
                            uint32_t *stats_dev /* [2] or NULL */);
/* Labels in 3-D, II: the label of what a rendering shows.  label_dev is a label block uint8 [n_frames][nw][nv][nu] -- what
 * mcrt_label_volume_frames wrote for a swept volume, or mcrt_recon_label_frames for a freehand one --, view the mcrt_render_view of the
 * rendering and depth_dev the [n_frames][ny][nx] that mcrt_render_frames wrote with it (MIP: the step of the maximum; SURFACE: the step at
 * which the transmittance fell to a half; MEAN: -1, nothing is "seen").  Per frame and pixel (i, j), in float, one rounding per operation,
 * no fma:
 *   s = depth;   if !(s >= 0 && s < (float)n_steps): out = MCRT_LABEL_NONE                          (a NaN too)
 *   p_c = ((origin_c + (float)i * di_c) + (float)j * dj_c) + s * ds_c            c = u, v, w
 *         (mcrt_render_frames' own expression: for the s it wrote, p is bit for bit the point it sampled at that step)
 *   f = floorf(p_c);  a = p_c - f;  k_c = f + (a >= 0.5f ? 1 : 0)                (the nearest rule of the label gathers)
 *   out = 0 <= k_c < n_c for every c (compared in float) ? label[frame][k_w][k_v][k_u] : MCRT_LABEL_NONE
 * Every output pixel is written.  Asynchronous on the context's stream, one launch; allocates nothing and uploads nothing.  Errors and limits
 * are mcrt_render_frames' for the block and the view (null ctx / label_dev / view / depth_dev / out_dev, zero sizes, a view entry that is not
 * finite: MCRT_ERR_INVALID; n_steps outside 1..4096, nu, nv or nw >= 2^24, nu*nv*nw or nx*ny >= 2^31, n_frames > 65535: MCRT_ERR_LIMIT), and
 * MCRT_ERR_INVALID for an out_dev that overlaps label_dev or depth_dev.  On an error nothing is launched.  Groups: call it on mcrt_group_root(). */
int mcrt_render_label_frames(mcrt_ctx *ctx, const uint8_t *label_dev /* [n_frames][nw][nv][nu] */, uint32_t n_frames, uint32_t nu, uint32_t nv, uint32_t nw,
                             const mcrt_render_view *view, const float *depth_dev /* [n_frames][ny][nx] */, uint8_t *out_dev /* [n_frames][ny][nx] */);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Colour Doppler: a slow-time ensemble, the Kasai autocorrelator, the flow overlay and the true axial velocity per sample.  Every scene
 * file marks meshes as vascular and carries a BLOOD material; a colour line is N pulses (the ensemble) fired down the same scan-line, and
 * the phase the moving echo turns by from pulse to pulse is the velocity.  The reference has no counterpart.  THE MODEL: the ensemble is
 * SYNTHESISED from one traced frame and not traced N times (every frame id has its own Philox key, so the clutter of two traces
 * decorrelates far more than blood would).  The raw trace is split by tissue label into what stands still and what moves
 * (mcrt_flow_split_frames); both images go through the existing PSF and mcrt_detect_frames(iq_dev); and the ensemble of a sample is
 *   z_n = static + moving * p^n + noise_n,   n = 0 .. N-1,
 * with the phasor p of the sample's material and scan-line: the narrow-band model the autocorrelator of Kasai et al. (1985) is derived under.
 * LEFT OUT: velocity profiles (a material has ONE velocity vector), transit-time and axial-shift decorrelation of moving speckle, the
 * blood echo the PSF leaks outside the lumen (it keeps the label of where it lands), power / variance displays, persistence.  (A velocity
 * profile, a pulsatile waveform and the spectral display are the spectral chain's, below: mcrt_spectral_series_frames and what follows it.)
 * An opt-in chain; without it no call and no bit changes.
 *
 * Throughout, every float operation is rounded once: no fma, correctly rounded / and sqrtf, no device transcendental. */
#define MCRT_FLOW_WALL_NONE 0u
#define MCRT_FLOW_WALL_MEAN 1u
#define MCRT_FLOW_WALL_LINEAR 2u
typedef struct {
    uint32_t n_packets;     /* N, the pulses of the ensemble: 2..16; default 8 */
    uint32_t wall;          /* the clutter ("wall") filter over the ensemble, MCRT_FLOW_WALL_*; default MEAN */
    uint32_t avg_rows;      /* half-window of the spatial average along the scan-line: 0..8; default 2 */
    uint32_t avg_lines;     /* ... and across scan-lines: 0..4; default 1 */
    float prf_hz;           /* pulse repetition frequency, finite and > 0; default 4000 (read by mcrt_flow_nyquist alone) */
    float freq_mhz;         /* the colour pulse's centre frequency; <= 0 (default 0): the caller's (the context's) frequency (mcrt_flow_nyquist alone) */
    float sigma;            /* the receiver noise per I/Q component, finite and >= 0, used when no sigma_dev is given; default 0 */
    uint32_t seed;          /* Philox key word 0 of the noise streams; default 0x464C4F57 */
} mcrt_flow_opts;           /* 32 bytes */
/* the defaults above.  MCRT_ERR_INVALID for a null o.  Host only. */
int mcrt_default_flow_opts(mcrt_flow_opts *o);
/* the velocity whose phase step is pi, in double:  f = o->freq_mhz > 0 ? (double)o->freq_mhz : freq_mhz;
 *   *v_nyq_mm_s = (speed_of_sound * 1000.0 * (double)o->prf_hz) / (4.0 * (f * 1.0e6))           (1500 m/s, 4.5 MHz, 4 kHz: 333.33 mm/s)
 * Host only.  MCRT_ERR_INVALID for a null pointer, options out of range, or an f or a speed_of_sound that is not finite and > 0. */
int mcrt_flow_nyquist(const mcrt_flow_opts *o, double freq_mhz, double speed_of_sound, double *v_nyq_mm_s);
/* the phasor and the true axial velocity of every (material, scan-line).  vel_mm_s [n_labels][3]: a velocity vector per material
 * [mm/s]; dir [E][3]: the scan-lines' directions (mcrt_transducer's).  In double, with the floats widened exactly:
 *   v_t = 0.0 - ((vx * dx + vy * dy) + vz * dz)          the velocity TOWARDS the probe, positive
 *   truth[l][e] = (float)v_t;      phi = 3.141592653589793 * v_t / v_nyq_mm_s;      phasor[l][e] = ((float)cos(phi), (float)sin(phi))
 * and a material whose three components are all zero gets exactly truth +0.0f and phasor (1.0f, +0.0f).  Host only.  MCRT_ERR_INVALID
 * for a null pointer, n_labels == 0 or n_elements == 0, a v_nyq_mm_s that is not finite and > 0, or any vel / dir that is not finite;
 * MCRT_ERR_LIMIT for n_labels > 254; on an error nothing is written. */
int mcrt_flow_phasors(double v_nyq_mm_s, const float *vel_mm_s /* [n_labels][3] */, const float *dir /* [E][3] */, uint32_t n_labels, uint32_t n_elements,
                      float *phasor /* [n_labels][E][2] */, float *truth /* [n_labels][E] */);
/* the integer noise draws of one image's ensemble, d[n][e][r][0..1] (I, Q): one Philox4x32-10 block o[0..3] per (e, r, n) with the counter
 * (e, r, 0x464C4F57, n) and the key (seed, image_id);
 *   d_I = ((o0 & 0xffff) + (o0 >> 16) + (o1 & 0xffff) + (o1 >> 16)) - 131070,   d_Q the same of o2, o3
 * an Irwin-Hall sum of four 16-bit uniforms about its mean: variance exactly 1431655765, so inv_std = (float)(1.0 / sqrt(1431655765.0)).
 * Counter word 2 differs from mcrt_noise_frames' (0x4E4F4953) and from the tracer's (a bounce, < 16): the streams cannot coincide.  Host
 * only.  MCRT_ERR_INVALID for a null d, zero sizes or n_packets outside 2..16; MCRT_ERR_LIMIT for n_rows > 2048. */
int mcrt_flow_draws(uint32_t seed, uint32_t image_id, uint32_t n_elements, uint32_t n_rows, uint32_t n_packets, int32_t *d /* [N][E][R][2] */);
/* the colour table of the overlay, lut[i] = (r, g, b).  kind 0, the red-towards / blue-away map, in integer arithmetic:
 *   i == 128:       (0, 0, 0)
 *   i = 129..255:   k = i - 128;  (128 + k, k <= 64 ? 0 : (k - 64) * 4, 0)                  red to yellow
 *   i = 1..127:     k = 128 - i;  (0, k <= 64 ? 0 : (k - 64) * 4, 128 + k)                  blue to cyan
 *   i == 0:         lut[1]
 * Host only.  MCRT_ERR_INVALID for a null lut or another kind. */
int mcrt_colour_map(uint32_t kind, uint8_t *lut /* [256][3] */);
/* the raw trace split by label, before the PSF:  with l = tissue_dev[f][e][r] and  mv = l < n_labels && moving[l] != 0,
 *   out_dev[f][0][e][r] = mv ? +0.0f : rf's own bits;      out_dev[f][1][e][r] = mv ? rf's own bits : +0.0f
 * (MCRT_LABEL_NONE and any label >= n_labels stand still; a NaN goes where its label sends it).  moving [n_labels] is HOST memory, free
 * when the call returns.  Every element of out_dev [F][2][E][R] is written; rf_dev and tissue_dev are read only.  What follows is
 * mcrt_convolve_frames* and mcrt_detect_frames(iq_dev) over the 2 F images, untouched.  Asynchronous on the context's stream.
 * MCRT_ERR_INVALID for a null pointer, zero sizes, n_labels == 0, or an out_dev that overlaps rf_dev or tissue_dev; MCRT_ERR_LIMIT for
 * n_labels > 254 or a stack of 2^31 samples or more; on any error nothing is launched.  Groups: call it on mcrt_group_root(). */
int mcrt_flow_split_frames(mcrt_ctx *ctx, const float *rf_dev /* [F][E][R] */, const uint8_t *tissue_dev /* [F][E][R] */, uint32_t n_frames,
                           uint32_t n_elements, uint32_t n_rows, const uint8_t *moving /* [n_labels] */, uint32_t n_labels, float *out_dev /* [F][2][E][R] */);
/* the colour processor.  Per sample (f, e, r) with l = tissue_dev[f][e][r], N = o->n_packets, (c, s) = l < n_labels ? phasor[l][e] : (1, 0):
 * 1. THE ENSEMBLE.  m_0 = iq_moving_dev[f][e][r];  m_(n+1) = (a * c - b * s, a * s + b * c) of m_n = (a, b): four products, one
 *    subtraction, one addition.  k = sigma_f * inv_std with sigma_f = sigma_dev ? sigma_dev[f] : o->sigma.  Per component
 *      z_n = (static + m_n) + k * (float)d_n
 *    where the first addition is skipped when iq_static_dev is NULL and the noise term when k == 0 (no Philox block is computed then);
 *    d_n are mcrt_flow_draws' of the image id first_image_id + f.
 * 2. THE WALL FILTER over n, per component.  NONE: w = z.  MEAN: w_n = z_n - (the PAIRWISE sum of z_n) / (float)N -- level by level
 *    neighbours are added in pairs, (z_0 + z_1), (z_2 + z_3), ..., an odd last term is carried up as it is, until one term is left: N
 *    equal terms then sum to N times the term exactly where N is a power of two, and what stands still leaves the filter as +0.0f.
 *    LINEAR: after MEAN, with t_n = (float)(2 n - (N - 1)):  w_n = w_n - t_n * ((sum of t_n * w_n) / (sum of t_n * t_n)), both sums
 *    ascending from 0.0f.
 * 3. THE AUTOCORRELATION, every sum ascending from 0.0f, the products before the sums:
 *      r0 = sum over n of (w_n.re * w_n.re + w_n.im * w_n.im)
 *      r1 = sum over n = 0 .. N-2 of w_(n+1) * conj(w_n):  re += (a * c + b * d),  im += (b * c - a * d)  with w_(n+1) = (a, b), w_n = (c, d)
 * 4. THE AVERAGE, for each of the three planes x = r0, Re r1, Im r1, with a = o->avg_rows and b = o->avg_lines:
 *      s[e][r] = sum over dr = -a .. a ascending, rows r + dr inside [0, R), of x[e][r + dr]              (from 0.0f)
 *      S[e][r] = sum over de = -b .. b ascending, lines e + de inside [0, E), of s[e + de][r]            (from 0.0f)
 *      out = S / (float)cnt,  cnt = (rows inside) * (lines inside)
 *    The separable order is the contract; a window larger than the image is the whole image.
 * 5. THE OUTPUTS, each a device pointer or NULL, at least one given:
 *      corr_dev [F][3][E][R]   the planes r0, Re r1, Im r1 (plane-major: mcrt_scan_convert_frames over 3 F frames gathers it as it is)
 *      vel_dev [F][E][R]       mcrt_det_atan2f(Im, Re) * (float)(v_nyq_mm_s / 3.141592653589793)
 *      var_dev [F][E][R]       r0 > 0 ? v : 0.0f  with v = 1.0f - sqrtf(Re * Re + Im * Im) / r0, then v < 0 -> 0.0f, v > 1 -> 1.0f (a NaN stays)
 *      truth_dev [F][E][R]     l < n_labels ? truth[l][e] : 0.0f -- the registered ground truth, not aliased
 * mcrt_det_atan2f(y, x), float throughout:  ax = |x|, ay = |y|;  ay > ax ? (hi, lo) = (ay, ax) : (hi, lo) = (ax, ay);  hi == 0 gives +0.0f;
 *   t = lo / hi;  s = t * t;  P = c5;  P = P * s + c_j for j = 4 .. 0 (a multiply, then an add);  a = t * P;
 *   c0..c5 = 0.99997726f, -0.33262347f, 0.19354346f, -0.11643287f, 0.05265332f, -0.01172120f;
 *   ay > ax: a = 1.5707964f - a;   x < 0: a = 3.1415927f - a;   y < 0: a = -a.       Within 1e-5 rad of atan2 (measured 1.96e-6).
 * phasor [n_labels][E][2] and truth [n_labels][E] are HOST tables (mcrt_flow_phasors'), finite, free when the call returns; they live in
 * buffers of the context and are copied only when they differ from what is there.  Every element of every output given is written; the
 * inputs are read only; any overlap of an output with an input or with another output is MCRT_ERR_INVALID.  The per-sample correlation
 * lives in a grow-only buffer of the context: nothing is allocated after the first call at a size.  Asynchronous on the context's stream.
 * MCRT_ERR_INVALID for a null ctx, iq_moving_dev, tissue_dev, phasor, truth or o, zero sizes, n_labels == 0, options out of range, a
 * v_nyq_mm_s that is not finite and > 0, a table entry that is not finite, no output; MCRT_ERR_LIMIT for n_rows > 2048, n_labels > 254, a
 * stack of 2^31 samples or more, image ids that pass 2^32; on any error nothing is launched and nothing is written.  Groups: call it on
 * mcrt_group_root(). */
int mcrt_flow_frames(mcrt_ctx *ctx, const float *iq_static_dev /* [F][E][R][2] or NULL */, const float *iq_moving_dev /* [F][E][R][2] */,
                     const uint8_t *tissue_dev /* [F][E][R] */, uint32_t n_frames, uint32_t n_elements, uint32_t n_rows, const mcrt_flow_opts *o,
                     double v_nyq_mm_s, const float *phasor /* [n_labels][E][2] */, const float *truth /* [n_labels][E] */, uint32_t n_labels,
                     uint32_t first_image_id, const float *sigma_dev /* [F] or NULL */, float *corr_dev /* [F][3][E][R] or NULL */,
                     float *vel_dev /* [F][E][R] or NULL */, float *var_dev /* [F][E][R] or NULL */, float *truth_dev /* [F][E][R] or NULL */);
/* the overlay.  corr_img_dev [F][3][H][W] is mcrt_flow_frames' corr_dev through mcrt_scan_convert_frames (the autocorrelation is gathered
 * and not the velocity: r0 and r1 interpolate linearly across an aliasing boundary, an angle does not); grey_dev [F][H][W] the bytes of
 * mcrt_bmode_frames.  Per pixel, with (r0, re, im) the three planes and g the grey byte:
 *   ang = mcrt_det_atan2f(im, re);   v = ang * (float)(v_nyq_mm_s / 3.141592653589793)
 *   show = r0 > power_thr && fabsf(v) >= vel_thr_mm_s && g <= grey_max            (a NaN anywhere: not shown)
 *   idx = 128 + (int)rintf(ang * (float)(127.0 / 3.141592653589793)), clamped to 1 .. 255
 *   rgb_dev[f][y][x] = show ? lut[idx] : (g, g, g);      vel_img_dev[f][y][x] = show ? v : 0.0f        (vel_img_dev may be NULL)
 * lut [256][3] is HOST memory (mcrt_colour_map's or the caller's own), free when the call returns.  Asynchronous on the context's
 * stream.  MCRT_ERR_INVALID for a null ctx, corr_img_dev, grey_dev, lut, o or rgb_dev, zero sizes, a threshold that is not finite, a
 * vel_thr_mm_s < 0, grey_max > 255, a v_nyq_mm_s that is not finite and > 0, an output that overlaps an input or the other output;
 * MCRT_ERR_LIMIT for 2^31 pixels or more; on any error nothing is launched.  Groups: call it on mcrt_group_root(). */
typedef struct { float power_thr; float vel_thr_mm_s; uint32_t grey_max; } mcrt_colour_opts;      /* defaults 0, 0, 255; 12 bytes */
int mcrt_default_colour_opts(mcrt_colour_opts *o);
int mcrt_colour_frames(mcrt_ctx *ctx, const float *corr_img_dev /* [F][3][H][W] */, const uint8_t *grey_dev /* [F][H][W] */, uint32_t n_frames,
                       uint32_t height, uint32_t width, const uint8_t *lut /* [256][3] */, const mcrt_colour_opts *o, double v_nyq_mm_s,
                       uint8_t *rgb_dev /* [F][H][W][3] */, float *vel_img_dev /* [F][H][W] or NULL */);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Spectral (pulsed-wave) Doppler: a sample gate on one scan-line, a slow-time series of thousands of pulses under a pulsatile speed
 * waveform and a velocity profile across the lumen, its short-time FFT, and the sonogram (velocity over time).  The reference has no
 * counterpart.  THE MODEL is synthesised from ONE traced frame, as the colour ensemble is and for the same reason.  A GATE is G
 * consecutive RF rows of one scan-line of one image.  The static I/Q of a gate row stands still; the moving I/Q of row r turns by the
 * phase theta_r(t) = rate_r * Phi(t) at pulse t, where Phi(t) is the accumulated phase of the vessel's centre-line speed waveform (the
 * pulsatile flow) and rate_r the row's share of that speed times the cosine to the beam (the velocity profile).  Rows at different
 * depths of the lumen turn at different rates: a small gate on the axis gives a narrow line at the peak velocity, a gate across the
 * lumen fills the spectrum from 0 to the peak, and the gate's moving speckle decorrelates over the series as a consequence.
 * PHASES ARE INTEGERS, so the device and any mirror agree whatever the order: Phi(t) is an int64 in units of 2^-32 turn, rate_r an
 * int32 in Q16 with |rate| <= 65536, and the rotor comes from a 4096-entry cos/sin table built on the host (its worst spur under a Hann
 * window stays below -68 dB; 1024 entries give -60 dB, too coarse for a 60 dB display).
 * LEFT OUT: the chord through the lumen stands in for the radial distance (the profile is exact only for a beam that crosses the
 * vessel's axis); one waveform per call; transit-time broadening; spectral display on swept, compounded or banded frames; audio
 * resampling (the I/Q series itself is the output); automatic peak-velocity tracing and the indices (PI, RI).
 * An opt-in chain; without it no call and no bit changes.
 *
 * Throughout, every float operation is rounded once: no fma, correctly rounded / and sqrt, no device transcendental except the log10f
 * of mcrt_sonogram_frames. */
#define MCRT_SPECTRAL_WALL_NONE 0u
#define MCRT_SPECTRAL_WALL_MEAN 1u
typedef struct {
    uint32_t n_pulses;      /* T, the pulses of the series: 1..16384; default 2048 */
    uint32_t gate_rows;     /* G, the RF rows of a gate: 1..64; default 8 */
    uint32_t n_fft;         /* N, the window of the short-time FFT: 32, 64, 128, 256 or 512; default 128 */
    uint32_t hop;           /* pulses from one spectrum (column) to the next: 1..N; default 32 */
    uint32_t wall;          /* the clutter filter over a window, MCRT_SPECTRAL_WALL_*; default MEAN */
    uint32_t wall_bins;     /* bins |i - N/2| < wall_bins of a spectrum are written as +0.0f: 0..N/4; default 2 */
    float sigma;            /* the receiver noise per I/Q component of ONE row, finite and >= 0, used when no sigma_dev is given; default 0 */
    uint32_t seed;          /* Philox key word 0 of the noise stream; default 0x53504543 */
} mcrt_spectral_opts;       /* 32 bytes */
typedef struct { uint32_t image, line, row0; } mcrt_gate;      /* rows row0 .. row0 + G - 1 of scan-line `line` of image `image`; 12 bytes */
/* the defaults above.  MCRT_ERR_INVALID for a null o.  Host only. */
int mcrt_default_spectral_opts(mcrt_spectral_opts *o);
/* The host-only helpers below refuse null pointers, zero sizes and non-finite input with MCRT_ERR_INVALID and sizes past a limit with
 * MCRT_ERR_LIMIT; on an error nothing is written.
 * the rotor table:  a = 6.283185307179586 * i / 4096.0 in double;  lut[i] = ((float)cos(a), (float)sin(a)). */
int mcrt_spectral_rotor(float *lut /* [4096][2] */);
/* the accumulated phase of a centre-line speed waveform [mm/s], in units of 2^-32 turn:
 *   step_t = llrint((double)speed_mm_s[t] / v_nyq_mm_s * 2147483648.0);      phase[0] = 0;   phase[t + 1] = phase[t] + step_t
 * (the Nyquist velocity is half a turn per pulse).  MCRT_ERR_INVALID for a v_nyq_mm_s that is not finite and > 0 or a speed that is not
 * finite; MCRT_ERR_LIMIT for n_pulses > 16384 or a |step_t| above 2^32 -- twice the Nyquist velocity: aliasing up to
 * there is allowed and shows as aliasing. */
int mcrt_spectral_phase(double v_nyq_mm_s, const float *speed_mm_s /* [T] */, uint32_t n_pulses, int64_t *phase /* [T] */);
/* the velocity profile across a lumen, a share in [0, 1] of the centre-line speed per gate row r = row0 .. row0 + G - 1 of ONE
 * scan-line's tissue labels (mcrt_label_frames') tissue_line [R].  With l = tissue_line[r]: a row with l >= n_labels or moving[l] == 0
 * gets +0.0f.  Otherwise [a, b] is the longest run of rows with label l that holds r, over the whole scan-line and not only the gate, and
 *   x = (r - (a + b) / 2.0) / ((b - a + 1) / 2.0);      frac = (float)(1.0 - pow(fabs(x), exponent))        in double
 * exponent == 0 gives 1.0f (plug flow), 2 a parabola.  MCRT_ERR_INVALID for n_labels == 0, row0 + G > R, an exponent that is not finite
 * or neither 0 nor >= 1; MCRT_ERR_LIMIT for G > 64 or n_labels > 254. */
int mcrt_spectral_profile(const uint8_t *tissue_line /* [R] */, uint32_t n_rows, uint32_t row0, uint32_t gate_rows, const uint8_t *moving /* [n_labels] */,
                          uint32_t n_labels, double exponent, float *frac /* [G] */);
/* the rows' rates in Q16:  rate = (int32_t)llrint(65536.0 * (double)frac * axial).  axial, in [-1, 1], is the cosine towards the probe:
 * 0.0 - (v^ . dir_e) of the material's unit velocity and the gate line's direction, as in mcrt_flow_phasors.  MCRT_ERR_INVALID for an
 * axial outside [-1, 1] or a frac outside [0, 1]; MCRT_ERR_LIMIT for G > 64. */
int mcrt_spectral_rates(const float *frac /* [G] */, uint32_t gate_rows, double axial, int32_t *rate /* [G] */);
/* the window of the short-time FFT.  kind 0: all 1.0f;  kind 1 (Hann): h[n] = (float)(0.5 - 0.5 * cos(6.283185307179586 * n / N)) in
 * double.  MCRT_ERR_INVALID for another kind or an N that is not 32, 64, 128, 256 or 512. */
int mcrt_spectral_window(uint32_t kind, uint32_t n_fft, float *h /* [N] */);
/* the twiddles of the FFT:  a = 6.283185307179586 * k / N in double;  tw[k] = ((float)cos(a), (float)(0.0 - sin(a))),  k < N/2.  The
 * library keeps this table per N on the device; the export exists for mirrors.  MCRT_ERR_INVALID for an N as above. */
int mcrt_spectral_twiddles(uint32_t n_fft, float *tw /* [N/2][2] */);
/* the integer noise draws of one gate's series, d[t][0..1] (I, Q): one Philox4x32-10 block per pulse with the counter
 * (line, row0, 0x53504543, t) and the key (seed, image_id); d_I and d_Q are mcrt_flow_draws' Irwin-Hall sums of o0, o1 and o2, o3, with
 * the same inv_std = (float)(1.0 / sqrt(1431655765.0)).  Counter word 2 differs from the tracer's (< 16), mcrt_noise_frames'
 * (0x4E4F4953) and mcrt_flow_frames' (0x464C4F57).  MCRT_ERR_LIMIT for n_pulses > 16384. */
int mcrt_spectral_draws(uint32_t seed, uint32_t image_id, uint32_t line, uint32_t row0, uint32_t n_pulses, int32_t *d /* [T][2] */);
/* a pulsatile speed waveform -- a convenience, not physiology.  In double, then cast to float:
 *   u = t * beats_per_min / (60.0 * prf_hz);   x = u - floor(u);   s = sin(3.141592653589793 * x / 0.3)
 *   speed[t] = (float)(v_min + (v_peak - v_min) * (x < 0.3 ? s * s : 0.0))
 * MCRT_ERR_INVALID for a prf_hz or a beats_per_min that is not finite and > 0 or a speed that is not finite; MCRT_ERR_LIMIT for
 * n_pulses > 16384. */
int mcrt_pulse_waveform(double prf_hz, double beats_per_min, double v_peak_mm_s, double v_min_mm_s, uint32_t n_pulses, float *speed_mm_s /* [T] */);
/* THE SERIES of every gate, series_dev [n_gates][T][2].  iq_static_dev (or NULL) and iq_moving_dev [F][E][R][2] are the detected pairs of
 * what stands still and what moves (mcrt_flow_split_frames, the PSF, mcrt_detect_frames(iq_dev)), T = o->n_pulses, G = o->gate_rows.
 * Per gate j = (image, line, row0), with the rows r = row0 .. row0 + G - 1 ascending, w_r = weight[r - row0], S_r and M_r the static and
 * the moving pair of (image, line, r):
 *   zs = sum over r of (w_r * S_r), per component, from 0.0f;  without a static stack zs = (+0.0f, +0.0f)
 *   A_r = (w_r * M_r.re, w_r * M_r.im)
 * and per pulse t:
 *   theta = (uint32_t)((phase[t] * (int64_t)rate[j][r - row0]) >> 16)            (an arithmetic shift: the product may be negative)
 *   idx = ((theta + 0x80000u) >> 20) & 4095;      (c, s) = lut[idx]              (mcrt_spectral_rotor's table)
 *   acc.re += (A_r.re * c - A_r.im * s);   acc.im += (A_r.re * s + A_r.im * c)   over r ascending from 0.0f, the products before the sums
 *   z_t = (zs + acc) + k * (float)d_t                                            per component
 * with k = (sigma_f * wnorm) * inv_std, sigma_f = sigma_dev ? sigma_dev[image] : o->sigma, wnorm = (float)sqrt(sum of (double)w_r *
 * (double)w_r, ascending) -- the noise of G summed rows is that of one receiver -- and d_t mcrt_spectral_draws' of (o->seed,
 * first_image_id + image, line, row0).  At k == 0 the noise term is skipped and no Philox block is computed.
 * gates [n_gates], weight [G], rate [n_gates][G] and phase [T] are HOST tables, free when the call returns; they live in buffers of the
 * context and are copied only when they differ from what is there.  Every element of series_dev is written; the inputs are read only.
 * Asynchronous on the context's stream.  MCRT_ERR_INVALID for a null ctx, iq_moving_dev, gates, weight, rate, phase, o or series_dev,
 * zero sizes, options out of range, a weight that is not finite, a |rate| above 65536, a gate with image >= F, line >= E or
 * row0 + G > R, a series_dev that overlaps an input; MCRT_ERR_LIMIT for n_gates > 65535, n_gates * T >= 2^28, a stack of 2^31 samples
 * or more, image ids that pass 2^32; on any error nothing is launched and nothing is written.  Groups: call it on mcrt_group_root(). */
int mcrt_spectral_series_frames(mcrt_ctx *ctx, const float *iq_static_dev /* [F][E][R][2] or NULL */, const float *iq_moving_dev /* [F][E][R][2] */,
                                uint32_t n_frames, uint32_t n_elements, uint32_t n_rows, const mcrt_gate *gates /* [n_gates] */, uint32_t n_gates,
                                const float *weight /* [G] */, const int32_t *rate /* [n_gates][G] */, const int64_t *phase /* [T] */,
                                const mcrt_spectral_opts *o, uint32_t first_image_id, const float *sigma_dev /* [F] or NULL */,
                                float *series_dev /* [n_gates][T][2] */);
/* THE SPECTRA of every gate's series: n_cols = (T - N) / hop + 1 columns of N = o->n_fft bins (a last partial window is dropped).  Per
 * (gate, column c), complex floats throughout:
 * 1. x_n = series[c * hop + n], n < N.  Wall MEAN: x_n = x_n - (the PAIRWISE sum of x) / (float)N per component -- mcrt_flow_frames'
 *    pairwise sum; N is a power of two, so it is a plain tree: what stands still leaves as +0.0f.
 * 2. y_n = (x_n.re * h_n, x_n.im * h_n) with the window h (mcrt_spectral_window's or the caller's own).
 * 3. THE FFT, radix 2, decimation in time: y is permuted by bit reversal (y'[rev(n)] = y[n], rev over log2 N bits), then for the stages
 *    s = 1 .. log2 N with half = 2^(s-1), for every block base b (a multiple of 2 half) and j < half:
 *      w = tw[j * (N >> s)];  u = y[b + j];  v = y[b + j + half];     (mcrt_spectral_twiddles' table)
 *      t = (v.re * w.re - v.im * w.im, v.re * w.im + v.im * w.re);    y[b + j] = u + t;   y[b + j + half] = u - t
 *    The complex multiply is always done, for w = 1 too: NaN and infinities propagate alike everywhere.
 * 4. P_k = X_k.re * X_k.re + X_k.im * X_k.im, in VELOCITY ORDER: out[i] = P[(i + N/2) mod N], so i = N/2 is zero velocity and bin i is
 *    (i - N/2) * 2 v_nyq / N, positive towards the probe.  Bins with |i - N/2| < wall_bins are written as +0.0f.
 * 5. mean = den > 0 ? (num / den) * (float)(2.0 * v_nyq_mm_s / N) : 0.0f, with num = the pairwise sum over i of
 *    out[i] * (float)((int)i - N/2) and den = the pairwise sum of out[i].
 * power_dev [n_gates][n_cols][N] and mean_dev [n_gates][n_cols], each a device pointer or NULL, at least one given; window [N] is a
 * finite HOST table, kept in the context like the tables above.  series_dev is read only.  Asynchronous on the context's stream.
 * MCRT_ERR_INVALID for a null ctx, series_dev, window or o, n_gates == 0, options out of range, T < N, a window entry or a v_nyq_mm_s
 * that is not finite (v_nyq_mm_s > 0), no output, an output that overlaps the series or the other output; MCRT_ERR_LIMIT for
 * n_gates > 65535 or n_gates * T >= 2^28; on any error nothing is launched and nothing is written.  Groups: on mcrt_group_root(). */
int mcrt_spectral_frames(mcrt_ctx *ctx, const float *series_dev /* [n_gates][T][2] */, uint32_t n_gates, const float *window /* [N] */,
                         const mcrt_spectral_opts *o, double v_nyq_mm_s, float *power_dev /* [n_gates][n_cols][N] or NULL */,
                         float *mean_dev /* [n_gates][n_cols] or NULL */);
/* THE SONOGRAM as displayed: a row is a velocity, a column a time, row 0 the highest velocity towards the probe:
 *   out_dev[g][N - 1 - i][c] = byte of p = power_dev[g][c][i],  a NaN or an infinite p counting as 0
 *   ref = o->ref > 0 ? o->ref : the gate's largest finite power (exact and independent of order; 0 when there is none)
 *   v = p > 0 ? ((10.0f * log10f(p / ref) + gain_db) + dynamic_range_db) / dynamic_range_db : 0,  clamped to [0, 1];
 *   byte = (uint8_t)(v * 255.0f + 0.5f)
 * As in mcrt_bmode_frames, the device's log10f is not correctly rounded and may move a level by one.  peak_dev [n_gates] (or NULL)
 * receives each gate's largest finite power (0.0f when there is none), whatever ref is.  Asynchronous on the context's stream.
 * MCRT_ERR_INVALID for a null ctx, power_dev, o or out_dev, zero sizes, an N that is not 32 .. 512 as above, a dynamic_range_db that is
 * not finite and > 0, a gain_db or ref that is not finite, overlapping buffers; MCRT_ERR_LIMIT for n_gates > 65535 or
 * n_gates * n_cols >= 2^28; on any error nothing is launched.  Groups: on mcrt_group_root(). */
typedef struct { float dynamic_range_db; float gain_db; float ref; } mcrt_sonogram_opts;      /* defaults 40, 0, 0; 12 bytes */
int mcrt_default_sonogram_opts(mcrt_sonogram_opts *o);
int mcrt_sonogram_frames(mcrt_ctx *ctx, const float *power_dev /* [n_gates][n_cols][N] */, uint32_t n_gates, uint32_t n_cols, uint32_t n_fft,
                         const mcrt_sonogram_opts *o, float *peak_dev /* [n_gates] or NULL */, uint8_t *out_dev /* [n_gates][N][n_cols] */);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Strain elastography: quasi-static strain imaging compares a scan-line's analytic signal before and after a slight compression by
 * the probe; stiff tissue strains less than soft tissue.  The reference has no counterpart.  THE MODEL is synthesised from ONE traced
 * frame, as the Doppler ensembles are and for the same reason (a second trace has another Philox key and decorrelates completely).
 * COMPRESSION: every scan-line is a column of springs in series under one stress; the caller gives a Young's modulus per material, a
 * row's strain is applied * ref_modulus / modulus[label], the displacement U is the running sum of the strains down the line, and the
 * post-compression line is the pre-compression ANALYTIC line (mcrt_detect_frames' iq_dev) read at q + U(q) by a linear interpolation of
 * its baseband: each of the two neighbouring samples is first turned by the carrier phase of its fractional offset (a plain linear
 * interpolation at 0.3475 cycles per row would lose up to half the amplitude).  Optional receiver noise on the post frame is the only
 * other decorrelation.  TRACKING: per sample the complex cross-correlation of a window of the pre line with the post line at the
 * integer lags -L .. L; the lag of the largest normalised magnitude wins, the sub-sample part is the PHASE of the winning correlation
 * over 2 pi carrier (the phase-sensitive estimator scanners use at low sampling rates), and the strain is the least-squares slope of
 * the displacement over a row window.  Displacements are integers in Q24 rows and phases integers in 2^-32 turn, so the device and any
 * mirror agree whatever the order.  Past about 2 % of strain the estimator degrades, as a real one does (the window decorrelates and at
 * 3 % a search of 16 rows loses lock); the table caps a row's strain at 1/32.
 * LEFT OUT: lateral and elevational motion; stress decay and stress concentration (the model is one-dimensional); a rigid compressor
 * plate (each scan-line takes its own total displacement); guided or multi-level search; lateral averaging of the correlation;
 * shear-wave methods; the strain ratio as a call; elastograms of swept, compounded, elevation-summed or banded frames.
 * An opt-in chain; without it no call and no bit changes.
 *
 * Throughout, every float operation is rounded once: no fma, correctly rounded / and sqrtf, no device transcendental; every sum
 * ascends from 0.0f. */
typedef struct {
    uint32_t window_rows;   /* a, the half-window of the cross-correlation: 0..32; default 16 */
    uint32_t search_rows;   /* L, the largest lag searched: 0..16; default 8 */
    uint32_t lsq_rows;      /* g, the half-window of the least-squares slope: 1..32; default 12 */
    float sigma;            /* the receiver noise per I/Q component of the post frame, finite and >= 0, used when no sigma_dev is given; default 0 */
    uint32_t seed;          /* Philox key word 0 of the noise stream; default 0x5354524E */
} mcrt_strain_opts;         /* 20 bytes */
/* the defaults above.  MCRT_ERR_INVALID for a null o.  Host only. */
int mcrt_default_strain_opts(mcrt_strain_opts *o);
/* the strain of every material in Q24, in double:
 *   eps_q24[l] = modulus[l] == 0 ? 0 : llrint(applied * ref_modulus / modulus[l] * 16777216.0)
 * A modulus of exactly 0 is rigid (strain 0); a negative `applied` is a decompression.  Host only.  MCRT_ERR_INVALID for a null
 * pointer, n_labels == 0, an applied or a modulus that is not finite, a modulus < 0, a ref_modulus that is not finite and > 0, or an
 * |eps_q24[l]| above 2^19 (a strain above 1/32); MCRT_ERR_LIMIT for n_labels > 254; on an error nothing is written. */
int mcrt_strain_table(const double *modulus /* [n_labels] */, uint32_t n_labels, double applied, double ref_modulus, int32_t *eps_q24 /* [n_labels] */);
/* the integer noise draws of one post-compression image, d[e][r][0..1] (I, Q): one Philox4x32-10 block per sample with the counter
 * (e, r, 0x5354524E, 0) and the key (seed, image_id); d_I and d_Q are mcrt_flow_draws' Irwin-Hall sums of o0, o1 and o2, o3, with the
 * same inv_std = (float)(1.0 / sqrt(1431655765.0)).  Counter word 2 differs from the tracer's (< 16), mcrt_noise_frames' (0x4E4F4953),
 * mcrt_flow_frames' (0x464C4F57) and mcrt_spectral_series_frames' (0x53504543).  Host only.  MCRT_ERR_INVALID for a null d or zero
 * sizes; MCRT_ERR_LIMIT for n_rows > 2048. */
int mcrt_strain_draws(uint32_t seed, uint32_t image_id, uint32_t n_elements, uint32_t n_rows, int32_t *d /* [E][R][2] */);
/* the colour table of the elastogram, lut[i] = (r, g, b), i = 128 the reference strain.  kind 0, stiff blue through green to soft red,
 * in integer arithmetic:
 *   i = 0..128:     u = min(255, 2 i);      (0, u, 255 - u)              blue (no strain) to green (the reference strain)
 *   i = 129..255:   u = 2 (i - 128);        (u, 255 - u, 0)              green to red (twice the reference strain)
 * Host only.  MCRT_ERR_INVALID for a null lut or another kind.  (mcrt_colour_map keeps its one kind.) */
int mcrt_strain_map(uint32_t kind, uint8_t *lut /* [256][3] */);
/* THE COMPRESSION.  iq_dev [F][E][R][2] is mcrt_detect_frames' iq_dev, tissue_dev [F][E][R] mcrt_label_frames' labels, eps_q24
 * [n_labels] mcrt_strain_table's (or the caller's own, |eps| <= 2^19), carrier_q32 = llrint(cycles_per_row * 4294967296.0) with
 * cycles_per_row in (0, 0.5] (mcrt_psf_carrier's), lut mcrt_spectral_rotor's table.  With eps(l) = l < n_labels ? eps_q24[l] : 0
 * (MCRT_LABEL_NONE and any label past the table do not strain), per scan-line (f, e) and row q, pre = iq_dev[f][e]:
 *   U[0] = 0;   U[q] = U[q-1] + eps(tissue[q-1])                                   (int32: |U| < 2^30)
 *   s = ((int64)q << 24) + U[q];   s0 = s >> 24 (an arithmetic shift);   fr = s & 0xFFFFFF
 *   A = 0 <= s0 < R ? pre[s0] : (+0.0f, +0.0f);      B = 0 <= s0 + 1 < R ? pre[s0 + 1] : (+0.0f, +0.0f)
 *   w1 = (float)fr * 0x1p-24f (exact);   w0 = 1.0f - w1
 *   th0 = (uint32_t)((carrier_q32 * (int64)fr) >> 24);   th1 = (uint32_t)((carrier_q32 * ((int64)fr - (1 << 24))) >> 24)     (arithmetic shifts)
 *   (c, s) = lut[((th + 0x80000u) >> 20) & 4095];    turn(z, th) = (z.re * c - z.im * s, z.re * s + z.im * c)   (four products, one subtraction, one addition)
 *   post[q] = (w0 * turn(A, th0) + w1 * turn(B, th1)) + k * (float)d[e][q]           per component: two products, their sum, then the noise
 * with k = sigma_f * inv_std, sigma_f = sigma_dev ? sigma_dev[f] : o->sigma, and d mcrt_strain_draws' of (o->seed, first_image_id + f).
 * At k == 0 the noise term is skipped and no Philox block is computed.  With all strains 0 and k == 0, post equals pre wherever pre is
 * finite (fr = 0: the rotor is (1, 0), w1 * B = 0).  The outputs, each a device pointer or NULL, at least one given:
 *   post_iq_dev [F][E][R][2]     the post-compression pairs
 *   truth_disp_dev [F][E][R]     (float)U[q] * 0x1p-24f     the true displacement in rows, positive: the sample is read from deeper down
 *   truth_strain_dev [F][E][R]   (float)eps(tissue[q]) * 0x1p-24f
 * eps_q24 is a HOST table, free when the call returns; it lives in a buffer of the context and is copied only when it differs from
 * what is there (o->window_rows, search_rows and lsq_rows are checked and not read).  Every element of every output given is written;
 * the inputs are read only.  Asynchronous on the context's stream.  MCRT_ERR_INVALID for a null ctx, iq_dev, tissue_dev, eps_q24 or o,
 * zero sizes, n_labels == 0, a cycles_per_row outside (0, 0.5], options out of range, an |eps_q24[l]| above 2^19, no output, an output
 * that overlaps an input or another output; MCRT_ERR_LIMIT for n_rows > 2048, n_labels > 254, a stack of 2^31 samples or more, image
 * ids that pass 2^32; on any error nothing is launched and nothing is written.  Groups: call it on mcrt_group_root(). */
int mcrt_strain_compress_frames(mcrt_ctx *ctx, const float *iq_dev /* [F][E][R][2] */, const uint8_t *tissue_dev /* [F][E][R] */, uint32_t n_frames,
                                uint32_t n_elements, uint32_t n_rows, const int32_t *eps_q24 /* [n_labels] */, uint32_t n_labels, double cycles_per_row,
                                const mcrt_strain_opts *o, uint32_t first_image_id, const float *sigma_dev /* [F] or NULL */,
                                float *post_iq_dev /* [F][E][R][2] or NULL */, float *truth_disp_dev /* [F][E][R] or NULL */,
                                float *truth_strain_dev /* [F][E][R] or NULL */);
/* THE TRACKER.  pre and post are the two stacks of pairs [F][E][R][2], a = o->window_rows, L = o->search_rows, g = o->lsq_rows.  Per
 * scan-line and row r, with the window offsets i = -a .. a ascending and every sum from 0.0f:
 *   e1 = sum over i, row r + i inside [0, R), of (pre[r+i].re * pre[r+i].re + pre[r+i].im * pre[r+i].im)
 *   P[q] = the same sum of post about row q (rows q + i inside [0, R)); the energy at lag k is P[r + k]
 *   c_k = sum over i, rows r + i AND r + i + k inside [0, R), of post[r+i+k] * conj(pre[r+i]):
 *         re += (a * c + b * d),  im += (b * c - a * d)   with post[r+i+k] = (a, b), pre[r+i] = (c, d)   (the products before the sums)
 *   rho2_k = (c_k.re * c_k.re + c_k.im * c_k.im) / (e1 * P[r + k])
 * THE LAG.  The best candidate starts as k = 0; then k = -1, +1, -2, +2, ..., -L, +L are visited in this order, a candidate whose row
 * r + k lies outside [0, R) is skipped, and a candidate replaces the best only when its rho2 is strictly greater.  A NaN never
 * compares greater: it never wins, and a NaN at lag 0 stays (the outputs of such a sample are those of c_0).
 * THE OUTPUTS, each a device pointer or NULL, at least one given, all [F][E][R]:
 *   disp_dev     mcrt_det_atan2f(c_k.im, c_k.re) * (float)(1.0 / (6.283185307179586 * cycles_per_row)) - (float)k       of the best k, in rows;
 *                positive is compression: the U of mcrt_strain_compress_frames
 *   rho_dev      sqrtf(rho2_k), the correlation coefficient of the best k
 *   strain_dev   with j_lo = max(0, r - g), j_hi = min(R - 1, r + g) and t_j = (float)(2 j - (j_lo + j_hi)):
 *                (2.0f * (sum over j = j_lo .. j_hi of t_j * disp[j])) / (sum of t_j * t_j),   +0.0f where j_lo == j_hi
 * A zero window (e1 * P == 0) gives rho NaN and disp from c_0.  Without a disp_dev the displacement lives in a grow-only buffer of the
 * context: nothing is allocated after the first call at a size.  The inputs are read only; every element of every output given is
 * written.  Asynchronous on the context's stream.  MCRT_ERR_INVALID for a null ctx, pre_iq_dev, post_iq_dev or o, zero sizes, options
 * out of range, a cycles_per_row outside (0, 0.5], no output, an output that overlaps an input or another output; MCRT_ERR_LIMIT for
 * n_rows > 2048 or a stack of 2^31 samples or more; on any error nothing is launched and nothing is written.  Groups: on
 * mcrt_group_root(). */
int mcrt_strain_frames(mcrt_ctx *ctx, const float *pre_iq_dev /* [F][E][R][2] */, const float *post_iq_dev /* [F][E][R][2] */, uint32_t n_frames,
                       uint32_t n_elements, uint32_t n_rows, const mcrt_strain_opts *o, double cycles_per_row, float *disp_dev /* [F][E][R] or NULL */,
                       float *rho_dev /* [F][E][R] or NULL */, float *strain_dev /* [F][E][R] or NULL */);
/* THE ELASTOGRAM.  strain_img_dev and rho_img_dev [F][H][W] are mcrt_strain_frames' strain_dev and rho_dev through
 * mcrt_scan_convert_frames, grey_dev [F][H][W] the bytes of mcrt_bmode_frames.  Per pixel, with g the grey byte:
 *   x = strain / ref_strain;   t = rintf(x * 128.0f);   idx = t < 0 ? 0 : t > 255 ? 255 : (int)t
 *   show = x == x && rho >= rho_min && g >= grey_min                                  (a NaN anywhere: not shown)
 *   rgb_dev[f][y][x][ch] = show ? (g * (256 - alpha) + lut[idx][ch] * alpha + 128) >> 8 : g
 * lut [256][3] is HOST memory (mcrt_strain_map's or the caller's own), free when the call returns.  Asynchronous on the context's
 * stream.  MCRT_ERR_INVALID for a null pointer, zero sizes, a ref_strain that is not finite or is 0, a rho_min that is not finite,
 * grey_min > 255, alpha > 256, an rgb_dev that overlaps an input; MCRT_ERR_LIMIT for 2^31 pixels or more; on any error nothing is
 * launched.  Groups: call it on mcrt_group_root(). */
typedef struct {
    float ref_strain;       /* the strain shown as the table's middle (green), finite and not 0; default 0.01 */
    float rho_min;          /* pixels with a smaller correlation coefficient stay grey; default 0.7 */
    uint32_t grey_min;      /* pixels with a darker B-mode byte stay grey: 0..255; default 0 */
    uint32_t alpha;         /* the colour's share in 1/256: 0..256; default 160 */
} mcrt_elastogram_opts;     /* 16 bytes */
int mcrt_default_elastogram_opts(mcrt_elastogram_opts *o);
int mcrt_elastogram_frames(mcrt_ctx *ctx, const float *strain_img_dev /* [F][H][W] */, const float *rho_img_dev /* [F][H][W] */,
                           const uint8_t *grey_dev /* [F][H][W] */, uint32_t n_frames, uint32_t height, uint32_t width, const uint8_t *lut /* [256][3] */,
                           const mcrt_elastogram_opts *o, uint8_t *rgb_dev /* [F][H][W][3] */);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Shear-wave elastography: the quantitative mode.  A radiation-force push on one scan-line launches a shear wave sideways, the
 * scanner tracks the tissue's axial displacement at a few kHz, and the wave's local speed c gives the stiffness, E = 3 rho c^2.  The
 * reference has no counterpart.  THE MODEL is one-dimensional and lateral, as the strain model is one-dimensional and axial, and is
 * synthesised from ONE traced frame, as the Doppler ensembles and the compression are and for the same reason (a second trace has
 * another Philox key and decorrelates completely).  A push on scan-line push_line over the rows [row0, row1) starts a wave that
 * leaves that line in both directions and travels along each RF row on its own; each material has a shear speed, and a speed of
 * exactly 0 is a fluid: the wave does not pass, and nothing behind it ever arrives.  TRACKING: pulse n's analytic line is the pre line
 * read at q + u(n) by mcrt_strain_compress_frames' interpolation; the displacement estimate is the phase of the lag-0 correlation of a
 * window of that line with the pre line (the displacements are a small fraction of a row: no lag search); a sample's arrival is its
 * time to peak, refined by a parabola through the maximum and its neighbours; the speed is the pitch over the least-squares slope of
 * the time to peak across scan-lines.  Arrival times and displacements are integers, so the device and any mirror agree whatever
 * the order of the sums.
 * LEFT OUT: reflection and refraction of the shear wave; dispersion and viscosity; axial propagation and the push's real beam shape;
 * multiple pushes and directional filtering; time-profile cross-correlation in place of time to peak; Voigt or other models.
 * An opt-in chain; without it no call and no bit changes.
 *
 * Throughout, every float operation is rounded once: no fma, correctly rounded / and sqrtf, no device transcendental; every sum
 * ascends from 0.0f.
 *
 * THE INTEGERS.  A tick is 2^-16 of a tracking pulse interval.  NEVER = 2^40 ticks.
 *   slow_q16[l]  = llrint(65536.0 * 65536.0 * prf_hz / (speed_m_s[l] * 1e6))      ticks per um in Q16; 0 for a speed of exactly 0 (a fluid)
 *   pitch_q8[r]  = llrint(256.0 * pitch_um(r)),  pitch_um(r) = 1000 (radius_mm + r depth_mm / R) total_angle / E: the arc between
 *                  neighbouring scan-lines at the depth of row r.  THE CONVENTION is mcrt_scan_maps': E scan-lines share the total
 *                  angle, neighbours are total_angle / E apart (its column coordinate is (angle + total_angle / 2) / total_angle * E), row
 *                  r lies r depth_mm / R below the arc, depth_mm = max_travel_us * speed_of_sound * 0.001.
 *   cost(l, r)   = l < n_labels && slow_q16[l] != 0 ? (slow_q16[l] * (int64)pitch_q8[r]) >> 24 : NEVER       (MCRT_LABEL_NONE, a label
 *                  past the table and a fluid block the crossing; slow_q16 <= 2^38 and pitch_q8 < 2^24: the product is below 2^62)
 *   A[p][r] = 0 on the push line p;  A[e][r] = min(NEVER, A[e-1][r] + cost(tissue[e-1][r], r)) for e > p,
 *                                    A[e][r] = min(NEVER, A[e+1][r] + cost(tissue[e+1][r], r)) for e < p:
 *                  a crossing costs what the tissue it LEAVES costs, as the strain sum takes the row it leaves.  Saturating sums of
 *                  non-negative terms: the order is free, and A == NEVER means "never".
 *   pa(e)        = ((int64)peak_q24 * amp(|e - p|)) >> 16,   amp(d) = d < n_amp ? amp_q16[d] : 0                (arithmetic shifts)
 *   t            = ((int64)n << 16) - A[e][r];    idx = t >> 10          (the shape table's step is 1/64 pulse)
 *   u(e, r, n)   = row0 <= r < row1 && A[e][r] < NEVER && t >= 0 && idx < n_shape ? (pa(e) * (int64)shape_q16[idx]) >> 16 : 0
 *                  the particle displacement in Q24 rows, |u| <= 2^23 (|peak_q24| <= 2^23, table entries <= 65536); positive reads deeper
 * row0 = push_row0, row1 = push_rows ? push_row0 + push_rows : R. */
typedef struct {
    uint32_t n_pulses;      /* T, the tracking pulses: 4..256; default 64 */
    uint32_t window_rows;   /* a, the half-window of the correlation: 0..16; default 8 */
    float prf_hz;           /* the tracking pulse rate, finite and > 0; default 10000 (the speed call's scale; the table has its own) */
    float sigma;            /* the receiver noise per I/Q component of every tracking line, finite and >= 0, used when no sigma_dev is given; default 0 */
    uint32_t seed;          /* Philox key word 0 of the noise stream; default 0x53484552 */
    uint32_t push_line;     /* p, the pushed scan-line, < n_elements; default 0 */
    uint32_t push_row0;     /* the first pushed row, < n_rows; default 0 */
    uint32_t push_rows;     /* the pushed rows; 0: to the end of the line; push_row0 + push_rows <= n_rows; default 0 */
    int32_t peak_q24;       /* the peak displacement on the push line in Q24 rows, |peak_q24| <= 2^23; default 1677722 (0.1 row) */
    uint32_t speed_lines;   /* b, the half-window of the slope across scan-lines: 1..16; default 4 */
    uint32_t avg_rows;      /* the peak times are averaged over +- avg_rows rows before the fit: 0..16; default 2 */
    float density;          /* g/cm^3, finite and > 0: modulus [kPa] = 3 density speed^2; default 1 */
} mcrt_shear_opts;          /* 48 bytes */
/* the defaults above.  MCRT_ERR_INVALID for a null o.  Host only. */
int mcrt_default_shear_opts(mcrt_shear_opts *o);
/* slow_q16 (above, in double) and speed_f[l] = (float)speed_m_s[l], the truth table.  Host only.  MCRT_ERR_INVALID for a null pointer,
 * n_labels == 0, a prf_hz that is not finite and > 0, a speed that is not finite or is < 0, or a slow_q16[l] of a speed > 0 outside
 * [1, 2^38]; MCRT_ERR_LIMIT for n_labels > 254; on an error nothing is written. */
int mcrt_shear_table(const double *speed_m_s /* [n_labels] */, uint32_t n_labels, double prf_hz, int64_t *slow_q16 /* [n_labels] */,
                     float *speed_f /* [n_labels] */);
/* pitch_q8 (above, in double) and pitch_mm[r] = (float)(pitch_um(r) * 0.001), each [n_rows] or NULL, at least one given.  Host only.
 * MCRT_ERR_INVALID for both null, zero sizes, a radius_mm that is not finite or is < 0, a total_angle_rad that is not finite and > 0,
 * max_travel_us * speed_of_sound == 0; MCRT_ERR_LIMIT for n_rows > 2048 or a pitch_q8 of 0 or >= 2^24; on an error nothing is written. */
int mcrt_shear_pitch(uint32_t n_elements, uint32_t n_rows, double radius_mm, double total_angle_rad, uint32_t max_travel_us, uint32_t speed_of_sound,
                     uint32_t *pitch_q8 /* [n_rows] or NULL */, float *pitch_mm /* [n_rows] or NULL */);
/* the default time profile, a raised cosine of width_pulses, n_shape = 64 width_pulses entries, in double:
 *   shape_q16[i] = llrint(65536.0 * (0.5 - 0.5 * cos(6.283185307179586 * (i + 0.5) / n_shape)))
 * Host only.  MCRT_ERR_INVALID for a null table or width_pulses == 0; MCRT_ERR_LIMIT for width_pulses > 256. */
int mcrt_shear_shape(uint32_t width_pulses, uint32_t *shape_q16 /* [64 * width_pulses] */);
/* the default geometric decay over line distance, in double: amp_q16[d] = llrint(65536.0 / sqrt(1.0 + d / d0_lines)).  Host only.
 * MCRT_ERR_INVALID for a null table, n == 0 or a d0_lines that is not finite and > 0. */
int mcrt_shear_decay(uint32_t n, double d0_lines, uint32_t *amp_q16 /* [n] */);
/* the integer noise draws of tracking pulse `pulse` of one image, d[e][r][0..1] (I, Q): one Philox4x32-10 block per sample with the
 * counter (e, r, 0x53484552, pulse) and the key (seed, image_id); mcrt_flow_draws' Irwin-Hall sums and inv_std.  Counter word 2 differs
 * from the tracer's (< 16), mcrt_noise_frames' (0x4E4F4953), mcrt_flow_frames' (0x464C4F57), mcrt_spectral_series_frames' (0x53504543)
 * and mcrt_strain_compress_frames' (0x5354524E).  Host only.  MCRT_ERR_INVALID for a null d or zero sizes; MCRT_ERR_LIMIT for
 * n_rows > 2048 or pulse >= 256. */
int mcrt_shear_draws(uint32_t seed, uint32_t image_id, uint32_t n_elements, uint32_t n_rows, uint32_t pulse, int32_t *d /* [E][R][2] */);
/* the colour table of the shear-wave elastogram, lut[i] = (r, g, b), i = 128 the reference modulus.  kind 0, SOFT blue through green to
 * STIFF red, the convention of shear-wave displays and the opposite of mcrt_strain_map's reading, in integer arithmetic:
 *   i = 0..128:     u = min(255, 2 i);      (0, u, 255 - u)              blue (no stiffness) to green (the reference modulus)
 *   i = 129..255:   u = 2 (i - 128);        (u, 255 - u, 0)              green to red (twice the reference modulus)
 * mcrt_elastogram_frames shows it as it is: the gathered modulus for strain_img_dev, the gathered quality for rho_img_dev, ref_strain =
 * the reference kPa.  Host only.  MCRT_ERR_INVALID for a null lut or another kind. */
int mcrt_shear_map(uint32_t kind, uint8_t *lut /* [256][3] */);
/* THE WAVE AND THE TRACKER.  iq_dev [F][E][R][2] is mcrt_detect_frames' iq_dev, tissue_dev [F][E][R] mcrt_label_frames' labels; slow_q16,
 * speed_f, pitch_q8, shape_q16 and amp_q16 are HOST tables (the helpers' or the caller's own within the helpers' ranges), free when the
 * call returns: they live in buffers of the context and are copied only when they differ from what is there.  T = o->n_pulses, a =
 * o->window_rows.  Per frame f, scan-line e, row r and pulse n = 0 .. T-1, with pre = iq_dev[f][e]:
 *   z_n[q]  = warp(pre, q, u(e, q, n)) + k * (float)d_n[e][q]            warp: mcrt_strain_compress_frames' post[q] with U[q] = u (s0, fr, w0, w1,
 *             th0, th1 and the rotor lookup are its own); k = sigma_f * inv_std, sigma_f = sigma_dev ? sigma_dev[f] : o->sigma, d_n
 *             mcrt_shear_draws' of (o->seed, first_image_id + f, n); at k == 0 the noise term is skipped and no block is computed
 *   c_n     = sum over i = -a .. a ascending, rows r + i inside [0, R), of z_n[r+i] * conj(pre[r+i]):
 *             re += (a * c + b * d),  im += (b * c - a * d)   with z_n[r+i] = (a, b), pre[r+i] = (c, d)   (the products before the sums)
 *   d_n     = mcrt_det_atan2f(c_n.im, c_n.re) * (float)(1.0 / (6.283185307179586 * cycles_per_row))          the displacement estimate, rows
 * THE PEAK.  The best pulse starts as n = 0; a later pulse replaces it only when its d_n is strictly greater: the first maximum wins, a
 * NaN never wins, and a NaN at n = 0 stays.  With m the best pulse and (um, u0, up) = (d_{m-1}, d_m, d_{m+1}):
 * THE OUTPUTS, each a device pointer or NULL, at least one given:
 *   peak_time_dev [F][E][R]      (float)m + (0.5f * (um - up)) / ((um - 2.0f * u0) + up);  NaN where m == 0, m == T-1 or the denominator is 0
 *   peak_disp_dev [F][E][R]      u0
 *   disp_dev [F][T][E][R]        d_n, the movie
 *   truth_arrival_dev [F][E][R]  (float)A[e][r] * 0x1p-16f, in pulses;  +inf where A == NEVER
 *   truth_speed_dev [F][E][R]    speed_f[tissue[e][r]];  +0.0f for MCRT_LABEL_NONE and a label past the table
 * With peak_q24 == 0 and k == 0 every d_n is +0.0f wherever pre is finite and not zero, as pulse n's line is pre (the zero-strain
 * identity).  A lives in a grow-only buffer of the context: nothing is allocated after the first call at a size.  The inputs are read
 * only; every element of every output given is written.  Asynchronous on the context's stream.  MCRT_ERR_INVALID for a null ctx, iq_dev,
 * tissue_dev, table or o, zero sizes, n_labels, n_shape or n_amp == 0, a cycles_per_row outside (0, 0.5], options out of range (n_pulses,
 * window_rows, prf_hz, sigma, |peak_q24|, push_line >= n_elements, push_row0 >= n_rows, push_row0 + push_rows > n_rows, speed_lines,
 * avg_rows, density), a slow_q16[l] outside [0, 2^38], a pitch_q8[r] of 0 or >= 2^24, a shape_q16 or amp_q16 entry above 65536, no
 * output, an output that overlaps an input or another output; MCRT_ERR_LIMIT for n_rows > 2048, n_labels > 254, n_shape > 16384, n_amp >
 * 65536, a stack or a movie of 2^31 samples or more, image ids that pass 2^32; on any error nothing is launched and nothing is written.
 * Groups: call it on mcrt_group_root(). */
int mcrt_shear_wave_frames(mcrt_ctx *ctx, const float *iq_dev /* [F][E][R][2] */, const uint8_t *tissue_dev /* [F][E][R] */, uint32_t n_frames,
                           uint32_t n_elements, uint32_t n_rows, const int64_t *slow_q16 /* [n_labels] */, const float *speed_f /* [n_labels] */,
                           uint32_t n_labels, const uint32_t *pitch_q8 /* [R] */, const uint32_t *shape_q16 /* [n_shape] */, uint32_t n_shape,
                           const uint32_t *amp_q16 /* [n_amp] */, uint32_t n_amp, double cycles_per_row, const mcrt_shear_opts *o,
                           uint32_t first_image_id, const float *sigma_dev /* [F] or NULL */, float *peak_time_dev /* [F][E][R] or NULL */,
                           float *peak_disp_dev /* [F][E][R] or NULL */, float *disp_dev /* [F][T][E][R] or NULL */,
                           float *truth_arrival_dev /* [F][E][R] or NULL */, float *truth_speed_dev /* [F][E][R] or NULL */);
/* THE SPEED.  peak_time_dev [F][E][R] is mcrt_shear_wave_frames'; pitch_mm [R] is a HOST table (mcrt_shear_pitch's), kept as the others
 * are.  b = o->speed_lines, v = o->avg_rows, p = o->push_line, kf = (float)((double)o->prf_hz * 0.001), d3 = 3.0f * o->density.  Per
 * sample (e, r) the window of lines j = e - b .. e + b is NOT clipped: where e - b < 0, e + b >= E or e - b <= p <= e + b the sample is
 * not valid.  Otherwise, with the rows i = max(0, r - v) .. min(R - 1, r + v) ascending:
 *   y_j   = (sum of peak_time[j][i] over the rows where it is not NaN) / (float)(their count);  no such row: the sample is not valid
 *   t_j   = (float)(2 j - 2 e);   den = sum of t_j * t_j;   mean = (sum of y_j) / (float)(2 b + 1)                (j ascending)
 *   num   = sum of t_j * y_j;     syy = sum of (y_j - mean) * (y_j - mean)
 *   slope = (2.0f * num) / den, negated where e < p: pulses per scan-line, signed away from the push; not > 0: the sample is not valid
 *   r2    = (num * num) / (den * syy)
 * THE OUTPUTS, each a device pointer or NULL, at least one given, all [F][E][R]:
 *   speed_dev     (pitch_mm[r] * kf) / slope, in m/s;                NaN where the sample is not valid
 *   modulus_dev   d3 * (speed * speed), in kPa;                      NaN where the sample is not valid
 *   quality_dev   r2 > 1 ? 1 : r2 >= 0 ? r2 : +0.0f  (a NaN: 0);     +0.0f where the sample is not valid
 * The input is read only; every element of every output given is written.  Asynchronous on the context's stream.  MCRT_ERR_INVALID
 * for a null ctx, peak_time_dev, pitch_mm or o, zero sizes, options out of range (mcrt_shear_wave_frames' list), a pitch_mm[r] that is
 * not finite and > 0, no output, an output that overlaps the input or another output; MCRT_ERR_LIMIT for n_rows > 2048 or a stack of
 * 2^31 samples or more; on any error nothing is launched and nothing is written.  Groups: on mcrt_group_root(). */
int mcrt_shear_speed_frames(mcrt_ctx *ctx, const float *peak_time_dev /* [F][E][R] */, uint32_t n_frames, uint32_t n_elements, uint32_t n_rows,
                            const float *pitch_mm /* [R] */, const mcrt_shear_opts *o, float *speed_dev /* [F][E][R] or NULL */,
                            float *modulus_dev /* [F][E][R] or NULL */, float *quality_dev /* [F][E][R] or NULL */);

/* ---------------------------------------------------------------------------------------------------------------------------
 * M-mode: one scan-line fired at the pulse repetition rate, depth down the picture, time across it -- the mode that measures wall
 * motion, vessel distension and the fetal heart rate.  The reference has no counterpart.  THE MODEL is strain's column of springs with
 * a time axis, anchored at the probe face, and is synthesised from ONE traced frame, as the Doppler ensembles, the compression and the
 * shear wave are and for the same reason (a second trace has another Philox key and decorrelates completely).  Each material has a
 * DILATION dil_q24[l], the peak axial strain of that material over the cycle in Q24, with mcrt_strain_compress_frames' sign: positive
 * is compression, so a lumen that widens in systole has a negative one.  A waveform w_q16[t] in [-65536, 65536] (the heart beat, a
 * palpation) scales the column's displacement at pulse t, and bulk_q24[t] (|bulk| <= 32 rows) shifts the whole line rigidly (breathing,
 * a probe that slips).  Pulse t's analytic line is the pre line read at q + U(q, t) by mcrt_strain_compress_frames' interpolation, plus
 * optional receiver noise; its envelope is the M-line.  The display sweeps the M-lines across the picture: a column is a time, a row a
 * depth.
 * LEFT OUT: lateral and elevational motion; motion that differs between scan-lines; speckle decorrelation other than receiver noise;
 * anatomical (oblique) M-mode; colour M-mode; tissue Doppler as a call (iq_out_dev has the moving analytic lines for it); more than one
 * waveform per call; M-mode of swept, compounded, elevation-summed or banded frames.
 * An opt-in chain; without it no call and no bit changes.
 *
 * Throughout, every float operation is rounded once: no fma, correctly rounded / and sqrtf, no device transcendental except the one
 * log10f of the display; every sum ascends from 0.0f.
 *
 * THE INTEGERS.  Per M-line (image f, scan-line e), row q and pulse t, with tissue = tissue_dev[f][e] and
 * dil(l) = l < n_labels ? dil_q24[l] : 0 (MCRT_LABEL_NONE and any label past the table do not move):
 *   D[0] = 0;   D[q] = D[q-1] + dil(tissue[q-1])                                       (int64: |D| <= 2048 * 2^22 = 2^33; the order is free)
 *   u64    = ((D[q] * (int64)w_q16[t]) >> 16) + (int64)bulk_q24[t]                     (an arithmetic shift; |u64| < 2^34)
 *   U(q,t) = u64 < -(127 << 24) ? -(127 << 24) : u64 > (127 << 24) ? (127 << 24) : u64     a displacement past 127 rows saturates there
 * in Q24 rows; positive reads deeper down, as the U of mcrt_strain_compress_frames does. */
typedef struct { uint32_t image, line; } mcrt_mline;      /* an M-line: scan-line `line` of image `image` of the stack; 8 bytes */
typedef struct {
    uint32_t n_pulses;      /* T, the pulses of every M-line: 1..16384; default 1024 */
    float sigma;            /* the receiver noise per I/Q component of every pulse, finite and >= 0, used when no sigma_dev is given; default 0 */
    uint32_t seed;          /* Philox key word 0 of the noise stream; default 0x4D4D4F44 */
} mcrt_mmode_opts;          /* 12 bytes */
/* the defaults above.  MCRT_ERR_INVALID for a null o.  Host only. */
int mcrt_default_mmode_opts(mcrt_mmode_opts *o);
/* the dilation of every material in Q24, in double: dil_q24[l] = llrint(dilation[l] * 16777216.0).  Host only.  MCRT_ERR_INVALID for a
 * null pointer, n_labels == 0, a dilation that is not finite, or a |dil_q24[l]| above 2^22 (a dilation above 25 %); MCRT_ERR_LIMIT for
 * n_labels > 254; on an error nothing is written. */
int mcrt_mmode_table(const double *dilation /* [n_labels] */, uint32_t n_labels, int32_t *dil_q24 /* [n_labels] */);
/* a default waveform, a convenience, not physiology: mcrt_pulse_waveform's systolic half-sine squared over the first 30 % of every
 * cycle, in double, per pulse t:
 *   u = t * beats_per_min / (60.0 * prf_hz);   x = u - floor(u);   s = sin(3.141592653589793 * x / 0.3)
 *   w_q16[t] = llrint(65536.0 * (x < 0.3 ? s * s : 0.0))
 * Host only.  MCRT_ERR_INVALID for a null table, n_pulses == 0, a prf_hz or beats_per_min that is not finite and > 0; MCRT_ERR_LIMIT for
 * n_pulses > 16384; on an error nothing is written. */
int mcrt_mmode_waveform(double prf_hz, double beats_per_min, uint32_t n_pulses, int32_t *w_q16 /* [n_pulses] */);
/* a default bulk motion, a sinusoid of amplitude_rows rows at cycles_per_min, in double, per pulse t:
 *   bulk_q24[t] = llrint(amplitude_rows * 16777216.0 * sin(6.283185307179586 * t * cycles_per_min / (60.0 * prf_hz)))
 * Host only.  MCRT_ERR_INVALID for a null table, n_pulses == 0, a prf_hz that is not finite and > 0, a cycles_per_min or amplitude_rows
 * that is not finite, or an |amplitude_rows| above 32; MCRT_ERR_LIMIT for n_pulses > 16384; on an error nothing is written. */
int mcrt_mmode_bulk(double prf_hz, double cycles_per_min, double amplitude_rows, uint32_t n_pulses, int32_t *bulk_q24 /* [n_pulses] */);
/* the integer noise draws of one M-line, d[t][r][0..1] (I, Q): one Philox4x32-10 block per (line, row, pulse) with the counter
 * (line, r, 0x4D4D4F44, t) and the key (seed, image_id); mcrt_flow_draws' Irwin-Hall sums and inv_std.  Counter word 2 differs from the
 * tracer's (< 16), mcrt_noise_frames' (0x4E4F4953), mcrt_flow_frames' (0x464C4F57), mcrt_spectral_series_frames' (0x53504543),
 * mcrt_strain_compress_frames' (0x5354524E) and mcrt_shear_wave_frames' (0x53484552).  Host only.  MCRT_ERR_INVALID for a null d or
 * zero sizes; MCRT_ERR_LIMIT for n_rows > 2048 or n_pulses > 16384. */
int mcrt_mmode_draws(uint32_t seed, uint32_t image_id, uint32_t line, uint32_t n_rows, uint32_t n_pulses, int32_t *d /* [T][R][2] */);
/* THE M-LINES.  iq_dev [F][E][R][2] is mcrt_detect_frames' iq_dev, tissue_dev [F][E][R] mcrt_label_frames' labels; lines [n_lines],
 * dil_q24 [n_labels] (mcrt_mmode_table's or the caller's own, |dil| <= 2^22), w_q16 [T] (|w| <= 65536) and bulk_q24 [T]
 * (|bulk| <= 32 << 24) are HOST tables, free when the call returns: they live in buffers of the context and are copied only when they
 * differ from what is there.  T = o->n_pulses, carrier_q32 = llrint(cycles_per_row * 4294967296.0) with cycles_per_row in (0, 0.5]
 * (mcrt_psf_carrier's), lut mcrt_spectral_rotor's table.  Per M-line j = (f, e), pulse t and row q, with pre = iq_dev[f][e] and U(q,t)
 * of THE INTEGERS:
 *   z(q,t)   = warp(pre, q, U(q,t)) + k * (float)d[t][q]      warp: mcrt_strain_compress_frames' post[q] with U[q] = U(q,t) (s0, fr, w0, w1,
 *              th0, th1 and the rotor lookup are its own: s0 = q + (U >> 24), fr = U & 0xFFFFFF); k = sigma_f * inv_std, sigma_f =
 *              sigma_dev ? sigma_dev[f] : o->sigma, d mcrt_mmode_draws' of (o->seed, first_image_id + f, e); at k == 0 the noise term is
 *              skipped and no Philox block is computed
 *   env(q,t) = sqrtf(z.re * z.re + z.im * z.im)                (two products, their sum, the root)
 * THE OUTPUTS, each a device pointer or NULL, at least one given:
 *   env_dev [n_lines][T][R]           env(q,t), the M-line of every pulse
 *   iq_out_dev [n_lines][T][R][2]     z(q,t), the moving analytic lines
 *   truth_disp_dev [n_lines][T][R]    (float)U(q,t) * 0x1p-24f      the true displacement in rows, positive: the sample is read from deeper down
 *   truth_label_dev [n_lines][T][R]   (uint8) the material of the sample each output shows: tissue[sr] with sr = s0 + (fr >> 23), the
 *                                     nearer of the two samples read; MCRT_LABEL_NONE where sr is outside [0, R)
 * With all dilations 0, every bulk 0 and k == 0, env(q,t) is sqrtf(re * re + im * im) of the pre line for every t wherever pre is
 * finite (the zero-strain identity); a bulk of k << 24 shows the pre line k rows further down, zeros beyond its ends.  The same line
 * may be named more than once.  The inputs are read only; every element of every output given is written.  Nothing is allocated after
 * the first call at a size.  Asynchronous on the context's stream.  MCRT_ERR_INVALID for a null ctx, iq_dev, tissue_dev, table or o,
 * zero sizes, n_labels == 0, n_lines == 0, a cycles_per_row outside (0, 0.5], options out of range (n_pulses, sigma), a line with
 * image >= n_frames or line >= n_elements, a |dil_q24[l]| above 2^22, a |w_q16[t]| above 65536, a |bulk_q24[t]| above 32 << 24, no
 * output, an output that overlaps an input or another output; MCRT_ERR_LIMIT for n_rows > 2048, n_labels > 254, n_lines > 65535, a
 * stack of 2^31 samples or more, n_lines * T * n_rows >= 2^31, image ids that pass 2^32; on any error nothing is launched and nothing
 * is written.  Groups: call it on mcrt_group_root(). */
int mcrt_mmode_lines_frames(mcrt_ctx *ctx, const float *iq_dev /* [F][E][R][2] */, const uint8_t *tissue_dev /* [F][E][R] */, uint32_t n_frames,
                            uint32_t n_elements, uint32_t n_rows, const mcrt_mline *lines /* [n_lines] */, uint32_t n_lines,
                            const int32_t *dil_q24 /* [n_labels] */, uint32_t n_labels, const int32_t *w_q16 /* [T] */, const int32_t *bulk_q24 /* [T] */,
                            double cycles_per_row, const mcrt_mmode_opts *o, uint32_t first_image_id, const float *sigma_dev /* [F] or NULL */,
                            float *env_dev /* [n_lines][T][R] or NULL */, float *iq_out_dev /* [n_lines][T][R][2] or NULL */,
                            float *truth_disp_dev /* [n_lines][T][R] or NULL */, uint8_t *truth_label_dev /* [n_lines][T][R] or NULL */);
typedef struct {
    uint32_t hop;               /* pulses per picture column, >= 1; default 4 */
    uint32_t height;            /* H, the picture's rows: 1..4096; default 400 */
    uint32_t row_lo, row_hi;    /* the rows [row_lo, row_hi) of the line that are shown; row_hi 0: n_rows; defaults 0, 0 */
    float dynamic_range_db;     /* finite and > 0; default 60 */
    float gain_db;              /* finite; default 0 */
    float ref;                  /* finite; > 0: the amplitude shown as 0 dB; otherwise each line's own peak; default 0 */
} mcrt_mmode_display_opts;      /* 28 bytes */
/* the defaults above.  MCRT_ERR_INVALID for a null o.  Host only. */
int mcrt_default_mmode_display_opts(mcrt_mmode_display_opts *o);
/* the depth resampling table of the sweep, H picture rows over the line's rows [row_lo, row_hi) (row_hi spelled out), in double, per
 * picture row y:
 *   p = row_lo + (y + 0.5) * (row_hi - row_lo) / H - 0.5;   f = floor(p)
 *   idx[y] = f < row_lo ? row_lo : f > row_hi - 1 ? row_hi - 1 : f                     the first tap i0; the second is min(i0 + 1, row_hi - 1)
 *   wt[y]  = f clamped either way ? 0.0f : min(1.0f, max(0.0f, (float)(p - f)))        the second tap's weight
 * Host only.  MCRT_ERR_INVALID for a null table, H == 0 or H > 4096, row_lo >= row_hi; MCRT_ERR_LIMIT for row_hi > 2048; on an error
 * nothing is written. */
int mcrt_mmode_rows(uint32_t row_lo, uint32_t row_hi, uint32_t height, uint32_t *idx /* [H] */, float *wt /* [H] */);
/* THE SWEEP as displayed.  env_dev [n_lines][T][R] is mcrt_mmode_lines_frames'; W = T / o->hop columns (a last partial column is
 * dropped), H = o->height rows, the shown rows [row_lo, row_hi) with row_hi = o->row_hi ? o->row_hi : R, and (idx, wt) mcrt_mmode_rows'
 * table of them (made by the call, kept in the context as the other tables are).  Per line j, column c and row r, with DR =
 * o->dynamic_range_db:
 *   a[c][r] = (sum over k = 0 .. hop-1 ascending, from 0.0f, of env[j][c * hop + k][r]) / (float)hop
 *   a NaN or an infinite a counts as 0;   peak = the largest a that counts over all columns and the shown rows (exact, whatever the
 *   order; 0 when there is none);   ref = o->ref > 0 ? o->ref : peak
 *   g[c][r] = a > 0 ? min(1, max(0, ((20.0f * log10f(a / ref) + o->gain_db) + DR) / DR)) : 0      compression before interpolation, as in mcrt_bmode_frames
 *   v = (1.0f - wt[y]) * g[c][i0] + wt[y] * g[c][i1],   i0 = idx[y], i1 = min(i0 + 1, row_hi - 1)
 *   out_dev[j][y][c] = (uint8_t)(v * 255.0f + 0.5f)
 * The optional outputs, each a device pointer or NULL:
 *   peak_dev [n_lines]            peak, whatever ref is
 *   mean_dev [n_lines][W][R]      a[c][r] of EVERY row, before the NaN rule (the float a test can hold bit for bit)
 *   label_out_dev [n_lines][H][W] truth_label_dev[j][c * hop][rn], rn = min(i0 + (wt[y] >= 0.5f), row_hi - 1): pulse c * hop at the
 *                                 nearest shown row, registered with out_dev pixel for pixel; needs truth_label_dev [n_lines][T][R]
 *   disp_out_dev [n_lines][H][W]  truth_disp_dev[j][c * hop][rn] likewise; needs truth_disp_dev [n_lines][T][R]
 * The inputs are read only; every element of every output given is written.  Without a peak_dev the peaks live in a grow-only buffer
 * of the context: nothing is allocated after the first call at a size.  Asynchronous on the context's stream.  MCRT_ERR_INVALID for a
 * null ctx, env_dev, o or out_dev, zero sizes, hop == 0, W == 0 (hop > T), height outside 1..4096, row_lo >= row_hi or row_hi > R,
 * a dynamic_range_db that is not finite and > 0, a gain_db or ref that is not finite, a label_out_dev without truth_label_dev or a
 * disp_out_dev without truth_disp_dev, an output that overlaps an input or another output; MCRT_ERR_LIMIT for n_rows > 2048,
 * n_pulses > 16384, n_lines > 65535, n_lines * T * R >= 2^31 or n_lines * H * W >= 2^31; on any error nothing is launched and nothing
 * is written.  Groups: on mcrt_group_root(). */
int mcrt_mmode_picture_frames(mcrt_ctx *ctx, const float *env_dev /* [n_lines][T][R] */, const uint8_t *truth_label_dev /* [n_lines][T][R] or NULL */,
                              const float *truth_disp_dev /* [n_lines][T][R] or NULL */, uint32_t n_lines, uint32_t n_pulses, uint32_t n_rows,
                              const mcrt_mmode_display_opts *o, float *peak_dev /* [n_lines] or NULL */, float *mean_dev /* [n_lines][W][R] or NULL */,
                              uint8_t *out_dev /* [n_lines][H][W] */, uint8_t *label_out_dev /* [n_lines][H][W] or NULL */,
                              float *disp_out_dev /* [n_lines][H][W] or NULL */);

/* device [E][R]  ->  host [R][E] row-major (the cv::Mat layout of rfimage.h:217); synchronous */
int mcrt_export_rf(mcrt_ctx *ctx, const float *rf_dev, uint32_t n_elements, uint32_t n_rows, float *host_rows_by_cols);

/* host [R][E] row-major (the cv::Mat layout)  ->  device [E][R]: the inverse of mcrt_export_rf, for callers that deposit
 * echoes on the host (rf_image::add_echo, rfimage.h:33-40) and post-process on the GPU; synchronous */
int mcrt_import_rf(mcrt_ctx *ctx, const float *host_rows_by_cols, uint32_t n_elements, uint32_t n_rows, float *rf_dev);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Several GPUs of one node behind the same calls (the reference's frame loop main.cpp:92-152 is one GPU-less thread).
 * Paths are independent and deposit only into their own scan-line's column (main.cpp:128,139 use ray_i as the column), so the
 * scan-lines are cut into contiguous shards -- rank g of G traces [g*E/G, (g+1)*E/G), the first E % G ranks one more -- with scene,
 * texture and transducer replicated; every rank's [F][E_g][R] block then crosses xGMI once (hipMemcpyPeerAsync on the rank's own copy
 * stream) into GPU devices[0], where one kernel lays the blocks out as the [F][E][R] frames a single context would have produced, bit
 * for bit (RF bins are integer sums: no partition changes them).  PSF, envelope and scan conversion need neighbouring columns
 * (rfimage.h:113-118) and run on the gathered frames: call mcrt_convolve_frames (or mcrt_convolve_frames_depth) / mcrt_envelope_frames / mcrt_scan_convert_frames, or
 * mcrt_bmode_frames for the 8-bit display, on mcrt_group_root() -- no group call of their own is needed.
 * A group owns one tracing context per listed device (each driven by its own host thread, so G GPUs are fed in parallel) and a root
 * context on devices[0] for the gathered frames.  A device may be listed more than once: its contexts then share that GPU (how the
 * one-GPU test box runs a two-rank group).  Passes are DOUBLE-BUFFERED: mcrt_group_trace_frames returns once everything is enqueued,
 * the ranks' next pass does not wait for the root's stream, so post-processing pass k on the root overlaps the trace of pass k+1
 * (alternate two rf_dev buffers to use it).  Errors: the first failing rank's status, its message prefixed with "rank r:". */
typedef struct mcrt_group mcrt_group;
int mcrt_group_create(const int *devices, uint32_t n_devices, mcrt_group **out);
int mcrt_group_destroy(mcrt_group *grp);
int mcrt_group_size(const mcrt_group *grp);                        /* ranks (0 for NULL) */
mcrt_ctx *mcrt_group_root(mcrt_group *grp);                        /* context on devices[0] that owns the gathered frames: post-processing, mcrt_alloc, exports */
mcrt_ctx *mcrt_group_member(mcrt_group *grp, uint32_t rank);       /* the rank's tracing context (statistics, timing, mcrt_cast_rays on one shard) */
/* the contiguous scan-line shard of `rank` when n_elements are cut over n_ranks (no group needed) */
int mcrt_group_shard(uint32_t rank, uint32_t n_ranks, uint32_t n_elements, uint32_t *e_begin, uint32_t *e_end);
/* the replicated set-up calls: the single-context call of the same name on every rank (concurrently), params also on the root (the ranks
 * first: a set of parameters a context refuses leaves the whole group on the old ones).  Scene data is HOST memory in every group call: a
 * device pointer belongs to one GPU and is refused.  With the host SAH builder (the default) the tree is built ONCE, on the calling
 * thread, and every rank uploads a copy (round 4 built it once per rank); the device LBVH builder runs per rank on its own GPU. */
int mcrt_group_set_params(mcrt_group *grp, const mcrt_params *p);
int mcrt_group_set_bvh_builder(mcrt_group *grp, int builder);
int mcrt_group_upload_scene(mcrt_group *grp, const float *tri_xyz_host, const uint32_t *tri_mesh, uint32_t n_tri, const mcrt_mesh *meshes, uint32_t n_mesh,
                            const float *materials, uint32_t n_mat, uint32_t start_mat, const float spacing[3]);
int mcrt_group_update_triangles(mcrt_group *grp, const float *tri_xyz_host, uint32_t n_tri);
/* seconds the last mcrt_group_upload_scene / _update_triangles spent in the host builder (once) and in the ranks' concurrent uploads */
int mcrt_group_last_scene_seconds(mcrt_group *grp, double *build_s, double *upload_s);
int mcrt_group_refit_triangles(mcrt_group *grp, const float *tri_xyz_host, uint32_t n_tri);
int mcrt_group_upload_texture(mcrt_group *grp, const float *voxels, uint32_t n);                  /* NULL: the reference's texture, generated once */
int mcrt_group_set_transducer(mcrt_group *grp, const float *pos, const float *dir, uint32_t n_elements);   /* all E elements */
/* mcrt_trace_frames over the whole group: rf_dev is a device buffer [n_frames][E][R] ON devices[0]; asynchronous -- the frames are
 * complete on the ROOT context's stream (anything enqueued on mcrt_group_root() afterwards sees them; mcrt_group_synchronize waits). */
int mcrt_group_trace_frames(mcrt_group *grp, uint32_t frame_id, uint32_t n_frames, float *rf_dev);
/* ... with a probe pose per frame (mcrt_trace_frames_poses); pos / dir: HOST tables [n_frames][E][3], copied before the call returns */
int mcrt_group_trace_frames_poses(mcrt_group *grp, uint32_t frame_id, uint32_t n_frames, const float *pos, const float *dir, float *rf_dev);
/* waits for every rank and the root; reports a rank's device error word as mcrt_synchronize does */
int mcrt_group_synchronize(mcrt_group *grp);
/* per rank, the device time of its last mcrt_group_trace_frames* pass: trace (k_init .. k_finalize) and its block's peer copy, in ms
 * (HIP events on the rank's streams; synchronises).  trace_ms / copy_ms: [mcrt_group_size()] each, either may be NULL */
int mcrt_group_last_pass_ms(mcrt_group *grp, float *trace_ms, float *copy_ms);

/* device memory helpers for callers without their own allocator */
int mcrt_alloc(mcrt_ctx *ctx, size_t bytes, void **dev);
int mcrt_free(mcrt_ctx *ctx, void *dev);
int mcrt_memcpy_d2h(mcrt_ctx *ctx, void *host, const void *dev, size_t bytes);
int mcrt_memcpy_h2d(mcrt_ctx *ctx, void *dev, const void *host, size_t bytes);

/* instrumentation: counted BVH nodes / triangles / RF steps of the next trace calls (slower build
 * of the kernel); enable=0 returns to the timed kernel */
int mcrt_enable_stats(mcrt_ctx *ctx, int enable);
int mcrt_get_stats(mcrt_ctx *ctx, mcrt_stats *out, int reset);
/* average device time of the trace kernel over the launches since the last reset (HIP events on the
 * context's stream), in milliseconds; n = launches measured */
int mcrt_enable_timing(mcrt_ctx *ctx, int enable);      /* 1: the walk's launches; 2: also k_shade's and k_march's (each on the stream it runs on) */
int mcrt_get_kernel_time(mcrt_ctx *ctx, double *avg_ms, uint32_t *n, int reset);
/* the same per kernel: [0] the walk, [1] k_shade, [2] k_march (the last two only under mcrt_enable_timing(ctx, 2)) */
int mcrt_get_kernel_times(mcrt_ctx *ctx, double avg_ms[3], uint32_t n[3], int reset);

/* ---- host-side pieces of the path (no GPU needed) ---- */
int mcrt_build_bvh(const float *tri_xyz, const uint32_t *tri_mesh, uint32_t n_tri, mcrt_bvh *out);
void mcrt_free_bvh(mcrt_bvh *bvh);
int mcrt_get_bvh(mcrt_ctx *ctx, mcrt_bvh *out /* borrowed pointers, valid until next upload */);
int mcrt_build_bvh4(const mcrt_bvh *bvh2, mcrt_bvh4 *out);
void mcrt_free_bvh4(mcrt_bvh4 *bvh4);
/* The BVH4 as the closest-hit walk reads it (borrowed; valid until the next upload / update / refit).  The default
 * lane-per-ray walk stores node boxes as half floats rounded outwards (64-byte nodes: the walk is bound by the number of
 * 16-byte pieces it fetches); the boxes returned here are those decoded values, so a CPU walk of this tree visits exactly the
 * nodes the GPU walk visits.  Hits never depend on the node boxes (closest hit). */
int mcrt_get_bvh4(mcrt_ctx *ctx, mcrt_bvh4 *out /* borrowed */);
/* the exact row look-up table used instead of the per-echo double division (see DESIGN.md "RF rows"):
 * thr[r] = smallest double t with fl(t / row_dt) >= r, r = 0..n_rows */
int mcrt_row_thresholds(double row_dt_us, uint32_t n_rows, double *thr);
/* volume<n,res>::volume() volume.h:19-35 */
int mcrt_generate_texture(float *voxels, uint32_t n);
/* psf<>::psf psf.h:34-58 */
int mcrt_psf_kernels(float freq, float var_x, float var_y, uint32_t res_um, float *axial, uint32_t n_ax, float *lateral, uint32_t n_lat);
/* transducer<N>::transducer transducer.h:24-62 */
int mcrt_transducer_elements(uint32_t n_elements, double radius_cm, double separation_mm,
                             const float position[3], const float angles_deg[3], float *pos, float *dir);

/* contract-math probe used by the parity tests: evaluates op over n inputs ON THE GPU.
 * op: 0 log_d, 1 exp_d, 2 sin_d, 3 cos_d, 4 sqrt_d, 5 div_d(x,y), 6 logf, 7 expf, 8 powf(x,y),
 *     9 sqrtf, 10 divf(x,y), 11 pow_d(x,y), 12/13 low 31 bits / remaining bits of the fixed-point echo rint(x*2^40).  x,y,out are host double arrays (float ops use the
 * value converted to float). */
int mcrt_debug_math(mcrt_ctx *ctx, int op, const double *x, const double *y, double *out, uint32_t n);
int mcrt_debug_philox(mcrt_ctx *ctx, const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);
/* diagnostic builds of the library (-DMCRT_STAMP, or -DMCRT_STAMP_LITE for the timeline alone) only: out[0..15] per-phase cycle
 * sums of k_trace, out[16+4b..] the launch timeline of bounce b (100 MHz clock: ~earliest wave start, ~earliest empty queue,
 * latest wave end, summed wave lifetimes; the first two stored complemented), out[60..119] per-bounce wavefront counts, start
 * times, longest lifetime and node-step iterations, out[120..129] cycle sums of k_march's sections (tools/stamps.py decodes them); all zero otherwise */
int mcrt_debug_stamps(mcrt_ctx *ctx, uint64_t out[200], int reset);
/* the same diagnostic builds: per bounce b < 10, out[256 b + ...]: [0..63] wavefronts of the walk by the time they END, [64..127] by the time they
 * find the ray queue dry (20 us bins on the wavefront's own clock), [128..191] by the node-step iterations (bins of 8) since their last successful claim, [192..255] by the time since their last successful claim; all zero otherwise */
int mcrt_debug_tail_histograms(mcrt_ctx *ctx, uint64_t out[2560], int reset);
/* which of the RF accumulation's fast paths the context's LAST traced frame ran with (they are switched on by checks made on the
 * device, and a check that fails silently costs a third of the frame): out[0] the reciprocal-multiply voxel quotient (verified
 * exhaustively against IEEE division for params.tex_res), out[1] the branch-free voxel cell, out[2] the entries of the padded
 * { threshold, bin } image of k_march's fast variant (0: generic variant), out[3] reserved (0) */
int mcrt_debug_fast_paths(mcrt_ctx *ctx, uint32_t out[4]);
/* what bounce 1 BY BEAMS did in the context's LAST traced pass (its first scan-line group): out[0] 1 when bounce 1 ran by beams -- a staged pass with
 * one probe pose, where bounce 1 would otherwise run as ray packets --, else 0 and the rest 0; out[1] rays whose closest hit the beams' lists
 * decided, out[2] leftover rays walked through the tree, out[3] beams whose list is incomplete (cut at its capacity), out[4] beams refused for their spread,
 * out[5] beams that have rays at all.  Waits for the stream. */
int mcrt_debug_beam(mcrt_ctx *ctx, uint32_t out[6]);
/* mcrt_debug_beam for bounce b (bounce 1, and the bounces 2 .. MCRT_BEAM_LAST whose rays are grouped by the triangle they left): out[0 .. 5] as
 * mcrt_debug_beam's -- out[1] + out[2] is the bounce's ray count --, out[6] sampled rays whose group found no slot of the group table (their
 * groups are walked), out[7] slots of the table claimed.  All 0 where bounce b did not run by beams.  Waits for the stream. */
int mcrt_debug_beam_bounce(mcrt_ctx *ctx, uint32_t b, uint32_t out[8]);
/* the BEAM ORDER of bounce b in the context's last traced pass (its first scan-line group) -- the permutation of the bounce's queue, grouped by beam,
 * through which the rays are tested against their beams' lists, a wavefront per 64 words of it: out[0] 1 when bounce b ran by beams and was ordered,
 * out[1] rays placed (the bounce's ray count), out[2] segments: beams that have rays, the pseudo-beam of the rays without a beam among them, out[3] pad
 * lanes (every segment is rounded up to whole wavefronts: at most 63 per segment), out[4] the (wavefront, beam) pairs the first pass over the lists met --
 * counted only in a context created with MCRT_TUNING=1 MCRT_BEAM_PAIRS=1, ordered or not, else 0.  All 0 where bounce b did not run by beams.  Waits for the stream. */
int mcrt_debug_beam_order(mcrt_ctx *ctx, uint32_t b, uint32_t out[5]);
/* the layout of a beam order on the HOST, the arithmetic of the kernel that lays it out (no context, no device): counts[n] rays per beam, the last the
 * pseudo-beam's -> bases[n], where each beam's segment begins (an exclusive prefix over the counts rounded up to multiples of 64; an empty beam has no
 * words), out[0] rays placed, out[1] segments, out[2] pad lanes, out[3] the order's length.  MCRT_ERR_LIMIT where the length passes 2^32 - 1. */
int mcrt_debug_beam_layout(const uint32_t *counts, uint32_t n, uint32_t *bases, uint32_t out[4]);
/* the same layout by the DEVICE kernel that lays a beam order out, run alone: counts[n] are uploaded as the beams' counters, an order buffer of
 * mcrt_debug_beam_layout's length (out[3]) and 64 words more is filled with MCRT_DEBUG_BEAM_SENTINEL, the kernel runs, and bases[n], out[4] (as mcrt_debug_beam_layout's) and
 * the order buffer come back: order_words[out[3] + 64] holds the pad word 0xffffffff in the padding of every segment and the sentinel wherever the kernel wrote
 * nothing (the rays' own places, and the 64 guard words past the length).  order_words may be null.  n >= 1; MCRT_ERR_LIMIT as mcrt_debug_beam_layout.  Buffers of its own; waits for the device. */
#define MCRT_DEBUG_BEAM_SENTINEL 0x5eed5eedu
int mcrt_debug_beam_scan(mcrt_ctx *ctx, const uint32_t *counts, uint32_t n, uint32_t *bases, uint32_t out[4], uint32_t *order_words);
/* what the BEAM STAGE of bounce b left behind in the context's last traced pass or debug call (its first scan-line group), copied as it lies: info[0] beams,
 * info[1] the capacity of a candidate list, info[2] entries of it the first pass tests, info[3] slots of the group table (0 at bounce 1, whose beams are
 * addressed directly: (scan-line x 2 + history) x 6 + 2 x dominant axis + sign), info[4] lists;
 * records[info[0]][MCRT_DEBUG_BEAM_REC] words -- floats unless said: 0-3 the slopes' bounds umin umax vmin vmax | 4-6, 7-9 the start points' bounds lo, hi | 10 the
 * largest coordinate | 11 the margin m | 12 xref, where depth 0 lies along the dominant axis | 13 s_end, the depth up to which the list is complete (+inf:
 * all of it; -inf with 0 entries: the collection outgrew its tables) | 14 entries (integer) | 15 its list (integer).  A beam without rays, or refused, has
 * umin = vmin = +inf, umax = vmax = -inf, s_end = -inf and 0 entries;
 * lists[info[4]][info[1]][16] words: vertex 0 and the triangle's id (integer) | vertex 1 and the depth at which the triangle's padded bounds begin, less m |
 * vertex 2 and the triangle's edge tolerance | 0 0 0 0; the entries past a record's count are stale;
 * keys[info[3]]: the group table, 0 a free slot, else bit 63 | scan-line << 40 | (medium & 0xff) << 32 | the triangle the rays left; the beams of slot s are 6 s .. 6 s + 5.
 * The beamed bounces of a pass share these buffers, so only the LAST bounce the pass launched by beams can be read: MCRT_ERR_INVALID for any other b, as where
 * bounce b did not run by beams.  records, lists and keys may each be null (info alone sizes them).  Copies only; waits for the stream. */
#define MCRT_DEBUG_BEAM_REC 16
int mcrt_debug_beam_records(mcrt_ctx *ctx, uint32_t b, uint32_t info[5], uint32_t *records, uint32_t *lists, uint64_t *keys);
/* beside every entry of mcrt_debug_beam_records' lists, what the beam stage stored of the entry's TRIANGLE ALONE and tests its rays with: info as
 * mcrt_debug_beam_records'; entries[info[4]][info[1]][MCRT_DEBUG_BEAM_ENTRY] words of floats: the plane n.x n.y n.z dot(v0, n), n = (v1 - v0) x (v2 - v0) |
 * the triangle's padded bounds lo.x lo.y lo.z | hi.x hi.y hi.z (pad = 2e-4 x the largest extent + the scene's absolute pad); the entries past a record's
 * count are stale;
 * begin_id[info[4]][info[1]][2]: the two further words stored there, which the list test reads in place of the list's own -- the depth at which the padded
 * bounds begin (the list's word 7) and the triangle's id (the list's word 3).  The same bounce, the same errors; entries and begin_id may each be null.
 * Copies only; waits for the stream. */
#define MCRT_DEBUG_BEAM_ENTRY 10
int mcrt_debug_beam_entries(mcrt_ctx *ctx, uint32_t b, uint32_t info[5], uint32_t *entries, uint32_t *begin_id);
/* TEST HOOK, refused (MCRT_ERR_INVALID) unless the context was created with MCRT_TEST_HOOKS set in the environment: ORs `bits` into the
 * context's device error word on its stream, as an abandoned launch would (bit 0: traversal stack ran out, bit 1: kernel watchdog
 * expired) -- what mcrt_synchronize reports and what turns finalised RF images into NaN until it is asked */
int mcrt_debug_set_error(mcrt_ctx *ctx, uint32_t bits);

#ifdef __cplusplus
}
#endif
#endif
