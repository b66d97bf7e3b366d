// mcrt_image.cpp -- the image stages of the C-ABI (include/mcrt.h): PSF, elevation, envelope, scan conversion, B-mode, compounding,
// volume imaging and rendering, speckle reduction, receiver noise, automatic gain, freehand reconstruction, RF export / import.  Host C++ only.  Of a context (mcrt_ctx.h) these read
// its device, its stream, p.speed_of_sound, c.max_travel_us, knobs.render_row_tile, knobs.speckle_fuse, knobs.autogain_copies, knobs.autogain_hist_words, the pose staging (mcrt::stage_poses:
// the two recon calls) and the image stages' own state (ImageStages), nothing else.
#include "mcrt_ctx.h"
#include "mcrt_kernels.h"
#include "mcrt_voxels.h"            // recon_tiling

#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <vector>
#include <algorithm>

using mcrt::set_error;

static bool ranges_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes)
{
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + a_bytes, b0 = (uintptr_t)b, b1 = b0 + b_bytes;
    return a0 < b1 && b0 < a1;
}

// A call's input and its optional outputs must not share memory: the input against each output that is there, in turn, and (among) that output against the ones
// before it.  The first pair that overlaps is the one reported.
struct Range { const void *p; size_t bytes; const char *name; };
static int check_overlap(const char *fn, const Range &in, const Range *outs, int n, bool among)
{
    for (int i = 0; i < n; i++) {
        if (!outs[i].p) continue;
        if (ranges_overlap(in.p, in.bytes, outs[i].p, outs[i].bytes)) return set_error(MCRT_ERR_INVALID, "%s: %s and %s overlap", fn, in.name, outs[i].name);
        for (int j = 0; among && j < i; j++)
            if (outs[j].p && ranges_overlap(outs[j].p, outs[j].bytes, outs[i].p, outs[i].bytes)) return set_error(MCRT_ERR_INVALID, "%s: %s and %s overlap", fn, outs[j].name, outs[i].name);
    }
    return MCRT_OK;
}

static int ensure_tmp(mcrt_ctx *c, size_t n)
{
    if (n > c->img.d_tmp.cap) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(c->img.d_tmp.alloc(n));
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
    HIP_TRY(mcrt::launch_convolve(rf_dev, c->img.d_tmp, n_frames, E, R, t, c->stream));
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
    MCRT_TRY(c->img.lat_rows.put(lat_rows, R, n_lat, (size_t)MCRT_MAX_ROWS * 32, c->stream));
    mcrt::ConvTaps t; memset(&t, 0, sizeof t);
    memcpy(t.ax, ax, 4 * n_ax); t.n_ax = n_ax; t.n_lat = n_lat;
    HIP_TRY(mcrt::launch_convolve_depth(rf_dev, c->img.d_tmp, n_frames, E, R, t, c->img.lat_rows.dev, c->stream));
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
    MCRT_TRY(c->img.elev_rows.put(w_rows, R, K, (size_t)MCRT_MAX_ROWS * 32, c->stream));
    HIP_TRY(mcrt::launch_elevation(planes_dev, rf_dev, n_frames, K, E, R, c->img.elev_rows.dev, c->stream));
    return MCRT_OK;
}

// ---- frequency compounding (the contracts are in include/mcrt.h) ----
// Everything is checked before anything is launched; the caller's axial table [B][R][n_ax] goes to the device tap-major [B][n_ax][R], lat_rows as
// mcrt_convolve_frames_depth's does (StagedTable).
extern "C" int mcrt_convolve_bands_frames(mcrt_ctx *c, const float *rf_dev, uint32_t n_frames, uint32_t E, uint32_t R, uint32_t B, const float *ax_rows, uint32_t n_ax,
                                          const float *lateral, const float *lat_rows, uint32_t n_lat, float *bands_dev)
{
    CTX_TRY(c);
    static const char fn[] = "mcrt_convolve_bands_frames";
    if (!rf_dev || !bands_dev || !ax_rows || E == 0 || R == 0 || n_frames == 0) return set_error(MCRT_ERR_INVALID, "%s: bad arguments", fn);
    if (!lateral == !lat_rows) return set_error(MCRT_ERR_INVALID, "%s: exactly one of lateral and lat_rows must be given (%s)", fn, lateral ? "both are" : "neither is");
    if (B == 0 || B > 8) return set_error(MCRT_ERR_INVALID, "%s: n_bands must be 1..8 (%u)", fn, B);
    if (n_ax == 0 || n_ax > 16 || n_lat == 0 || n_lat > 32) return set_error(MCRT_ERR_LIMIT, "kernel sizes must be 1..16 axial, 1..32 lateral");
    if (R > MCRT_MAX_ROWS) return set_error(MCRT_ERR_LIMIT, "%s: at most %d rows", fn, MCRT_MAX_ROWS);
    if ((double)n_frames * (double)B * (double)E * (double)R >= 0x1p40) return set_error(MCRT_ERR_LIMIT, "%s: the band stack is too large", fn);
    const size_t n = (size_t)n_frames * E * R;
    if (ranges_overlap(rf_dev, 4 * n, bands_dev, 4 * n * B)) return set_error(MCRT_ERR_INVALID, "%s: rf_dev and bands_dev overlap", fn);
    MCRT_TRY(ensure_tmp(c, n * B));
    MCRT_TRY(c->img.band_ax.put(ax_rows, R, n_ax, (size_t)MCRT_MAX_ROWS * 16 * 8, c->stream, B));
    if (lat_rows) MCRT_TRY(c->img.lat_rows.put(lat_rows, R, n_lat, (size_t)MCRT_MAX_ROWS * 32, c->stream));
    mcrt::ConvTaps t; memset(&t, 0, sizeof t);
    if (lateral) memcpy(t.lat, lateral, 4 * n_lat);
    t.n_ax = n_ax; t.n_lat = n_lat;
    HIP_TRY(mcrt::launch_convolve_bands(rf_dev, c->img.d_tmp, bands_dev, n_frames, B, E, R, t, c->img.band_ax.dev, lat_rows ? c->img.lat_rows.dev.p : nullptr, c->stream));
    return MCRT_OK;
}

// k_elevation as it is, with the band weights' own table
extern "C" int mcrt_band_fold_frames(mcrt_ctx *c, const float *bands_dev, uint32_t n_frames, uint32_t B, uint32_t E, uint32_t R, const float *w_rows, float *rf_dev)
{
    CTX_TRY(c);
    static const char fn[] = "mcrt_band_fold_frames";
    if (!bands_dev || !rf_dev || !w_rows || n_frames == 0 || E == 0 || R == 0) return set_error(MCRT_ERR_INVALID, "%s: bad arguments", fn);
    if (B == 0 || B > 8) return set_error(MCRT_ERR_INVALID, "%s: n_bands must be 1..8 (%u)", fn, B);
    if (R > MCRT_MAX_ROWS) return set_error(MCRT_ERR_LIMIT, "%s: at most %d rows", fn, MCRT_MAX_ROWS);
    if ((double)n_frames * (double)B * (double)E * (double)R >= 0x1p40) return set_error(MCRT_ERR_LIMIT, "%s: the band stack is too large", fn);
    if (ranges_overlap(bands_dev, 4 * (size_t)n_frames * B * E * R, rf_dev, 4 * (size_t)n_frames * E * R)) return set_error(MCRT_ERR_INVALID, "%s: bands_dev and rf_dev overlap", fn);
    MCRT_TRY(c->img.band_w.put(w_rows, R, B, (size_t)MCRT_MAX_ROWS * 8, c->stream));
    HIP_TRY(mcrt::launch_elevation(bands_dev, rf_dev, n_frames, B, E, R, c->img.band_w.dev, c->stream));
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

// The contract is in include/mcrt.h.  Everything is checked before anything is launched; the taps are built on the host (mcrt_detect_taps) and
// the ones at the odd offsets travel as kernel arguments, so the call allocates and uploads nothing.
extern "C" int mcrt_detect_frames(mcrt_ctx *c, const float *rf_dev, uint32_t n_frames, uint32_t E, uint32_t R, const mcrt_detect_opts *o, float *env_dev, float *iq_dev)
{
    CTX_TRY(c);
    static const char fn[] = "mcrt_detect_frames";
    if (!rf_dev || !o || E == 0 || R == 0 || n_frames == 0) return set_error(MCRT_ERR_INVALID, "%s: bad arguments", fn);
    if (!env_dev && !iq_dev) return set_error(MCRT_ERR_INVALID, "%s: neither env_dev nor iq_dev is given", fn);
    float taps[63];
    MCRT_TRY(mcrt_detect_taps(o, taps));
    if (R > MCRT_MAX_ROWS) return set_error(MCRT_ERR_LIMIT, "%s: at most %d rows", fn, MCRT_MAX_ROWS);
    if ((double)n_frames * (double)E * (double)R >= 0x1p40) return set_error(MCRT_ERR_LIMIT, "%s: the stack is too large", fn);
    const size_t n = (size_t)n_frames * E * R;
    const Range in{ rf_dev, 4 * n, "rf_dev" };
    const Range outs[2] = { { env_dev == rf_dev ? nullptr : env_dev, 4 * n, "env_dev" }, { iq_dev, 8 * n, "iq_dev" } };   // env_dev == rf_dev: in place
    MCRT_TRY(check_overlap(fn, in, outs, 2, true));
    mcrt::DetectArgs a; memset(&a, 0, sizeof a);
    a.rf = rf_dev; a.env = env_dev; a.iq = (float2 *)iq_dev; a.lines = (size_t)n_frames * E; a.R = R;
    const uint32_t M = (o->n_taps - 1u) / 2u;
    a.nt = (M + 1u) / 2u;
    for (uint32_t k = 0; k < a.nt; k++) a.t[k] = taps[M + 2u * k + 1u];
    HIP_TRY(mcrt::launch_detect(a, c->stream));
    return MCRT_OK;
}

// ---- colour Doppler (the contracts are in include/mcrt.h; the defaults, the option ranges, the phasors, the draws and the colour table are
// host code: mcrt_host.cpp) ----
extern "C" int mcrt_flow_split_frames(mcrt_ctx *c, const float *rf_dev, const uint8_t *tissue_dev, uint32_t n_frames, uint32_t E, uint32_t R, const uint8_t *moving,
                                      uint32_t n_labels, float *out_dev)
{
    CTX_TRY(c);
    static const char fn[] = "mcrt_flow_split_frames";
    if (!rf_dev || !tissue_dev || !moving || !out_dev) return set_error(MCRT_ERR_INVALID, "%s: null pointer", fn);
    if (n_frames == 0 || E == 0 || R == 0 || n_labels == 0) return set_error(MCRT_ERR_INVALID, "%s: zero sizes (n_frames %u, n_elements %u, n_rows %u, n_labels %u)", fn, n_frames, E, R, n_labels);
    if (n_labels > 254u) return set_error(MCRT_ERR_LIMIT, "%s: at most 254 labels (%u)", fn, n_labels);
    if ((double)n_frames * (double)E * (double)R >= 0x1p31) return set_error(MCRT_ERR_LIMIT, "%s: a stack of 2^31 samples or more (%u x %u x %u)", fn, n_frames, E, R);
    const size_t n = (size_t)n_frames * E * R;
    const Range out{ out_dev, 8 * n, "out_dev" };
    const Range ins[2] = { { rf_dev, 4 * n, "rf_dev" }, { tissue_dev, n, "tissue_dev" } };
    MCRT_TRY(check_overlap(fn, out, ins, 2, false));
    mcrt::FlowSplitArgs a; memset(&a, 0, sizeof a);
    a.rf = rf_dev; a.tissue = tissue_dev; a.out = out_dev; a.plane = E * R; a.n = (uint32_t)n;
    for (uint32_t l = 0; l < n_labels; l++)
        if (moving[l]) a.moving[l >> 5] |= 1u << (l & 31u);
    HIP_TRY(mcrt::launch_flow_split(a, c->stream));
    return MCRT_OK;
}

// Everything is checked before anything is enqueued; then the two tables (only when they differ from the ones on the device), the
// per-sample autocorrelation into the context's buffer (k_flow<N, WALL>) and the window average with the estimates (k_flow_avg).
extern "C" int mcrt_flow_frames(mcrt_ctx *c, const float *iq_static_dev, const float *iq_moving_dev, const uint8_t *tissue_dev, uint32_t n_frames, uint32_t E, uint32_t R,
                                const mcrt_flow_opts *o, double v_nyq_mm_s, const float *phasor, const float *truth, uint32_t n_labels, uint32_t first_image_id,
                                const float *sigma_dev, float *corr_dev, float *vel_dev, float *var_dev, float *truth_dev)
{
    CTX_TRY(c);
    static const char fn[] = "mcrt_flow_frames";
    if (!iq_moving_dev || !tissue_dev || !phasor || !truth || !o) return set_error(MCRT_ERR_INVALID, "%s: null pointer", fn);
    if (n_frames == 0 || E == 0 || R == 0 || n_labels == 0) return set_error(MCRT_ERR_INVALID, "%s: zero sizes (n_frames %u, n_elements %u, n_rows %u, n_labels %u)", fn, n_frames, E, R, n_labels);
    MCRT_TRY(mcrt::flow_check(fn, o));
    if (!(std::isfinite(v_nyq_mm_s) && v_nyq_mm_s > 0.0)) return set_error(MCRT_ERR_INVALID, "%s: v_nyq_mm_s must be finite and > 0 (%g)", fn, v_nyq_mm_s);
    if (!corr_dev && !vel_dev && !var_dev && !truth_dev) return set_error(MCRT_ERR_INVALID, "%s: no output is given", fn);
    if (n_labels > 254u) return set_error(MCRT_ERR_LIMIT, "%s: at most 254 labels (%u)", fn, n_labels);
    if (R > MCRT_MAX_ROWS) return set_error(MCRT_ERR_LIMIT, "%s: n_rows: at most %d rows (%u)", fn, MCRT_MAX_ROWS, R);
    if ((double)n_frames * (double)E * (double)R >= 0x1p31) return set_error(MCRT_ERR_LIMIT, "%s: a stack of 2^31 samples or more (%u x %u x %u)", fn, n_frames, E, R);
    if ((uint64_t)first_image_id + n_frames > 0x100000000ull) return set_error(MCRT_ERR_LIMIT, "%s: first_image_id: the ids of %u images from %u on pass 2^32", fn, n_frames, first_image_id);
    const size_t n_tab = (size_t)n_labels * E;
    for (size_t i = 0; i < n_tab; i++)
        if (!std::isfinite(phasor[2 * i]) || !std::isfinite(phasor[2 * i + 1]) || !std::isfinite(truth[i]))
            return set_error(MCRT_ERR_INVALID, "%s: the phasor or the truth of label %zu, scan-line %zu is not finite", fn, i / E, i % E);
    const size_t n = (size_t)n_frames * E * R;
    const Range outs[4] = { { corr_dev, 12 * n, "corr_dev" }, { vel_dev, 4 * n, "vel_dev" }, { var_dev, 4 * n, "var_dev" }, { truth_dev, 4 * n, "truth_dev" } };
    const Range ins[4] = { { iq_static_dev, 8 * n, "iq_static_dev" }, { iq_moving_dev, 8 * n, "iq_moving_dev" }, { tissue_dev, n, "tissue_dev" }, { sigma_dev, 4 * (size_t)n_frames, "sigma_dev" } };
    for (int i = 0; i < 4; i++)
        if (ins[i].p) MCRT_TRY(check_overlap(fn, ins[i], outs, 4, i == 1));      // (iq_moving_dev is always there: the outputs among themselves once)
    if (3 * n > c->img.d_flow.cap) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(c->img.d_flow.alloc(3 * n));
    }
    MCRT_TRY(c->img.flow_phasor.put(phasor, (uint32_t)(2 * n_tab), 1, 2 * n_tab, c->stream));
    MCRT_TRY(c->img.flow_truth.put(truth, (uint32_t)n_tab, 1, n_tab, c->stream));
    mcrt::FlowArgs a; memset(&a, 0, sizeof a);
    a.iq_static = (const float2 *)iq_static_dev; a.iq_moving = (const float2 *)iq_moving_dev; a.tissue = tissue_dev;
    a.phasor = (const float2 *)c->img.flow_phasor.dev.p; a.truth = c->img.flow_truth.dev.p; a.sigma_dev = sigma_dev; a.raw = c->img.d_flow;
    a.corr = corr_dev; a.vel = vel_dev; a.var = var_dev; a.truth_out = truth_dev;
    a.F = n_frames; a.E = E; a.R = R; a.n_labels = n_labels; a.lines = n_frames * E; a.chunks = (R + FLOW_WAVE_ROWS - 1u) / FLOW_WAVE_ROWS;
    a.n_packets = o->n_packets; a.wall = o->wall; a.avg_rows = o->avg_rows; a.avg_lines = o->avg_lines; a.seed = o->seed; a.first_id = first_image_id;
    a.sigma = o->sigma; a.inv_std = (float)(1.0 / std::sqrt(1431655765.0)); a.vscale = (float)(v_nyq_mm_s / 3.141592653589793);
    HIP_TRY(mcrt::launch_flow(a, c->stream));
    return MCRT_OK;
}

// ---- spectral Doppler (the contracts are in include/mcrt.h; the defaults, the option ranges and the table builders are host code:
// mcrt_host.cpp).  Each call checks everything before anything is enqueued; then its host tables (only those that differ from what the
// device holds) and its kernel. ----
static int spectral_sizes(const char *fn, uint32_t n_gates, uint32_t T)
{
    if (n_gates > 65535u) return set_error(MCRT_ERR_LIMIT, "%s: at most 65535 gates (%u)", fn, n_gates);
    if ((uint64_t)n_gates * T >= (1ull << 28)) return set_error(MCRT_ERR_LIMIT, "%s: n_gates * n_pulses must stay below 2^28 (%u x %u)", fn, n_gates, T);
    return MCRT_OK;
}

extern "C" int mcrt_spectral_series_frames(mcrt_ctx *c, const float *iq_static_dev, const float *iq_moving_dev, uint32_t n_frames, uint32_t E, uint32_t R,
                                           const mcrt_gate *gates, uint32_t n_gates, const float *weight, const int32_t *rate, const int64_t *phase,
                                           const mcrt_spectral_opts *o, uint32_t first_image_id, const float *sigma_dev, float *series_dev)
{
    CTX_TRY(c);
    static const char fn[] = "mcrt_spectral_series_frames";
    if (!iq_moving_dev || !gates || !weight || !rate || !phase || !o || !series_dev) return set_error(MCRT_ERR_INVALID, "%s: null pointer", fn);
    if (n_frames == 0 || E == 0 || R == 0 || n_gates == 0) return set_error(MCRT_ERR_INVALID, "%s: zero sizes (n_frames %u, n_elements %u, n_rows %u, n_gates %u)", fn, n_frames, E, R, n_gates);
    MCRT_TRY(mcrt::spectral_check(fn, o));
    const uint32_t G = o->gate_rows, T = o->n_pulses;
    MCRT_TRY(spectral_sizes(fn, n_gates, T));
    if ((double)n_frames * (double)E * (double)R >= 0x1p31) return set_error(MCRT_ERR_LIMIT, "%s: a stack of 2^31 samples or more (%u x %u x %u)", fn, n_frames, E, R);
    if ((uint64_t)first_image_id + n_frames > 0x100000000ull) return set_error(MCRT_ERR_LIMIT, "%s: first_image_id: the ids of %u images from %u on pass 2^32", fn, n_frames, first_image_id);
    double w2 = 0.0;
    for (uint32_t i = 0; i < G; i++) {
        if (!std::isfinite(weight[i])) return set_error(MCRT_ERR_INVALID, "%s: weight[%u] is not finite", fn, i);
        w2 += (double)weight[i] * (double)weight[i];
    }
    for (uint32_t j = 0; j < n_gates; j++) {
        if (gates[j].image >= n_frames || gates[j].line >= E || (uint64_t)gates[j].row0 + G > R)
            return set_error(MCRT_ERR_INVALID, "%s: gate %u (image %u, line %u, rows %u + %u) is outside the stack %u x %u x %u", fn, j, gates[j].image, gates[j].line, gates[j].row0, G, n_frames, E, R);
        for (uint32_t i = 0; i < G; i++)
            if (rate[(size_t)j * G + i] > 65536 || rate[(size_t)j * G + i] < -65536) return set_error(MCRT_ERR_INVALID, "%s: rate[%u][%u] = %d is outside +-65536", fn, j, i, rate[(size_t)j * G + i]);
    }
    const size_t n = (size_t)n_frames * E * R;
    const Range out{ series_dev, 8 * (size_t)n_gates * T, "series_dev" };
    const Range ins[3] = { { iq_static_dev, 8 * n, "iq_static_dev" }, { iq_moving_dev, 8 * n, "iq_moving_dev" }, { sigma_dev, 4 * (size_t)n_frames, "sigma_dev" } };
    MCRT_TRY(check_overlap(fn, out, ins, 3, false));
    static const std::vector<float> rotor = [] { std::vector<float> l(8192); mcrt_spectral_rotor(l.data()); return l; }();
    MCRT_TRY(c->img.spec_rotor.put(rotor.data(), 8192, c->stream));
    MCRT_TRY(c->img.spec_gates.put(gates, 3 * (size_t)n_gates, c->stream));
    MCRT_TRY(c->img.spec_weight.put(weight, G, c->stream));
    MCRT_TRY(c->img.spec_rate.put(rate, (size_t)n_gates * G, c->stream));
    MCRT_TRY(c->img.spec_phase.put(phase, 2 * (size_t)T, c->stream));
    mcrt::GateSeriesArgs a; memset(&a, 0, sizeof a);
    a.iq_static = (const float2 *)iq_static_dev; a.iq_moving = (const float2 *)iq_moving_dev; a.sigma_dev = sigma_dev; a.series = (float2 *)series_dev;
    a.gates = c->img.spec_gates.as<uint32_t>(); a.weight = c->img.spec_weight.as<float>(); a.rate = c->img.spec_rate.as<int32_t>();
    a.phase = c->img.spec_phase.as<long long>(); a.lut = c->img.spec_rotor.as<float2>();
    a.E = E; a.R = R; a.G = G; a.T = T; a.n_gates = n_gates; a.chunks = (T + 63u) / 64u; a.seed = o->seed; a.first_id = first_image_id;
    a.sigma = o->sigma; a.wnorm = (float)std::sqrt(w2); a.inv_std = (float)(1.0 / std::sqrt(1431655765.0));
    HIP_TRY(mcrt::launch_gate_series(a, c->stream));
    return MCRT_OK;
}

extern "C" int mcrt_spectral_frames(mcrt_ctx *c, const float *series_dev, uint32_t n_gates, const float *window, const mcrt_spectral_opts *o, double v_nyq_mm_s,
                                    float *power_dev, float *mean_dev)
{
    CTX_TRY(c);
    static const char fn[] = "mcrt_spectral_frames";
    if (!series_dev || !window || !o) return set_error(MCRT_ERR_INVALID, "%s: null pointer", fn);
    if (n_gates == 0) return set_error(MCRT_ERR_INVALID, "%s: n_gates is zero", fn);
    MCRT_TRY(mcrt::spectral_check(fn, o));
    const uint32_t T = o->n_pulses, N = o->n_fft;
    if (T < N) return set_error(MCRT_ERR_INVALID, "%s: a series of %u pulses is shorter than one window of %u", fn, T, N);
    if (!(std::isfinite(v_nyq_mm_s) && v_nyq_mm_s > 0.0)) return set_error(MCRT_ERR_INVALID, "%s: v_nyq_mm_s must be finite and > 0 (%g)", fn, v_nyq_mm_s);
    if (!power_dev && !mean_dev) return set_error(MCRT_ERR_INVALID, "%s: no output is given", fn);
    for (uint32_t i = 0; i < N; i++)
        if (!std::isfinite(window[i])) return set_error(MCRT_ERR_INVALID, "%s: window[%u] is not finite", fn, i);
    MCRT_TRY(spectral_sizes(fn, n_gates, T));
    const uint32_t n_cols = (T - N) / o->hop + 1u;
    const Range in{ series_dev, 8 * (size_t)n_gates * T, "series_dev" };
    const Range outs[2] = { { power_dev, 4 * (size_t)n_gates * n_cols * N, "power_dev" }, { mean_dev, 4 * (size_t)n_gates * n_cols, "mean_dev" } };
    MCRT_TRY(check_overlap(fn, in, outs, 2, true));
    uint32_t slot = 0;
    while ((32u << slot) != N) slot++;
    StagedWords &tw = c->img.spec_tw[slot];
    if (!tw.valid) {
        std::vector<float> t(N);
        MCRT_TRY(mcrt_spectral_twiddles(N, t.data()));
        MCRT_TRY(tw.put(t.data(), N, c->stream));
    }
    MCRT_TRY(c->img.spec_window.put(window, N, c->stream));
    mcrt::SpectrumArgs a; memset(&a, 0, sizeof a);
    a.series = (const float2 *)series_dev; a.window = c->img.spec_window.as<float>(); a.tw = tw.as<float2>(); a.power = power_dev; a.mean = mean_dev;
    a.n_gates = n_gates; a.T = T; a.n_cols = n_cols; a.N = N; a.hop = o->hop; a.wall = o->wall; a.wall_bins = o->wall_bins;
    a.vscale = (float)(2.0 * v_nyq_mm_s / N);
    HIP_TRY(mcrt::launch_spectrum(a, c->stream));
    return MCRT_OK;
}

extern "C" int mcrt_sonogram_frames(mcrt_ctx *c, const float *power_dev, uint32_t n_gates, uint32_t n_cols, uint32_t N, const mcrt_sonogram_opts *o, float *peak_dev,
                                    uint8_t *out_dev)
{
    CTX_TRY(c);
    static const char fn[] = "mcrt_sonogram_frames";
    if (!power_dev || !o || !out_dev) return set_error(MCRT_ERR_INVALID, "%s: null pointer", fn);
    if (n_gates == 0 || n_cols == 0) return set_error(MCRT_ERR_INVALID, "%s: zero sizes (n_gates %u, n_cols %u)", fn, n_gates, n_cols);
    if (N != 32u && N != 64u && N != 128u && N != 256u && N != 512u) return set_error(MCRT_ERR_INVALID, "%s: n_fft must be 32, 64, 128, 256 or 512 (%u)", fn, N);
    if (!(std::isfinite(o->dynamic_range_db) && o->dynamic_range_db > 0.0f)) return set_error(MCRT_ERR_INVALID, "%s: dynamic_range_db must be finite and > 0 (%g)", fn, (double)o->dynamic_range_db);
    if (!std::isfinite(o->gain_db) || !std::isfinite(o->ref)) return set_error(MCRT_ERR_INVALID, "%s: gain_db and ref must be finite (%g, %g)", fn, (double)o->gain_db, (double)o->ref);
    MCRT_TRY(spectral_sizes(fn, n_gates, n_cols));
    const size_t n = (size_t)n_gates * n_cols * N;
    const Range in{ power_dev, 4 * n, "power_dev" };
    const Range outs[2] = { { peak_dev, 4 * (size_t)n_gates, "peak_dev" }, { out_dev, n, "out_dev" } };
    MCRT_TRY(check_overlap(fn, in, outs, 2, true));
    const bool own_ref = o->ref > 0.0f;
    float *peak = peak_dev;
    if (!peak && !own_ref) {
        if (n_gates > c->img.d_sono_peak.cap) {
            HIP_TRY(hipStreamSynchronize(c->stream));
            HIP_TRY(c->img.d_sono_peak.alloc(n_gates));
        }
        peak = c->img.d_sono_peak;
    }
    mcrt::SonogramArgs a; memset(&a, 0, sizeof a);
    a.power = power_dev; a.peak = peak; a.out = out_dev; a.n_gates = n_gates; a.n_cols = n_cols; a.N = N;
    a.ref = o->ref; a.gain = o->gain_db; a.dr = o->dynamic_range_db;
    if (peak) {
        HIP_TRY(hipMemsetAsync(peak, 0, 4 * (size_t)n_gates, c->stream));
        HIP_TRY(mcrt::launch_sonogram_peak(a, c->stream));
    }
    if (own_ref) a.peak = nullptr;
    HIP_TRY(mcrt::launch_sonogram(a, c->stream));
    return MCRT_OK;
}

// ---- strain elastography (the contracts are in include/mcrt.h; the defaults, the option ranges, the strain table, the draws and the
// colour table are host code: mcrt_host.cpp).  Each call checks everything before anything is enqueued. ----
static int strain_sizes(const char *fn, uint32_t n_frames, uint32_t E, uint32_t R, double cycles_per_row)
{
    if (n_frames == 0 || E == 0 || R == 0) return set_error(MCRT_ERR_INVALID, "%s: zero sizes (n_frames %u, n_elements %u, n_rows %u)", fn, n_frames, E, R);
    if (!(cycles_per_row > 0.0 && cycles_per_row <= 0.5)) return set_error(MCRT_ERR_INVALID, "%s: cycles_per_row must be in (0, 0.5] (%g)", fn, cycles_per_row);
    if (R > MCRT_MAX_ROWS) return set_error(MCRT_ERR_LIMIT, "%s: n_rows: at most %d rows (%u)", fn, MCRT_MAX_ROWS, R);
    if ((double)n_frames * (double)E * (double)R >= 0x1p31) return set_error(MCRT_ERR_LIMIT, "%s: a stack of 2^31 samples or more (%u x %u x %u)", fn, n_frames, E, R);
    return MCRT_OK;
}

extern "C" int mcrt_strain_compress_frames(mcrt_ctx *c, const float *iq_dev, const uint8_t *tissue_dev, uint32_t n_frames, uint32_t E, uint32_t R,
                                           const int32_t *eps_q24, uint32_t n_labels, double cycles_per_row, const mcrt_strain_opts *o, uint32_t first_image_id,
                                           const float *sigma_dev, float *post_iq_dev, float *truth_disp_dev, float *truth_strain_dev)
{
    CTX_TRY(c);
    static const char fn[] = "mcrt_strain_compress_frames";
    if (!iq_dev || !tissue_dev || !eps_q24 || !o) return set_error(MCRT_ERR_INVALID, "%s: null pointer", fn);
    if (n_labels == 0) return set_error(MCRT_ERR_INVALID, "%s: n_labels is zero", fn);
    MCRT_TRY(strain_sizes(fn, n_frames, E, R, cycles_per_row));
    MCRT_TRY(mcrt::strain_check(fn, o));
    if (!post_iq_dev && !truth_disp_dev && !truth_strain_dev) return set_error(MCRT_ERR_INVALID, "%s: no output is given", fn);
    if (n_labels > 254u) return set_error(MCRT_ERR_LIMIT, "%s: at most 254 labels (%u)", fn, n_labels);
    if ((uint64_t)first_image_id + n_frames > 0x100000000ull) return set_error(MCRT_ERR_LIMIT, "%s: first_image_id: the ids of %u images from %u on pass 2^32", fn, n_frames, first_image_id);
    for (uint32_t l = 0; l < n_labels; l++)
        if (eps_q24[l] > 524288 || eps_q24[l] < -524288) return set_error(MCRT_ERR_INVALID, "%s: eps_q24[%u] = %d is outside +-2^19", fn, l, eps_q24[l]);
    const size_t n = (size_t)n_frames * E * R;
    const Range outs[3] = { { post_iq_dev, 8 * n, "post_iq_dev" }, { truth_disp_dev, 4 * n, "truth_disp_dev" }, { truth_strain_dev, 4 * n, "truth_strain_dev" } };
    const Range ins[3] = { { iq_dev, 8 * n, "iq_dev" }, { tissue_dev, n, "tissue_dev" }, { sigma_dev, 4 * (size_t)n_frames, "sigma_dev" } };
    for (int i = 0; i < 3; i++)
        if (ins[i].p) MCRT_TRY(check_overlap(fn, ins[i], outs, 3, i == 0));      // (iq_dev is always there: the outputs among themselves once)
    static const std::vector<float> rotor = [] { std::vector<float> l(8192); mcrt_spectral_rotor(l.data()); return l; }();
    MCRT_TRY(c->img.spec_rotor.put(rotor.data(), 8192, c->stream));
    MCRT_TRY(c->img.strain_eps.put(eps_q24, n_labels, c->stream));
    mcrt::StrainWarpArgs a; memset(&a, 0, sizeof a);
    a.iq = (const float2 *)iq_dev; a.tissue = tissue_dev; a.eps = c->img.strain_eps.as<int32_t>(); a.lut = c->img.spec_rotor.as<float2>(); a.sigma_dev = sigma_dev;
    a.post = (float2 *)post_iq_dev; a.truth_disp = truth_disp_dev; a.truth_strain = truth_strain_dev;
    a.carrier_q32 = std::llrint(cycles_per_row * 4294967296.0); a.E = E; a.R = R; a.lines = n_frames * E; a.n_labels = n_labels;
    a.seed = o->seed; a.first_id = first_image_id; a.sigma = o->sigma; a.inv_std = (float)(1.0 / std::sqrt(1431655765.0));
    HIP_TRY(mcrt::launch_strain_warp(a, c->stream));
    return MCRT_OK;
}

extern "C" int mcrt_strain_frames(mcrt_ctx *c, const float *pre_iq_dev, const float *post_iq_dev, uint32_t n_frames, uint32_t E, uint32_t R, const mcrt_strain_opts *o,
                                  double cycles_per_row, float *disp_dev, float *rho_dev, float *strain_dev)
{
    CTX_TRY(c);
    static const char fn[] = "mcrt_strain_frames";
    if (!pre_iq_dev || !post_iq_dev || !o) return set_error(MCRT_ERR_INVALID, "%s: null pointer", fn);
    MCRT_TRY(strain_sizes(fn, n_frames, E, R, cycles_per_row));
    MCRT_TRY(mcrt::strain_check(fn, o));
    if (!disp_dev && !rho_dev && !strain_dev) return set_error(MCRT_ERR_INVALID, "%s: no output is given", fn);
    const size_t n = (size_t)n_frames * E * R;
    const Range outs[3] = { { disp_dev, 4 * n, "disp_dev" }, { rho_dev, 4 * n, "rho_dev" }, { strain_dev, 4 * n, "strain_dev" } };
    MCRT_TRY(check_overlap(fn, Range{ pre_iq_dev, 8 * n, "pre_iq_dev" }, outs, 3, true));
    MCRT_TRY(check_overlap(fn, Range{ post_iq_dev, 8 * n, "post_iq_dev" }, outs, 3, false));
    float *disp = disp_dev;
    if (!disp) {
        if (n > c->img.d_strain_disp.cap) {
            HIP_TRY(hipStreamSynchronize(c->stream));
            HIP_TRY(c->img.d_strain_disp.alloc(n));
        }
        disp = c->img.d_strain_disp;
    }
    mcrt::StrainTrackArgs a; memset(&a, 0, sizeof a);
    a.pre = (const float2 *)pre_iq_dev; a.post = (const float2 *)post_iq_dev; a.disp = disp; a.rho = rho_dev; a.strain = strain_dev;
    a.R = R; a.lines = n_frames * E; a.chunks = (R + STRAIN_TILE_ROWS - 1u) / STRAIN_TILE_ROWS;
    a.window = o->window_rows; a.search = o->search_rows; a.lsq = o->lsq_rows; a.scale = (float)(1.0 / (6.283185307179586 * cycles_per_row));
    HIP_TRY(mcrt::launch_strain_track(a, c->stream));
    return MCRT_OK;
}

// ---- shear-wave elastography (the contracts are in include/mcrt.h; the defaults, the option ranges, the tables, the draws and the colour
// table are host code: mcrt_host.cpp).  Each call checks everything before anything is enqueued. ----
static int shear_sizes(const char *fn, uint32_t n_frames, uint32_t E, uint32_t R)
{
    if (n_frames == 0 || E == 0 || R == 0) return set_error(MCRT_ERR_INVALID, "%s: zero sizes (n_frames %u, n_elements %u, n_rows %u)", fn, n_frames, E, R);
    if (R > MCRT_MAX_ROWS) return set_error(MCRT_ERR_LIMIT, "%s: n_rows: at most %d rows (%u)", fn, MCRT_MAX_ROWS, R);
    if ((double)n_frames * (double)E * (double)R >= 0x1p31) return set_error(MCRT_ERR_LIMIT, "%s: a stack of 2^31 samples or more (%u x %u x %u)", fn, n_frames, E, R);
    return MCRT_OK;
}

extern "C" int mcrt_shear_wave_frames(mcrt_ctx *c, const float *iq_dev, const uint8_t *tissue_dev, uint32_t n_frames, uint32_t E, uint32_t R, const int64_t *slow_q16,
                                      const float *speed_f, uint32_t n_labels, const uint32_t *pitch_q8, const uint32_t *shape_q16, uint32_t n_shape,
                                      const uint32_t *amp_q16, uint32_t n_amp, double cycles_per_row, const mcrt_shear_opts *o, uint32_t first_image_id,
                                      const float *sigma_dev, float *peak_time_dev, float *peak_disp_dev, float *disp_dev, float *truth_arrival_dev,
                                      float *truth_speed_dev)
{
    CTX_TRY(c);
    static const char fn[] = "mcrt_shear_wave_frames";
    if (!iq_dev || !tissue_dev || !slow_q16 || !speed_f || !pitch_q8 || !shape_q16 || !amp_q16 || !o) return set_error(MCRT_ERR_INVALID, "%s: null pointer", fn);
    if (n_labels == 0 || n_shape == 0 || n_amp == 0) return set_error(MCRT_ERR_INVALID, "%s: an empty table (n_labels %u, n_shape %u, n_amp %u)", fn, n_labels, n_shape, n_amp);
    MCRT_TRY(shear_sizes(fn, n_frames, E, R));
    if (!(cycles_per_row > 0.0 && cycles_per_row <= 0.5)) return set_error(MCRT_ERR_INVALID, "%s: cycles_per_row must be in (0, 0.5] (%g)", fn, cycles_per_row);
    MCRT_TRY(mcrt::shear_check(fn, o, E, R));
    if (!peak_time_dev && !peak_disp_dev && !disp_dev && !truth_arrival_dev && !truth_speed_dev) return set_error(MCRT_ERR_INVALID, "%s: no output is given", fn);
    if (n_labels > 254u) return set_error(MCRT_ERR_LIMIT, "%s: at most 254 labels (%u)", fn, n_labels);
    if (n_shape > 16384u) return set_error(MCRT_ERR_LIMIT, "%s: at most 16384 entries of the time profile (%u)", fn, n_shape);
    if (n_amp > 65536u) return set_error(MCRT_ERR_LIMIT, "%s: at most 65536 entries of the decay (%u)", fn, n_amp);
    const uint32_t T = o->n_pulses;
    if (disp_dev && (double)n_frames * (double)T * (double)E * (double)R >= 0x1p31)
        return set_error(MCRT_ERR_LIMIT, "%s: a movie of 2^31 samples or more (%u x %u x %u x %u)", fn, n_frames, T, E, R);
    if ((uint64_t)first_image_id + n_frames > 0x100000000ull) return set_error(MCRT_ERR_LIMIT, "%s: first_image_id: the ids of %u images from %u on pass 2^32", fn, n_frames, first_image_id);
    for (uint32_t l = 0; l < n_labels; l++)
        if (slow_q16[l] < 0 || slow_q16[l] > (1ll << 38)) return set_error(MCRT_ERR_INVALID, "%s: slow_q16[%u] = %lld is outside [0, 2^38]", fn, l, (long long)slow_q16[l]);
    for (uint32_t r = 0; r < R; r++)
        if (pitch_q8[r] == 0u || pitch_q8[r] >= (1u << 24)) return set_error(MCRT_ERR_INVALID, "%s: pitch_q8[%u] = %u is outside [1, 2^24)", fn, r, pitch_q8[r]);
    for (uint32_t i = 0; i < n_shape; i++)
        if (shape_q16[i] > 65536u) return set_error(MCRT_ERR_INVALID, "%s: shape_q16[%u] = %u is above 65536", fn, i, shape_q16[i]);
    for (uint32_t i = 0; i < n_amp; i++)
        if (amp_q16[i] > 65536u) return set_error(MCRT_ERR_INVALID, "%s: amp_q16[%u] = %u is above 65536", fn, i, amp_q16[i]);
    const size_t n = (size_t)n_frames * E * R;
    const Range outs[5] = { { peak_time_dev, 4 * n, "peak_time_dev" }, { peak_disp_dev, 4 * n, "peak_disp_dev" }, { disp_dev, 4 * n * T, "disp_dev" },
                            { truth_arrival_dev, 4 * n, "truth_arrival_dev" }, { truth_speed_dev, 4 * n, "truth_speed_dev" } };
    const Range ins[3] = { { iq_dev, 8 * n, "iq_dev" }, { tissue_dev, n, "tissue_dev" }, { sigma_dev, 4 * (size_t)n_frames, "sigma_dev" } };
    for (int i = 0; i < 3; i++)
        if (ins[i].p) MCRT_TRY(check_overlap(fn, ins[i], outs, 5, i == 0));      // (iq_dev is always there: the outputs among themselves once)
    if (n > c->img.d_shear_arrival.cap) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(c->img.d_shear_arrival.alloc(n));
    }
    static const std::vector<float> rotor = [] { std::vector<float> l(8192); mcrt_spectral_rotor(l.data()); return l; }();
    MCRT_TRY(c->img.spec_rotor.put(rotor.data(), 8192, c->stream));
    MCRT_TRY(c->img.shear_slow.put(slow_q16, 2 * (size_t)n_labels, c->stream));
    MCRT_TRY(c->img.shear_speed.put(speed_f, n_labels, c->stream));
    MCRT_TRY(c->img.shear_pitch.put(pitch_q8, R, c->stream));
    MCRT_TRY(c->img.shear_shape.put(shape_q16, n_shape, c->stream));
    MCRT_TRY(c->img.shear_amp.put(amp_q16, n_amp, c->stream));
    mcrt::ShearWaveArgs a; memset(&a, 0, sizeof a);
    a.iq = (const float2 *)iq_dev; a.tissue = tissue_dev; a.slow = c->img.shear_slow.as<long long>(); a.speed_f = c->img.shear_speed.as<float>();
    a.pitch = c->img.shear_pitch.as<uint32_t>(); a.shape = c->img.shear_shape.as<uint32_t>(); a.amp = c->img.shear_amp.as<uint32_t>();
    a.lut = c->img.spec_rotor.as<float2>(); a.sigma_dev = sigma_dev; a.arrival = c->img.d_shear_arrival;
    a.peak_time = peak_time_dev; a.peak_disp = peak_disp_dev; a.disp = disp_dev; a.truth_arrival = truth_arrival_dev; a.truth_speed = truth_speed_dev;
    a.carrier_q32 = std::llrint(cycles_per_row * 4294967296.0);
    a.F = n_frames; a.E = E; a.R = R; a.chunks = (R + SHEAR_TILE_ROWS - 1u) / SHEAR_TILE_ROWS; a.n_labels = n_labels; a.n_shape = n_shape; a.n_amp = n_amp;
    a.T = T; a.window = o->window_rows; a.push_line = o->push_line; a.row0 = o->push_row0; a.row1 = o->push_rows ? o->push_row0 + o->push_rows : R;
    a.peak_q24 = o->peak_q24; a.seed = o->seed; a.first_id = first_image_id; a.sigma = o->sigma; a.inv_std = (float)(1.0 / std::sqrt(1431655765.0));
    a.scale = (float)(1.0 / (6.283185307179586 * cycles_per_row));
    HIP_TRY(mcrt::launch_shear_wave(a, c->stream));
    return MCRT_OK;
}

extern "C" int mcrt_shear_speed_frames(mcrt_ctx *c, const float *peak_time_dev, uint32_t n_frames, uint32_t E, uint32_t R, const float *pitch_mm,
                                       const mcrt_shear_opts *o, float *speed_dev, float *modulus_dev, float *quality_dev)
{
    CTX_TRY(c);
    static const char fn[] = "mcrt_shear_speed_frames";
    if (!peak_time_dev || !pitch_mm || !o) return set_error(MCRT_ERR_INVALID, "%s: null pointer", fn);
    MCRT_TRY(shear_sizes(fn, n_frames, E, R));
    MCRT_TRY(mcrt::shear_check(fn, o, E, R));
    if (!speed_dev && !modulus_dev && !quality_dev) return set_error(MCRT_ERR_INVALID, "%s: no output is given", fn);
    for (uint32_t r = 0; r < R; r++)
        if (!(std::isfinite(pitch_mm[r]) && pitch_mm[r] > 0.0f)) return set_error(MCRT_ERR_INVALID, "%s: pitch_mm[%u] must be finite and > 0 (%g)", fn, r, (double)pitch_mm[r]);
    const size_t n = (size_t)n_frames * E * R;
    const Range outs[3] = { { speed_dev, 4 * n, "speed_dev" }, { modulus_dev, 4 * n, "modulus_dev" }, { quality_dev, 4 * n, "quality_dev" } };
    MCRT_TRY(check_overlap(fn, Range{ peak_time_dev, 4 * n, "peak_time_dev" }, outs, 3, true));
    MCRT_TRY(c->img.shear_pitch_mm.put(pitch_mm, R, c->stream));
    mcrt::ShearSpeedArgs a; memset(&a, 0, sizeof a);
    a.peak_time = peak_time_dev; a.pitch_mm = c->img.shear_pitch_mm.as<float>(); a.speed = speed_dev; a.modulus = modulus_dev; a.quality = quality_dev;
    a.F = n_frames; a.E = E; a.R = R; a.chunks = (R + SHEAR_TILE_ROWS - 1u) / SHEAR_TILE_ROWS; a.push_line = o->push_line; a.lines = o->speed_lines; a.avg = o->avg_rows;
    a.kf = (float)((double)o->prf_hz * 0.001); a.d3 = 3.0f * o->density;
    HIP_TRY(mcrt::launch_shear_speed(a, c->stream));
    return MCRT_OK;
}

// ---- M-mode (the contracts are in include/mcrt.h; the defaults, the option ranges, the tables, the draws and the depth table are host
// code: mcrt_host.cpp).  Each call checks everything before anything is enqueued. ----
static int mmode_sizes(const char *fn, uint32_t n_lines, uint32_t T, uint32_t R)
{
    if (R > MCRT_MAX_ROWS) return set_error(MCRT_ERR_LIMIT, "%s: n_rows: at most %d rows (%u)", fn, MCRT_MAX_ROWS, R);
    if (T > 16384u) return set_error(MCRT_ERR_LIMIT, "%s: at most 16384 pulses (%u)", fn, T);
    if (n_lines > 65535u) return set_error(MCRT_ERR_LIMIT, "%s: at most 65535 lines (%u)", fn, n_lines);
    if ((double)n_lines * (double)T * (double)R >= 0x1p31) return set_error(MCRT_ERR_LIMIT, "%s: 2^31 samples or more (%u lines x %u pulses x %u rows)", fn, n_lines, T, R);
    return MCRT_OK;
}

extern "C" int mcrt_mmode_lines_frames(mcrt_ctx *c, const float *iq_dev, const uint8_t *tissue_dev, uint32_t n_frames, uint32_t E, uint32_t R, const mcrt_mline *lines,
                                       uint32_t n_lines, const int32_t *dil_q24, uint32_t n_labels, const int32_t *w_q16, const int32_t *bulk_q24, double cycles_per_row,
                                       const mcrt_mmode_opts *o, uint32_t first_image_id, const float *sigma_dev, float *env_dev, float *iq_out_dev,
                                       float *truth_disp_dev, uint8_t *truth_label_dev)
{
    CTX_TRY(c);
    static const char fn[] = "mcrt_mmode_lines_frames";
    if (!iq_dev || !tissue_dev || !lines || !dil_q24 || !w_q16 || !bulk_q24 || !o) return set_error(MCRT_ERR_INVALID, "%s: null pointer", fn);
    if (n_labels == 0 || n_lines == 0) return set_error(MCRT_ERR_INVALID, "%s: an empty table (n_labels %u, n_lines %u)", fn, n_labels, n_lines);
    MCRT_TRY(strain_sizes(fn, n_frames, E, R, cycles_per_row));
    MCRT_TRY(mcrt::mmode_check(fn, o));
    if (!env_dev && !iq_out_dev && !truth_disp_dev && !truth_label_dev) return set_error(MCRT_ERR_INVALID, "%s: no output is given", fn);
    if (n_labels > 254u) return set_error(MCRT_ERR_LIMIT, "%s: at most 254 labels (%u)", fn, n_labels);
    const uint32_t T = o->n_pulses;
    MCRT_TRY(mmode_sizes(fn, n_lines, T, R));
    if ((uint64_t)first_image_id + n_frames > 0x100000000ull) return set_error(MCRT_ERR_LIMIT, "%s: first_image_id: the ids of %u images from %u on pass 2^32", fn, n_frames, first_image_id);
    for (uint32_t j = 0; j < n_lines; j++)
        if (lines[j].image >= n_frames || lines[j].line >= E)
            return set_error(MCRT_ERR_INVALID, "%s: line %u (image %u, scan-line %u) is outside the stack %u x %u", fn, j, lines[j].image, lines[j].line, n_frames, E);
    for (uint32_t l = 0; l < n_labels; l++)
        if (dil_q24[l] > 4194304 || dil_q24[l] < -4194304) return set_error(MCRT_ERR_INVALID, "%s: dil_q24[%u] = %d is outside +-2^22", fn, l, dil_q24[l]);
    for (uint32_t t = 0; t < T; t++) {
        if (w_q16[t] > 65536 || w_q16[t] < -65536) return set_error(MCRT_ERR_INVALID, "%s: w_q16[%u] = %d is outside +-65536", fn, t, w_q16[t]);
        if (bulk_q24[t] > (32 << 24) || bulk_q24[t] < -(32 << 24)) return set_error(MCRT_ERR_INVALID, "%s: bulk_q24[%u] = %d is outside +-32 rows", fn, t, bulk_q24[t]);
    }
    const size_t n = (size_t)n_frames * E * R, m = (size_t)n_lines * T * R;
    const Range outs[4] = { { env_dev, 4 * m, "env_dev" }, { iq_out_dev, 8 * m, "iq_out_dev" }, { truth_disp_dev, 4 * m, "truth_disp_dev" }, { truth_label_dev, m, "truth_label_dev" } };
    const Range ins[3] = { { iq_dev, 8 * n, "iq_dev" }, { tissue_dev, n, "tissue_dev" }, { sigma_dev, 4 * (size_t)n_frames, "sigma_dev" } };
    for (int i = 0; i < 3; i++)
        if (ins[i].p) MCRT_TRY(check_overlap(fn, ins[i], outs, 4, i == 0));      // (iq_dev is always there: the outputs among themselves once)
    static const std::vector<float> rotor = [] { std::vector<float> l(8192); mcrt_spectral_rotor(l.data()); return l; }();
    MCRT_TRY(c->img.spec_rotor.put(rotor.data(), 8192, c->stream));
    MCRT_TRY(c->img.mmode_lines.put(lines, 2 * (size_t)n_lines, c->stream));
    MCRT_TRY(c->img.mmode_dil.put(dil_q24, n_labels, c->stream));
    MCRT_TRY(c->img.mmode_w.put(w_q16, T, c->stream));
    MCRT_TRY(c->img.mmode_bulk.put(bulk_q24, T, c->stream));
    mcrt::MmodeLinesArgs a; memset(&a, 0, sizeof a);
    a.iq = (const float2 *)iq_dev; a.tissue = tissue_dev; a.lines = c->img.mmode_lines.as<uint32_t>(); a.dil = c->img.mmode_dil.as<int32_t>();
    a.w = c->img.mmode_w.as<int32_t>(); a.bulk = c->img.mmode_bulk.as<int32_t>(); a.lut = c->img.spec_rotor.as<float2>(); a.sigma_dev = sigma_dev;
    a.env = env_dev; a.iq_out = (float2 *)iq_out_dev; a.truth_disp = truth_disp_dev; a.truth_label = truth_label_dev;
    a.carrier_q32 = std::llrint(cycles_per_row * 4294967296.0); a.E = E; a.R = R; a.T = T; a.n_lines = n_lines;
    a.chunks = (T + MMODE_PULSE_CHUNK - 1u) / MMODE_PULSE_CHUNK; a.n_labels = n_labels;
    a.seed = o->seed; a.first_id = first_image_id; a.sigma = o->sigma; a.inv_std = (float)(1.0 / std::sqrt(1431655765.0));
    HIP_TRY(mcrt::launch_mmode_lines(a, c->stream));
    return MCRT_OK;
}

extern "C" int mcrt_mmode_picture_frames(mcrt_ctx *c, const float *env_dev, const uint8_t *truth_label_dev, const float *truth_disp_dev, uint32_t n_lines, uint32_t T,
                                         uint32_t R, const mcrt_mmode_display_opts *o, float *peak_dev, float *mean_dev, uint8_t *out_dev, uint8_t *label_out_dev,
                                         float *disp_out_dev)
{
    CTX_TRY(c);
    static const char fn[] = "mcrt_mmode_picture_frames";
    if (!env_dev || !o || !out_dev) return set_error(MCRT_ERR_INVALID, "%s: null pointer", fn);
    if (n_lines == 0 || T == 0 || R == 0) return set_error(MCRT_ERR_INVALID, "%s: zero sizes (n_lines %u, n_pulses %u, n_rows %u)", fn, n_lines, T, R);
    MCRT_TRY(mmode_sizes(fn, n_lines, T, R));
    MCRT_TRY(mcrt::mmode_display_check(fn, o, T, R));
    if (label_out_dev && !truth_label_dev) return set_error(MCRT_ERR_INVALID, "%s: label_out_dev needs truth_label_dev", fn);
    if (disp_out_dev && !truth_disp_dev) return set_error(MCRT_ERR_INVALID, "%s: disp_out_dev needs truth_disp_dev", fn);
    const uint32_t W = T / o->hop, H = o->height, row_hi = o->row_hi ? o->row_hi : R;
    if ((double)n_lines * (double)H * (double)W >= 0x1p31) return set_error(MCRT_ERR_LIMIT, "%s: pictures of 2^31 pixels or more (%u x %u x %u)", fn, n_lines, H, W);
    const size_t m = (size_t)n_lines * T * R, px = (size_t)n_lines * H * W;
    const Range outs[5] = { { peak_dev, 4 * (size_t)n_lines, "peak_dev" }, { mean_dev, 4 * (size_t)n_lines * W * R, "mean_dev" }, { out_dev, px, "out_dev" },
                            { label_out_dev, px, "label_out_dev" }, { disp_out_dev, 4 * px, "disp_out_dev" } };
    const Range ins[3] = { { env_dev, 4 * m, "env_dev" }, { truth_label_dev, m, "truth_label_dev" }, { truth_disp_dev, 4 * m, "truth_disp_dev" } };
    for (int i = 0; i < 3; i++)
        if (ins[i].p) MCRT_TRY(check_overlap(fn, ins[i], outs, 5, i == 0));      // (env_dev is always there: the outputs among themselves once)
    std::vector<uint32_t> idx(H); std::vector<float> wt(H);
    MCRT_TRY(mcrt_mmode_rows(o->row_lo, row_hi, H, idx.data(), wt.data()));
    const bool own_ref = o->ref > 0.0f;
    float *peak = peak_dev;
    if (!peak && !own_ref) {
        if (n_lines > c->img.d_mmode_peak.cap) {
            HIP_TRY(hipStreamSynchronize(c->stream));
            HIP_TRY(c->img.d_mmode_peak.alloc(n_lines));
        }
        peak = c->img.d_mmode_peak;
    }
    MCRT_TRY(c->img.mmode_idx.put(idx.data(), H, c->stream));
    MCRT_TRY(c->img.mmode_wt.put(wt.data(), H, c->stream));
    mcrt::MmodePictureArgs a; memset(&a, 0, sizeof a);
    a.env = env_dev; a.truth_label = truth_label_dev; a.truth_disp = truth_disp_dev; a.idx = c->img.mmode_idx.as<uint32_t>(); a.wt = c->img.mmode_wt.as<float>();
    a.peak = peak; a.mean = mean_dev; a.out = out_dev; a.label_out = label_out_dev; a.disp_out = disp_out_dev;
    a.n_lines = n_lines; a.T = T; a.R = R; a.W = W; a.H = H; a.hop = o->hop; a.row_lo = o->row_lo; a.row_hi = row_hi;
    a.ref = o->ref; a.gain = o->gain_db; a.dr = o->dynamic_range_db;
    if (peak || mean_dev) {
        if (peak) HIP_TRY(hipMemsetAsync(peak, 0, 4 * (size_t)n_lines, c->stream));
        HIP_TRY(mcrt::launch_mmode_peak(a, c->stream));
    }
    if (own_ref) a.peak = nullptr;
    HIP_TRY(mcrt::launch_mmode_picture(a, c->stream));
    return MCRT_OK;
}

// the scan-conversion maps of a geometry on the device, in cache m: the plain maps (cp null: mcrt_scan_maps, one view) or the N views of a steer
// list (mcrt_compound_maps), [N][2][n_pad]
static int ensure_maps(mcrt_ctx *c, MapCache &m, uint32_t E, uint32_t R, double radius_mm, double total_angle, uint32_t orows, uint32_t ocols, const mcrt_compound *cp, const float **maps)
{
    const uint32_t N = cp ? cp->n_views : 1u, sos = c->p.speed_of_sound;
    MapCache::Key key;
    key.add(E).add(R).add(orows).add(ocols).add(sos).add(N).add(radius_mm).add(total_angle).add(c->c.max_travel_us);
    if (cp) key.add(cp->steer_rad, 4 * (size_t)N);
    const size_t n = (size_t)orows * ocols, n_pad = MapCache::pad(n);
    return m.get(key, 2 * (size_t)N * n_pad, c->stream, [&](std::vector<float> &out) -> int {
        // (the rf_image template parameter is max_travel_time.to<unsigned int>(), main.cpp:36 -- the same truncation as max_rows uses)
        const uint32_t travel = (uint32_t)c->c.max_travel_us;
        for (uint32_t v = 0; v < N; v++) {
            float *mc = &out[(size_t)(2u * v) * n_pad], *mr = mc + n_pad;
            MCRT_TRY(cp ? mcrt_compound_maps(E, R, radius_mm, total_angle, travel, sos, orows, ocols, cp->steer_rad[v], mr, mc)
                        : mcrt_scan_maps(E, R, radius_mm, total_angle, travel, sos, orows, ocols, mr, mc));
        }
        return MCRT_OK;
    }, maps);
}

extern "C" int mcrt_scan_convert_frames(mcrt_ctx *c, const float *rf_dev, uint32_t n_frames, uint32_t E, uint32_t R, double radius_mm, double total_angle,
                                        float *out_dev, uint32_t orows, uint32_t ocols)
{
    CTX_TRY(c);
    if (!rf_dev || !out_dev || E == 0 || R == 0 || orows == 0 || ocols == 0 || n_frames == 0) return set_error(MCRT_ERR_INVALID, "mcrt_scan_convert: bad arguments");
    if (n_frames > 65535u) return set_error(MCRT_ERR_LIMIT, "mcrt_scan_convert: at most 65535 images per call");
    const float *maps = nullptr;
    MCRT_TRY(ensure_maps(c, c->img.maps, E, R, radius_mm, total_angle, orows, ocols, nullptr, &maps));
    HIP_TRY(mcrt::launch_remap(rf_dev, n_frames, E, R, maps, maps + MapCache::pad((size_t)orows * ocols), out_dev, orows * ocols, c->stream));
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
    if (!c->img.d_disp) HIP_TRY(c->img.d_disp.alloc(65536));   // (the peaks of the largest pass: 65535 frames)
    if (tgc_db) MCRT_TRY(c->img.tgc.put(k.data(), R, 1, MCRT_MAX_ROWS, c->stream));
    const size_t taps = (size_t)n_frames * lines * R;
    MCRT_TRY(ensure_tmp(c, taps));     // the grey levels of the pass (the scratch mcrt_convolve uses too)
    const float *tgc = tgc_db ? c->img.tgc.dev.p : nullptr;
    if (p->ref > 0.0f) HIP_TRY(mcrt::launch_bmode_grey(rf_dev, n_frames, lines, R, tgc, nullptr, p->ref, peak_dev, p->mode, p->gain_db, p->dynamic_range_db, c->img.d_tmp, c->stream));
    else {
        float *peak = peak_dev ? peak_dev : c->img.d_disp.p;
        HIP_TRY(hipMemsetAsync(peak, 0, 4 * (size_t)n_frames, c->stream));
        HIP_TRY(mcrt::launch_bmode_peak(rf_dev, n_frames, lines, R, tgc, peak, c->stream));
        HIP_TRY(mcrt::launch_bmode_grey(rf_dev, n_frames, lines, R, tgc, peak, 0.0f, nullptr, p->mode, p->gain_db, p->dynamic_range_db, c->img.d_tmp, c->stream));
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

// the pass description of k_bmode, k_compound, k_volume and k_label_gather: n_frames pictures of n points, out_elem_bytes each (1: a lane
// may store a word per frame where the picture's size and the pointer keep it aligned)
static mcrt::PixelPass pixel_pass(uint32_t n_frames, uint32_t n, float alpha, const void *out, uint32_t out_elem_bytes)
{
    const uint32_t vec = out_elem_bytes == 1u && n % 4u == 0u && (uintptr_t)out % 4u == 0u ? 1u : 0u;
    return mcrt::PixelPass{ n, (uint32_t)MapCache::pad(n), n_frames, display_frames_per_chunk(n_frames, n, alpha), vec };
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
    const float *maps = nullptr;
    MCRT_TRY(ensure_maps(c, c->img.maps, E, R, p->radius_mm, p->total_angle_rad, p->out_rows, p->out_cols, nullptr, &maps));
    MCRT_TRY(bmode_grey_pass(c, rf_dev, n_frames, E, R, p, tgc_db, k, peak_dev));
    mcrt::BmodeArgs a;
    a.grey = c->img.d_tmp; a.map_col = maps; a.map_row = maps + MapCache::pad((size_t)p->out_rows * p->out_cols); a.state = state_dev; a.out = out_dev; a.alpha = p->persistence;
    a.E = E; a.R = R; a.reset = p->reset_state ? 1u : 0u; a.pass = pixel_pass(n_frames, p->out_rows * p->out_cols, a.alpha, out_dev, 1u);
    HIP_TRY(mcrt::launch_bmode(a, c->stream));
    return MCRT_OK;
}

// ---- the colour overlay of colour Doppler (the contract is in include/mcrt.h, beside mcrt_flow_frames) ----
// Everything is checked before anything is enqueued; the colour table goes to the device as 256 floats, each the exact integer
// r | g << 8 | b << 16 (only when it differs from the one there).
extern "C" int mcrt_colour_frames(mcrt_ctx *c, const float *corr_img_dev, const uint8_t *grey_dev, uint32_t n_frames, uint32_t H, uint32_t W, const uint8_t *lut,
                                  const mcrt_colour_opts *o, double v_nyq_mm_s, uint8_t *rgb_dev, float *vel_img_dev)
{
    CTX_TRY(c);
    static const char fn[] = "mcrt_colour_frames";
    if (!corr_img_dev || !grey_dev || !lut || !o || !rgb_dev) return set_error(MCRT_ERR_INVALID, "%s: null pointer", fn);
    if (n_frames == 0 || H == 0 || W == 0) return set_error(MCRT_ERR_INVALID, "%s: zero sizes (n_frames %u, height %u, width %u)", fn, n_frames, H, W);
    if (!std::isfinite(o->power_thr)) return set_error(MCRT_ERR_INVALID, "%s: power_thr must be finite (%g)", fn, (double)o->power_thr);
    if (!(std::isfinite(o->vel_thr_mm_s) && o->vel_thr_mm_s >= 0.0f)) return set_error(MCRT_ERR_INVALID, "%s: vel_thr_mm_s must be finite and >= 0 (%g)", fn, (double)o->vel_thr_mm_s);
    if (o->grey_max > 255u) return set_error(MCRT_ERR_INVALID, "%s: grey_max must be 0 .. 255 (%u)", fn, o->grey_max);
    if (!(std::isfinite(v_nyq_mm_s) && v_nyq_mm_s > 0.0)) return set_error(MCRT_ERR_INVALID, "%s: v_nyq_mm_s must be finite and > 0 (%g)", fn, v_nyq_mm_s);
    if ((double)n_frames * (double)H * (double)W >= 0x1p31) return set_error(MCRT_ERR_LIMIT, "%s: 2^31 pixels or more (%u x %u x %u)", fn, n_frames, H, W);
    const size_t n = (size_t)n_frames * H * W;
    const Range outs[2] = { { rgb_dev, 3 * n, "rgb_dev" }, { vel_img_dev, 4 * n, "vel_img_dev" } };
    MCRT_TRY(check_overlap(fn, Range{ corr_img_dev, 12 * n, "corr_img_dev" }, outs, 2, true));
    MCRT_TRY(check_overlap(fn, Range{ grey_dev, n, "grey_dev" }, outs, 2, false));
    float packed[256];
    for (uint32_t i = 0; i < 256u; i++) packed[i] = (float)((uint32_t)lut[3 * i] | (uint32_t)lut[3 * i + 1] << 8 | (uint32_t)lut[3 * i + 2] << 16);
    MCRT_TRY(c->img.colour_lut.put(packed, 256, 1, 256, c->stream));
    mcrt::ColourArgs a; memset(&a, 0, sizeof a);
    a.corr = corr_img_dev; a.grey = grey_dev; a.lut = c->img.colour_lut.dev.p; a.rgb = rgb_dev; a.vel = vel_img_dev;
    a.power_thr = o->power_thr; a.vel_thr = o->vel_thr_mm_s; a.vscale = (float)(v_nyq_mm_s / 3.141592653589793); a.iscale = (float)(127.0 / 3.141592653589793);
    a.grey_max = o->grey_max; a.pass = pixel_pass(n_frames, H * W, 0.0f, vel_img_dev, 4u);
    HIP_TRY(mcrt::launch_colour(a, c->stream));
    return MCRT_OK;
}

// ---- the overlay of strain elastography (the contract is in include/mcrt.h, beside mcrt_strain_frames) ----
// Everything is checked before anything is enqueued; the colour table goes to the device as mcrt_colour_frames' does, in a table of its own.
extern "C" int mcrt_elastogram_frames(mcrt_ctx *c, const float *strain_img_dev, const float *rho_img_dev, const uint8_t *grey_dev, uint32_t n_frames, uint32_t H, uint32_t W,
                                      const uint8_t *lut, const mcrt_elastogram_opts *o, uint8_t *rgb_dev)
{
    CTX_TRY(c);
    static const char fn[] = "mcrt_elastogram_frames";
    if (!strain_img_dev || !rho_img_dev || !grey_dev || !lut || !o || !rgb_dev) return set_error(MCRT_ERR_INVALID, "%s: null pointer", fn);
    if (n_frames == 0 || H == 0 || W == 0) return set_error(MCRT_ERR_INVALID, "%s: zero sizes (n_frames %u, height %u, width %u)", fn, n_frames, H, W);
    if (!(std::isfinite(o->ref_strain) && o->ref_strain != 0.0f)) return set_error(MCRT_ERR_INVALID, "%s: ref_strain must be finite and not 0 (%g)", fn, (double)o->ref_strain);
    if (!std::isfinite(o->rho_min)) return set_error(MCRT_ERR_INVALID, "%s: rho_min must be finite (%g)", fn, (double)o->rho_min);
    if (o->grey_min > 255u) return set_error(MCRT_ERR_INVALID, "%s: grey_min must be 0 .. 255 (%u)", fn, o->grey_min);
    if (o->alpha > 256u) return set_error(MCRT_ERR_INVALID, "%s: alpha must be 0 .. 256 (%u)", fn, o->alpha);
    if ((double)n_frames * (double)H * (double)W >= 0x1p31) return set_error(MCRT_ERR_LIMIT, "%s: 2^31 pixels or more (%u x %u x %u)", fn, n_frames, H, W);
    const size_t n = (size_t)n_frames * H * W;
    const Range out{ rgb_dev, 3 * n, "rgb_dev" };
    const Range ins[3] = { { strain_img_dev, 4 * n, "strain_img_dev" }, { rho_img_dev, 4 * n, "rho_img_dev" }, { grey_dev, n, "grey_dev" } };
    MCRT_TRY(check_overlap(fn, out, ins, 3, false));
    float packed[256];
    for (uint32_t i = 0; i < 256u; i++) packed[i] = (float)((uint32_t)lut[3 * i] | (uint32_t)lut[3 * i + 1] << 8 | (uint32_t)lut[3 * i + 2] << 16);
    MCRT_TRY(c->img.elasto_lut.put(packed, 256, 1, 256, c->stream));
    mcrt::ElastogramArgs a; memset(&a, 0, sizeof a);
    a.strain = strain_img_dev; a.rho = rho_img_dev; a.grey = grey_dev; a.lut = c->img.elasto_lut.dev.p; a.rgb = rgb_dev;
    a.ref_strain = o->ref_strain; a.rho_min = o->rho_min; a.grey_min = o->grey_min; a.alpha = o->alpha;
    a.pass = pixel_pass(n_frames, H * W, 0.0f, rgb_dev, 1u);
    HIP_TRY(mcrt::launch_elastogram(a, c->stream));
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
    MCRT_TRY(ensure_maps(c, c->img.cmaps, E, R, radius_mm, total_angle, orows, ocols, cp, &a.maps));
    a.src = rf_dev; a.state = nullptr; a.out = out_dev; a.alpha = 0.0f;
    a.E = E; a.R = R; a.N = N; a.reset = 1u; a.pass = pixel_pass(n_frames, n, 0.0f, out_dev, 4u);
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
    MCRT_TRY(ensure_maps(c, c->img.cmaps, E, R, p->radius_mm, p->total_angle_rad, p->out_rows, p->out_cols, cp, &a.maps));
    MCRT_TRY(bmode_grey_pass(c, rf_dev, n_frames, N * E, R, p, tgc_db, k, peak_dev));
    a.src = c->img.d_tmp; a.state = state_dev; a.out = out_dev; a.alpha = p->persistence;
    a.E = E; a.R = R; a.N = N; a.reset = p->reset_state ? 1u : 0u; a.pass = pixel_pass(n_frames, n, a.alpha, out_dev, 1u);
    HIP_TRY(mcrt::launch_compound(a, true, c->stream));
    return MCRT_OK;
}

extern "C" int mcrt_bmode_compound_frames(mcrt_ctx *c, const float *rf_dev, uint32_t n_frames, uint32_t E, uint32_t R, const mcrt_bmode_params *p,
                                          const mcrt_compound *cp, const float *tgc_db, float *state_dev, float *peak_dev, uint8_t *out_dev)
{
    return mcrt_bmode_compound_frames_opts(c, rf_dev, n_frames, E, R, p, cp, tgc_db, state_dev, peak_dev, out_dev, nullptr);
}

// ---- volume imaging (the contracts are in include/mcrt.h) ----
// the three maps of a grid on the device, [3][n_pad]: plane, column, row (mcrt_volume_maps)
static int ensure_volume_maps(mcrt_ctx *c, uint32_t E, uint32_t R, double radius_mm, double total_angle, const mcrt_sweep *sw, const mcrt_volume_grid *g, const float **maps)
{
    const uint32_t sos = c->p.speed_of_sound;
    MapCache::Key key;
    key.add(E).add(R).add(sos).add(sw->n_planes).add(sw->step_rad).add(sw->pivot_mm).add(g->nu).add(g->nv).add(g->nw);
    key.add(radius_mm).add(total_angle).add(c->c.max_travel_us).add(g->origin_mm).add(g->du_mm).add(g->dv_mm).add(g->dw_mm);
    const size_t n_pad = MapCache::pad((size_t)g->nu * g->nv * g->nw);
    return c->img.vmaps.get(key, 3 * n_pad, c->stream, [&](std::vector<float> &m) {
        return mcrt_volume_maps(E, R, radius_mm, total_angle, (uint32_t)c->c.max_travel_us, sos, sw, g, &m[0], &m[2 * n_pad], &m[n_pad]);
    }, maps);
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
    a.src = src; a.maps = maps; a.out = out; a.E = E; a.R = R; a.K = K; a.pass = pixel_pass(n_frames, n, 0.0f, out, out8 ? 1u : 4u);
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
    HIP_TRY(mcrt::launch_volume(volume_args(c->img.d_tmp, maps, out_dev, n_frames, E, R, K, n, true), true, c->stream));
    return MCRT_OK;
}

// ---- volume rendering (the contract is in include/mcrt.h; the defaults and the view helper are host code: mcrt_host.cpp) ----
// what mcrt_render_frames and mcrt_render_label_frames ask of the block and the view alike: the argument errors, then the limits
static int render_view_invalid(const char *fn, uint32_t n_frames, uint32_t nu, uint32_t nv, uint32_t nw, const mcrt_render_view *view)
{
    if (n_frames == 0 || nu == 0 || nv == 0 || nw == 0) return set_error(MCRT_ERR_INVALID, "%s: zero sizes (n_frames %u, block %u x %u x %u)", fn, n_frames, nu, nv, nw);
    if (view->nx == 0 || view->ny == 0) return set_error(MCRT_ERR_INVALID, "%s: view: zero picture size (nx %u, ny %u)", fn, view->nx, view->ny);
    for (int k = 0; k < 3; k++)
        if (!(std::isfinite(view->origin[k]) && std::isfinite(view->di[k]) && std::isfinite(view->dj[k]) && std::isfinite(view->ds[k])))
            return set_error(MCRT_ERR_INVALID, "%s: view: origin, di, dj or ds has an entry that is not finite (component %d)", fn, k);
    return MCRT_OK;
}
static int render_view_limits(const char *fn, uint32_t n_frames, uint32_t nu, uint32_t nv, uint32_t nw, const mcrt_render_view *view)
{
    if (view->n_steps == 0 || view->n_steps > 4096u) return set_error(MCRT_ERR_LIMIT, "%s: view: n_steps must be 1..4096 (%u)", fn, view->n_steps);
    if (nu >= (1u << 24) || nv >= (1u << 24) || nw >= (1u << 24)) return set_error(MCRT_ERR_LIMIT, "%s: nu, nv and nw must be below 2^24 (%u x %u x %u)", fn, nu, nv, nw);
    if ((double)nu * (double)nv * (double)nw >= 0x1p31) return set_error(MCRT_ERR_LIMIT, "%s: 2^31 voxels or more (%u x %u x %u)", fn, nu, nv, nw);
    if ((uint64_t)view->nx * view->ny >= 0x80000000ull) return set_error(MCRT_ERR_LIMIT, "%s: view: 2^31 pixels or more (%u x %u)", fn, view->nx, view->ny);
    if (n_frames > 65535u) return set_error(MCRT_ERR_LIMIT, "%s: at most 65535 frames per call (%u)", fn, n_frames);
    return MCRT_OK;
}
static mcrt::ViewArgs view_args(const mcrt_render_view *view, uint32_t n_frames, uint32_t nu, uint32_t nv, uint32_t nw)
{
    mcrt::ViewArgs a;
    for (int k = 0; k < 3; k++) { a.origin[k] = view->origin[k]; a.di[k] = view->di[k]; a.dj[k] = view->dj[k]; a.ds[k] = view->ds[k]; }
    a.nx = view->nx; a.ny = view->ny; a.n_steps = view->n_steps; a.F = n_frames; a.nu = nu; a.nv = nv; a.nw = nw;
    return a;
}

// Everything is checked before anything is launched; the derived floats are made here, in double, rounded once.
extern "C" int mcrt_render_frames(mcrt_ctx *c, const void *vol_dev, int in_u8, uint32_t n_frames, uint32_t nu, uint32_t nv, uint32_t nw,
                                  const mcrt_render_view *view, const mcrt_render_opts *o, float *out_dev, uint8_t *out8_dev, float *depth_dev)
{
    CTX_TRY(c);
    static const char fn[] = "mcrt_render_frames";
    if (!vol_dev || !view) return set_error(MCRT_ERR_INVALID, "%s: null %s", fn, vol_dev ? "view" : "vol_dev");
    if (!out_dev && !out8_dev && !depth_dev) return set_error(MCRT_ERR_INVALID, "%s: out_dev, out8_dev and depth_dev are all null", fn);
    MCRT_TRY(render_view_invalid(fn, n_frames, nu, nv, nw, view));
    mcrt_render_opts d;
    if (!o) { mcrt_default_render_opts(&d, in_u8); o = &d; }
    if (o->mode != MCRT_RENDER_MIP && o->mode != MCRT_RENDER_MEAN && o->mode != MCRT_RENDER_SURFACE) return set_error(MCRT_ERR_INVALID, "%s: unknown mode %u", fn, o->mode);
    if (!(std::isfinite(o->lo) && std::isfinite(o->hi) && o->hi > o->lo)) return set_error(MCRT_ERR_INVALID, "%s: lo, hi must be finite with hi > lo (%g, %g)", fn, (double)o->lo, (double)o->hi);
    if (!(o->threshold >= 0.0f && o->threshold < 1.0f)) return set_error(MCRT_ERR_INVALID, "%s: threshold must be in [0,1) (%g)", fn, (double)o->threshold);
    if (!(o->ramp > 0.0f && o->ramp <= 1.0f)) return set_error(MCRT_ERR_INVALID, "%s: ramp must be in (0,1] (%g)", fn, (double)o->ramp);
    const float inv_range = (float)(1.0 / ((double)o->hi - (double)o->lo)), inv_ramp = (float)(1.0 / (double)o->ramp);
    if (!std::isfinite(inv_range)) return set_error(MCRT_ERR_INVALID, "%s: lo, hi: the window is too narrow, 1 / (hi - lo) is no finite float (%g, %g)", fn, (double)o->lo, (double)o->hi);
    if (!std::isfinite(inv_ramp)) return set_error(MCRT_ERR_INVALID, "%s: ramp is too small, 1 / ramp is no finite float (%g)", fn, (double)o->ramp);
    if (!(o->opacity > 0.0f && o->opacity <= 1.0f)) return set_error(MCRT_ERR_INVALID, "%s: opacity must be in (0,1] (%g)", fn, (double)o->opacity);
    if (!(o->depth_cue >= 0.0f && o->depth_cue <= 1.0f)) return set_error(MCRT_ERR_INVALID, "%s: depth_cue must be in [0,1] (%g)", fn, (double)o->depth_cue);
    if (!(o->t_cut >= 0.0f && o->t_cut < 1.0f)) return set_error(MCRT_ERR_INVALID, "%s: t_cut must be in [0,1) (%g)", fn, (double)o->t_cut);
    MCRT_TRY(render_view_limits(fn, n_frames, nu, nv, nw, view));
    const size_t nvox = (size_t)nu * nv * nw, npix = (size_t)view->nx * view->ny, vol_bytes = (in_u8 ? 1u : 4u) * (size_t)n_frames * nvox;
    const Range outs[3] = { { out_dev, 4 * n_frames * npix, "out_dev" }, { out8_dev, n_frames * npix, "out8_dev" }, { depth_dev, 4 * n_frames * npix, "depth_dev" } };
    MCRT_TRY(check_overlap(fn, Range{ vol_dev, vol_bytes, "vol_dev" }, outs, 3, false));     // (the outputs are not held against each other)
    mcrt::RenderArgs a;
    a.vol = vol_dev; a.out = out_dev; a.out8 = out8_dev; a.depth = depth_dev; a.view = view_args(view, n_frames, nu, nv, nw);
    a.mode = o->mode; a.row_tile = c->knobs.render_row_tile ? 1u : 0u;
    a.lo = o->lo; a.inv_range = inv_range;
    a.threshold = o->threshold; a.inv_ramp = inv_ramp; a.opacity = o->opacity; a.depth_cue = o->depth_cue; a.t_cut = o->t_cut;
    a.inv_steps = view->n_steps > 1u ? (float)(1.0 / (double)(view->n_steps - 1u)) : 0.0f;
    HIP_TRY(mcrt::launch_render(a, in_u8 != 0, c->stream));
    return MCRT_OK;
}

// the label of what a rendering shows (the contract is in include/mcrt.h): one launch, nothing allocated or uploaded
extern "C" int mcrt_render_label_frames(mcrt_ctx *c, const uint8_t *label_dev, uint32_t n_frames, uint32_t nu, uint32_t nv, uint32_t nw, const mcrt_render_view *view,
                                        const float *depth_dev, uint8_t *out_dev)
{
    CTX_TRY(c);
    static const char fn[] = "mcrt_render_label_frames";
    if (!label_dev || !view || !depth_dev || !out_dev)
        return set_error(MCRT_ERR_INVALID, "%s: null %s", fn, !label_dev ? "label_dev" : !view ? "view" : !depth_dev ? "depth_dev" : "out_dev");
    MCRT_TRY(render_view_invalid(fn, n_frames, nu, nv, nw, view));
    MCRT_TRY(render_view_limits(fn, n_frames, nu, nv, nw, view));
    const size_t nvox = (size_t)nu * nv * nw, npix = (size_t)view->nx * view->ny;
    if (ranges_overlap(label_dev, n_frames * nvox, out_dev, n_frames * npix)) return set_error(MCRT_ERR_INVALID, "%s: label_dev and out_dev overlap", fn);
    if (ranges_overlap(depth_dev, 4 * n_frames * npix, out_dev, n_frames * npix)) return set_error(MCRT_ERR_INVALID, "%s: depth_dev and out_dev overlap", fn);
    mcrt::RenderLabelArgs a;
    a.labels = label_dev; a.depth = depth_dev; a.out = out_dev; a.view = view_args(view, n_frames, nu, nv, nw);
    HIP_TRY(mcrt::launch_render_label(a, c->stream));
    return MCRT_OK;
}

// ---- speckle reduction (the contract is in include/mcrt.h; the defaults and the tables are host code: mcrt_host.cpp) ----
// Everything is checked before anything is launched.  L = ceil(n_iter / T) launches of T = knobs.speckle_fuse iterations; launch k = 1..L
// writes out_dev when L - k is even and the scratch when it is odd, and reads what launch k - 1 wrote: the last one lands in out_dev and no
// launch reads what it writes.  The first launch reads in_dev -- in place with an odd L that is the buffer it writes, so the stack is
// first copied into the scratch, which then is both the input and the other half of the ping-pong.
extern "C" int mcrt_speckle_frames(mcrt_ctx *c, const float *in_dev, uint32_t n_frames, uint32_t height, uint32_t width, const mcrt_speckle_opts *o, float *out_dev)
{
    CTX_TRY(c);
    static const char fn[] = "mcrt_speckle_frames";
    if (!in_dev || !out_dev) return set_error(MCRT_ERR_INVALID, "%s: null %s", fn, in_dev ? "out_dev" : "in_dev");
    if (n_frames == 0 || height == 0 || width == 0) return set_error(MCRT_ERR_INVALID, "%s: zero sizes (n_frames %u, height %u, width %u)", fn, n_frames, height, width);
    mcrt_speckle_opts d;
    if (!o) { mcrt_default_speckle_opts(&d); o = &d; }
    float q0sq[256], kq[256], lam4 = 0.0f;
    MCRT_TRY(mcrt_speckle_tables(o, q0sq, kq, &lam4));
    if ((double)n_frames * (double)height * (double)width >= 0x1p31) return set_error(MCRT_ERR_LIMIT, "%s: a stack of 2^31 floats or more (%u x %u x %u)", fn, n_frames, height, width);
    const size_t n = (size_t)n_frames * height * width;
    if (in_dev != out_dev && ranges_overlap(in_dev, 4 * n, out_dev, 4 * n)) return set_error(MCRT_ERR_INVALID, "%s: in_dev and out_dev overlap without being the same buffer", fn);
    if (o->n_iter == 0u) {
        if (in_dev != out_dev) HIP_TRY(hipMemcpyAsync(out_dev, in_dev, 4 * n, hipMemcpyDeviceToDevice, c->stream));
        return MCRT_OK;
    }
    const uint32_t T = c->knobs.speckle_fuse, L = (o->n_iter + T - 1u) / T;
    if (L > 1u || in_dev == out_dev) MCRT_TRY(ensure_tmp(c, n));
    float *tmp = c->img.d_tmp;
    const float *src = in_dev;
    if (in_dev == out_dev && (L & 1u)) {
        HIP_TRY(hipMemcpyAsync(tmp, in_dev, 4 * n, hipMemcpyDeviceToDevice, c->stream));
        src = tmp;
    }
    for (uint32_t k = 1; k <= L; k++) {
        mcrt::SpeckleArgs a;
        memset(&a, 0, sizeof a);
        const uint32_t t0 = (k - 1u) * T;
        a.src = src; a.dst = ((L - k) & 1u) ? tmp : out_dev;
        a.H = height; a.W = width; a.n = std::min(T, o->n_iter - t0); a.first = k == 1u ? 1u : 0u; a.lam4 = lam4;
        for (uint32_t s = 0; s < a.n; s++) { a.q0sq[s] = q0sq[t0 + s]; a.kq[s] = kq[t0 + s]; }
        HIP_TRY(mcrt::launch_srad(a, n_frames, T, c->stream));
        src = a.dst;
    }
    return MCRT_OK;
}

// ---- 3-D speckle reduction over voxel blocks (the contract is in include/mcrt.h; the defaults, the weights and the tables are host code: mcrt_host.cpp) ----
// mcrt_speckle_frames' scheme with one iteration per launch: launch k = 1..n_iter writes out_dev when n_iter - k is even and the scratch when
// it is odd; in place with an odd n_iter the stack is first copied into the scratch.
extern "C" int mcrt_speckle_volume_frames(mcrt_ctx *c, const float *in_dev, uint32_t n_frames, uint32_t nu, uint32_t nv, uint32_t nw, const mcrt_speckle3d_opts *o, float *out_dev)
{
    CTX_TRY(c);
    static const char fn[] = "mcrt_speckle_volume_frames";
    if (!in_dev || !out_dev) return set_error(MCRT_ERR_INVALID, "%s: null %s", fn, in_dev ? "out_dev" : "in_dev");
    if (n_frames == 0 || nu == 0 || nv == 0 || nw == 0) return set_error(MCRT_ERR_INVALID, "%s: zero sizes (n_frames %u, nu %u, nv %u, nw %u)", fn, n_frames, nu, nv, nw);
    mcrt_speckle3d_opts d;
    if (!o) { mcrt_default_speckle3d_opts(&d); o = &d; }
    float q0sq[256], kq[256], k[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    MCRT_TRY(mcrt_speckle3d_tables(o, q0sq, kq, k));
    if (nu >= (1u << 24) || nv >= (1u << 24) || nw >= (1u << 24)) return set_error(MCRT_ERR_LIMIT, "%s: nu, nv and nw must be below 2^24 (%u x %u x %u)", fn, nu, nv, nw);
    if ((double)n_frames * (double)nu * (double)nv * (double)nw >= 0x1p31)
        return set_error(MCRT_ERR_LIMIT, "%s: a stack of 2^31 floats or more (%u x %u x %u x %u)", fn, n_frames, nw, nv, nu);
    const size_t n = (size_t)n_frames * nu * nv * nw;
    if (in_dev != out_dev && ranges_overlap(in_dev, 4 * n, out_dev, 4 * n)) return set_error(MCRT_ERR_INVALID, "%s: in_dev and out_dev overlap without being the same buffer", fn);
    if (o->n_iter == 0u) {
        if (in_dev != out_dev) HIP_TRY(hipMemcpyAsync(out_dev, in_dev, 4 * n, hipMemcpyDeviceToDevice, c->stream));
        return MCRT_OK;
    }
    const uint32_t L = o->n_iter;
    if (L > 1u || in_dev == out_dev) MCRT_TRY(ensure_tmp(c, n));
    float *tmp = c->img.d_tmp;
    const float *src = in_dev;
    if (in_dev == out_dev && (L & 1u)) {
        HIP_TRY(hipMemcpyAsync(tmp, in_dev, 4 * n, hipMemcpyDeviceToDevice, c->stream));
        src = tmp;
    }
    for (uint32_t t = 1; t <= L; t++) {
        mcrt::Speckle3Args a;
        memset(&a, 0, sizeof a);
        a.src = src; a.dst = ((L - t) & 1u) ? tmp : out_dev;
        a.nu = nu; a.nv = nv; a.nw = nw; a.first = t == 1u ? 1u : 0u;
        a.wu = o->weight[0]; a.wv = o->weight[1]; a.ww = o->weight[2];
        a.a = k[0]; a.b = k[1]; a.hs = k[2]; a.lamw = k[3];
        a.q0sq = q0sq[t - 1u]; a.kq = kq[t - 1u];
        HIP_TRY(mcrt::launch_srad3(a, n_frames, c->stream));
        src = a.dst;
    }
    return MCRT_OK;
}

// ---- receiver noise (the contract is in include/mcrt.h; the defaults and the host's draws are host code: mcrt_host.cpp) ----
// Everything is checked before anything is enqueued; then the gain table (only when it differs from the one on the device), in SNR_DB
// mode the peaks (memset + k_bmode_peak without TGC, a frame's n_images * E scan-lines as one image: the reduction fits unchanged), and k_noise.
extern "C" int mcrt_noise_frames(mcrt_ctx *c, float *rf_dev, uint32_t n_frames, uint32_t n_images, uint32_t E, uint32_t R, uint32_t first_image_id,
                                 const mcrt_noise_opts *o, const float *element_gain, float *sigma_dev)
{
    CTX_TRY(c);
    static const char fn[] = "mcrt_noise_frames";
    if (!rf_dev) return set_error(MCRT_ERR_INVALID, "%s: null rf_dev", fn);
    if (n_frames == 0 || n_images == 0 || E == 0 || R == 0)
        return set_error(MCRT_ERR_INVALID, "%s: zero sizes (n_frames %u, n_images %u, n_elements %u, n_rows %u)", fn, n_frames, n_images, E, R);
    mcrt_noise_opts d;
    if (!o) { mcrt_default_noise_opts(&d); o = &d; }
    if (o->mode != MCRT_NOISE_SNR_DB && o->mode != MCRT_NOISE_ABS) return set_error(MCRT_ERR_INVALID, "%s: unknown mode %u", fn, o->mode);
    const bool snr = o->mode == MCRT_NOISE_SNR_DB;
    if (snr && !std::isfinite(o->snr_db)) return set_error(MCRT_ERR_INVALID, "%s: snr_db must be finite (%g)", fn, (double)o->snr_db);
    if (!snr && !(std::isfinite(o->sigma) && o->sigma >= 0.0f)) return set_error(MCRT_ERR_INVALID, "%s: sigma must be finite and >= 0 (%g)", fn, (double)o->sigma);
    for (uint32_t e = 0; element_gain && e < E; e++)
        if (!std::isfinite(element_gain[e])) return set_error(MCRT_ERR_INVALID, "%s: element_gain[%u] is not finite", fn, e);
    if (R > MCRT_MAX_ROWS) return set_error(MCRT_ERR_LIMIT, "%s: n_rows: at most %d rows (%u)", fn, MCRT_MAX_ROWS, R);
    const uint64_t images = (uint64_t)n_frames * n_images;
    if (images > 65535ull) return set_error(MCRT_ERR_LIMIT, "%s: n_frames * n_images: at most 65535 images per call (%u x %u)", fn, n_frames, n_images);
    if ((uint64_t)first_image_id + images > 0x100000000ull)
        return set_error(MCRT_ERR_LIMIT, "%s: first_image_id: the ids of %llu images from %u on pass 2^32", fn, (unsigned long long)images, first_image_id);
    if ((double)images * (double)E * (double)R >= 0x1p31)
        return set_error(MCRT_ERR_LIMIT, "%s: a stack of 2^31 samples or more (%u x %u x %u x %u)", fn, n_frames, n_images, E, R);
    if (!snr && o->sigma == 0.0f && !element_gain) {            // the identity: nothing is launched
        if (sigma_dev) HIP_TRY(hipMemsetAsync(sigma_dev, 0, 4 * (size_t)n_frames, c->stream));
        return MCRT_OK;
    }
    if (snr && !c->img.d_disp) HIP_TRY(c->img.d_disp.alloc(65536));   // (the peaks of the largest pass, as mcrt_bmode_frames has them)
    if (element_gain) MCRT_TRY(c->img.gain.put(element_gain, E, 1, E, c->stream));
    mcrt::NoiseArgs a;
    a.rf = rf_dev; a.peak = nullptr; a.gain = element_gain ? c->img.gain.dev.p : nullptr; a.sigma_out = sigma_dev;
    a.N = n_images; a.E = E; a.R = R; a.lines = (uint32_t)images * E; a.chunks = (R + NOISE_WAVE_ROWS - 1u) / NOISE_WAVE_ROWS;
    a.seed = o->seed; a.first_id = first_image_id;
    a.c = snr ? (float)std::pow(10.0, -(double)o->snr_db / 20.0) : o->sigma;
    a.inv_std = (float)(1.0 / std::sqrt(2863311530.0));
    if (snr) {
        a.peak = c->img.d_disp.p;
        HIP_TRY(hipMemsetAsync(c->img.d_disp.p, 0, 4 * (size_t)n_frames, c->stream));
        HIP_TRY(mcrt::launch_bmode_peak(rf_dev, n_frames, n_images * E, R, nullptr, c->img.d_disp.p, c->stream));
    }
    HIP_TRY(mcrt::launch_noise(a, c->stream));
    return MCRT_OK;
}

// ---- automatic gain (the contract is in include/mcrt.h; the defaults, the option ranges and the host's curve are host code: mcrt_host.cpp) ----
// Everything is checked before anything is enqueued.  The histograms [frames][n_bands][2048] are the context's and stay within
// knobs.autogain_hist_words: the pass is walked in chunks of as many frames as fit (a frame has at most 512 bands, so one always does), per
// chunk a clear, k_autogain_hist, k_autogain_curve and, with apply, k_autogain_apply -- frames are independent, so chunks change nothing.
extern "C" int mcrt_autogain_frames(mcrt_ctx *c, float *rf_dev, uint32_t n_frames, uint32_t n_images, uint32_t E, uint32_t R, const mcrt_autogain_opts *o,
                                    const float *floor_dev, float *gain_dev, int32_t *band_bin_dev, uint32_t *pen_dev)
{
    CTX_TRY(c);
    static const char fn[] = "mcrt_autogain_frames";
    if (!rf_dev) return set_error(MCRT_ERR_INVALID, "%s: null rf_dev", fn);
    if (n_frames == 0 || n_images == 0 || E == 0 || R == 0)
        return set_error(MCRT_ERR_INVALID, "%s: zero sizes (n_frames %u, n_images %u, n_elements %u, n_rows %u)", fn, n_frames, n_images, E, R);
    mcrt_autogain_opts d;
    if (!o) { mcrt_default_autogain_opts(&d); o = &d; }
    MCRT_TRY(mcrt::autogain_check(fn, o));
    if (R > MCRT_MAX_ROWS) return set_error(MCRT_ERR_LIMIT, "%s: n_rows: at most %d rows (%u)", fn, MCRT_MAX_ROWS, R);
    const uint64_t images = (uint64_t)n_frames * n_images;
    if (images > 65535ull) return set_error(MCRT_ERR_LIMIT, "%s: n_frames * n_images: at most 65535 images per call (%u x %u)", fn, n_frames, n_images);
    if ((double)images * (double)E * (double)R >= 0x1p31)
        return set_error(MCRT_ERR_LIMIT, "%s: a stack of 2^31 samples or more (%u x %u x %u x %u)", fn, n_frames, n_images, E, R);
    const uint32_t lines = n_images * E, nB = (R + o->band_rows - 1u) / o->band_rows;
    const size_t band_words = (size_t)nB * AUTOGAIN_BINS;
    const uint32_t chunk = (uint32_t)std::min<size_t>(n_frames, std::max<size_t>(1u, c->knobs.autogain_hist_words / band_words));
    HIP_TRY(c->img.d_aghist.grow((size_t)chunk * band_words));
    if (!gain_dev) HIP_TRY(c->img.d_aggain.grow((size_t)n_frames * R));
    mcrt::AutogainArgs a;
    a.hist = c->img.d_aghist.p;
    a.lines = lines; a.R = R; a.band_rows = o->band_rows; a.n_bands = nB;
    a.shares = (uint32_t)std::min<uint64_t>(lines, std::max<uint64_t>(1u, ((uint64_t)lines * std::min(o->band_rows, R) + AUTOGAIN_WG_SAMPLES - 1u) / AUTOGAIN_WG_SAMPLES));
    a.min_permille = o->min_permille; a.floor = o->floor; a.floor_scale = o->floor_scale; a.max_gain = o->max_gain; a.inv_max_gain = 1.0f / o->max_gain;
    a.chunks = (R + NOISE_WAVE_ROWS - 1u) / NOISE_WAVE_ROWS;
    float *gain = gain_dev ? gain_dev : c->img.d_aggain.p;
    for (uint32_t f0 = 0; f0 < n_frames; f0 += chunk) {
        const uint32_t F = std::min(chunk, n_frames - f0);
        a.rf = rf_dev + (size_t)f0 * lines * R;
        a.floor_dev = floor_dev ? floor_dev + f0 : nullptr;
        a.gain = gain + (size_t)f0 * R;
        a.band_bin = band_bin_dev ? band_bin_dev + (size_t)f0 * nB : nullptr;
        a.pen = pen_dev ? pen_dev + f0 : nullptr;
        HIP_TRY(hipMemsetAsync(a.hist, 0, 4 * (size_t)F * band_words, c->stream));
        HIP_TRY(mcrt::launch_autogain_hist(a, F, c->knobs.autogain_copies, c->stream));
        HIP_TRY(mcrt::launch_autogain_curve(a, F, c->stream));
        if (o->apply) HIP_TRY(mcrt::launch_autogain_apply(a, F, c->stream));
    }
    return MCRT_OK;
}

// ---- freehand 3-D reconstruction (the contracts are in include/mcrt.h; the defaults and the transform are host code: mcrt_host.cpp) ----
// What mcrt_recon_frames and mcrt_recon_label_frames ask and do alike, in parts as the view checks are: each call has option checks of its own between them, and
// which fault of several a call reports is part of its behaviour.  The argument errors, the fill options, the block, the limits, and what is enqueued first.
static int recon_invalid(const char *fn, uint32_t n_frames, uint32_t E, uint32_t R, double row_mm, double unit_mm)
{
    if (n_frames == 0 || E == 0 || R == 0) return set_error(MCRT_ERR_INVALID, "%s: zero sizes (n_frames %u, n_elements %u, n_rows %u)", fn, n_frames, E, R);
    if (!(std::isfinite(row_mm) && row_mm > 0.0)) return set_error(MCRT_ERR_INVALID, "%s: row_mm must be finite and > 0 (%g)", fn, row_mm);
    if (!(std::isfinite(unit_mm) && unit_mm > 0.0)) return set_error(MCRT_ERR_INVALID, "%s: unit_mm must be finite and > 0 (%g)", fn, unit_mm);
    return MCRT_OK;
}
static int recon_fill_invalid(const char *fn, uint32_t fill_radius, uint32_t fill_min)
{
    if (fill_radius > RECON_MAX_FILL) return set_error(MCRT_ERR_INVALID, "%s: fill_radius must be 0..%d (%u)", fn, RECON_MAX_FILL, fill_radius);
    return fill_min == 0u ? set_error(MCRT_ERR_INVALID, "%s: fill_min must be >= 1", fn) : MCRT_OK;
}
// the one place that fills a ReconBlock: the grid's transform (which refuses a grid itself), row_u (the caller says what it says when that is no finite float), the
// rest as the caller has it.  The limits follow: n_samples is checked before it is used, and pos / dir may still be host tables (recon_begin)
static int recon_block(mcrt::ReconBlock &k, uint32_t n_frames, uint32_t E, uint32_t R, const float *pos, const float *dir, double row_mm, double unit_mm, const mcrt_volume_grid *g,
                       uint32_t fill_radius, uint32_t fill_min, uint32_t *stats_dev)
{
    MCRT_TRY(mcrt_recon_transform(g, unit_mm, k.A, k.b));
    k.row_u = (float)(row_mm / unit_mm); k.pos = pos; k.dir = dir; k.stats = stats_dev;
    k.R = R; k.n_samples = (uint32_t)((size_t)n_frames * E * R); k.nu = g->nu; k.nv = g->nv; k.nw = g->nw; k.fill_radius = fill_radius; k.fill_min = fill_min;
    return MCRT_OK;
}
static int recon_limits(const char *fn, uint32_t n_frames, uint32_t E, uint32_t R, const mcrt_volume_grid *g, uint32_t fill_radius)
{
    if (R > MCRT_MAX_ROWS) return set_error(MCRT_ERR_LIMIT, "%s: at most %d rows (%u)", fn, MCRT_MAX_ROWS, R);
    if (n_frames > 65535u) return set_error(MCRT_ERR_LIMIT, "%s: at most 65535 frames per call (%u)", fn, n_frames);
    if ((double)n_frames * (double)E * (double)R >= 0x1p31) return set_error(MCRT_ERR_LIMIT, "%s: a stack of 2^31 samples or more (%u x %u x %u)", fn, n_frames, E, R);
    if ((double)g->nu * (double)g->nv * (double)g->nw >= 0x1p31) return set_error(MCRT_ERR_LIMIT, "%s: grid: 2^31 voxels or more (%u x %u x %u)", fn, g->nu, g->nv, g->nw);
    mcrt::ReconTiling t;
    if (!mcrt::recon_tiling(g->nu, g->nv, g->nw, fill_radius, t))        // (the radius was looked at before)
        return set_error(MCRT_ERR_LIMIT, "%s: grid: 2^24 tiles of %d x %d x %d voxels or more (%u x %u x %u): too thin a block", fn, RECON_TU, RECON_TV, RECON_TW, g->nu, g->nv, g->nw);
    return MCRT_OK;
}
// after the last check, what both calls enqueue first: the call's scratch grown to `words` (after a stream synchronise: an earlier call may still be using it), host pose
// tables through the context's pose staging (as mcrt_trace_frames_poses stages them), one clear of the scratch and one of stats_dev
template <class T> static int recon_begin(mcrt_ctx *c, mcrt::ReconBlock &k, uint32_t n_frames, uint32_t E, Buf<T> &scratch, size_t words)
{
    if (words > scratch.cap) { HIP_TRY(hipStreamSynchronize(c->stream)); HIP_TRY(scratch.alloc(words)); }
    const float *tab[2] = { k.pos, k.dir };
    MCRT_TRY(mcrt::stage_poses(c, (size_t)n_frames * E, tab));
    k.pos = tab[0]; k.dir = tab[1];
    HIP_TRY(hipMemsetAsync(scratch, 0, sizeof(T) * words, c->stream));
    if (k.stats) HIP_TRY(hipMemsetAsync(k.stats, 0, 8, c->stream));
    return MCRT_OK;
}

// Everything is checked before anything is launched.  Then, on the context's stream: recon_begin, k_recon_splat, k_recon_resolve.
extern "C" int mcrt_recon_frames(mcrt_ctx *c, const float *stack_dev, uint32_t n_frames, uint32_t E, uint32_t R, const float *pos, const float *dir,
                                 double row_mm, double unit_mm, const mcrt_volume_grid *g, const mcrt_recon_opts *o, float *out_dev, uint32_t *count_dev,
                                 uint32_t *stats_dev)
{
    CTX_TRY(c);
    static const char fn[] = "mcrt_recon_frames";
    if (!stack_dev || !pos || !dir || !g || !out_dev)
        return set_error(MCRT_ERR_INVALID, "%s: null %s", fn, !stack_dev ? "stack_dev" : !pos ? "pos" : !dir ? "dir" : !g ? "grid" : "out_dev");
    MCRT_TRY(recon_invalid(fn, n_frames, E, R, row_mm, unit_mm));
    mcrt_recon_opts d;
    if (!o) { mcrt_default_recon_opts(&d); o = &d; }
    if (o->mode != MCRT_RECON_MEAN && o->mode != MCRT_RECON_MAX) return set_error(MCRT_ERR_INVALID, "%s: unknown mode %u", fn, o->mode);
    if (!(std::isfinite(o->value_max) && o->value_max > 0.0f)) return set_error(MCRT_ERR_INVALID, "%s: value_max must be finite and > 0 (%g)", fn, (double)o->value_max);
    MCRT_TRY(recon_fill_invalid(fn, o->fill_radius, o->fill_min));
    if (!std::isfinite(o->empty)) return set_error(MCRT_ERR_INVALID, "%s: empty must be finite", fn);
    mcrt::ReconArgs a;
    memset(&a, 0, sizeof a);
    MCRT_TRY(recon_block(a.blk, n_frames, E, R, pos, dir, row_mm, unit_mm, g, o->fill_radius, o->fill_min, stats_dev));
    a.qscale = 0x1p31 / (double)o->value_max;
    if (!(std::isfinite(a.blk.row_u) && std::isfinite(a.qscale))) return set_error(MCRT_ERR_INVALID, "%s: row_mm / unit_mm or 2^31 / value_max is not finite (%g, %g)", fn, (double)a.blk.row_u, a.qscale);
    MCRT_TRY(recon_limits(fn, n_frames, E, R, g, o->fill_radius));
    const size_t ns = (size_t)n_frames * E * R, n = (size_t)g->nu * g->nv * g->nw;
    const Range outs[3] = { { out_dev, 4 * n, "out_dev" }, { count_dev, 4 * n, "count_dev" }, { stats_dev, 8, "stats_dev" } };
    MCRT_TRY(check_overlap(fn, Range{ stack_dev, 4 * ns, "stack_dev" }, outs, 3, true));
    const size_t words = n + (n + 1u) / 2u;               // n sums, then n counts
    MCRT_TRY(recon_begin(c, a.blk, n_frames, E, c->img.d_recon, words));
    a.stack = stack_dev; a.sum = c->img.d_recon; a.count = (uint32_t *)(c->img.d_recon.p + n); a.out = out_dev; a.count_out = count_dev;
    a.mode = o->mode; a.value_max = o->value_max; a.empty = o->empty;
    HIP_TRY(mcrt::launch_recon_splat(a, c->stream));
    HIP_TRY(mcrt::launch_recon_resolve(a, c->stream));
    return MCRT_OK;
}

// a freehand label volume by majority vote: mcrt_recon_frames' checks with the tissue stack in the float stack's place; then recon_begin,
// k_recon_label_splat, k_recon_label_resolve
extern "C" int mcrt_recon_label_frames(mcrt_ctx *c, const uint8_t *stack_dev, uint32_t n_frames, uint32_t E, uint32_t R, const float *pos, const float *dir,
                                       double row_mm, double unit_mm, const mcrt_volume_grid *g, const mcrt_recon_label_opts *o, uint8_t *out_dev,
                                       uint32_t *count_dev, uint32_t *votes_dev, uint32_t *stats_dev)
{
    CTX_TRY(c);
    static const char fn[] = "mcrt_recon_label_frames";
    if (!stack_dev || !pos || !dir || !g || !o)
        return set_error(MCRT_ERR_INVALID, "%s: null %s", fn, !stack_dev ? "stack_dev" : !pos ? "pos" : !dir ? "dir" : !g ? "grid" : "options");
    if (!out_dev && !count_dev && !votes_dev && !stats_dev) return set_error(MCRT_ERR_INVALID, "%s: out_dev, count_dev, votes_dev and stats_dev are all null", fn);
    MCRT_TRY(recon_invalid(fn, n_frames, E, R, row_mm, unit_mm));
    if (o->n_labels == 0u || o->n_labels > 254u) return set_error(MCRT_ERR_INVALID, "%s: n_labels must be 1..254 (%u)", fn, o->n_labels);
    MCRT_TRY(recon_fill_invalid(fn, o->fill_radius, o->fill_min));
    mcrt::ReconLabelArgs a;
    memset(&a, 0, sizeof a);
    MCRT_TRY(recon_block(a.blk, n_frames, E, R, pos, dir, row_mm, unit_mm, g, o->fill_radius, o->fill_min, stats_dev));
    if (!std::isfinite(a.blk.row_u)) return set_error(MCRT_ERR_INVALID, "%s: row_mm / unit_mm is not finite (%g)", fn, (double)a.blk.row_u);
    MCRT_TRY(recon_limits(fn, n_frames, E, R, g, o->fill_radius));
    const size_t ns = (size_t)n_frames * E * R, n = (size_t)g->nu * g->nv * g->nw, words = n * o->n_labels;
    if (words >= 0x80000000ull) return set_error(MCRT_ERR_LIMIT, "%s: a vote table of 2^31 words or more (%u x %u x %u voxels x %u labels)", fn, g->nu, g->nv, g->nw, o->n_labels);
    const Range outs[4] = { { out_dev, n, "out_dev" }, { count_dev, 4 * n, "count_dev" }, { votes_dev, 4 * n, "votes_dev" }, { stats_dev, 8, "stats_dev" } };
    MCRT_TRY(check_overlap(fn, Range{ stack_dev, ns, "stack_dev" }, outs, 4, true));
    MCRT_TRY(recon_begin(c, a.blk, n_frames, E, c->img.d_votes, words));
    a.stack = stack_dev; a.votes = c->img.d_votes; a.out = out_dev; a.count_out = count_dev; a.votes_out = votes_dev;
    a.n_vox = (uint32_t)n; a.n_labels = o->n_labels;
    HIP_TRY(mcrt::launch_recon_label_splat(a, c->stream));
    if (out_dev || count_dev || votes_dev) HIP_TRY(mcrt::launch_recon_label_resolve(a, c->stream));
    return MCRT_OK;
}

// ---- labels as pictures (the contracts are in include/mcrt.h): nearest-neighbour gathers through the float calls' own cached maps ----
static mcrt::LabelGatherArgs label_gather_args(const uint8_t *src, const float *plane, const float *col, const float *row, uint8_t *out, uint32_t n_frames, uint32_t E, uint32_t R,
                                               uint32_t K, uint32_t n)
{
    mcrt::LabelGatherArgs a;
    a.src = src; a.map_plane = plane; a.map_col = col; a.map_row = row; a.out = out; a.E = E; a.R = R; a.K = K; a.pass = pixel_pass(n_frames, n, 0.0f, out, 1u);
    return a;
}

extern "C" int mcrt_label_scan_convert_frames(mcrt_ctx *c, const uint8_t *tissue_dev, uint32_t n_frames, uint32_t E, uint32_t R, double radius_mm, double total_angle,
                                              uint8_t *out_dev, uint32_t orows, uint32_t ocols)
{
    CTX_TRY(c);
    static const char fn[] = "mcrt_label_scan_convert_frames";
    if (!tissue_dev || !out_dev || E == 0 || R == 0 || orows == 0 || ocols == 0 || n_frames == 0) return set_error(MCRT_ERR_INVALID, "%s: bad arguments", fn);
    if (n_frames > 65535u) return set_error(MCRT_ERR_LIMIT, "%s: at most 65535 images per call", fn);
    if ((uint64_t)orows * ocols > 0x7ffffffcull) return set_error(MCRT_ERR_LIMIT, "%s: output image too large", fn);
    const uint32_t n = orows * ocols;
    if (ranges_overlap(tissue_dev, (size_t)n_frames * E * R, out_dev, (size_t)n_frames * n)) return set_error(MCRT_ERR_INVALID, "%s: tissue_dev and out_dev overlap", fn);
    const float *maps = nullptr;
    MCRT_TRY(ensure_maps(c, c->img.maps, E, R, radius_mm, total_angle, orows, ocols, nullptr, &maps));
    HIP_TRY(mcrt::launch_label_gather(label_gather_args(tissue_dev, nullptr, maps, maps + MapCache::pad(n), out_dev, n_frames, E, R, 1u, n), c->stream));
    return MCRT_OK;
}

extern "C" int mcrt_label_volume_frames(mcrt_ctx *c, const uint8_t *tissue_dev, uint32_t n_frames, uint32_t E, uint32_t R, double radius_mm, double total_angle,
                                        const mcrt_sweep *sw, const mcrt_volume_grid *g, uint8_t *out_dev)
{
    CTX_TRY(c);
    static const char fn[] = "mcrt_label_volume_frames";
    if (!tissue_dev || !out_dev) return set_error(MCRT_ERR_INVALID, "%s: null %s", fn, tissue_dev ? "out_dev" : "tissue_dev");
    MCRT_TRY(volume_args_check(fn, n_frames, E, R, total_angle, sw, g));
    const uint32_t K = sw->n_planes, n = g->nu * g->nv * g->nw;
    if (ranges_overlap(tissue_dev, (size_t)n_frames * K * E * R, out_dev, (size_t)n_frames * n)) return set_error(MCRT_ERR_INVALID, "%s: tissue_dev and out_dev overlap", fn);
    const float *maps = nullptr;
    MCRT_TRY(ensure_volume_maps(c, E, R, radius_mm, total_angle, sw, g, &maps));
    const size_t n_pad = MapCache::pad(n);
    HIP_TRY(mcrt::launch_label_gather(label_gather_args(tissue_dev, maps, maps + n_pad, maps + 2 * n_pad, out_dev, n_frames, E, R, K, n), c->stream));
    return MCRT_OK;
}

extern "C" int mcrt_export_rf(mcrt_ctx *c, const float *rf_dev, uint32_t E, uint32_t R, float *host)
{
    CTX_TRY(c);
    if (!rf_dev || !host || E == 0 || R == 0) return set_error(MCRT_ERR_INVALID, "mcrt_export_rf: bad arguments");
    MCRT_TRY(ensure_tmp(c, (size_t)E * R));
    HIP_TRY(mcrt::launch_transpose(rf_dev, c->img.d_tmp, E, R, c->stream));
    HIP_TRY(hipMemcpyAsync(host, c->img.d_tmp, (size_t)E * R * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MCRT_OK;
}

extern "C" int mcrt_import_rf(mcrt_ctx *c, const float *host, uint32_t E, uint32_t R, float *rf_dev)
{
    CTX_TRY(c);
    if (!rf_dev || !host || E == 0 || R == 0) return set_error(MCRT_ERR_INVALID, "mcrt_import_rf: bad arguments");
    MCRT_TRY(ensure_tmp(c, (size_t)E * R));
    HIP_TRY(hipMemcpyAsync(c->img.d_tmp, host, (size_t)E * R * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(mcrt::launch_transpose(c->img.d_tmp, rf_dev, R, E, c->stream));          // [R][E] -> [E][R]
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MCRT_OK;
}
