"""ctypes view of include/mcrt.h."""
import ctypes as C
import os
import subprocess
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.environ.get("MCRT_LIB") or os.path.join(_HERE, "libmcrt_hip.so")   # MCRT_LIB: tuning builds only
_LIB = None


class McrtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"mcrt error {code}: {msg}")
        self.code = code


class Params(C.Structure):
    _fields_ = [("n_elements", C.c_uint32), ("n_samples", C.c_uint32), ("max_depth", C.c_uint32), ("n_rows", C.c_uint32),
                ("frequency", C.c_float), ("intensity_epsilon", C.c_float), ("initial_intensity", C.c_float),
                ("ray_start_offset", C.c_float), ("speed_of_sound", C.c_uint32), ("depth_cm", C.c_double),
                ("seed", C.c_uint32), ("sanitize_tir", C.c_uint32), ("tex_n", C.c_uint32), ("tex_res", C.c_float)]


class MeshRec(C.Structure):
    _fields_ = [("mat_inside", C.c_uint32), ("mat_outside", C.c_uint32), ("vascular", C.c_uint32), ("_pad", C.c_uint32)]


class BvhNode(C.Structure):
    _fields_ = [("lo0", C.c_float * 3), ("c0", C.c_int32), ("hi0", C.c_float * 3), ("c1", C.c_int32),
                ("lo1", C.c_float * 3), ("pad0", C.c_uint32), ("hi1", C.c_float * 3), ("pad1", C.c_uint32)]


class Bvh(C.Structure):
    _fields_ = [("n_nodes", C.c_uint32), ("n_tri", C.c_uint32), ("max_depth", C.c_uint32), ("pad_abs", C.c_float),
                ("nodes", C.c_void_p), ("tri", C.c_void_p)]


class Bvh4(C.Structure):
    _fields_ = [("n_nodes", C.c_uint32), ("max_stack", C.c_uint32), ("nodes", C.c_void_p)]


class Stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("queries", "nodes_visited", "tris_tested", "segments", "rf_steps", "hits")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class BmodeParams(C.Structure):
    """mcrt_bmode_params (include/mcrt.h): 48 bytes, the doubles at offsets 32 and 40"""
    _fields_ = [("mode", C.c_uint32), ("dynamic_range_db", C.c_float), ("gain_db", C.c_float), ("ref", C.c_float), ("persistence", C.c_float),
                ("reset_state", C.c_uint32), ("out_rows", C.c_uint32), ("out_cols", C.c_uint32), ("radius_mm", C.c_double), ("total_angle_rad", C.c_double)]


class Focus(C.Structure):
    """mcrt_focus (include/mcrt.h): 40 bytes, focus_mm at offset 4, focal_range_mm at 36"""
    _fields_ = [("n_focus", C.c_uint32), ("focus_mm", C.c_float * 8), ("focal_range_mm", C.c_float)]


class Bands(C.Structure):
    """mcrt_bands (include/mcrt.h): 80 bytes, band_mhz at offset 4, band_weight at 36, var_x at 68, downshift_mhz_per_mm at 72, min_mhz at 76"""
    _fields_ = [("n_bands", C.c_uint32), ("band_mhz", C.c_float * 8), ("band_weight", C.c_float * 8), ("var_x", C.c_float),
                ("downshift_mhz_per_mm", C.c_float), ("min_mhz", C.c_float)]


class DetectOpts(C.Structure):
    """mcrt_detect_opts (include/mcrt.h): 4 bytes"""
    _fields_ = [("n_taps", C.c_uint32)]


class FlowOpts(C.Structure):
    """mcrt_flow_opts (include/mcrt.h): 32 bytes"""
    _fields_ = [("n_packets", C.c_uint32), ("wall", C.c_uint32), ("avg_rows", C.c_uint32), ("avg_lines", C.c_uint32), ("prf_hz", C.c_float),
                ("freq_mhz", C.c_float), ("sigma", C.c_float), ("seed", C.c_uint32)]


class ColourOpts(C.Structure):
    """mcrt_colour_opts (include/mcrt.h): 12 bytes"""
    _fields_ = [("power_thr", C.c_float), ("vel_thr_mm_s", C.c_float), ("grey_max", C.c_uint32)]


class SpectralOpts(C.Structure):
    """mcrt_spectral_opts (include/mcrt.h): 32 bytes"""
    _fields_ = [("n_pulses", C.c_uint32), ("gate_rows", C.c_uint32), ("n_fft", C.c_uint32), ("hop", C.c_uint32), ("wall", C.c_uint32),
                ("wall_bins", C.c_uint32), ("sigma", C.c_float), ("seed", C.c_uint32)]


class Gate(C.Structure):
    """mcrt_gate (include/mcrt.h): 12 bytes"""
    _fields_ = [("image", C.c_uint32), ("line", C.c_uint32), ("row0", C.c_uint32)]


class SonogramOpts(C.Structure):
    """mcrt_sonogram_opts (include/mcrt.h): 12 bytes"""
    _fields_ = [("dynamic_range_db", C.c_float), ("gain_db", C.c_float), ("ref", C.c_float)]


class StrainOpts(C.Structure):
    """mcrt_strain_opts (include/mcrt.h): 20 bytes"""
    _fields_ = [("window_rows", C.c_uint32), ("search_rows", C.c_uint32), ("lsq_rows", C.c_uint32), ("sigma", C.c_float), ("seed", C.c_uint32)]


class ShearOpts(C.Structure):
    """mcrt_shear_opts (include/mcrt.h): 48 bytes"""
    _fields_ = [("n_pulses", C.c_uint32), ("window_rows", C.c_uint32), ("prf_hz", C.c_float), ("sigma", C.c_float), ("seed", C.c_uint32), ("push_line", C.c_uint32),
                ("push_row0", C.c_uint32), ("push_rows", C.c_uint32), ("peak_q24", C.c_int32), ("speed_lines", C.c_uint32), ("avg_rows", C.c_uint32), ("density", C.c_float)]


class Mline(C.Structure):
    """mcrt_mline (include/mcrt.h): 8 bytes"""
    _fields_ = [("image", C.c_uint32), ("line", C.c_uint32)]


class MmodeOpts(C.Structure):
    """mcrt_mmode_opts (include/mcrt.h): 12 bytes"""
    _fields_ = [("n_pulses", C.c_uint32), ("sigma", C.c_float), ("seed", C.c_uint32)]


class MmodeDisplayOpts(C.Structure):
    """mcrt_mmode_display_opts (include/mcrt.h): 28 bytes"""
    _fields_ = [("hop", C.c_uint32), ("height", C.c_uint32), ("row_lo", C.c_uint32), ("row_hi", C.c_uint32), ("dynamic_range_db", C.c_float),
                ("gain_db", C.c_float), ("ref", C.c_float)]


class ElastogramOpts(C.Structure):
    """mcrt_elastogram_opts (include/mcrt.h): 16 bytes"""
    _fields_ = [("ref_strain", C.c_float), ("rho_min", C.c_float), ("grey_min", C.c_uint32), ("alpha", C.c_uint32)]


class Compound(C.Structure):
    """mcrt_compound (include/mcrt.h): 68 bytes, steer_rad at offset 4"""
    _fields_ = [("n_views", C.c_uint32), ("steer_rad", C.c_float * 16)]


class CompoundOpts(C.Structure):
    """mcrt_compound_opts (include/mcrt.h): 72 bytes, feather_lines at offset 4, view_weight at 8"""
    _fields_ = [("mode", C.c_uint32), ("feather_lines", C.c_float), ("view_weight", C.c_float * 16)]


class Sweep(C.Structure):
    """mcrt_sweep (include/mcrt.h): 12 bytes"""
    _fields_ = [("n_planes", C.c_uint32), ("step_rad", C.c_float), ("pivot_mm", C.c_float)]


class VolumeGrid(C.Structure):
    """mcrt_volume_grid (include/mcrt.h): 112 bytes, du_mm at 24, dv_mm at 48, dw_mm at 72, nu at 96"""
    _fields_ = [("origin_mm", C.c_double * 3), ("du_mm", C.c_double * 3), ("dv_mm", C.c_double * 3), ("dw_mm", C.c_double * 3),
                ("nu", C.c_uint32), ("nv", C.c_uint32), ("nw", C.c_uint32), ("_pad", C.c_uint32)]


class LabelOpts(C.Structure):
    """mcrt_label_opts (include/mcrt.h): 8 bytes, start_offset at offset 4"""
    _fields_ = [("rule", C.c_uint32), ("start_offset", C.c_float)]


class TransmitOpts(C.Structure):
    """mcrt_transmit_opts (include/mcrt.h): 12 bytes"""
    _fields_ = [("mode", C.c_uint32), ("rule", C.c_uint32), ("start_offset", C.c_float)]


class RenderView(C.Structure):
    """mcrt_render_view (include/mcrt.h): 64 bytes, di at 12, dj at 24, ds at 36, nx at 48"""
    _fields_ = [("origin", C.c_float * 3), ("di", C.c_float * 3), ("dj", C.c_float * 3), ("ds", C.c_float * 3),
                ("nx", C.c_uint32), ("ny", C.c_uint32), ("n_steps", C.c_uint32), ("_pad", C.c_uint32)]


class RenderOpts(C.Structure):
    """mcrt_render_opts (include/mcrt.h): 32 bytes"""
    _fields_ = [("mode", C.c_uint32), ("lo", C.c_float), ("hi", C.c_float), ("threshold", C.c_float), ("ramp", C.c_float), ("opacity", C.c_float),
                ("depth_cue", C.c_float), ("t_cut", C.c_float)]


class SpeckleOpts(C.Structure):
    """mcrt_speckle_opts (include/mcrt.h): 16 bytes"""
    _fields_ = [("n_iter", C.c_uint32), ("q0", C.c_float), ("rho", C.c_float), ("lambda_", C.c_float)]


class Speckle3dOpts(C.Structure):
    """mcrt_speckle3d_opts (include/mcrt.h): 28 bytes"""
    _fields_ = [("n_iter", C.c_uint32), ("q0", C.c_float), ("rho", C.c_float), ("lambda_", C.c_float), ("weight", C.c_float * 3)]


class ReconOpts(C.Structure):
    """mcrt_recon_opts (include/mcrt.h): 20 bytes"""
    _fields_ = [("mode", C.c_uint32), ("value_max", C.c_float), ("fill_radius", C.c_uint32), ("fill_min", C.c_uint32), ("empty", C.c_float)]


class ReconLabelOpts(C.Structure):
    """mcrt_recon_label_opts (include/mcrt.h): 12 bytes"""
    _fields_ = [("n_labels", C.c_uint32), ("fill_radius", C.c_uint32), ("fill_min", C.c_uint32)]


class NoiseOpts(C.Structure):
    """mcrt_noise_opts (include/mcrt.h): 16 bytes"""
    _fields_ = [("mode", C.c_uint32), ("snr_db", C.c_float), ("sigma", C.c_float), ("seed", C.c_uint32)]


class AutogainOpts(C.Structure):
    """mcrt_autogain_opts (include/mcrt.h): 24 bytes"""
    _fields_ = [("band_rows", C.c_uint32), ("min_permille", C.c_uint32), ("floor", C.c_float), ("floor_scale", C.c_float), ("max_gain", C.c_float),
                ("apply", C.c_uint32)]


NODE_DTYPE = np.dtype([("lo0", "<f4", 3), ("c0", "<i4"), ("hi0", "<f4", 3), ("c1", "<i4"),
                       ("lo1", "<f4", 3), ("pad0", "<u4"), ("hi1", "<f4", 3), ("pad1", "<u4")])
SEGMENT_DTYPE = np.dtype([("from", "<f4", 3), ("to", "<f4", 3), ("dir", "<f4", 3),
                          ("reflected_intensity", "<f4"), ("initial_intensity", "<f4"), ("attenuation", "<f4"),
                          ("distance_traveled", "<f8"), ("media", "<i4"), ("tri", "<i4")])
assert NODE_DTYPE.itemsize == 64 and SEGMENT_DTYPE.itemsize == 64 and C.sizeof(BvhNode) == 64 and C.sizeof(BmodeParams) == 48 and C.sizeof(Focus) == 40 and C.sizeof(Compound) == 68 and C.sizeof(CompoundOpts) == 72
assert C.sizeof(Sweep) == 12 and C.sizeof(VolumeGrid) == 112 and C.sizeof(LabelOpts) == 8 and C.sizeof(RenderView) == 64 and C.sizeof(RenderOpts) == 32 and C.sizeof(SpeckleOpts) == 16 and C.sizeof(NoiseOpts) == 16 and C.sizeof(ReconOpts) == 20
assert C.sizeof(ReconLabelOpts) == 12 and C.sizeof(AutogainOpts) == 24 and C.sizeof(TransmitOpts) == 12 and C.sizeof(Speckle3dOpts) == 28 and Speckle3dOpts.weight.offset == 16
assert C.sizeof(Bands) == 80 and Bands.band_weight.offset == 36 and Bands.var_x.offset == 68 and Bands.min_mhz.offset == 76 and C.sizeof(DetectOpts) == 4
assert C.sizeof(FlowOpts) == 32 and FlowOpts.prf_hz.offset == 16 and FlowOpts.seed.offset == 28 and C.sizeof(ColourOpts) == 12
assert C.sizeof(SpectralOpts) == 32 and SpectralOpts.sigma.offset == 24 and C.sizeof(Gate) == 12 and C.sizeof(SonogramOpts) == 12
assert C.sizeof(StrainOpts) == 20 and StrainOpts.sigma.offset == 12 and C.sizeof(ElastogramOpts) == 16 and ElastogramOpts.grey_min.offset == 8
assert C.sizeof(ShearOpts) == 48 and ShearOpts.sigma.offset == 12 and ShearOpts.peak_q24.offset == 32 and ShearOpts.density.offset == 44
assert C.sizeof(Mline) == 8 and C.sizeof(MmodeOpts) == 12 and MmodeOpts.seed.offset == 8 and C.sizeof(MmodeDisplayOpts) == 28 and MmodeDisplayOpts.dynamic_range_db.offset == 16

# every symbol include/mcrt.h declares (tests/test_abi.py checks the .so exports each one)
SYMBOLS = ["mcrt_last_error", "mcrt_version", "mcrt_device_count", "mcrt_create", "mcrt_destroy", "mcrt_set_stream",
           "mcrt_synchronize", "mcrt_default_params", "mcrt_set_params", "mcrt_get_params", "mcrt_import_rf", "mcrt_set_bvh_builder", "mcrt_upload_scene", "mcrt_update_triangles", "mcrt_refit_triangles", "mcrt_upload_texture",
           "mcrt_set_transducer", "mcrt_trace_frame", "mcrt_trace_frames", "mcrt_trace_frames_poses", "mcrt_envelope_frames", "mcrt_scan_convert_frames", "mcrt_trace_frame_debug", "mcrt_cast_rays", "mcrt_convolve", "mcrt_convolve_frames", "mcrt_convolve_frames_depth",
           "mcrt_envelope", "mcrt_scan_convert", "mcrt_default_bmode", "mcrt_bmode_frames", "mcrt_export_rf", "mcrt_alloc", "mcrt_free", "mcrt_memcpy_d2h",
           "mcrt_memcpy_h2d", "mcrt_enable_stats", "mcrt_get_stats", "mcrt_enable_timing", "mcrt_get_kernel_time", "mcrt_get_kernel_times",
           "mcrt_build_bvh", "mcrt_free_bvh", "mcrt_get_bvh", "mcrt_build_bvh4", "mcrt_free_bvh4", "mcrt_get_bvh4", "mcrt_row_thresholds", "mcrt_generate_texture", "mcrt_psf_kernels", "mcrt_psf_focus_kernels",
           "mcrt_transducer_elements", "mcrt_transducer_elevation_axis", "mcrt_elevation_planes", "mcrt_psf_elevation_kernels", "mcrt_elevation_frames", "mcrt_debug_math", "mcrt_debug_philox", "mcrt_debug_stamps", "mcrt_debug_tail_histograms", "mcrt_debug_set_error", "mcrt_debug_fast_paths", "mcrt_debug_beam", "mcrt_debug_beam_bounce", "mcrt_debug_beam_order", "mcrt_debug_beam_layout", "mcrt_debug_beam_scan", "mcrt_debug_beam_records", "mcrt_debug_beam_entries", "mcrt_scan_maps",
           "mcrt_group_create", "mcrt_group_destroy", "mcrt_group_size", "mcrt_group_root", "mcrt_group_member", "mcrt_group_shard", "mcrt_group_set_params",
           "mcrt_group_set_bvh_builder", "mcrt_group_upload_scene", "mcrt_group_update_triangles", "mcrt_group_refit_triangles", "mcrt_group_upload_texture",
           "mcrt_group_set_transducer", "mcrt_group_trace_frames", "mcrt_group_trace_frames_poses", "mcrt_group_synchronize", "mcrt_group_last_pass_ms", "mcrt_group_last_scene_seconds",
           "mcrt_transducer_steered", "mcrt_compound_maps", "mcrt_compound_frames", "mcrt_bmode_compound_frames",
           "mcrt_default_compound_opts", "mcrt_compound_weights", "mcrt_compound_frames_opts", "mcrt_bmode_compound_frames_opts",
           "mcrt_transducer_swept", "mcrt_volume_maps", "mcrt_volume_frames", "mcrt_bmode_volume_frames",
           "mcrt_default_label_opts", "mcrt_label_frames", "mcrt_label_scan_convert_frames", "mcrt_label_volume_frames",
           "mcrt_default_transmit_opts", "mcrt_transmit_boundary", "mcrt_transmit_frames",
           "mcrt_default_render_opts", "mcrt_render_view_for_grid", "mcrt_render_frames",
           "mcrt_default_speckle_opts", "mcrt_speckle_tables", "mcrt_speckle_frames",
           "mcrt_default_speckle3d_opts", "mcrt_speckle3d_weights", "mcrt_speckle3d_tables", "mcrt_speckle_volume_frames",
           "mcrt_default_noise_opts", "mcrt_noise_draws", "mcrt_noise_frames",
           "mcrt_default_autogain_opts", "mcrt_autogain_curve", "mcrt_autogain_frames",
           "mcrt_default_bands", "mcrt_psf_band_kernels", "mcrt_convolve_bands_frames", "mcrt_band_fold_frames",
           "mcrt_default_detect_opts", "mcrt_detect_taps", "mcrt_detect_gain", "mcrt_psf_carrier", "mcrt_detect_frames",
           "mcrt_default_flow_opts", "mcrt_flow_nyquist", "mcrt_flow_phasors", "mcrt_flow_draws", "mcrt_colour_map", "mcrt_flow_split_frames", "mcrt_flow_frames",
           "mcrt_default_colour_opts", "mcrt_colour_frames",
           "mcrt_default_spectral_opts", "mcrt_spectral_rotor", "mcrt_spectral_phase", "mcrt_spectral_profile", "mcrt_spectral_rates", "mcrt_spectral_window",
           "mcrt_spectral_twiddles", "mcrt_spectral_draws", "mcrt_pulse_waveform", "mcrt_spectral_series_frames", "mcrt_spectral_frames",
           "mcrt_default_sonogram_opts", "mcrt_sonogram_frames",
           "mcrt_default_strain_opts", "mcrt_strain_table", "mcrt_strain_draws", "mcrt_strain_map", "mcrt_strain_compress_frames", "mcrt_strain_frames",
           "mcrt_default_elastogram_opts", "mcrt_elastogram_frames",
           "mcrt_default_shear_opts", "mcrt_shear_table", "mcrt_shear_pitch", "mcrt_shear_shape", "mcrt_shear_decay", "mcrt_shear_draws", "mcrt_shear_map",
           "mcrt_shear_wave_frames", "mcrt_shear_speed_frames",
           "mcrt_default_mmode_opts", "mcrt_mmode_table", "mcrt_mmode_waveform", "mcrt_mmode_bulk", "mcrt_mmode_draws", "mcrt_default_mmode_display_opts",
           "mcrt_mmode_rows", "mcrt_mmode_lines_frames", "mcrt_mmode_picture_frames",
           "mcrt_default_recon_opts", "mcrt_recon_transform", "mcrt_recon_frames",
           "mcrt_default_recon_label_opts", "mcrt_recon_label_frames", "mcrt_render_label_frames"]


def build_library(force=False):
    """Compile libmcrt_hip.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    srcs = [os.path.join(_HERE, "csrc", f) for f in os.listdir(os.path.join(_HERE, "csrc"))]
    srcs.append(os.path.join(_HERE, "..", "include", "mcrt.h"))
    stale = (not os.path.exists(_SO)) or any(os.path.getmtime(s) > os.path.getmtime(_SO) for s in srcs)
    if force or stale:
        subprocess.check_call(["make", "-C", _HERE, "libmcrt_hip.so"] + (["-B"] if force else []))
    return _SO


def load_library():
    """Load the HIP library.  There is no fallback: a missing library is an error."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(_SO):
        raise McrtError(-4, f"{_SO} is missing: run __graft_entry__.build() (make -C mcray-tracing_amd); there is no CPU fallback")
    L = C.CDLL(_SO)
    L.mcrt_last_error.restype = C.c_char_p
    vp, u32, i32 = C.c_void_p, C.c_uint32, C.c_int
    sig = {
        "mcrt_create": [i32, C.POINTER(vp)], "mcrt_destroy": [vp], "mcrt_set_stream": [vp, vp], "mcrt_synchronize": [vp],
        "mcrt_default_params": [C.POINTER(Params)], "mcrt_set_params": [vp, C.POINTER(Params)], "mcrt_get_params": [vp, C.POINTER(Params)], "mcrt_import_rf": [vp, vp, u32, u32, vp],
        "mcrt_upload_scene": [vp, vp, vp, u32, vp, u32, vp, u32, u32, vp],
        "mcrt_upload_texture": [vp, vp, u32], "mcrt_set_transducer": [vp, vp, vp, u32],
        "mcrt_trace_frame": [vp, u32, u32, u32, vp], "mcrt_trace_frames": [vp, u32, u32, u32, u32, vp], "mcrt_trace_frame_debug": [vp, u32, u32, u32, vp, vp, vp, vp],
        "mcrt_cast_rays": [vp, u32, u32, u32, vp, vp, vp],
        "mcrt_convolve": [vp, vp, u32, u32, vp, u32, vp, u32], "mcrt_envelope": [vp, vp, u32, u32],
        "mcrt_scan_convert": [vp, vp, u32, u32, C.c_double, C.c_double, vp, u32, u32],
        "mcrt_convolve_frames": [vp, vp, u32, u32, u32, vp, u32, vp, u32], "mcrt_convolve_frames_depth": [vp, vp, u32, u32, u32, vp, u32, vp, u32],
        "mcrt_trace_frames_poses": [vp, u32, u32, u32, u32, vp, vp, vp], "mcrt_envelope_frames": [vp, vp, u32, u32, u32],
        "mcrt_scan_convert_frames": [vp, vp, u32, u32, u32, C.c_double, C.c_double, vp, u32, u32],
        "mcrt_default_bmode": [C.POINTER(BmodeParams)], "mcrt_bmode_frames": [vp, vp, u32, u32, u32, C.POINTER(BmodeParams), vp, vp, vp, vp],
        "mcrt_set_bvh_builder": [vp, i32], "mcrt_update_triangles": [vp, vp, u32], "mcrt_refit_triangles": [vp, vp, u32],
        "mcrt_export_rf": [vp, vp, u32, u32, vp], "mcrt_alloc": [vp, C.c_size_t, C.POINTER(vp)], "mcrt_free": [vp, vp],
        "mcrt_memcpy_d2h": [vp, vp, vp, C.c_size_t], "mcrt_memcpy_h2d": [vp, vp, vp, C.c_size_t],
        "mcrt_enable_stats": [vp, i32], "mcrt_get_stats": [vp, C.POINTER(Stats), i32],
        "mcrt_enable_timing": [vp, i32], "mcrt_get_kernel_time": [vp, C.POINTER(C.c_double), C.POINTER(u32), i32], "mcrt_get_kernel_times": [vp, vp, vp, i32],
        "mcrt_build_bvh": [vp, vp, u32, C.POINTER(Bvh)], "mcrt_free_bvh": [C.POINTER(Bvh)], "mcrt_get_bvh": [vp, C.POINTER(Bvh)],
        "mcrt_build_bvh4": [C.POINTER(Bvh), C.POINTER(Bvh4)], "mcrt_free_bvh4": [C.POINTER(Bvh4)], "mcrt_get_bvh4": [vp, C.POINTER(Bvh4)],
        "mcrt_row_thresholds": [C.c_double, u32, vp],
        "mcrt_generate_texture": [vp, u32], "mcrt_psf_kernels": [C.c_float, C.c_float, C.c_float, u32, vp, u32, vp, u32],
        "mcrt_psf_focus_kernels": [C.c_float, u32, C.POINTER(Focus), u32, C.c_double, vp, u32],
        "mcrt_transducer_elements": [u32, C.c_double, C.c_double, vp, vp, vp, vp],
        "mcrt_transducer_elevation_axis": [vp, vp], "mcrt_elevation_planes": [vp, vp, u32, vp, u32, u32, vp, vp, vp],
        "mcrt_psf_elevation_kernels": [C.c_float, u32, C.POINTER(Focus), u32, C.c_double, i32, vp, u32],
        "mcrt_elevation_frames": [vp, vp, u32, u32, u32, u32, vp, vp],
        "mcrt_transducer_steered": [u32, C.c_double, C.c_double, vp, vp, C.c_float, vp, vp],
        "mcrt_compound_maps": [u32, u32, C.c_double, C.c_double, u32, u32, u32, u32, C.c_float, vp, vp],
        "mcrt_compound_frames": [vp, vp, u32, u32, u32, C.c_double, C.c_double, C.POINTER(Compound), vp, u32, u32],
        "mcrt_bmode_compound_frames": [vp, vp, u32, u32, u32, C.POINTER(BmodeParams), C.POINTER(Compound), vp, vp, vp, vp],
        "mcrt_default_compound_opts": [C.POINTER(CompoundOpts)],
        "mcrt_compound_weights": [u32, u32, C.c_double, C.c_double, u32, u32, u32, u32, C.c_float, C.c_float, C.c_float, vp],
        "mcrt_compound_frames_opts": [vp, vp, u32, u32, u32, C.c_double, C.c_double, C.POINTER(Compound), vp, u32, u32, C.POINTER(CompoundOpts)],
        "mcrt_bmode_compound_frames_opts": [vp, vp, u32, u32, u32, C.POINTER(BmodeParams), C.POINTER(Compound), vp, vp, vp, vp, C.POINTER(CompoundOpts)],
        "mcrt_transducer_swept": [u32, C.c_double, C.c_double, vp, vp, C.c_float, C.c_float, vp, vp],
        "mcrt_volume_maps": [u32, u32, C.c_double, C.c_double, u32, u32, C.POINTER(Sweep), C.POINTER(VolumeGrid), vp, vp, vp],
        "mcrt_volume_frames": [vp, vp, u32, u32, u32, C.c_double, C.c_double, C.POINTER(Sweep), C.POINTER(VolumeGrid), vp],
        "mcrt_bmode_volume_frames": [vp, vp, u32, u32, u32, C.POINTER(BmodeParams), C.POINTER(Sweep), C.POINTER(VolumeGrid), vp, vp, vp],
        "mcrt_default_label_opts": [C.POINTER(LabelOpts)],
        "mcrt_label_frames": [vp, u32, u32, u32, vp, vp, C.POINTER(LabelOpts), vp, vp, vp],
        "mcrt_default_transmit_opts": [C.POINTER(TransmitOpts)],
        "mcrt_transmit_boundary": [C.c_float, C.c_float, C.c_float, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float)],
        "mcrt_transmit_frames": [vp, u32, u32, u32, vp, vp, C.POINTER(TransmitOpts), vp, vp, vp],
        "mcrt_label_scan_convert_frames": [vp, vp, u32, u32, u32, C.c_double, C.c_double, vp, u32, u32],
        "mcrt_label_volume_frames": [vp, vp, u32, u32, u32, C.c_double, C.c_double, C.POINTER(Sweep), C.POINTER(VolumeGrid), vp],
        "mcrt_default_render_opts": [C.POINTER(RenderOpts), i32],
        "mcrt_render_view_for_grid": [C.POINTER(VolumeGrid), vp, vp, C.c_double, C.c_double, u32, u32, C.POINTER(RenderView)],
        "mcrt_render_frames": [vp, vp, i32, u32, u32, u32, u32, C.POINTER(RenderView), C.POINTER(RenderOpts), vp, vp, vp],
        "mcrt_default_speckle_opts": [C.POINTER(SpeckleOpts)],
        "mcrt_speckle_tables": [C.POINTER(SpeckleOpts), vp, vp, vp],
        "mcrt_speckle_frames": [vp, vp, u32, u32, u32, C.POINTER(SpeckleOpts), vp],
        "mcrt_default_speckle3d_opts": [C.POINTER(Speckle3dOpts)],
        "mcrt_speckle3d_weights": [C.POINTER(VolumeGrid), vp],
        "mcrt_speckle3d_tables": [C.POINTER(Speckle3dOpts), vp, vp, vp],
        "mcrt_speckle_volume_frames": [vp, vp, u32, u32, u32, u32, C.POINTER(Speckle3dOpts), vp],
        "mcrt_default_noise_opts": [C.POINTER(NoiseOpts)],
        "mcrt_noise_draws": [u32, u32, u32, u32, vp],
        "mcrt_noise_frames": [vp, vp, u32, u32, u32, u32, u32, C.POINTER(NoiseOpts), vp, vp],
        "mcrt_default_autogain_opts": [C.POINTER(AutogainOpts)],
        "mcrt_autogain_curve": [vp, u32, u32, C.c_float, C.POINTER(AutogainOpts), vp, vp, vp],
        "mcrt_autogain_frames": [vp, vp, u32, u32, u32, u32, C.POINTER(AutogainOpts), vp, vp, vp, vp],
        "mcrt_default_bands": [C.POINTER(Bands), C.c_float, C.c_float],
        "mcrt_psf_band_kernels": [C.POINTER(Bands), u32, u32, C.c_double, vp, u32, vp],
        "mcrt_convolve_bands_frames": [vp, vp, u32, u32, u32, u32, vp, u32, vp, vp, u32, vp],
        "mcrt_band_fold_frames": [vp, vp, u32, u32, u32, u32, vp, vp],
        "mcrt_default_detect_opts": [C.POINTER(DetectOpts)],
        "mcrt_detect_taps": [C.POINTER(DetectOpts), vp],
        "mcrt_detect_gain": [vp, u32, C.c_double, C.POINTER(C.c_double)],
        "mcrt_psf_carrier": [C.c_float, u32, C.POINTER(C.c_double)],
        "mcrt_detect_frames": [vp, vp, u32, u32, u32, C.POINTER(DetectOpts), vp, vp],
        "mcrt_default_flow_opts": [C.POINTER(FlowOpts)],
        "mcrt_flow_nyquist": [C.POINTER(FlowOpts), C.c_double, C.c_double, C.POINTER(C.c_double)],
        "mcrt_flow_phasors": [C.c_double, vp, vp, u32, u32, vp, vp],
        "mcrt_flow_draws": [u32, u32, u32, u32, u32, vp],
        "mcrt_colour_map": [u32, vp],
        "mcrt_flow_split_frames": [vp, vp, vp, u32, u32, u32, vp, u32, vp],
        "mcrt_flow_frames": [vp, vp, vp, vp, u32, u32, u32, C.POINTER(FlowOpts), C.c_double, vp, vp, u32, u32, vp, vp, vp, vp, vp],
        "mcrt_default_colour_opts": [C.POINTER(ColourOpts)],
        "mcrt_colour_frames": [vp, vp, vp, u32, u32, u32, vp, C.POINTER(ColourOpts), C.c_double, vp, vp],
        "mcrt_default_spectral_opts": [C.POINTER(SpectralOpts)],
        "mcrt_spectral_rotor": [vp],
        "mcrt_spectral_phase": [C.c_double, vp, u32, vp],
        "mcrt_spectral_profile": [vp, u32, u32, u32, vp, u32, C.c_double, vp],
        "mcrt_spectral_rates": [vp, u32, C.c_double, vp],
        "mcrt_spectral_window": [u32, u32, vp],
        "mcrt_spectral_twiddles": [u32, vp],
        "mcrt_spectral_draws": [u32, u32, u32, u32, u32, vp],
        "mcrt_pulse_waveform": [C.c_double, C.c_double, C.c_double, C.c_double, u32, vp],
        "mcrt_spectral_series_frames": [vp, vp, vp, u32, u32, u32, vp, u32, vp, vp, vp, C.POINTER(SpectralOpts), u32, vp, vp],
        "mcrt_spectral_frames": [vp, vp, u32, vp, C.POINTER(SpectralOpts), C.c_double, vp, vp],
        "mcrt_default_sonogram_opts": [C.POINTER(SonogramOpts)],
        "mcrt_sonogram_frames": [vp, vp, u32, u32, u32, C.POINTER(SonogramOpts), vp, vp],
        "mcrt_default_strain_opts": [C.POINTER(StrainOpts)],
        "mcrt_strain_table": [vp, u32, C.c_double, C.c_double, vp],
        "mcrt_strain_draws": [u32, u32, u32, u32, vp],
        "mcrt_strain_map": [u32, vp],
        "mcrt_strain_compress_frames": [vp, vp, vp, u32, u32, u32, vp, u32, C.c_double, C.POINTER(StrainOpts), u32, vp, vp, vp, vp],
        "mcrt_strain_frames": [vp, vp, vp, u32, u32, u32, C.POINTER(StrainOpts), C.c_double, vp, vp, vp],
        "mcrt_default_shear_opts": [C.POINTER(ShearOpts)],
        "mcrt_shear_table": [vp, u32, C.c_double, vp, vp],
        "mcrt_shear_pitch": [u32, u32, C.c_double, C.c_double, u32, u32, vp, vp],
        "mcrt_shear_shape": [u32, vp],
        "mcrt_shear_decay": [u32, C.c_double, vp],
        "mcrt_shear_draws": [u32, u32, u32, u32, u32, vp],
        "mcrt_shear_map": [u32, vp],
        "mcrt_shear_wave_frames": [vp, vp, vp, u32, u32, u32, vp, vp, u32, vp, vp, u32, vp, u32, C.c_double, C.POINTER(ShearOpts), u32, vp, vp, vp, vp, vp, vp],
        "mcrt_shear_speed_frames": [vp, vp, u32, u32, u32, vp, C.POINTER(ShearOpts), vp, vp, vp],
        "mcrt_default_mmode_opts": [C.POINTER(MmodeOpts)],
        "mcrt_mmode_table": [vp, u32, vp],
        "mcrt_mmode_waveform": [C.c_double, C.c_double, u32, vp],
        "mcrt_mmode_bulk": [C.c_double, C.c_double, C.c_double, u32, vp],
        "mcrt_mmode_draws": [u32, u32, u32, u32, u32, vp],
        "mcrt_default_mmode_display_opts": [C.POINTER(MmodeDisplayOpts)],
        "mcrt_mmode_rows": [u32, u32, u32, vp, vp],
        "mcrt_mmode_lines_frames": [vp, vp, vp, u32, u32, u32, vp, u32, vp, u32, vp, vp, C.c_double, C.POINTER(MmodeOpts), u32, vp, vp, vp, vp, vp],
        "mcrt_mmode_picture_frames": [vp, vp, vp, vp, u32, u32, u32, C.POINTER(MmodeDisplayOpts), vp, vp, vp, vp, vp],
        "mcrt_default_elastogram_opts": [C.POINTER(ElastogramOpts)],
        "mcrt_elastogram_frames": [vp, vp, vp, vp, u32, u32, u32, vp, C.POINTER(ElastogramOpts), vp],
        "mcrt_default_recon_opts": [C.POINTER(ReconOpts)],
        "mcrt_recon_transform": [C.POINTER(VolumeGrid), C.c_double, vp, vp],
        "mcrt_recon_frames": [vp, vp, u32, u32, u32, vp, vp, C.c_double, C.c_double, C.POINTER(VolumeGrid), C.POINTER(ReconOpts), vp, vp, vp],
        "mcrt_default_recon_label_opts": [C.POINTER(ReconLabelOpts), u32],
        "mcrt_recon_label_frames": [vp, vp, u32, u32, u32, vp, vp, C.c_double, C.c_double, C.POINTER(VolumeGrid), C.POINTER(ReconLabelOpts), vp, vp, vp, vp],
        "mcrt_render_label_frames": [vp, vp, u32, u32, u32, u32, C.POINTER(RenderView), vp, vp],
        "mcrt_debug_math": [vp, i32, vp, vp, vp, u32], "mcrt_debug_philox": [vp, vp, vp, vp], "mcrt_debug_stamps": [vp, vp, i32], "mcrt_debug_tail_histograms": [vp, vp, i32], "mcrt_debug_set_error": [vp, u32], "mcrt_debug_fast_paths": [vp, vp], "mcrt_debug_beam": [vp, vp], "mcrt_debug_beam_bounce": [vp, u32, vp], "mcrt_debug_beam_order": [vp, u32, vp], "mcrt_debug_beam_layout": [vp, u32, vp, vp], "mcrt_debug_beam_scan": [vp, vp, u32, vp, vp, vp], "mcrt_debug_beam_records": [vp, u32, vp, vp, vp, vp], "mcrt_debug_beam_entries": [vp, u32, vp, vp, vp],
        "mcrt_scan_maps": [u32, u32, C.c_double, C.c_double, u32, u32, u32, u32, vp, vp],
        "mcrt_group_create": [vp, u32, C.POINTER(vp)], "mcrt_group_destroy": [vp], "mcrt_group_size": [vp], "mcrt_group_root": [vp], "mcrt_group_member": [vp, u32],
        "mcrt_group_shard": [u32, u32, u32, C.POINTER(u32), C.POINTER(u32)], "mcrt_group_set_params": [vp, C.POINTER(Params)], "mcrt_group_set_bvh_builder": [vp, i32],
        "mcrt_group_upload_scene": [vp, vp, vp, u32, vp, u32, vp, u32, u32, vp], "mcrt_group_update_triangles": [vp, vp, u32], "mcrt_group_refit_triangles": [vp, vp, u32],
        "mcrt_group_upload_texture": [vp, vp, u32], "mcrt_group_set_transducer": [vp, vp, vp, u32], "mcrt_group_trace_frames": [vp, u32, u32, vp],
        "mcrt_group_trace_frames_poses": [vp, u32, u32, vp, vp, vp], "mcrt_group_synchronize": [vp], "mcrt_group_last_pass_ms": [vp, vp, vp],
        "mcrt_group_last_scene_seconds": [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)],
    }
    for name, args in sig.items():
        if name in ("mcrt_debug_beam", "mcrt_debug_beam_bounce", "mcrt_debug_beam_order", "mcrt_debug_beam_layout", "mcrt_debug_beam_scan", "mcrt_debug_beam_records", "mcrt_debug_beam_entries") and not hasattr(L, name):
            continue       # (a library of before the beams, loaded through MCRT_LIB for a comparison: Context.debug_beam / debug_beam_bounce / debug_beam_order then say that nothing ran)
        f = getattr(L, name)
        f.argtypes = args
        f.restype = None if name in ("mcrt_free_bvh", "mcrt_free_bvh4") else vp if name in ("mcrt_group_root", "mcrt_group_member") else C.c_int
    _LIB = L
    return L


def check(rc):
    if rc != 0:
        raise McrtError(rc, load_library().mcrt_last_error().decode())


def ptr(a):
    """host pointer of a numpy array / raw device pointer of a torch tensor / int passthrough"""
    if a is None:
        return None
    if isinstance(a, int):
        return C.c_void_p(a)
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(C.c_void_p)
    if hasattr(a, "data_ptr"):
        return C.c_void_p(a.data_ptr())
    raise TypeError(type(a))
