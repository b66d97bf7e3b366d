"""mcray_tracing_amd -- MI355X-native Monte-Carlo ultrasound ray tracer (hot path of
thepochynsons/MCRay-Tracing) behind the C-ABI of include/mcrt.h.

Python here is plumbing for tests and bench.py (ctypes over libmcrt_hip.so); the product is the
HIP library in csrc/ and the C++ host mirror of the reference API in host/.
"""
from ._lib import load_library, build_library, McrtError, Params, MeshRec, BvhNode, Stats, BmodeParams, Focus, Bands, DetectOpts, FlowOpts, ColourOpts, SpectralOpts, Gate, SonogramOpts, StrainOpts, ElastogramOpts, ShearOpts, Mline, MmodeOpts, MmodeDisplayOpts, Compound, Sweep, VolumeGrid, CompoundOpts, LabelOpts, TransmitOpts, RenderView, RenderOpts, SpeckleOpts, Speckle3dOpts, NoiseOpts, AutogainOpts, ReconOpts, ReconLabelOpts, SEGMENT_DTYPE  # noqa: F401
from .api import Context, Group, shard_range, Simulator, bmode_params, Transducer, Psf, host_build_bvh, host_build_bvh4, host_row_thresholds, host_texture, host_psf, host_psf_focus, focus_struct, bands_struct, host_psf_bands, detect_opts_struct, host_detect_taps, host_detect_gain, host_psf_carrier, flow_opts_struct, colour_opts_struct, host_flow_nyquist, host_flow_phasors, host_flow_draws, host_colour_map, FLOW_WALLS, spectral_opts_struct, sonogram_opts_struct, host_spectral_rotor, host_spectral_phase, host_spectral_profile, host_spectral_rates, host_spectral_window, host_spectral_twiddles, host_spectral_draws, host_pulse_waveform, SPECTRAL_WALLS, SPECTRAL_WINDOWS, strain_opts_struct, elastogram_opts_struct, host_strain_table, host_strain_draws, host_strain_map, shear_opts_struct, host_shear_table, host_shear_pitch, host_shear_shape, host_shear_decay, host_shear_draws, host_shear_map, mmode_opts_struct, mmode_display_opts_struct, host_mmode_table, host_mmode_waveform, host_mmode_bulk, host_mmode_draws, host_mmode_rows, row_pitch_mm, host_transducer, host_scan_maps, host_beam_layout, host_elevation_axis, host_elevation_planes, host_psf_elevation, host_transducer_steered, host_compound_maps, host_transducer_swept, host_volume_maps, sweep_struct, sweep_tilts, volume_grid, cplane_grid, sagittal_grid, compound_struct, compound_opts_struct, host_compound_weights, label_opts_struct, transmit_opts_struct, transmit_boundary, TRANSMIT_MODES, render_view, render_opts_struct, RENDER_MODES, speckle_opts_struct, host_speckle_tables, speckle3d_opts_struct, host_speckle3d_tables, host_speckle3d_weights, noise_opts_struct, host_noise_draws, autogain_opts_struct, host_autogain_curve, NOISE_SNR_DB, NOISE_ABS, recon_opts_struct, recon_label_opts_struct, host_recon_transform, RECON_MODES, LABEL_RULES, LABEL_NONE, LABEL_MAX_CROSSINGS, LABEL_CAPPED  # noqa: F401
from . import synth, scene_io  # noqa: F401


def __getattr__(name):          # torch is only needed by the multi-GPU helper
    if name == "dist":
        import importlib
        return importlib.import_module("mcray_tracing_amd.dist")
    raise AttributeError(name)

__all__ = ["load_library", "build_library", "McrtError", "Params", "BmodeParams", "bmode_params", "Context", "Group", "shard_range", "Simulator", "Transducer", "Psf",
           "synth", "scene_io", "host_build_bvh", "host_texture", "host_psf", "host_psf_focus", "host_transducer"]
