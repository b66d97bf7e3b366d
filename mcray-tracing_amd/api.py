"""Python mirror of the reference's host interface for the hot path, over the C-ABI.

  Transducer  <-> transducer<N>            (transducer.h:24-67)
  Psf         <-> psf<ax,lat,elev,res>     (psf.h:34-77)
  Simulator   <-> scene + rf_image + the frame loop body of main.cpp:102-148
  Context     <-> thin 1:1 wrapper of include/mcrt.h
"""
import collections
import contextlib
import ctypes as C
import math
import numpy as np

from . import _lib
from ._lib import Params, MeshRec, Stats, Bvh, Bvh4, BmodeParams, Focus, Bands, DetectOpts, FlowOpts, ColourOpts, SpectralOpts, Gate, SonogramOpts, StrainOpts, ElastogramOpts, ShearOpts, Mline, MmodeOpts, MmodeDisplayOpts, Compound, Sweep, VolumeGrid, CompoundOpts, LabelOpts, TransmitOpts, RenderView, RenderOpts, SpeckleOpts, Speckle3dOpts, NoiseOpts, AutogainOpts, ReconOpts, ReconLabelOpts, NODE_DTYPE, SEGMENT_DTYPE, check, ptr, load_library

DEFAULT_ANGLE = 1.0471975511965976      # the sector of main.cpp:28: 60 degrees [rad]


# ------------------------------------------------------------------ host-side pieces (no GPU)
def host_build_bvh(tri, tri_mesh):
    """-> (nodes structured array [n_nodes] of 64-B nodes, bvh_tri float32 [T,12], max_depth)"""
    L = load_library()
    tri = np.ascontiguousarray(tri, np.float32).reshape(-1, 9)
    tm = np.ascontiguousarray(tri_mesh, np.uint32)
    b = Bvh()
    check(L.mcrt_build_bvh(ptr(tri), ptr(tm), tri.shape[0], C.byref(b)))
    try:
        nodes = np.frombuffer(C.string_at(b.nodes, 64 * b.n_nodes), dtype=NODE_DTYPE).copy()
        btri = np.frombuffer(C.string_at(b.tri, 48 * b.n_tri), dtype=np.float32).reshape(-1, 12).copy()
        depth = int(b.max_depth)
    finally:
        L.mcrt_free_bvh(C.byref(b))
    return nodes, btri, depth


def host_build_bvh4(tri, tri_mesh):
    """-> (BVH2 nodes, leaf-order triangles [T,12], BVH4 nodes uint8 [n4,128], max_stack)"""
    L = load_library()
    tri = np.ascontiguousarray(tri, np.float32).reshape(-1, 9)
    tm = np.ascontiguousarray(tri_mesh, np.uint32)
    b = Bvh(); b4 = Bvh4()
    check(L.mcrt_build_bvh(ptr(tri), ptr(tm), tri.shape[0], C.byref(b)))
    try:
        check(L.mcrt_build_bvh4(C.byref(b), C.byref(b4)))
        nodes = np.frombuffer(C.string_at(b.nodes, 64 * b.n_nodes), dtype=NODE_DTYPE).copy()
        btri = np.frombuffer(C.string_at(b.tri, 48 * b.n_tri), dtype=np.float32).reshape(-1, 12).copy()
        n4 = np.frombuffer(C.string_at(b4.nodes, 128 * b4.n_nodes), dtype=np.uint8).reshape(-1, 128).copy()
        ms = int(b4.max_stack)
    finally:
        L.mcrt_free_bvh(C.byref(b)); L.mcrt_free_bvh4(C.byref(b4))
    return nodes, btri, n4, ms


def host_row_thresholds(row_dt_us, n_rows):
    thr = np.zeros(n_rows + 1, np.float64)
    check(load_library().mcrt_row_thresholds(row_dt_us, n_rows, ptr(thr)))
    return thr


def host_texture(n=256):
    out = np.empty((n, n, n, 2), np.float32)
    check(load_library().mcrt_generate_texture(ptr(out), n))
    return out


def host_psf(freq=4.5, var_x=0.05, var_y=0.2, res_um=145, n_ax=7, n_lat=13):
    ax = np.zeros(n_ax, np.float32); lat = np.zeros(n_lat, np.float32)
    check(load_library().mcrt_psf_kernels(freq, var_x, var_y, res_um, ptr(ax), n_ax, ptr(lat), n_lat))
    return ax, lat


def focus_struct(focus_mm=(), focal_range_mm=20.0):
    """mcrt_focus from a sequence of focal depths [mm] (more than 8 give n_focus > 8, which the library refuses)"""
    f = Focus()
    fm = [float(x) for x in (focus_mm or ())]
    f.n_focus = len(fm)
    for i, x in enumerate(fm[:8]):
        f.focus_mm[i] = x
    f.focal_range_mm = focal_range_mm
    return f


def host_psf_focus(var_y, res_um, n_rows, row_mm, focus_mm, focal_range_mm=20.0, n_lat=13):
    """mcrt_psf_focus_kernels: the lateral taps of every RF row, float32 [n_rows][n_lat] (focal zones; the model is in include/mcrt.h).
    focal_range_mm = 20 is a display choice that no measurement backs."""
    out = np.zeros((n_rows, n_lat), np.float32)
    f = focus_struct(focus_mm, focal_range_mm)
    check(load_library().mcrt_psf_focus_kernels(var_y, res_um, C.byref(f), n_rows, row_mm, ptr(out), n_lat))
    return out


def bands_struct(band_mhz, weights=None, var_x=0.05, downshift_mhz_per_mm=0.0, min_mhz=0.0):
    """mcrt_bands from a sequence of centre frequencies [MHz] (more than 8 give n_bands > 8, which the library refuses); weights: one per
    band, None: equal ones"""
    b = Bands()
    fm = [float(x) for x in band_mhz]
    w = [1.0] * len(fm) if weights is None else [float(x) for x in weights]
    if len(w) != len(fm):
        raise ValueError("weights takes one weight per band (%d), got %d" % (len(fm), len(w)))
    b.n_bands = len(fm)
    for i, (f, x) in enumerate(list(zip(fm, w))[:8]):
        b.band_mhz[i] = f; b.band_weight[i] = x
    b.var_x, b.downshift_mhz_per_mm, b.min_mhz = var_x, downshift_mhz_per_mm, min_mhz
    return b


def host_psf_bands(bands, res_um, n_rows, row_mm, n_ax=7):
    """mcrt_psf_band_kernels: (ax_rows float32 [B][n_rows][n_ax], w_rows float32 [n_rows][B]) of a Bands struct -- the axial taps of every
    band and RF row and the bands' weights (frequency compounding and the depth downshift; the model is in include/mcrt.h)"""
    B = min(max(int(bands.n_bands), 0), 8)
    ax = np.zeros((B, n_rows, max(int(n_ax), 0)), np.float32); w = np.zeros((n_rows, B), np.float32)
    check(load_library().mcrt_psf_band_kernels(C.byref(bands), res_um, n_rows, row_mm, ptr(ax), n_ax, ptr(w)))
    return ax, w


def detect_opts_struct(n_taps=None):
    """mcrt_detect_opts from keywords over mcrt_default_detect_opts: n_taps (3, 7, 11, ..., 63; 31) -- the library refuses any other"""
    o = DetectOpts()
    check(load_library().mcrt_default_detect_opts(C.byref(o)))
    if n_taps is not None:
        o.n_taps = int(n_taps)
    return o


def host_detect_taps(n_taps=31):
    """mcrt_detect_taps: the FIR Hilbert transformer of quadrature detection, float32 [n_taps] (antisymmetric, the even offsets +0.0)"""
    o = DetectOpts(); o.n_taps = int(n_taps) & 0xFFFFFFFF
    taps = np.zeros(min(max(int(n_taps), 0), 63), np.float32)
    check(load_library().mcrt_detect_taps(C.byref(o), ptr(taps)))
    return taps


def host_detect_gain(taps, cycles):
    """mcrt_detect_gain: the transformer's magnitude response at `cycles` cycles per RF row (1 in its passband, 0 at 0 and at 0.5)"""
    t = np.ascontiguousarray(taps, np.float32)
    g = C.c_double()
    check(load_library().mcrt_detect_gain(ptr(t), t.size, float(cycles), C.byref(g)))
    return g.value


def host_psf_carrier(freq, res_um=145):
    """mcrt_psf_carrier: the digital carrier of the axial pulse at freq MHz, cycles per RF row in 0..0.5 (0.3475 at 4.5 MHz and 145 um)"""
    c = C.c_double()
    check(load_library().mcrt_psf_carrier(freq, res_um, C.byref(c)))
    return c.value


FLOW_WALLS = {"none": 0, "mean": 1, "linear": 2}      # MCRT_FLOW_WALL_*


def flow_opts_struct(n_packets=None, wall=None, avg_rows=None, avg_lines=None, prf_hz=None, freq_mhz=None, sigma=None, seed=None):
    """mcrt_flow_opts from keywords over mcrt_default_flow_opts: n_packets (2..16; 8), wall ("none" | "mean" | "linear" or the number; mean),
    avg_rows (0..8; 2), avg_lines (0..4; 1), prf_hz (4000), freq_mhz (<= 0: the caller's; 0), sigma (0), seed -- the library checks the ranges"""
    o = FlowOpts()
    check(load_library().mcrt_default_flow_opts(C.byref(o)))
    if wall is not None:
        if isinstance(wall, str) and wall not in FLOW_WALLS:
            raise ValueError("wall must be one of %s, got %r" % (sorted(FLOW_WALLS), wall))
        o.wall = FLOW_WALLS[wall] if isinstance(wall, str) else int(wall) & 0xFFFFFFFF
    for name, v in (("n_packets", n_packets), ("avg_rows", avg_rows), ("avg_lines", avg_lines), ("seed", seed)):
        if v is not None:
            setattr(o, name, int(v) & 0xFFFFFFFF)
    for name, v in (("prf_hz", prf_hz), ("freq_mhz", freq_mhz), ("sigma", sigma)):
        if v is not None:
            setattr(o, name, float(v))
    return o


def colour_opts_struct(power_thr=None, vel_thr_mm_s=None, grey_max=None):
    """mcrt_colour_opts from keywords over mcrt_default_colour_opts (0, 0, 255)"""
    o = ColourOpts()
    check(load_library().mcrt_default_colour_opts(C.byref(o)))
    if power_thr is not None:
        o.power_thr = float(power_thr)
    if vel_thr_mm_s is not None:
        o.vel_thr_mm_s = float(vel_thr_mm_s)
    if grey_max is not None:
        o.grey_max = int(grey_max) & 0xFFFFFFFF
    return o


def host_flow_nyquist(freq_mhz, speed_of_sound=1500.0, opts=None, **kw):
    """mcrt_flow_nyquist: the velocity [mm/s] whose phase step from pulse to pulse is pi (333.33 at 1500 m/s, 4.5 MHz and 4 kHz)"""
    o = opts if opts is not None else flow_opts_struct(**kw)
    v = C.c_double()
    check(load_library().mcrt_flow_nyquist(C.byref(o), float(freq_mhz), float(speed_of_sound), C.byref(v)))
    return v.value


def host_flow_phasors(v_nyq_mm_s, vel_mm_s, dirs):
    """mcrt_flow_phasors: (phasor float32 [n_labels][E][2], truth float32 [n_labels][E]) of a velocity vector per material [n_labels][3] and
    the scan-lines' directions [E][3]; truth is the velocity towards the probe"""
    vel = np.ascontiguousarray(vel_mm_s, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    ph = np.zeros((vel.shape[0], d.shape[0], 2), np.float32); tr = np.zeros((vel.shape[0], d.shape[0]), np.float32)
    check(load_library().mcrt_flow_phasors(float(v_nyq_mm_s), ptr(vel), ptr(d), vel.shape[0], d.shape[0], ptr(ph), ptr(tr)))
    return ph, tr


def host_flow_draws(seed, image_id, n_elements, n_rows, n_packets):
    """mcrt_flow_draws: the integer draws of one image's ensemble, int32 [n_packets][n_elements][n_rows][2] (noise = d * sigma / sqrt(1431655765))"""
    d = np.zeros((min(max(int(n_packets), 0), 16), max(int(n_elements), 0), max(int(n_rows), 0), 2), np.int32)
    check(load_library().mcrt_flow_draws(int(seed) & 0xFFFFFFFF, int(image_id) & 0xFFFFFFFF, n_elements, n_rows, n_packets, ptr(d)))
    return d


def host_colour_map(kind=0):
    """mcrt_colour_map: the colour table of the overlay, uint8 [256][3] (kind 0: red towards the probe, blue away, 128 black)"""
    lut = np.zeros((256, 3), np.uint8)
    check(load_library().mcrt_colour_map(int(kind) & 0xFFFFFFFF, ptr(lut)))
    return lut


SPECTRAL_WALLS = {"none": 0, "mean": 1}               # MCRT_SPECTRAL_WALL_*
SPECTRAL_WINDOWS = {"rect": 0, "hann": 1}             # the kinds of mcrt_spectral_window


def spectral_opts_struct(n_pulses=None, gate_rows=None, n_fft=None, hop=None, wall=None, wall_bins=None, sigma=None, seed=None):
    """mcrt_spectral_opts from keywords over mcrt_default_spectral_opts: n_pulses (1..16384; 2048), gate_rows (1..64; 8), n_fft (32, 64, 128,
    256, 512; 128), hop (1..n_fft; 32), wall ("none" | "mean" or the number; mean), wall_bins (0..n_fft/4; 2), sigma (0), seed -- the
    library checks the ranges"""
    o = SpectralOpts()
    check(load_library().mcrt_default_spectral_opts(C.byref(o)))
    if wall is not None:
        if isinstance(wall, str) and wall not in SPECTRAL_WALLS:
            raise ValueError("wall must be one of %s, got %r" % (sorted(SPECTRAL_WALLS), wall))
        o.wall = SPECTRAL_WALLS[wall] if isinstance(wall, str) else int(wall) & 0xFFFFFFFF
    for name, v in (("n_pulses", n_pulses), ("gate_rows", gate_rows), ("n_fft", n_fft), ("hop", hop), ("wall_bins", wall_bins), ("seed", seed)):
        if v is not None:
            setattr(o, name, int(v) & 0xFFFFFFFF)
    if sigma is not None:
        o.sigma = float(sigma)
    return o


def sonogram_opts_struct(dynamic_range_db=None, gain_db=None, ref=None):
    """mcrt_sonogram_opts from keywords over mcrt_default_sonogram_opts (40 dB, 0 dB, ref 0: each gate's own largest finite power)"""
    o = SonogramOpts()
    check(load_library().mcrt_default_sonogram_opts(C.byref(o)))
    for name, v in (("dynamic_range_db", dynamic_range_db), ("gain_db", gain_db), ("ref", ref)):
        if v is not None:
            setattr(o, name, float(v))
    return o


def host_spectral_rotor():
    """mcrt_spectral_rotor: the cos/sin table of the series' rotor, float32 [4096][2]"""
    lut = np.zeros((4096, 2), np.float32)
    check(load_library().mcrt_spectral_rotor(ptr(lut)))
    return lut


def host_spectral_phase(v_nyq_mm_s, speed_mm_s):
    """mcrt_spectral_phase: the accumulated phase int64 [T], in units of 2^-32 turn, of a centre-line speed waveform [T] in mm/s"""
    s = np.ascontiguousarray(speed_mm_s, np.float32).reshape(-1)
    ph = np.zeros(s.size, np.int64)
    check(load_library().mcrt_spectral_phase(float(v_nyq_mm_s), ptr(s), s.size, ptr(ph)))
    return ph


def host_spectral_profile(tissue_line, row0, gate_rows, moving, exponent=2.0):
    """mcrt_spectral_profile: the share of the centre-line speed per gate row, float32 [gate_rows], from one scan-line's tissue labels
    uint8 [R] and a byte per label (non-zero: the material moves); exponent 0: plug flow, 2: a parabola"""
    t = np.ascontiguousarray(tissue_line, np.uint8).reshape(-1); mv = np.ascontiguousarray(moving, np.uint8).reshape(-1)
    frac = np.zeros(min(max(int(gate_rows), 0), 64), np.float32)
    check(load_library().mcrt_spectral_profile(ptr(t), t.size, row0, gate_rows, ptr(mv), mv.size, float(exponent), ptr(frac)))
    return frac


def host_spectral_rates(frac, axial):
    """mcrt_spectral_rates: the rows' rates in Q16, int32 [G], of their shares and the cosine towards the probe"""
    f = np.ascontiguousarray(frac, np.float32).reshape(-1)
    rate = np.zeros(min(f.size, 64), np.int32)
    check(load_library().mcrt_spectral_rates(ptr(f), f.size, float(axial), ptr(rate)))
    return rate


def host_spectral_window(kind, n_fft):
    """mcrt_spectral_window: float32 [n_fft]; kind "rect" | "hann" or the number"""
    if isinstance(kind, str) and kind not in SPECTRAL_WINDOWS:
        raise ValueError("window must be one of %s, got %r" % (sorted(SPECTRAL_WINDOWS), kind))
    h = np.zeros(min(max(int(n_fft), 0), 512), np.float32)
    check(load_library().mcrt_spectral_window(SPECTRAL_WINDOWS[kind] if isinstance(kind, str) else int(kind) & 0xFFFFFFFF, n_fft, ptr(h)))
    return h


def host_spectral_twiddles(n_fft):
    """mcrt_spectral_twiddles: the FFT's twiddles, float32 [n_fft / 2][2]"""
    tw = np.zeros((min(max(int(n_fft), 0), 512) // 2, 2), np.float32)
    check(load_library().mcrt_spectral_twiddles(n_fft, ptr(tw)))
    return tw


def host_spectral_draws(seed, image_id, line, row0, n_pulses):
    """mcrt_spectral_draws: the integer draws of one gate's series, int32 [n_pulses][2] (noise = d * sigma * wnorm / sqrt(1431655765))"""
    d = np.zeros((min(max(int(n_pulses), 0), 16384), 2), np.int32)
    check(load_library().mcrt_spectral_draws(int(seed) & 0xFFFFFFFF, int(image_id) & 0xFFFFFFFF, line, row0, n_pulses, ptr(d)))
    return d


def host_pulse_waveform(prf_hz, beats_per_min, v_peak, v_min, n_pulses):
    """mcrt_pulse_waveform: a pulsatile centre-line speed [mm/s], float32 [n_pulses] -- a sin^2 systole over 0.3 of the beat above v_min"""
    s = np.zeros(min(max(int(n_pulses), 0), 16384), np.float32)
    check(load_library().mcrt_pulse_waveform(float(prf_hz), float(beats_per_min), float(v_peak), float(v_min), n_pulses, ptr(s)))
    return s


def strain_opts_struct(window_rows=None, search_rows=None, lsq_rows=None, sigma=None, seed=None):
    """mcrt_strain_opts from keywords over mcrt_default_strain_opts: window_rows (0..32; 16), search_rows (0..16; 8), lsq_rows (1..32; 12),
    sigma (0), seed -- the library checks the ranges"""
    o = StrainOpts()
    check(load_library().mcrt_default_strain_opts(C.byref(o)))
    for name, v in (("window_rows", window_rows), ("search_rows", search_rows), ("lsq_rows", lsq_rows), ("seed", seed)):
        if v is not None:
            setattr(o, name, int(v) & 0xFFFFFFFF)
    if sigma is not None:
        o.sigma = float(sigma)
    return o


def elastogram_opts_struct(ref_strain=None, rho_min=None, grey_min=None, alpha=None):
    """mcrt_elastogram_opts from keywords over mcrt_default_elastogram_opts (0.01, 0.7, 0, 160)"""
    o = ElastogramOpts()
    check(load_library().mcrt_default_elastogram_opts(C.byref(o)))
    for name, v in (("ref_strain", ref_strain), ("rho_min", rho_min)):
        if v is not None:
            setattr(o, name, float(v))
    for name, v in (("grey_min", grey_min), ("alpha", alpha)):
        if v is not None:
            setattr(o, name, int(v) & 0xFFFFFFFF)
    return o


def host_strain_table(modulus, applied=0.01, ref_modulus=1.0):
    """mcrt_strain_table: the strain of every material in Q24, int32 [n_labels], of a Young's modulus per material (0: rigid), the applied
    strain of the reference modulus and that modulus"""
    m = np.ascontiguousarray(modulus, np.float64).reshape(-1)
    eps = np.zeros(min(m.size, 254), np.int32)
    check(load_library().mcrt_strain_table(ptr(m), m.size, float(applied), float(ref_modulus), ptr(eps)))
    return eps


def host_strain_draws(seed, image_id, n_elements, n_rows):
    """mcrt_strain_draws: the integer draws of one post-compression image, int32 [n_elements][n_rows][2] (noise = d * sigma / sqrt(1431655765))"""
    d = np.zeros((max(int(n_elements), 0), min(max(int(n_rows), 0), 2048), 2), np.int32)
    check(load_library().mcrt_strain_draws(int(seed) & 0xFFFFFFFF, int(image_id) & 0xFFFFFFFF, n_elements, n_rows, ptr(d)))
    return d


def host_strain_map(kind=0):
    """mcrt_strain_map: the colour table of the elastogram, uint8 [256][3] (kind 0: stiff blue, the reference strain green at 128, soft red)"""
    lut = np.zeros((256, 3), np.uint8)
    check(load_library().mcrt_strain_map(int(kind) & 0xFFFFFFFF, ptr(lut)))
    return lut


def shear_opts_struct(n_pulses=None, window_rows=None, prf_hz=None, sigma=None, seed=None, push_line=None, push_row0=None, push_rows=None, peak_q24=None,
                      speed_lines=None, avg_rows=None, density=None):
    """mcrt_shear_opts from keywords over mcrt_default_shear_opts: n_pulses (4..256; 64), window_rows (0..16; 8), prf_hz (10000), sigma (0), seed,
    push_line (0), push_row0 (0), push_rows (0: to the end of the line), peak_q24 (|.| <= 2^23; 1677722, 0.1 row), speed_lines (1..16; 4),
    avg_rows (0..16; 2), density (g/cm^3; 1) -- the library checks the ranges"""
    o = ShearOpts()
    check(load_library().mcrt_default_shear_opts(C.byref(o)))
    for name, v in (("n_pulses", n_pulses), ("window_rows", window_rows), ("seed", seed), ("push_line", push_line), ("push_row0", push_row0), ("push_rows", push_rows),
                    ("speed_lines", speed_lines), ("avg_rows", avg_rows)):
        if v is not None:
            setattr(o, name, int(v) & 0xFFFFFFFF)
    if peak_q24 is not None:
        o.peak_q24 = int(peak_q24)
    for name, v in (("prf_hz", prf_hz), ("sigma", sigma), ("density", density)):
        if v is not None:
            setattr(o, name, float(v))
    return o


def host_shear_table(speed_m_s, prf_hz=10000.0):
    """mcrt_shear_table: (slow_q16 int64 [n_labels], speed_f float32 [n_labels]) of a shear speed per material [m/s] (0: a fluid, the wave
    does not pass) at the tracking pulse rate"""
    c = np.ascontiguousarray(speed_m_s, np.float64).reshape(-1)
    slow = np.zeros(min(c.size, 254), np.int64); speed = np.zeros(min(c.size, 254), np.float32)
    check(load_library().mcrt_shear_table(ptr(c), c.size, float(prf_hz), ptr(slow), ptr(speed)))
    return slow, speed


def host_shear_pitch(n_elements, n_rows, radius_mm, total_angle, max_travel_us=100, speed_of_sound=1500):
    """mcrt_shear_pitch: (pitch_q8 uint32 [n_rows], pitch_mm float32 [n_rows]): the arc between neighbouring scan-lines at the depth of
    every row, by host_scan_maps' geometry"""
    rows = min(max(int(n_rows), 0), 2048)
    q8 = np.zeros(rows, np.uint32); mm = np.zeros(rows, np.float32)
    check(load_library().mcrt_shear_pitch(n_elements, n_rows, float(radius_mm), float(total_angle), max_travel_us, speed_of_sound, ptr(q8), ptr(mm)))
    return q8, mm


def host_shear_shape(width_pulses=12):
    """mcrt_shear_shape: the default time profile of the particle displacement, a raised cosine of width_pulses, uint32 [64 * width_pulses] in Q16"""
    s = np.zeros(64 * min(max(int(width_pulses), 0), 256), np.uint32)
    check(load_library().mcrt_shear_shape(width_pulses, ptr(s) if s.size else None))
    return s


def host_shear_decay(n, d0_lines=8.0):
    """mcrt_shear_decay: the default decay of the amplitude over line distance, 1 / sqrt(1 + d / d0_lines), uint32 [n] in Q16"""
    a = np.zeros(max(int(n), 0), np.uint32)
    check(load_library().mcrt_shear_decay(n, float(d0_lines), ptr(a) if a.size else None))
    return a


def host_shear_draws(seed, image_id, n_elements, n_rows, pulse):
    """mcrt_shear_draws: the integer draws of one tracking pulse of one image, int32 [n_elements][n_rows][2] (noise = d * sigma / sqrt(1431655765))"""
    d = np.zeros((max(int(n_elements), 0), min(max(int(n_rows), 0), 2048), 2), np.int32)
    check(load_library().mcrt_shear_draws(int(seed) & 0xFFFFFFFF, int(image_id) & 0xFFFFFFFF, n_elements, n_rows, pulse, ptr(d)))
    return d


def host_shear_map(kind=0):
    """mcrt_shear_map: the colour table of the shear-wave elastogram, uint8 [256][3] (kind 0: soft blue, the reference modulus green at 128, stiff red)"""
    lut = np.zeros((256, 3), np.uint8)
    check(load_library().mcrt_shear_map(int(kind) & 0xFFFFFFFF, ptr(lut)))
    return lut


def mmode_opts_struct(n_pulses=None, sigma=None, seed=None):
    """mcrt_mmode_opts from keywords over mcrt_default_mmode_opts: n_pulses (1..16384; 1024), sigma (0), seed -- the library checks the ranges"""
    o = MmodeOpts()
    check(load_library().mcrt_default_mmode_opts(C.byref(o)))
    for name, v in (("n_pulses", n_pulses), ("seed", seed)):
        if v is not None:
            setattr(o, name, int(v) & 0xFFFFFFFF)
    if sigma is not None:
        o.sigma = float(sigma)
    return o


def mmode_display_opts_struct(hop=None, height=None, row_lo=None, row_hi=None, dynamic_range_db=None, gain_db=None, ref=None):
    """mcrt_mmode_display_opts from keywords over mcrt_default_mmode_display_opts: hop (pulses per column, >= 1; 4), height (1..4096; 400),
    row_lo and row_hi (the rows shown; 0, 0: the whole line), dynamic_range_db (60), gain_db (0), ref (0: each line's own peak)"""
    o = MmodeDisplayOpts()
    check(load_library().mcrt_default_mmode_display_opts(C.byref(o)))
    for name, v in (("hop", hop), ("height", height), ("row_lo", row_lo), ("row_hi", row_hi)):
        if v is not None:
            setattr(o, name, int(v) & 0xFFFFFFFF)
    for name, v in (("dynamic_range_db", dynamic_range_db), ("gain_db", gain_db), ("ref", ref)):
        if v is not None:
            setattr(o, name, float(v))
    return o


def host_mmode_table(dilation):
    """mcrt_mmode_table: the dilation of every material in Q24, int32 [n_labels], of a peak axial strain per material (positive: compression;
    at most 25 %)"""
    d = np.ascontiguousarray(dilation, np.float64).reshape(-1)
    q = np.zeros(min(d.size, 254), np.int32)
    check(load_library().mcrt_mmode_table(ptr(d), d.size, ptr(q)))
    return q


def host_mmode_waveform(prf_hz, beats_per_min, n_pulses):
    """mcrt_mmode_waveform: a default waveform in Q16, int32 [n_pulses] -- host_pulse_waveform's systolic half-sine squared (a convenience,
    not physiology)"""
    w = np.zeros(min(max(int(n_pulses), 0), 16384), np.int32)
    check(load_library().mcrt_mmode_waveform(float(prf_hz), float(beats_per_min), n_pulses, ptr(w) if w.size else None))
    return w


def host_mmode_bulk(prf_hz, cycles_per_min, amplitude_rows, n_pulses):
    """mcrt_mmode_bulk: a sinusoidal rigid shift of the whole line in Q24 rows, int32 [n_pulses] (|amplitude_rows| <= 32)"""
    b = np.zeros(min(max(int(n_pulses), 0), 16384), np.int32)
    check(load_library().mcrt_mmode_bulk(float(prf_hz), float(cycles_per_min), float(amplitude_rows), n_pulses, ptr(b) if b.size else None))
    return b


def host_mmode_draws(seed, image_id, line, n_rows, n_pulses):
    """mcrt_mmode_draws: the integer draws of one M-line, int32 [n_pulses][n_rows][2] (noise = d * sigma / sqrt(1431655765))"""
    d = np.zeros((min(max(int(n_pulses), 0), 16384), min(max(int(n_rows), 0), 2048), 2), np.int32)
    check(load_library().mcrt_mmode_draws(int(seed) & 0xFFFFFFFF, int(image_id) & 0xFFFFFFFF, int(line) & 0xFFFFFFFF, n_rows, n_pulses, ptr(d)))
    return d


def host_mmode_rows(row_lo, row_hi, height):
    """mcrt_mmode_rows: the depth resampling table of the sweep, (idx uint32 [height], wt float32 [height]): the first tap and the second
    tap's weight of every picture row over the line's rows [row_lo, row_hi)"""
    H = min(max(int(height), 0), 4096)
    idx = np.zeros(H, np.uint32); wt = np.zeros(H, np.float32)
    check(load_library().mcrt_mmode_rows(row_lo, row_hi, height, ptr(idx) if H else None, ptr(wt) if H else None))
    return idx, wt


def row_pitch_mm(frequency):
    """the RF row pitch [mm] of a context at `frequency` MHz: axial_res_um / 1000 with axial_res_um = (unsigned)(1.45f / f * 1000.0f)
    (main.cpp:25,36; 0.322 at 4.5 MHz)"""
    res_f = np.float32(np.float32(1.45) / np.float32(frequency))
    return int(np.float32(res_f * np.float32(1000.0))) / 1000.0


def _element_tables(fn, n_elements, radius_cm, sep_mm, position, angles_deg, *how):
    """(pos, dir), each float32 [n_elements][3], of mcrt_transducer_elements or a kin of it that takes `how` after the angles"""
    pos = np.zeros((n_elements, 3), np.float32); d = np.zeros((n_elements, 3), np.float32)
    p = np.asarray(position, np.float32); a = np.asarray(angles_deg, np.float32)
    check(getattr(load_library(), fn)(n_elements, radius_cm, sep_mm, ptr(p), ptr(a), *how, ptr(pos), ptr(d)))
    return pos, d


def host_transducer(n_elements, radius_cm, sep_mm, position, angles_deg):
    return _element_tables("mcrt_transducer_elements", n_elements, radius_cm, sep_mm, position, angles_deg)


def host_elevation_axis(angles_deg):
    """mcrt_transducer_elevation_axis: the probe's elevation direction, float32 [3] ((0,0,1) through the probe's rotations)"""
    a = np.asarray(angles_deg, np.float32); out = np.zeros(3, np.float32)
    check(load_library().mcrt_transducer_elevation_axis(ptr(a), ptr(out)))
    return out


def host_elevation_planes(pos, dirs, axis, n_planes, pitch_um):
    """mcrt_elevation_planes: K parallel copies of an element table spread along `axis` -> (pos [K][E][3], dir [K][E][3], z_mm [K])"""
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3); dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    axis = np.ascontiguousarray(axis, np.float32)
    E, K = pos.shape[0], max(int(n_planes), 0)
    po = np.zeros((K, E, 3), np.float32); do = np.zeros((K, E, 3), np.float32); z = np.zeros(K, np.float32)
    check(load_library().mcrt_elevation_planes(ptr(pos), ptr(dirs), E, ptr(axis), n_planes, pitch_um, ptr(po), ptr(do), ptr(z)))
    return po, do, z


def host_psf_elevation(var_z, pitch_um, n_rows, row_mm, focus_mm=(), focal_range_mm=20.0, n_planes=7, normalize=True):
    """mcrt_psf_elevation_kernels: the elevation weights of every RF row, float32 [n_rows][n_planes] (slice thickness; include/mcrt.h)"""
    out = np.zeros((n_rows, max(int(n_planes), 0)), np.float32)
    f = focus_struct(focus_mm, focal_range_mm)
    check(load_library().mcrt_psf_elevation_kernels(var_z, pitch_um, C.byref(f), n_rows, row_mm, 1 if normalize else 0, ptr(out), n_planes))
    return out


BEAM_PAD = 0xffffffff                 # MCRT_BEAM_PAD: a word of a beam order that holds no ray
BEAM_SCAN_SENTINEL = 0x5eed5eed       # MCRT_DEBUG_BEAM_SENTINEL: what mcrt_debug_beam_scan fills its order buffer with


def host_beam_layout(counts):
    """mcrt_debug_beam_layout: the layout of a beam order (csrc/mcrt_beam.hip, k_beam_scan) for `counts` rays per beam, the last the pseudo-beam's ->
    (bases uint32 [n], rays placed, segments, pad lanes, the order's length)"""
    counts = np.ascontiguousarray(counts, np.uint32)
    bases = np.zeros(len(counts), np.uint32)
    out = (C.c_uint32 * 4)()
    check(load_library().mcrt_debug_beam_layout(ptr(counts), len(counts), ptr(bases), out))
    return bases, int(out[0]), int(out[1]), int(out[2]), int(out[3])


def host_scan_maps(n_elements, n_rows, radius_mm=30.0, total_angle=DEFAULT_ANGLE, max_travel_us=100, speed_of_sound=1500, out_rows=400, out_cols=500):
    """rf_image::create_mapping (rfimage.h:183-215) as the library evaluates it: (map_row, map_col), each [out_rows][out_cols]"""
    return _sector_maps("mcrt_scan_maps", n_elements, n_rows, radius_mm, total_angle, max_travel_us, speed_of_sound, out_rows, out_cols)


def _sector_maps(fn, n_elements, n_rows, radius_mm, total_angle, max_travel_us, speed_of_sound, out_rows, out_cols, *steer):
    mr = np.zeros((out_rows, out_cols), np.float32); mc = np.zeros((out_rows, out_cols), np.float32)
    check(getattr(load_library(), fn)(n_elements, n_rows, radius_mm, total_angle, max_travel_us, speed_of_sound, out_rows, out_cols, *steer, ptr(mr), ptr(mc)))
    return mr, mc


def host_transducer_steered(n_elements, radius_cm, sep_mm, position, angles_deg, steer_rad):
    """mcrt_transducer_steered: mcrt_transducer_elements with every beam tilted in the image plane by steer_rad (the beams pivot on their
    elements; a positive steer tilts towards higher element numbers)"""
    return _element_tables("mcrt_transducer_steered", n_elements, radius_cm, sep_mm, position, angles_deg, steer_rad)


def host_compound_maps(n_elements, n_rows, steer_rad, radius_mm=30.0, total_angle=DEFAULT_ANGLE, max_travel_us=100, speed_of_sound=1500, out_rows=400,
                       out_cols=500):
    """mcrt_compound_maps: the scan-conversion maps of a view steered by steer_rad, (map_row, map_col), each [out_rows][out_cols]; NaN where
    no beam of the view passes the pixel.  steer_rad == 0: host_scan_maps' maps bit for bit."""
    return _sector_maps("mcrt_compound_maps", n_elements, n_rows, radius_mm, total_angle, max_travel_us, speed_of_sound, out_rows, out_cols, steer_rad)


def compound_struct(steer_rad):
    """mcrt_compound from a sequence of steering angles [rad] (more than 16 give n_views > 16, which the library refuses)"""
    st = [float(x) for x in steer_rad]
    cp = Compound()
    cp.n_views = len(st)
    for i, x in enumerate(st[:16]):
        cp.steer_rad[i] = x
    return cp


COMPOUND_MODES = {"mean": 0, "max": 1, "median": 2}


def compound_opts_struct(mode="mean", view_weights=None, feather_lines=0.0):
    """mcrt_compound_opts from keywords: mode "mean" / "max" / "median" (or the MCRT_COMPOUND_* number), view_weights a sequence of up to 16
    weights (None: every view 1; the views past the sequence keep 1), feather_lines the lateral edge ramp in scan-lines (0: off)"""
    o = CompoundOpts()
    check(load_library().mcrt_default_compound_opts(C.byref(o)))
    o.mode = COMPOUND_MODES[mode] if isinstance(mode, str) else int(mode)
    o.feather_lines = float(feather_lines)
    if view_weights is not None:
        w = [float(x) for x in view_weights]
        if len(w) > 16:
            raise ValueError("at most 16 view weights, got %d" % len(w))
        for i, x in enumerate(w):
            o.view_weight[i] = x
    return o


def _compound_defaults(mode, view_weights, feather_lines):
    """every compounding keyword at its default: the caller then uses the entry point without options"""
    return mode in ("mean", 0) and view_weights is None and feather_lines == 0.0


def host_compound_weights(n_elements, n_rows, steer_rad, view_weight=1.0, feather_lines=0.0, radius_mm=30.0, total_angle=DEFAULT_ANGLE,
                          max_travel_us=100, speed_of_sound=1500, out_rows=400, out_cols=500):
    """mcrt_compound_weights: what the view steered by steer_rad contributes with at every pixel, float32 [out_rows][out_cols] -- its weight
    times the lateral edge ramp where it covers the pixel, 0 elsewhere (the expression the kernel evaluates)"""
    w = np.zeros((out_rows, out_cols), np.float32)
    check(load_library().mcrt_compound_weights(n_elements, n_rows, radius_mm, total_angle, max_travel_us, speed_of_sound, out_rows, out_cols, steer_rad,
                                               view_weight, feather_lines, ptr(w)))
    return w


def host_transducer_swept(n_elements, radius_cm, sep_mm, position, angles_deg, tilt_rad, pivot_mm=0.0):
    """mcrt_transducer_swept: mcrt_transducer_elements with the array tilted by tilt_rad about the line parallel to the lateral axis through
    (0, pivot_mm, 0) of the probe-local frame (tilt 0: the plain tables bit for bit)"""
    return _element_tables("mcrt_transducer_swept", n_elements, radius_cm, sep_mm, position, angles_deg, tilt_rad, pivot_mm)


def sweep_struct(n_planes, step_rad, pivot_mm=0.0):
    """mcrt_sweep: n_planes planes step_rad apart, centred on tilt 0 (an even count has no plane AT 0), about the axis through (0, pivot_mm, 0)"""
    sw = Sweep()
    sw.n_planes, sw.step_rad, sw.pivot_mm = int(n_planes), float(step_rad), float(pivot_mm)
    return sw


def _as_sweep(sweep):
    """an mcrt_sweep from what the wrappers take: one as it is, or (K, step_rad[, pivot_mm])"""
    return sweep if isinstance(sweep, Sweep) else sweep_struct(*sweep)


def sweep_tilts(n_planes, step_rad):
    """the planes' tilts [rad], float32: theta_k = (k - (K-1)/2.0) * step_rad with step_rad as the float the library is given"""
    step = float(np.float32(step_rad))
    return np.array([(k - (n_planes - 1) / 2.0) * step for k in range(n_planes)], np.float32)


def volume_grid(origin_mm, du, dv, dw, nu, nv, nw=1):
    """mcrt_volume_grid: point (i, j, l) = origin + i*du + j*dv + l*dw [mm, the probe-local frame: x lateral, y the arc's axis, z elevation];
    the output is [nw][nv][nu].  nw = 1 is a cut."""
    g = VolumeGrid()
    for dst, src in ((g.origin_mm, origin_mm), (g.du_mm, du), (g.dv_mm, dv), (g.dw_mm, dw)):
        for i in range(3):
            dst[i] = float(src[i])
    g.nu, g.nv, g.nw, g._pad = int(nu), int(nv), int(nw), 0
    return g


def cplane_grid(depth_mm, nu, nv, pitch_mm, x0_mm=None, z0_mm=None):
    """the C-plane: the x-z picture at axial position y = depth_mm (from the arc's centre), [nv][nu] with u along x and v along z, pitch_mm
    apart, centred on the arc's axis unless x0_mm / z0_mm give the first point"""
    x0 = -(nu - 1) * pitch_mm / 2.0 if x0_mm is None else x0_mm
    z0 = -(nv - 1) * pitch_mm / 2.0 if z0_mm is None else z0_mm
    return volume_grid((x0, depth_mm, z0), (pitch_mm, 0, 0), (0, 0, pitch_mm), (0, 0, 0), nu, nv, 1)


def sagittal_grid(x_mm, nu, nv, pitch_mm, y0_mm, z0_mm=None):
    """the sagittal cut: the y-z picture at lateral position x = x_mm, [nv][nu] with u along z and v along y (depth downwards), pitch_mm apart,
    from axial position y0_mm on, centred in elevation unless z0_mm gives the first point"""
    z0 = -(nu - 1) * pitch_mm / 2.0 if z0_mm is None else z0_mm
    return volume_grid((x_mm, y0_mm, z0), (0, 0, pitch_mm), (0, pitch_mm, 0), (0, 0, 0), nu, nv, 1)


def host_volume_maps(n_elements, n_rows, sweep, grid, radius_mm=30.0, total_angle=DEFAULT_ANGLE, max_travel_us=100, speed_of_sound=1500):
    """mcrt_volume_maps: where in the stack [K][E][R] every point of grid lies, (map_plane, map_row, map_col), each [nw][nv][nu].
    sweep: an mcrt_sweep (sweep_struct) or (K, step_rad[, pivot_mm])"""
    sw = _as_sweep(sweep)
    shape = _grid_shape(grid)[0]
    mz = np.zeros(shape, np.float32); mr = np.zeros(shape, np.float32); mc = np.zeros(shape, np.float32)
    check(load_library().mcrt_volume_maps(n_elements, n_rows, radius_mm, total_angle, max_travel_us, speed_of_sound, C.byref(sw), C.byref(grid), ptr(mz), ptr(mr), ptr(mc)))
    return mz, mr, mc


BMODE_MODES = {"db": 0, "ref_log": 1}


RENDER_MODES = {"mip": 0, "mean": 1, "surface": 2}


def render_view(grid, direction, up=(0, 0, 1), pixel_mm=0.25, step_mm=0.25, nx=500, ny=400):
    """mcrt_render_view_for_grid: an orthographic camera on grid's block [mm, the probe-local frame], looking along `direction` at the block's
    centre with `up` towards the picture's top; nx x ny pixels pixel_mm apart, samples step_mm apart along the block's longest diagonal.
    -> RenderView: twelve floats in the block's index space, which may also be filled by hand"""
    v = RenderView()
    d = (C.c_double * 3)(*[float(x) for x in direction]); u = (C.c_double * 3)(*[float(x) for x in up])
    check(load_library().mcrt_render_view_for_grid(C.byref(grid), d, u, float(pixel_mm), float(step_mm), int(nx), int(ny), C.byref(v)))
    return v


def render_opts_struct(in_u8=False, mode=None, lo=None, hi=None, threshold=None, ramp=None, opacity=None, depth_cue=None, t_cut=None):
    """mcrt_render_opts from keywords over mcrt_default_render_opts(in_u8): mode "mip" / "mean" / "surface" or the MCRT_RENDER_* number"""
    o = RenderOpts()
    check(load_library().mcrt_default_render_opts(C.byref(o), 1 if in_u8 else 0))
    if mode is not None:
        o.mode = RENDER_MODES[mode] if isinstance(mode, str) else int(mode)
    for name, val in (("lo", lo), ("hi", hi), ("threshold", threshold), ("ramp", ramp), ("opacity", opacity), ("depth_cue", depth_cue), ("t_cut", t_cut)):
        if val is not None:
            setattr(o, name, float(val))
    return o


def speckle_opts_struct(n_iter=None, q0=None, rho=None, lambda_=None, **kw):
    """mcrt_speckle_opts from keywords over mcrt_default_speckle_opts: n_iter, q0, rho and the time step, lambda_ (or lam, or "lambda" in a
    dict: the word is Python's)"""
    o = SpeckleOpts()
    check(load_library().mcrt_default_speckle_opts(C.byref(o)))
    for k in ("lambda", "lam"):
        if k in kw:
            lambda_ = kw.pop(k)
    if kw:
        raise TypeError("unknown speckle options: %s" % ", ".join(sorted(kw)))
    if n_iter is not None:
        o.n_iter = int(n_iter)
    for name, val in (("q0", q0), ("rho", rho), ("lambda_", lambda_)):
        if val is not None:
            setattr(o, name, float(val))
    return o


def host_speckle_tables(opts=None, **kw):
    """mcrt_speckle_tables: the floats k_srad is given -> (q0sq [n_iter], kq [n_iter], lam4); opts: a SpeckleOpts, or the keywords of speckle_opts_struct"""
    o = opts if opts is not None else speckle_opts_struct(**kw)
    n = min(int(o.n_iter), 256)
    q0sq = np.zeros(n, np.float32); kq = np.zeros(n, np.float32); lam4 = np.zeros(1, np.float32)
    check(load_library().mcrt_speckle_tables(C.byref(o), ptr(q0sq), ptr(kq), ptr(lam4)))
    return q0sq, kq, np.float32(lam4[0])


def speckle3d_opts_struct(n_iter=None, q0=None, rho=None, lambda_=None, weights=None, **kw):
    """mcrt_speckle3d_opts from keywords over mcrt_default_speckle3d_opts: n_iter, q0, rho, the time step lambda_ (or lam, or "lambda" in a
    dict) and weights, one per axis (u, v, w)"""
    o = Speckle3dOpts()
    check(load_library().mcrt_default_speckle3d_opts(C.byref(o)))
    for k in ("lambda", "lam"):
        if k in kw:
            lambda_ = kw.pop(k)
    if kw:
        raise TypeError("unknown speckle3d options: %s" % ", ".join(sorted(kw)))
    if n_iter is not None:
        o.n_iter = int(n_iter)
    for name, val in (("q0", q0), ("rho", rho), ("lambda_", lambda_)):
        if val is not None:
            setattr(o, name, float(val))
    if weights is not None:
        w = [float(x) for x in weights]
        if len(w) != 3:
            raise ValueError("speckle3d: weights takes one weight per axis (u, v, w), got %d" % len(w))
        o.weight[:] = w
    return o


def host_speckle3d_tables(opts=None, **kw):
    """mcrt_speckle3d_tables: the floats k_srad3 is given -> (q0sq [n_iter], kq [n_iter], k [4]: a, b, hs, lamw); opts: a Speckle3dOpts, or the
    keywords of speckle3d_opts_struct"""
    o = opts if opts is not None else speckle3d_opts_struct(**kw)
    n = min(int(o.n_iter), 256)
    q0sq = np.zeros(n, np.float32); kq = np.zeros(n, np.float32); k = np.zeros(4, np.float32)
    check(load_library().mcrt_speckle3d_tables(C.byref(o), ptr(q0sq), ptr(kq), ptr(k)))
    return q0sq, kq, k


def host_speckle3d_weights(grid):
    """mcrt_speckle3d_weights: the weights (u, v, w) of a VolumeGrid's pitches, float32 [3]: (h_min / h_a)^2, 0 for an axis of one voxel"""
    w = np.zeros(3, np.float32)
    check(load_library().mcrt_speckle3d_weights(C.byref(grid), ptr(w)))
    return w


RECON_MODES = {"mean": 0, "max": 1}


def recon_opts_struct(mode=None, value_max=None, fill_radius=None, fill_min=None, empty=None):
    """mcrt_recon_opts from keywords over mcrt_default_recon_opts: mode "mean" / "max" or the MCRT_RECON_* number, value_max, fill_radius (0..3),
    fill_min, empty"""
    o = ReconOpts()
    check(load_library().mcrt_default_recon_opts(C.byref(o)))
    if mode is not None:
        o.mode = RECON_MODES[mode] if isinstance(mode, str) else int(mode)
    for name, val, kind in (("value_max", value_max, float), ("fill_radius", fill_radius, int), ("fill_min", fill_min, int), ("empty", empty, float)):
        if val is not None:
            setattr(o, name, kind(val))
    return o


def recon_label_opts_struct(n_labels, fill_radius=None, fill_min=None):
    """mcrt_recon_label_opts from keywords over mcrt_default_recon_label_opts: n_labels (1..254, the scene's material count: it has no
    default), fill_radius (0..3), fill_min"""
    o = ReconLabelOpts()
    check(load_library().mcrt_default_recon_label_opts(C.byref(o), int(n_labels)))
    for name, val in (("fill_radius", fill_radius), ("fill_min", fill_min)):
        if val is not None:
            setattr(o, name, int(val))
    return o


def host_recon_transform(grid, unit_mm=10.0):
    """mcrt_recon_transform: the floats k_recon_splat is given -> (A [3][3], b [3]): voxel index = b + A . P for a point P in scene units
    (unit_mm millimetres each) and a grid in world millimetres"""
    A = np.zeros((3, 3), np.float32); b = np.zeros(3, np.float32)
    check(load_library().mcrt_recon_transform(C.byref(grid), float(unit_mm), ptr(A), ptr(b)))
    return A, b


def _depth_mm_f(depth_cm, speed_of_sound):
    """the image depth [mm] as the scan-conversion and volume maps take it (mcrt_scan_maps' depth_mm_f): the float
    (float)(unsigned)(max_travel_us * speed_of_sound) * 0.001f with max_travel_us = (unsigned)(depth_cm / speed_of_sound * 10000)"""
    travel = int((depth_cm / float(speed_of_sound)) * 10000.0)
    return float(np.float32(np.float32((travel * int(speed_of_sound)) & 0xffffffff) * np.float32(0.001)))


NOISE_SNR_DB, NOISE_ABS = 0, 1      # MCRT_NOISE_*


def noise_opts_struct(snr_db=None, sigma=None, seed=None):
    """mcrt_noise_opts from keywords over mcrt_default_noise_opts: snr_db (the noise floor below each frame's own peak, MCRT_NOISE_SNR_DB) or
    sigma (an absolute standard deviation: giving it selects MCRT_NOISE_ABS), and the seed of the noise streams.  Both at once: ValueError"""
    if snr_db is not None and sigma is not None:
        raise ValueError("noise takes snr_db or sigma, not both")
    o = NoiseOpts()
    check(load_library().mcrt_default_noise_opts(C.byref(o)))
    if snr_db is not None:
        o.snr_db = float(snr_db)
    if sigma is not None:
        o.mode, o.sigma = NOISE_ABS, float(sigma)
    if seed is not None:
        o.seed = int(seed) & 0xFFFFFFFF
    return o


def host_noise_draws(seed, image_id, n_elements, n_rows):
    """mcrt_noise_draws: the integer draws d of one image, int32 [n_elements][n_rows] (noise = d * sigma_f / sqrt(2863311530))"""
    d = np.zeros((max(int(n_elements), 0), max(int(n_rows), 0)), np.int32)
    check(load_library().mcrt_noise_draws(int(seed) & 0xFFFFFFFF, int(image_id) & 0xFFFFFFFF, n_elements, n_rows, ptr(d)))
    return d


def autogain_opts_struct(band_rows=None, min_permille=None, floor=None, floor_scale=None, max_gain=None, max_gain_db=None, apply=None):
    """mcrt_autogain_opts from keywords over mcrt_default_autogain_opts.  max_gain_db gives max_gain in dB (max_gain = 10^(dB / 20), rounded
    to float once); both at once: ValueError"""
    if max_gain is not None and max_gain_db is not None:
        raise ValueError("autogain takes max_gain or max_gain_db, not both")
    o = AutogainOpts()
    check(load_library().mcrt_default_autogain_opts(C.byref(o)))
    if band_rows is not None:
        o.band_rows = int(band_rows)
    if min_permille is not None:
        o.min_permille = int(min_permille)
    if floor is not None:
        o.floor = float(floor)
    if floor_scale is not None:
        o.floor_scale = float(floor_scale)
    if max_gain is not None:
        o.max_gain = float(max_gain)
    if max_gain_db is not None:
        o.max_gain = float(np.float32(10.0 ** (float(max_gain_db) / 20.0)))
    if apply is not None:
        o.apply = 1 if apply else 0
    return o


def host_autogain_curve(hist, n_lines, n_rows, floor=0.0, **opts):
    """mcrt_autogain_curve: steps 3 to 8 of the automatic gain for one frame on the host, from its band histograms uint32 [n_bands][2048]
    (n_lines = n_images * n_elements) -> (row gains float32 [n_rows], band levels int32 [n_bands] with -1 for an invalid band, the
    penetration depth in rows).  opts: the keywords of autogain_opts_struct"""
    o = autogain_opts_struct(**opts)
    n_bands = (max(int(n_rows), 0) + max(o.band_rows, 1) - 1) // max(o.band_rows, 1)
    h = np.ascontiguousarray(hist, np.uint32)
    if o.band_rows >= 4 and 0 < n_rows <= 2048 and h.shape != (n_bands, 2048):
        raise ValueError("hist takes uint32 [%d][2048], got shape %s" % (n_bands, h.shape))
    k = np.zeros(max(int(n_rows), 0), np.float32); band = np.zeros(n_bands, np.int32); pen = C.c_uint32(0)
    check(load_library().mcrt_autogain_curve(ptr(h), n_lines, n_rows, float(floor), C.byref(o), ptr(k), ptr(band), C.byref(pen)))
    return k, band, int(pen.value)


LABEL_RULES = {"traced": 0, "geometric": 1}
LABEL_NONE = 255            # MCRT_LABEL_NONE: the tissue value of "no data" (outside the sector / sweep)
LABEL_MAX_CROSSINGS = 64    # MCRT_LABEL_MAX_CROSSINGS
LABEL_CAPPED = 1 << 31      # bit 31 of a crossings word: the walk stopped at the cap, or the GEOMETRIC stack overflowed


def label_opts_struct(rule="traced", start_offset=None):
    """mcrt_label_opts from keywords: rule "traced" (the media the tracer's rays carry, quirks included) / "geometric" (the anatomy of closed,
    nested meshes) or the MCRT_LABEL_* number; start_offset in scene units (None: the context's ray_start_offset)"""
    o = LabelOpts()
    check(load_library().mcrt_default_label_opts(C.byref(o)))
    o.rule = LABEL_RULES[rule] if isinstance(rule, str) else int(rule)
    if start_offset is not None:
        o.start_offset = float(start_offset)
    return o


TRANSMIT_MODES = {"total": 0, "boundaries": 1}


def transmit_opts_struct(mode="total", rule="traced", start_offset=None):
    """mcrt_transmit_opts from keywords: mode "total" (the attenuation along the beam and the loss at every boundary) / "boundaries" (the
    boundaries alone, piecewise constant) or the MCRT_TRANSMIT_* number; rule and start_offset as label_opts_struct"""
    o = TransmitOpts()
    check(load_library().mcrt_default_transmit_opts(C.byref(o)))
    o.mode = TRANSMIT_MODES[mode] if isinstance(mode, str) else int(mode)
    o.rule = LABEL_RULES[rule] if isinstance(rule, str) else int(rule)
    if start_offset is not None:
        o.start_offset = float(start_offset)
    return o


def transmit_boundary(z_before, z_after, inc, intensity):
    """mcrt_transmit_boundary (host only): what one crossing from impedance z_before into z_after at the cosine inc does to an intensity ->
    (reflected, transmitted) as float32"""
    refl, refr = C.c_float(), C.c_float()
    check(load_library().mcrt_transmit_boundary(float(z_before), float(z_after), float(inc), float(intensity), C.byref(refl), C.byref(refr)))
    return np.float32(refl.value), np.float32(refr.value)


def bmode_params(mode="db", dynamic_range_db=60.0, gain_db=0.0, ref=None, persistence=0.0, reset_state=True, radius_mm=30.0,
                 total_angle=DEFAULT_ANGLE, out_rows=400, out_cols=500):
    """mcrt_bmode_params from keywords (mode "db" / "ref_log", or the MCRT_BMODE_* number)"""
    p = BmodeParams()
    check(load_library().mcrt_default_bmode(C.byref(p)))
    p.mode = BMODE_MODES[mode] if isinstance(mode, str) else int(mode)
    p.dynamic_range_db, p.gain_db, p.ref, p.persistence = dynamic_range_db, gain_db, 0.0 if ref is None else ref, persistence
    p.reset_state = 1 if reset_state else 0
    p.out_rows, p.out_cols, p.radius_mm, p.total_angle_rad = out_rows, out_cols, radius_mm, total_angle
    return p


class Transducer:
    """transducer<N>(frequency, radius, element_separation, position, angles) -- transducer.h:24-62.
    main.cpp:28-29,66: total aperture 60 deg on a 3 cm radius; separation = amplitude * radius / N."""

    def __init__(self, n_elements=512, frequency=4.5, radius_cm=3.0, amplitude_deg=60.0, position=(0, 0, 0), angles_deg=(0, 0, 0), separation_mm=None):
        self.n_elements = n_elements
        self.frequency = frequency
        self.radius_cm = radius_cm
        self.amplitude_rad = (amplitude_deg * math.pi * 1.0) / 180.0
        if separation_mm is None:
            # millimeter_t sep = amplitude.to<float>() * radius / N  (float * centimeter_t -> cm, then -> mm: *10)
            separation_mm = ((float(np.float32(self.amplitude_rad)) * radius_cm) / n_elements) * 10.0
        self.separation_mm = separation_mm
        self.position = tuple(float(x) for x in position)
        self.angles = tuple(float(x) for x in angles_deg)
        self.update()

    def update(self):
        self.pos, self.dir = host_transducer(self.n_elements, self.radius_cm, self.separation_mm, self.position, self.angles)

    def element(self, i):
        return self.pos[i], self.dir[i]

    def planes(self, n_planes, pitch_um):
        """the element tables of n_planes parallel elevation planes pitch_um apart, centred on the probe's own plane
        (mcrt_elevation_planes along mcrt_transducer_elevation_axis): (pos [K][E][3], dir [K][E][3], z_mm [K])"""
        return host_elevation_planes(self.pos, self.dir, host_elevation_axis(self.angles), n_planes, pitch_um)

    def steered(self, steer_rad_list):
        """the element tables of the views of a compounded frame, one per steering angle [rad] (mcrt_transducer_steered):
        (pos [N][E][3], dir [N][E][3]); the positions are the probe's own in every view"""
        tabs = [host_transducer_steered(self.n_elements, self.radius_cm, self.separation_mm, self.position, self.angles, float(s)) for s in steer_rad_list]
        return np.stack([t[0] for t in tabs]), np.stack([t[1] for t in tabs])

    def swept(self, n_planes, step_rad, pivot_mm=0.0):
        """the element tables of the planes of a sweep (mcrt_transducer_swept at sweep_tilts' angles): (pos [K][E][3], dir [K][E][3])"""
        tabs = [host_transducer_swept(self.n_elements, self.radius_cm, self.separation_mm, self.position, self.angles, float(t), pivot_mm)
                for t in sweep_tilts(n_planes, step_rad)]
        return np.stack([t[0] for t in tabs]), np.stack([t[1] for t in tabs])

    def poses(self, positions, angles_deg):
        """the element tables of a freehand sweep, one pose (position [3] in scene units, angles_deg [3]) per frame -- this probe moved by hand,
        mcrt_transducer_elements per frame: (pos [F][E][3], dir [F][E][3])"""
        positions = np.asarray(positions, np.float32).reshape(-1, 3); angles_deg = np.asarray(angles_deg, np.float32).reshape(-1, 3)
        if positions.shape != angles_deg.shape:
            raise ValueError("poses takes one position and one set of angles per frame")
        tabs = [host_transducer(self.n_elements, self.radius_cm, self.separation_mm, p, a) for p, a in zip(positions, angles_deg)]
        return np.stack([t[0] for t in tabs]), np.stack([t[1] for t in tabs])


class Psf:
    """psf<axial,lateral,elevation,resolution_um>{freq, var_x, var_y, var_z} -- psf.h:34-58.
    focus_mm: focal depths [mm] (up to 8, ascending) for a lateral kernel per RF row (focal zones, include/mcrt.h); None or empty: the
    reference's one constant kernel.  focal_range_mm = 20 is a display choice that no measurement backs.
    Slice thickness (psf.h:16-18,42,77; include/mcrt.h): elevation_size planes elevation_pitch_um apart (None: resolution_um) weighted with
    var_z.  elevation_kernel is the constant kernel exp(-z_k^2 / (2 var_z)) as the reference leaves its lateral taps (centre 1);
    elevation_rows() the table mcrt_elevation_frames takes: a row per RF row, widening away from elevation_focus_mm (None: the same row
    everywhere), each divided by its sum unless elevation_normalize is False.
    Frequency compounding and the depth downshift (include/mcrt.h): bands = a sequence of centre frequencies [MHz], or a dict of band_mhz=,
    weights= and var_x= (the bands' own axial variance; None: var_x), gives an axial kernel per band and per RF row; downshift_mhz_per_mm
    lets every centre frequency fall with depth down to min_mhz (a downshift without bands is one band at freq).  The downshift has no
    default that the reference backs: 0, and a value is the caller's choice.  axial_rows() / band_weights() are the tables
    mcrt_convolve_bands_frames and mcrt_band_fold_frames take."""

    def __init__(self, freq=4.5, var_x=0.05, var_y=0.2, var_z=0.1, axial_size=7, lateral_size=13, resolution_um=145, focus_mm=None, focal_range_mm=20.0,
                 elevation_size=7, elevation_pitch_um=None, elevation_focus_mm=None, elevation_normalize=True, bands=None, downshift_mhz_per_mm=0.0, min_mhz=0.0):
        self.bands = None
        if bands is not None or downshift_mhz_per_mm != 0.0:
            bd = dict(bands) if isinstance(bands, dict) else dict(band_mhz=(freq,) if bands is None else tuple(bands))
            if bd.get("var_x") is None:
                bd["var_x"] = var_x
            self.bands = bands_struct(downshift_mhz_per_mm=downshift_mhz_per_mm, min_mhz=min_mhz, **bd)
        self._band_rows = {}
        self.axial_kernel, self.lateral_kernel = host_psf(freq, var_x, var_y, resolution_um, axial_size, lateral_size)
        self.var_y, self.resolution_um = var_y, resolution_um
        self.focus_mm = tuple(float(x) for x in focus_mm) if focus_mm is not None else ()
        self.focal_range_mm = focal_range_mm
        self._rows = {}
        self.var_z, self.elevation_size = var_z, elevation_size
        self.elevation_pitch_um = resolution_um if elevation_pitch_um is None else elevation_pitch_um
        self.elevation_focus_mm = tuple(float(x) for x in elevation_focus_mm) if elevation_focus_mm is not None else ()
        self.elevation_normalize = bool(elevation_normalize)
        # (a var_z the model refuses leaves the kernel zero, as the reference leaves it: only elevation_rows() then fails)
        self.elevation_kernel = (host_psf_elevation(var_z, self.elevation_pitch_um, 1, 1.0, (), focal_range_mm, elevation_size, False)[0]
                                 if var_z > 0 and math.isfinite(var_z) else np.zeros(elevation_size, np.float32))
        self._elev_rows = {}

    def elevation_rows(self, n_rows, row_mm):
        """the elevation weights of every RF row, float32 [n_rows][elevation_size], for rows row_mm apart (Simulator.row_mm)"""
        key = (n_rows, row_mm)
        if key not in self._elev_rows:
            self._elev_rows[key] = host_psf_elevation(self.var_z, self.elevation_pitch_um, n_rows, row_mm, self.elevation_focus_mm, self.focal_range_mm,
                                                      self.elevation_size, self.elevation_normalize)
        return self._elev_rows[key]

    @property
    def has_focus(self):
        return len(self.focus_mm) > 0

    @property
    def has_bands(self):
        return self.bands is not None

    def _band_tables(self, n_rows, row_mm):
        key = (n_rows, row_mm)
        if key not in self._band_rows:
            self._band_rows[key] = host_psf_bands(self.bands, self.resolution_um, n_rows, row_mm, self.axial_kernel.size)
        return self._band_rows[key]

    def axial_rows(self, n_rows, row_mm):
        """the axial taps of every band and RF row, float32 [B][n_rows][axial_size], for rows row_mm apart (Simulator.row_mm); bands= or a
        downshift only"""
        return self._band_tables(n_rows, row_mm)[0]

    def band_weights(self, n_rows, row_mm):
        """the bands' weights on every RF row, float32 [n_rows][B] (each row the weights over their sum)"""
        return self._band_tables(n_rows, row_mm)[1]

    def lateral_rows(self, n_rows, row_mm):
        """the lateral taps of every RF row, float32 [n_rows][lateral_size], for rows row_mm apart (Simulator.row_mm)"""
        key = (n_rows, row_mm)
        if key not in self._rows:
            self._rows[key] = host_psf_focus(self.var_y, self.resolution_um, n_rows, row_mm, self.focus_mm, self.focal_range_mm, self.lateral_kernel.size)
        return self._rows[key]


# ------------------------------------------------------------------ C-ABI context
def _scene_tables(sd):
    """(mcrt_mesh records, their count, spacing float32 [3]) of a scene, as mcrt_upload_scene / mcrt_group_upload_scene take them"""
    meshes = (MeshRec * len(sd.meshes))(*[MeshRec(a, b, c, 0) for a, b, c in sd.meshes])
    return meshes, len(sd.meshes), np.asarray(sd.spacing, np.float32)


def _tri9(tri):
    """(triangles, their count) of new vertex positions [T,9]: a numpy array is made contiguous float32, a CUDA torch tensor goes as it is"""
    if isinstance(tri, np.ndarray):
        tri = np.ascontiguousarray(tri, np.float32).reshape(-1, 9)
        return tri, tri.shape[0]
    return tri, tri.numel() // 9


def _tgc_rows(tgc_db, n_rows):
    """the TGC curve as float32 [n_rows], or None"""
    if tgc_db is None:
        return None
    tgc = np.ascontiguousarray(tgc_db, np.float32)
    if tgc.shape != (n_rows,):
        raise ValueError("tgc_db needs one value per RF row: %d, got shape %s" % (n_rows, tgc.shape))
    return tgc


def _pose_tables(what, pos, dirs, n_frames, n_elements):
    """(pos, dirs, n_frames) of pose tables [F][E][3] as the library takes them: numpy arrays made contiguous float32, CUDA torch tensors as they
    are -- n_frames, unless given, is their leading axis and their shape is checked --, or raw device pointers, which need n_frames"""
    if isinstance(pos, np.ndarray):
        pos = np.ascontiguousarray(pos, np.float32); dirs = np.ascontiguousarray(dirs, np.float32)
    if n_frames is None:
        if not hasattr(pos, "shape"):
            raise ValueError("%s: n_frames is required with raw device pointers for pos / dirs" % what)
        n_frames = pos.shape[0]
        assert tuple(pos.shape) == (n_frames, n_elements, 3) and tuple(dirs.shape) == tuple(pos.shape)
    return pos, dirs, n_frames


class _SceneCalls:
    """the scene-level calls a Context and a Group share: mcrt_<name> on the one, mcrt_group_<name> on the other (PREFIX)"""

    def _call(self, name, *args):
        check(getattr(self.L, self.PREFIX + name)(self.h, *args))

    def _assign_params(self, kw):
        for k, v in kw.items():
            if not hasattr(self.params, k):
                raise AttributeError(k)
            setattr(self.params, k, v)

    def set_bvh_builder(self, builder):
        """'sah' (host, default) or 'lbvh' (built on the GPU); applies to the next upload_scene / update_triangles"""
        self._call("set_bvh_builder", {"sah": 0, "lbvh": 1}[builder] if isinstance(builder, str) else int(builder))

    def upload_scene(self, sd):
        meshes, n_mesh, sp = _scene_tables(sd)
        self._call("upload_scene", ptr(sd.tri), ptr(sd.tri_mesh), sd.n_tri, C.cast(meshes, C.c_void_p), n_mesh, ptr(sd.materials), sd.materials.shape[0], sd.start_mat, ptr(sp))

    def upload_texture(self, vox=None, n=256):
        if vox is not None:
            vox = np.ascontiguousarray(vox, np.float32)
        self._call("upload_texture", ptr(vox), n)

    def set_transducer(self, pos, d):
        pos = np.ascontiguousarray(pos, np.float32); d = np.ascontiguousarray(d, np.float32)
        self._call("set_transducer", ptr(pos), ptr(d), pos.shape[0])


class Context(_SceneCalls):
    PREFIX = "mcrt_"

    def __init__(self, device=0, _borrowed=None):
        self.L = load_library()
        self.owned = _borrowed is None
        if self.owned:
            h = C.c_void_p()
            check(self.L.mcrt_create(device, C.byref(h)))
        else:                                   # a context that belongs to a Group (root / member): not destroyed here
            h = C.c_void_p(_borrowed)
        self.h = h
        self.params = Params()
        check(self.L.mcrt_default_params(C.byref(self.params)))

    def close(self):
        if getattr(self, "h", None):
            if self.owned:
                self.L.mcrt_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_params(self, **kw):
        self._assign_params(kw)
        check(self.L.mcrt_set_params(self.h, C.byref(self.params)))

    def set_stream(self, stream_ptr):
        check(self.L.mcrt_set_stream(self.h, C.c_void_p(stream_ptr) if stream_ptr else None))

    def synchronize(self):
        check(self.L.mcrt_synchronize(self.h))

    def debug_fast_paths(self):
        """(fast voxel quotient, branch-free voxel cell, entries of k_march's padded LDS image or 0) of the last traced frame"""
        out = (C.c_uint32 * 4)()
        check(self.L.mcrt_debug_fast_paths(self.h, out))
        return bool(out[0]), bool(out[1]), int(out[2])

    def debug_beam(self):
        """(bounce 1 ran by beams, rays the beams decided, leftover rays walked, beams cut at their capacity, beams refused, beams in use) of the last traced pass"""
        out = (C.c_uint32 * 6)()
        if hasattr(self.L, "mcrt_debug_beam"):
            check(self.L.mcrt_debug_beam(self.h, out))
        return bool(out[0]), int(out[1]), int(out[2]), int(out[3]), int(out[4]), int(out[5])

    def debug_beam_bounce(self, b):
        """debug_beam for bounce b, and (sampled rays whose group found no slot of the group table, slots claimed): mcrt_debug_beam_bounce"""
        out = (C.c_uint32 * 8)()
        if hasattr(self.L, "mcrt_debug_beam_bounce"):
            check(self.L.mcrt_debug_beam_bounce(self.h, int(b), out))
        return (bool(out[0]),) + tuple(int(v) for v in out[1:])

    def debug_beam_order(self, b):
        """(bounce b ran by beams through the beam order, rays placed, segments, pad lanes, (wavefront, beam) pairs the first pass met -- the last only
        with MCRT_BEAM_PAIRS=1) of the last traced pass: mcrt_debug_beam_order"""
        out = (C.c_uint32 * 5)()
        if hasattr(self.L, "mcrt_debug_beam_order"):
            check(self.L.mcrt_debug_beam_order(self.h, int(b), out))
        return (bool(out[0]),) + tuple(int(v) for v in out[1:])

    def debug_beam_records(self, b):
        """mcrt_debug_beam_records: what the beam stage of bounce b -- the LAST bounce the last traced pass or debug call ran by beams -- left behind, as a dict:
        n_beams, cap, near, groups, n_lists; records uint32 [n_beams][16] (view as float32: include/mcrt.h has the layout); lists uint32 [n_lists][cap][16]
        (v0 | id, v1 | begin depth, v2 | edge tolerance, 0 0 0 0); keys uint64 [groups].  McrtError where b is not that bounce."""
        info = (C.c_uint32 * 5)()
        check(self.L.mcrt_debug_beam_records(self.h, int(b), info, None, None, None))
        n_beams, cap, near, groups, n_lists = (int(v) for v in info)
        rec = np.zeros((n_beams, 16), np.uint32); lists = np.zeros((n_lists, cap, 16), np.uint32); keys = np.zeros(groups, np.uint64)
        check(self.L.mcrt_debug_beam_records(self.h, int(b), info, ptr(rec), ptr(lists), ptr(keys) if groups else None))
        return {"n_beams": n_beams, "cap": cap, "near": near, "groups": groups, "n_lists": n_lists, "records": rec, "lists": lists, "keys": keys}

    def debug_beam_entries(self, b):
        """mcrt_debug_beam_entries: what k_beam_collect stored of every list entry's triangle alone, for the bounce debug_beam_records(b) answers ->
        (entries uint32 [n_lists][cap][10] = the plane n.x n.y n.z dot(v0, n) | the padded bounds lo.x lo.y lo.z | hi.x hi.y hi.z, raw words of floats;
         begin_id uint32 [n_lists][cap][2] = the begin depth and the id stored beside them, which the list test reads in place of the list's words 7 and 3).
        Entries past a record's count are stale.  McrtError where b is not that bounce."""
        info = (C.c_uint32 * 5)()
        check(self.L.mcrt_debug_beam_entries(self.h, int(b), info, None, None))
        ent = np.zeros((int(info[4]), int(info[1]), 10), np.uint32); begin_id = np.zeros((int(info[4]), int(info[1]), 2), np.uint32)
        check(self.L.mcrt_debug_beam_entries(self.h, int(b), info, ptr(ent), ptr(begin_id)))
        return ent, begin_id

    def debug_beam_scan(self, counts):
        """mcrt_debug_beam_scan: the kernel that lays a beam order out (csrc/mcrt_beam.hip, k_beam_scan) run alone on `counts` rays per beam, the last the
        pseudo-beam's -> (bases uint32 [n], rays placed, segments, pad lanes, the order's length, the order buffer uint32 [length + 64]: BEAM_PAD in the padding
        of every segment, BEAM_SCAN_SENTINEL wherever the kernel wrote nothing -- the rays' places and the 64 guard words past the length)"""
        counts = np.ascontiguousarray(counts, np.uint32)
        bases = np.zeros(len(counts), np.uint32)
        order = np.zeros(host_beam_layout(counts)[4] + 64, np.uint32)
        out = (C.c_uint32 * 4)()
        check(self.L.mcrt_debug_beam_scan(self.h, ptr(counts), len(counts), ptr(bases), out, ptr(order)))
        return bases, int(out[0]), int(out[1]), int(out[2]), int(out[3]), order

    def debug_set_error(self, bits):
        """test hook: mark the context as an abandoned launch would (mcrt_debug_set_error)"""
        check(self.L.mcrt_debug_set_error(self.h, int(bits)))

    def update_triangles(self, tri):
        """new vertex positions [T,9] (numpy array, or a CUDA torch tensor) for the uploaded scene's triangles"""
        tri, n = _tri9(tri)
        check(self.L.mcrt_update_triangles(self.h, ptr(tri), n))

    def refit_triangles(self, tri):
        """new vertex positions [T,9] for the uploaded triangles, keeping the tree: boxes are refitted on the GPU"""
        tri, n = _tri9(tri)
        check(self.L.mcrt_refit_triangles(self.h, ptr(tri), n))

    def get_bvh(self):
        b = Bvh()
        check(self.L.mcrt_get_bvh(self.h, C.byref(b)))
        # (a tree built on the device has no BVH2: n_nodes == 0)
        nodes = np.frombuffer(C.string_at(b.nodes, 64 * b.n_nodes), dtype=NODE_DTYPE).copy() if b.n_nodes else np.zeros(0, NODE_DTYPE)
        btri = np.frombuffer(C.string_at(b.tri, 48 * b.n_tri), dtype=np.float32).reshape(-1, 12).copy()
        return nodes, btri, int(b.max_depth)

    def get_bvh4(self):
        b = Bvh4()
        check(self.L.mcrt_get_bvh4(self.h, C.byref(b)))
        return np.frombuffer(C.string_at(b.nodes, 128 * b.n_nodes), dtype=np.uint8).reshape(-1, 128).copy(), int(b.max_stack)

    # device memory
    def alloc(self, nbytes):
        p = C.c_void_p()
        check(self.L.mcrt_alloc(self.h, nbytes, C.byref(p)))
        return p.value

    def free(self, dev):
        check(self.L.mcrt_free(self.h, C.c_void_p(dev)))

    @contextlib.contextmanager
    def temp(self, nbytes):
        """`with ctx.temp(nbytes) as p:` -- device memory for the block, freed when it ends or raises"""
        p = self.alloc(nbytes)
        try:
            yield p
        finally:
            self.free(p)

    def d2h(self, dev, shape, dtype=np.float32):
        out = np.empty(shape, dtype)
        check(self.L.mcrt_memcpy_d2h(self.h, ptr(out), ptr(dev), out.nbytes))
        return out

    def h2d(self, dev, arr):
        arr = np.ascontiguousarray(arr)
        check(self.L.mcrt_memcpy_h2d(self.h, ptr(dev), ptr(arr), arr.nbytes))

    # frame
    def trace_frame(self, frame_id, rf_dev, e_begin=0, e_end=None):
        e_end = self.params.n_elements if e_end is None else e_end
        check(self.L.mcrt_trace_frame(self.h, frame_id, e_begin, e_end, ptr(rf_dev)))

    def trace_frames(self, frame_id, n_frames, rf_dev, e_begin=0, e_end=None):
        """n_frames consecutive frames in one pass; rf_dev holds [n_frames][e_end-e_begin][R] floats"""
        e_end = self.params.n_elements if e_end is None else e_end
        check(self.L.mcrt_trace_frames(self.h, frame_id, n_frames, e_begin, e_end, ptr(rf_dev)))

    def trace_frames_poses(self, frame_id, pos, dirs, rf_dev, e_begin=0, e_end=None, n_frames=None):
        """a pass with a probe pose per frame: pos / dirs [F][E][3] (numpy arrays, CUDA torch tensors, or raw device pointers with
        n_frames given); rf_dev [F][e_end-e_begin][R]"""
        e_end = self.params.n_elements if e_end is None else e_end
        pos, dirs, n_frames = _pose_tables("trace_frames_poses", pos, dirs, n_frames, self.params.n_elements)
        check(self.L.mcrt_trace_frames_poses(self.h, frame_id, n_frames, e_begin, e_end, ptr(pos), ptr(dirs), ptr(rf_dev)))

    def trace_frame_debug(self, frame_id, rf_dev, e_begin=0, e_end=None, want_hits=True, want_segs=False):
        e_end = self.params.n_elements if e_end is None else e_end
        ne, S, B = e_end - e_begin, self.params.n_samples, self.params.max_depth
        hits = np.full((ne, S, B), -3, np.int32) if want_hits else None
        segs = np.zeros((ne, S, B), SEGMENT_DTYPE) if want_segs else None
        cnt = np.zeros((ne, S), np.uint32) if want_segs else None
        check(self.L.mcrt_trace_frame_debug(self.h, frame_id, e_begin, e_end, ptr(rf_dev), ptr(hits), ptr(segs), ptr(cnt)))
        return hits, segs, cnt

    def cast_rays(self, frame_id, e_begin=0, e_end=None, want_hits=True):
        e_end = self.params.n_elements if e_end is None else e_end
        ne, S, B = e_end - e_begin, self.params.n_samples, self.params.max_depth
        segs = np.zeros((ne, S, B), SEGMENT_DTYPE); cnt = np.zeros((ne, S), np.uint32)
        hits = np.full((ne, S, B), -3, np.int32) if want_hits else None
        check(self.L.mcrt_cast_rays(self.h, frame_id, e_begin, e_end, ptr(segs), ptr(cnt), ptr(hits)))
        return segs, cnt, hits

    def convolve_frames(self, rf_dev, n_frames, n_elements, n_rows, axial, lateral):
        """rf_image::convolve on the [n_frames][E][R] images of a trace_frames pass, one launch per convolution pass"""
        ax = np.ascontiguousarray(axial, np.float32); lat = np.ascontiguousarray(lateral, np.float32)
        check(self.L.mcrt_convolve_frames(self.h, ptr(rf_dev), n_frames, n_elements, n_rows, ptr(ax), ax.size, ptr(lat), lat.size))

    def convolve_frames_depth(self, rf_dev, n_frames, n_elements, n_rows, axial, lat_rows):
        """mcrt_convolve_frames_depth: the convolution with the lateral taps of each RF row, lat_rows [n_rows][n_lat] (focal zones)"""
        ax = np.ascontiguousarray(axial, np.float32); lat = np.ascontiguousarray(lat_rows, np.float32)
        if lat.ndim != 2 or lat.shape[0] != n_rows:
            raise ValueError("lat_rows needs one row of taps per RF row: (%d, n_lat), got shape %s" % (n_rows, lat.shape))
        check(self.L.mcrt_convolve_frames_depth(self.h, ptr(rf_dev), n_frames, n_elements, n_rows, ptr(ax), ax.size, ptr(lat), lat.shape[1]))

    def convolve_bands_frames(self, rf_dev, n_frames, n_elements, n_rows, ax_rows, bands_dev, lateral=None, lat_rows=None):
        """mcrt_convolve_bands_frames: rf_dev [n_frames][E][R] convolved into bands_dev [n_frames][B][E][R] with the axial taps of each band and
        RF row, ax_rows [B][n_rows][n_ax], and either the lateral taps `lateral` [n_lat] or a row of them per RF row, lat_rows [n_rows][n_lat]"""
        ax = np.ascontiguousarray(ax_rows, np.float32)
        if ax.ndim != 3 or ax.shape[1] != n_rows:
            raise ValueError("ax_rows needs one row of taps per band and RF row: (B, %d, n_ax), got shape %s" % (n_rows, ax.shape))
        lat = np.ascontiguousarray(lateral, np.float32) if lateral is not None else None
        rows = np.ascontiguousarray(lat_rows, np.float32) if lat_rows is not None else None
        if rows is not None and (rows.ndim != 2 or rows.shape[0] != n_rows):
            raise ValueError("lat_rows needs one row of taps per RF row: (%d, n_lat), got shape %s" % (n_rows, rows.shape))
        n_lat = rows.shape[1] if rows is not None else lat.size if lat is not None else 0
        check(self.L.mcrt_convolve_bands_frames(self.h, ptr(rf_dev), n_frames, n_elements, n_rows, ax.shape[0], ptr(ax), ax.shape[2], ptr(lat), ptr(rows), n_lat, ptr(bands_dev)))

    def band_fold_frames(self, bands_dev, n_frames, n_bands, n_elements, n_rows, w_rows, rf_dev):
        """mcrt_band_fold_frames: the band stacks [n_frames][B][E][R] folded into rf_dev [n_frames][E][R] with w_rows [n_rows][B]"""
        w = np.ascontiguousarray(w_rows, np.float32)
        if w.shape != (n_rows, n_bands):
            raise ValueError("w_rows needs one row of weights per RF row: (%d, %d), got shape %s" % (n_rows, n_bands, w.shape))
        check(self.L.mcrt_band_fold_frames(self.h, ptr(bands_dev), n_frames, n_bands, n_elements, n_rows, ptr(w), ptr(rf_dev)))

    def elevation_frames(self, planes_dev, n_frames, n_planes, n_elements, n_rows, w_rows, rf_dev):
        """mcrt_elevation_frames: the plane stacks [n_frames][K][E][R] folded into rf_dev [n_frames][E][R] with w_rows [n_rows][K]"""
        w = np.ascontiguousarray(w_rows, np.float32)
        if w.shape != (n_rows, n_planes):
            raise ValueError("w_rows needs one row of weights per RF row: (%d, %d), got shape %s" % (n_rows, n_planes, w.shape))
        check(self.L.mcrt_elevation_frames(self.h, ptr(planes_dev), n_frames, n_planes, n_elements, n_rows, ptr(w), ptr(rf_dev)))

    def convolve(self, rf_dev, n_elements, n_rows, axial, lateral):
        ax =np.ascontiguousarray(axial, np.float32); lat = np.ascontiguousarray(lateral, np.float32)
        check(self.L.mcrt_convolve(self.h, ptr(rf_dev), n_elements, n_rows, ptr(ax), ax.size, ptr(lat), lat.size))

    def envelope(self, rf_dev, n_elements, n_rows):
        check(self.L.mcrt_envelope(self.h, ptr(rf_dev), n_elements, n_rows))

    def envelope_frames(self, rf_dev, n_frames, n_elements, n_rows):
        check(self.L.mcrt_envelope_frames(self.h, ptr(rf_dev), n_frames, n_elements, n_rows))

    def detect_frames(self, rf_dev, n_frames, n_elements, n_rows, env_dev=None, iq_dev=None, n_taps=None):
        """mcrt_detect_frames: quadrature detection of the stack [n_frames][E][R] -> env_dev [n_frames][E][R] (may be rf_dev: in place) and / or
        iq_dev [n_frames][E][R][2], the RF and its FIR Hilbert transform; n_taps: 3, 7, 11, ..., 63 (None: 31)"""
        o = detect_opts_struct(n_taps)
        check(self.L.mcrt_detect_frames(self.h, ptr(rf_dev), n_frames, n_elements, n_rows, C.byref(o), ptr(env_dev), ptr(iq_dev)))

    def flow_split_frames(self, rf_dev, tissue_dev, n_frames, n_elements, n_rows, moving, out_dev):
        """mcrt_flow_split_frames: the raw trace [n_frames][E][R] cut by its tissue labels into out_dev [n_frames][2][E][R] -- image 0 what
        stands still, image 1 what moves; moving: a host byte per label (non-zero: the material moves)"""
        mv = np.ascontiguousarray(moving, np.uint8).reshape(-1)
        check(self.L.mcrt_flow_split_frames(self.h, ptr(rf_dev), ptr(tissue_dev), n_frames, n_elements, n_rows, ptr(mv), mv.size, ptr(out_dev)))

    def flow_frames(self, iq_static_dev, iq_moving_dev, tissue_dev, n_frames, n_elements, n_rows, v_nyq_mm_s, phasor, truth, first_image_id=0,
                    sigma_dev=None, corr_dev=None, vel_dev=None, var_dev=None, truth_dev=None, opts=None, **kw):
        """mcrt_flow_frames: the colour processor -- the slow-time ensemble of every sample from the detected pairs [n_frames][E][R][2] of what
        stands still (or None) and what moves, the wall filter, the autocorrelation averaged over a window, and the Kasai estimates.
        phasor [n_labels][E][2] and truth [n_labels][E]: host tables (host_flow_phasors).  sigma_dev: [n_frames] floats on the device (the
        sigma_dev of noise_frames) or None: the options' sigma.  Outputs, each a device pointer or None: corr_dev [n_frames][3][E][R],
        vel_dev, var_dev and truth_dev [n_frames][E][R].  opts: a FlowOpts, or the keywords of flow_opts_struct"""
        o = opts if opts is not None else flow_opts_struct(**kw)
        ph = np.ascontiguousarray(phasor, np.float32); tr = np.ascontiguousarray(truth, np.float32)
        if ph.ndim != 3 or ph.shape[1:] != (n_elements, 2) or tr.shape != ph.shape[:2]:
            raise ValueError("phasor takes [n_labels][%d][2] and truth [n_labels][%d], got %s and %s" % (n_elements, n_elements, ph.shape, tr.shape))
        check(self.L.mcrt_flow_frames(self.h, ptr(iq_static_dev), ptr(iq_moving_dev), ptr(tissue_dev), n_frames, n_elements, n_rows, C.byref(o), float(v_nyq_mm_s),
                                      ptr(ph), ptr(tr), ph.shape[0], first_image_id, ptr(sigma_dev), ptr(corr_dev), ptr(vel_dev), ptr(var_dev), ptr(truth_dev)))

    def colour_frames(self, corr_img_dev, grey_dev, n_frames, height, width, v_nyq_mm_s, rgb_dev, vel_img_dev=None, lut=None, **opts):
        """mcrt_colour_frames: the flow overlay -- the gathered autocorrelation [n_frames][3][H][W] over the B-mode bytes [n_frames][H][W] ->
        rgb_dev [n_frames][H][W][3] bytes and, where given, vel_img_dev [n_frames][H][W] floats.  lut: uint8 [256][3] (None: host_colour_map());
        opts: the keywords of colour_opts_struct"""
        o = colour_opts_struct(**opts)
        table = np.ascontiguousarray(host_colour_map() if lut is None else lut, np.uint8)
        if table.shape != (256, 3):
            raise ValueError("lut takes uint8 [256][3], got shape %s" % (table.shape,))
        check(self.L.mcrt_colour_frames(self.h, ptr(corr_img_dev), ptr(grey_dev), n_frames, height, width, ptr(table), C.byref(o), float(v_nyq_mm_s),
                                        ptr(rgb_dev), ptr(vel_img_dev)))

    def spectral_series_frames(self, iq_static_dev, iq_moving_dev, n_frames, n_elements, n_rows, gates, weight, rate, phase, series_dev, first_image_id=0,
                               sigma_dev=None, opts=None, **kw):
        """mcrt_spectral_series_frames: the slow-time series of every sample gate, series_dev [n_gates][T][2], from the detected pairs
        [n_frames][E][R][2] of what stands still (or None) and what moves.  gates: (image, line, row0) per gate; weight float32 [G]; rate
        int32 [n_gates][G] (host_spectral_rates); phase int64 [T] (host_spectral_phase) -- host tables.  n_pulses and gate_rows default to
        the tables' own lengths.  opts: a SpectralOpts, or the keywords of spectral_opts_struct"""
        g = np.ascontiguousarray(gates, np.uint32).reshape(-1, 3)
        w = np.ascontiguousarray(weight, np.float32).reshape(-1); ph = np.ascontiguousarray(phase, np.int64).reshape(-1)
        rt = np.ascontiguousarray(rate, np.int32)
        if opts is None:
            kw.setdefault("n_pulses", ph.size); kw.setdefault("gate_rows", w.size)
        o = opts if opts is not None else spectral_opts_struct(**kw)
        if ph.size != o.n_pulses or w.size != o.gate_rows or rt.size != g.shape[0] * o.gate_rows:
            raise ValueError("the tables take phase [%d], weight [%d] and rate [%d][%d], got %s, %s and %s" % (o.n_pulses, o.gate_rows, g.shape[0], o.gate_rows,
                                                                                                             ph.shape, w.shape, rt.shape))
        check(self.L.mcrt_spectral_series_frames(self.h, ptr(iq_static_dev), ptr(iq_moving_dev), n_frames, n_elements, n_rows, ptr(g), g.shape[0], ptr(w), ptr(rt),
                                                 ptr(ph), C.byref(o), first_image_id, ptr(sigma_dev), ptr(series_dev)))

    def spectral_frames(self, series_dev, n_gates, v_nyq_mm_s, power_dev=None, mean_dev=None, window="hann", opts=None, **kw):
        """mcrt_spectral_frames: the short-time FFT of every gate's series [n_gates][T][2] -> power_dev [n_gates][n_cols][N] in velocity order
        and / or mean_dev [n_gates][n_cols], n_cols = (T - N) // hop + 1.  window: "rect" | "hann" or float32 [N]; opts: a SpectralOpts, or the
        keywords of spectral_opts_struct"""
        o = opts if opts is not None else spectral_opts_struct(**kw)
        h = host_spectral_window(window, o.n_fft) if isinstance(window, (str, int)) else np.ascontiguousarray(window, np.float32).reshape(-1)
        if h.size != o.n_fft:
            raise ValueError("window takes float32 [%d], got shape %s" % (o.n_fft, h.shape))
        check(self.L.mcrt_spectral_frames(self.h, ptr(series_dev), n_gates, ptr(h), C.byref(o), float(v_nyq_mm_s), ptr(power_dev), ptr(mean_dev)))

    def sonogram_frames(self, power_dev, n_gates, n_cols, n_fft, out_dev, peak_dev=None, **opts):
        """mcrt_sonogram_frames: the spectra [n_gates][n_cols][N] -> the displayed bytes out_dev [n_gates][N][n_cols], row 0 the highest
        velocity towards the probe, and, where given, each gate's largest finite power peak_dev [n_gates].  opts: the keywords of
        sonogram_opts_struct"""
        o = sonogram_opts_struct(**opts)
        check(self.L.mcrt_sonogram_frames(self.h, ptr(power_dev), n_gates, n_cols, n_fft, C.byref(o), ptr(peak_dev), ptr(out_dev)))

    def strain_compress_frames(self, iq_dev, tissue_dev, n_frames, n_elements, n_rows, eps_q24, cycles_per_row, first_image_id=0, sigma_dev=None,
                               post_iq_dev=None, truth_disp_dev=None, truth_strain_dev=None, opts=None, **kw):
        """mcrt_strain_compress_frames: the post-compression pairs of every scan-line from the detected pairs [n_frames][E][R][2] and the
        tissue labels [n_frames][E][R].  eps_q24: int32 [n_labels], a host table (host_strain_table); cycles_per_row: host_psf_carrier's.
        Outputs, each a device pointer or None: post_iq_dev [n_frames][E][R][2], truth_disp_dev and truth_strain_dev [n_frames][E][R].
        opts: a StrainOpts, or the keywords of strain_opts_struct"""
        o = opts if opts is not None else strain_opts_struct(**kw)
        eps = np.ascontiguousarray(eps_q24, np.int32).reshape(-1)
        check(self.L.mcrt_strain_compress_frames(self.h, ptr(iq_dev), ptr(tissue_dev), n_frames, n_elements, n_rows, ptr(eps), eps.size, float(cycles_per_row),
                                                 C.byref(o), first_image_id, ptr(sigma_dev), ptr(post_iq_dev), ptr(truth_disp_dev), ptr(truth_strain_dev)))

    def strain_frames(self, pre_iq_dev, post_iq_dev, n_frames, n_elements, n_rows, cycles_per_row, disp_dev=None, rho_dev=None, strain_dev=None, opts=None, **kw):
        """mcrt_strain_frames: speckle tracking between the two stacks of pairs [n_frames][E][R][2] -> disp_dev (rows, positive: compression),
        rho_dev (the correlation coefficient) and strain_dev (the least-squares slope of the displacement), each [n_frames][E][R] or None.
        opts: a StrainOpts, or the keywords of strain_opts_struct"""
        o = opts if opts is not None else strain_opts_struct(**kw)
        check(self.L.mcrt_strain_frames(self.h, ptr(pre_iq_dev), ptr(post_iq_dev), n_frames, n_elements, n_rows, C.byref(o), float(cycles_per_row),
                                        ptr(disp_dev), ptr(rho_dev), ptr(strain_dev)))

    def elastogram_frames(self, strain_img_dev, rho_img_dev, grey_dev, n_frames, height, width, rgb_dev, lut=None, **opts):
        """mcrt_elastogram_frames: the strain overlay -- the gathered strain and correlation coefficient [n_frames][H][W] over the B-mode bytes
        [n_frames][H][W] -> rgb_dev [n_frames][H][W][3] bytes.  lut: uint8 [256][3] (None: host_strain_map()); opts: the keywords of
        elastogram_opts_struct"""
        o = elastogram_opts_struct(**opts)
        table = np.ascontiguousarray(host_strain_map() if lut is None else lut, np.uint8)
        if table.shape != (256, 3):
            raise ValueError("lut takes uint8 [256][3], got shape %s" % (table.shape,))
        check(self.L.mcrt_elastogram_frames(self.h, ptr(strain_img_dev), ptr(rho_img_dev), ptr(grey_dev), n_frames, height, width, ptr(table), C.byref(o),
                                            ptr(rgb_dev)))

    def shear_wave_frames(self, iq_dev, tissue_dev, n_frames, n_elements, n_rows, slow_q16, speed_f, pitch_q8, shape_q16, amp_q16, cycles_per_row,
                          first_image_id=0, sigma_dev=None, peak_time_dev=None, peak_disp_dev=None, disp_dev=None, truth_arrival_dev=None,
                          truth_speed_dev=None, opts=None, **kw):
        """mcrt_shear_wave_frames: the shear wave of a push, tracked over slow time, from the detected pairs [n_frames][E][R][2] and the tissue
        labels [n_frames][E][R].  Host tables: slow_q16 int64 and speed_f float32 [n_labels] (host_shear_table), pitch_q8 uint32 [R]
        (host_shear_pitch), shape_q16 (host_shear_shape) and amp_q16 (host_shear_decay) uint32; cycles_per_row: host_psf_carrier's.
        Outputs, each a device pointer or None: peak_time_dev, peak_disp_dev, truth_arrival_dev, truth_speed_dev [n_frames][E][R] and disp_dev
        [n_frames][n_pulses][E][R].  opts: a ShearOpts, or the keywords of shear_opts_struct"""
        o = opts if opts is not None else shear_opts_struct(**kw)
        slow = np.ascontiguousarray(slow_q16, np.int64).reshape(-1); speed = np.ascontiguousarray(speed_f, np.float32).reshape(-1)
        if slow.size != speed.size:
            raise ValueError("slow_q16 and speed_f take one entry per label, got %d and %d" % (slow.size, speed.size))
        pitch = np.ascontiguousarray(pitch_q8, np.uint32).reshape(-1)
        if pitch.size != n_rows:
            raise ValueError("pitch_q8 takes one entry per row, got %d for %d rows" % (pitch.size, n_rows))
        shape = np.ascontiguousarray(shape_q16, np.uint32).reshape(-1); amp = np.ascontiguousarray(amp_q16, np.uint32).reshape(-1)
        check(self.L.mcrt_shear_wave_frames(self.h, ptr(iq_dev), ptr(tissue_dev), n_frames, n_elements, n_rows, ptr(slow), ptr(speed), slow.size, ptr(pitch),
                                            ptr(shape), shape.size, ptr(amp), amp.size, float(cycles_per_row), C.byref(o), first_image_id, ptr(sigma_dev),
                                            ptr(peak_time_dev), ptr(peak_disp_dev), ptr(disp_dev), ptr(truth_arrival_dev), ptr(truth_speed_dev)))

    def shear_speed_frames(self, peak_time_dev, n_frames, n_elements, n_rows, pitch_mm, speed_dev=None, modulus_dev=None, quality_dev=None, opts=None, **kw):
        """mcrt_shear_speed_frames: the least-squares slope of the time to peak [n_frames][E][R] across scan-lines -> speed_dev (m/s),
        modulus_dev (kPa) and quality_dev (the r^2 of the fit), each [n_frames][E][R] or None.  pitch_mm: float32 [R], a host table
        (host_shear_pitch).  opts: a ShearOpts, or the keywords of shear_opts_struct"""
        o = opts if opts is not None else shear_opts_struct(**kw)
        pitch = np.ascontiguousarray(pitch_mm, np.float32).reshape(-1)
        if pitch.size != n_rows:
            raise ValueError("pitch_mm takes one entry per row, got %d for %d rows" % (pitch.size, n_rows))
        check(self.L.mcrt_shear_speed_frames(self.h, ptr(peak_time_dev), n_frames, n_elements, n_rows, ptr(pitch), C.byref(o), ptr(speed_dev), ptr(modulus_dev),
                                             ptr(quality_dev)))

    def mmode_lines_frames(self, iq_dev, tissue_dev, n_frames, n_elements, n_rows, lines, dil_q24, w_q16, bulk_q24, cycles_per_row, first_image_id=0,
                           sigma_dev=None, env_dev=None, iq_out_dev=None, truth_disp_dev=None, truth_label_dev=None, opts=None, **kw):
        """mcrt_mmode_lines_frames: the pulses of the named scan-lines from the detected pairs [n_frames][E][R][2] and the tissue labels
        [n_frames][E][R].  lines: [n_lines][2] (image, scan-line); dil_q24: int32 [n_labels] (host_mmode_table); w_q16 and bulk_q24: int32
        [T] each (host_mmode_waveform, host_mmode_bulk), all host tables; n_pulses is their length; cycles_per_row: host_psf_carrier's.
        Outputs, each a device pointer or None: env_dev, truth_disp_dev (float32) and truth_label_dev (uint8) [n_lines][T][R], iq_out_dev
        [n_lines][T][R][2].  opts: a MmodeOpts, or the keywords of mmode_opts_struct (sigma, seed)"""
        ln = np.ascontiguousarray(lines, np.uint32).reshape(-1, 2)
        dil = np.ascontiguousarray(dil_q24, np.int32).reshape(-1)
        w = np.ascontiguousarray(w_q16, np.int32).reshape(-1)
        bulk = np.ascontiguousarray(bulk_q24, np.int32).reshape(-1)
        if w.size != bulk.size:
            raise ValueError("w_q16 and bulk_q24 take one entry per pulse each, got %d and %d" % (w.size, bulk.size))
        o = opts if opts is not None else mmode_opts_struct(n_pulses=w.size, **kw)
        if o.n_pulses != w.size:
            raise ValueError("the tables hold %d pulses, the options ask for %d" % (w.size, o.n_pulses))
        check(self.L.mcrt_mmode_lines_frames(self.h, ptr(iq_dev), ptr(tissue_dev), n_frames, n_elements, n_rows, ptr(ln), ln.shape[0], ptr(dil), dil.size, ptr(w),
                                             ptr(bulk), float(cycles_per_row), C.byref(o), first_image_id, ptr(sigma_dev), ptr(env_dev), ptr(iq_out_dev),
                                             ptr(truth_disp_dev), ptr(truth_label_dev)))

    def mmode_picture_frames(self, env_dev, n_lines, n_pulses, n_rows, out_dev, truth_label_dev=None, truth_disp_dev=None, peak_dev=None, mean_dev=None,
                             label_out_dev=None, disp_out_dev=None, opts=None, **kw):
        """mcrt_mmode_picture_frames: the sweep display of the M-lines' envelopes [n_lines][T][R] -> out_dev uint8 [n_lines][H][W], W = T // hop;
        optional peak_dev [n_lines], mean_dev [n_lines][W][R], and the truths registered pixel for pixel: label_out_dev uint8 (from
        truth_label_dev) and disp_out_dev float32 (from truth_disp_dev), each [n_lines][H][W].  opts: a MmodeDisplayOpts, or the keywords of
        mmode_display_opts_struct"""
        o = opts if opts is not None else mmode_display_opts_struct(**kw)
        check(self.L.mcrt_mmode_picture_frames(self.h, ptr(env_dev), ptr(truth_label_dev), ptr(truth_disp_dev), n_lines, n_pulses, n_rows, C.byref(o), ptr(peak_dev),
                                               ptr(mean_dev), ptr(out_dev), ptr(label_out_dev), ptr(disp_out_dev)))

    def scan_convert_frames(self, rf_dev, n_frames, n_elements, n_rows, out_dev, radius_mm=30.0, total_angle=DEFAULT_ANGLE, out_rows=400, out_cols=500):
        check(self.L.mcrt_scan_convert_frames(self.h, ptr(rf_dev), n_frames, n_elements, n_rows, radius_mm, total_angle, ptr(out_dev), out_rows, out_cols))

    def scan_convert(self, rf_dev, n_elements, n_rows, out_dev, radius_mm=30.0, total_angle=DEFAULT_ANGLE, out_rows=400, out_cols=500):
        check(self.L.mcrt_scan_convert(self.h, ptr(rf_dev), n_elements, n_rows, radius_mm, total_angle, ptr(out_dev), out_rows, out_cols))

    def bmode_frames(self, rf_dev, n_frames, n_elements, n_rows, out_dev, *, mode="db", dynamic_range_db=60.0, gain_db=0.0, ref=None, tgc_db=None,
                     persistence=0.0, state_dev=None, reset_state=True, peak_dev=None, radius_mm=30.0, total_angle=DEFAULT_ANGLE,
                     out_rows=400, out_cols=500):
        """mcrt_bmode_frames: [n_frames][E][R] device floats -> [n_frames][out_rows][out_cols] device bytes (log-compressed B-mode).
        mode "db" or "ref_log"; ref None (or <= 0): each frame's own peak; tgc_db: dB per RF row (n_rows values) or None."""
        p = bmode_params(mode=mode, dynamic_range_db=dynamic_range_db, gain_db=gain_db, ref=ref, persistence=persistence, reset_state=reset_state,
                         radius_mm=radius_mm, total_angle=total_angle, out_rows=out_rows, out_cols=out_cols)
        tgc = _tgc_rows(tgc_db, n_rows)
        check(self.L.mcrt_bmode_frames(self.h, ptr(rf_dev), n_frames, n_elements, n_rows, C.byref(p), ptr(tgc), ptr(state_dev), ptr(peak_dev), ptr(out_dev)))

    def compound_frames(self, rf_dev, n_frames, n_elements, n_rows, steer_rad, out_dev, radius_mm=30.0, total_angle=DEFAULT_ANGLE, out_rows=400, out_cols=500,
                        mode="mean", view_weights=None, feather_lines=0.0):
        """mcrt_compound_frames: the views [n_frames][N][E][R] of steer_rad's N angles -> device floats [n_frames][out_rows][out_cols], every
        pixel the mean of the views that cover it.  mode "mean" / "max" / "median", view_weights and feather_lines (a lateral edge ramp in
        scan-lines) go through mcrt_compound_frames_opts; with all three at their defaults the call is mcrt_compound_frames."""
        cp = compound_struct(steer_rad)
        if _compound_defaults(mode, view_weights, feather_lines):
            check(self.L.mcrt_compound_frames(self.h, ptr(rf_dev), n_frames, n_elements, n_rows, radius_mm, total_angle, C.byref(cp), ptr(out_dev), out_rows, out_cols))
            return
        o = compound_opts_struct(mode, view_weights, feather_lines)
        check(self.L.mcrt_compound_frames_opts(self.h, ptr(rf_dev), n_frames, n_elements, n_rows, radius_mm, total_angle, C.byref(cp), ptr(out_dev), out_rows, out_cols,
                                               C.byref(o)))

    def bmode_compound_frames(self, rf_dev, n_frames, n_elements, n_rows, steer_rad, out_dev, *, mode="db", dynamic_range_db=60.0, gain_db=0.0, ref=None,
                              tgc_db=None, persistence=0.0, state_dev=None, reset_state=True, peak_dev=None, radius_mm=30.0,
                              total_angle=DEFAULT_ANGLE, out_rows=400, out_cols=500, compound_mode="mean", view_weights=None, feather_lines=0.0):
        """mcrt_bmode_compound_frames: bmode_frames over the views [n_frames][N][E][R] of steer_rad's N angles; the automatic reference of a
        frame is the peak over all its views.  compound_mode "mean" / "max" / "median" (mode is the grey curve's), view_weights and
        feather_lines go through mcrt_bmode_compound_frames_opts; with all three at their defaults the call is mcrt_bmode_compound_frames."""
        p = bmode_params(mode=mode, dynamic_range_db=dynamic_range_db, gain_db=gain_db, ref=ref, persistence=persistence, reset_state=reset_state,
                         radius_mm=radius_mm, total_angle=total_angle, out_rows=out_rows, out_cols=out_cols)
        cp = compound_struct(steer_rad)
        tgc = _tgc_rows(tgc_db, n_rows)
        if _compound_defaults(compound_mode, view_weights, feather_lines):
            check(self.L.mcrt_bmode_compound_frames(self.h, ptr(rf_dev), n_frames, n_elements, n_rows, C.byref(p), C.byref(cp), ptr(tgc), ptr(state_dev),
                                                    ptr(peak_dev), ptr(out_dev)))
            return
        o = compound_opts_struct(compound_mode, view_weights, feather_lines)
        check(self.L.mcrt_bmode_compound_frames_opts(self.h, ptr(rf_dev), n_frames, n_elements, n_rows, C.byref(p), C.byref(cp), ptr(tgc), ptr(state_dev),
                                                     ptr(peak_dev), ptr(out_dev), C.byref(o)))

    def volume_frames(self, rf_dev, n_frames, n_elements, n_rows, sweep, grid, out_dev, radius_mm=30.0, total_angle=DEFAULT_ANGLE):
        """mcrt_volume_frames: the planes [n_frames][K][E][R] of a sweep -> device floats [n_frames][nw][nv][nu] at grid's points.
        sweep: an mcrt_sweep (sweep_struct) or (K, step_rad[, pivot_mm])"""
        sw = _as_sweep(sweep)
        check(self.L.mcrt_volume_frames(self.h, ptr(rf_dev), n_frames, n_elements, n_rows, radius_mm, total_angle, C.byref(sw), C.byref(grid), ptr(out_dev)))

    def bmode_volume_frames(self, rf_dev, n_frames, n_elements, n_rows, sweep, grid, out_dev, *, mode="db", dynamic_range_db=60.0, gain_db=0.0, ref=None,
                            tgc_db=None, persistence=0.0, peak_dev=None, radius_mm=30.0, total_angle=DEFAULT_ANGLE):
        """mcrt_bmode_volume_frames: bmode_frames over the planes [n_frames][K][E][R] of a sweep, bytes [n_frames][nw][nv][nu]; the automatic
        reference of a frame is the peak over its whole sweep.  persistence must stay 0 (the library refuses anything else)"""
        p = bmode_params(mode=mode, dynamic_range_db=dynamic_range_db, gain_db=gain_db, ref=ref, persistence=persistence, radius_mm=radius_mm,
                         total_angle=total_angle, out_rows=0, out_cols=0)
        sw = _as_sweep(sweep)
        tgc = _tgc_rows(tgc_db, n_rows)
        check(self.L.mcrt_bmode_volume_frames(self.h, ptr(rf_dev), n_frames, n_elements, n_rows, C.byref(p), C.byref(sw), C.byref(grid), ptr(tgc), ptr(peak_dev),
                                              ptr(out_dev)))

    def render_frames(self, vol_dev, n_frames, shape, view, out_dev=None, out8_dev=None, depth_dev=None, in_u8=False, **opts):
        """mcrt_render_frames: the voxel blocks [n_frames][nw][nv][nu] (shape = (nw, nv, nu); floats, or bytes with in_u8) seen through view
        (render_view, or a RenderView filled by hand) -> device floats, bytes and step indices [n_frames][ny][nx], each where a pointer is
        given.  opts: the keywords of render_opts_struct (mode, lo, hi, threshold, ramp, opacity, depth_cue, t_cut)"""
        nw, nv, nu = shape
        o = render_opts_struct(in_u8, **opts)
        check(self.L.mcrt_render_frames(self.h, ptr(vol_dev), 1 if in_u8 else 0, n_frames, nu, nv, nw, C.byref(view), C.byref(o), ptr(out_dev), ptr(out8_dev),
                                        ptr(depth_dev)))

    def speckle_frames(self, in_dev, n_frames, height, width, out_dev=None, **opts):
        """mcrt_speckle_frames: speckle-reducing anisotropic diffusion over the float stack [n_frames][height][width] (width contiguous: the
        enveloped RF stack is height = E, width = R) -> out_dev (None: in place).  opts: the keywords of speckle_opts_struct (n_iter, q0, rho,
        lambda_)"""
        o = speckle_opts_struct(**opts)
        check(self.L.mcrt_speckle_frames(self.h, ptr(in_dev), n_frames, height, width, C.byref(o), ptr(in_dev if out_dev is None else out_dev)))

    def speckle_volume_frames(self, in_dev, n_frames, shape, out_dev=None, **opts):
        """mcrt_speckle_volume_frames: the diffusion of speckle_frames with six neighbours over the float voxel blocks [n_frames][nw][nv][nu]
        (shape = (nw, nv, nu)) -> out_dev (None: in place).  opts: the keywords of speckle3d_opts_struct (n_iter, q0, rho, lambda_,
        weights)"""
        nw, nv, nu = shape
        o = speckle3d_opts_struct(**opts)
        check(self.L.mcrt_speckle_volume_frames(self.h, ptr(in_dev), n_frames, nu, nv, nw, C.byref(o), ptr(in_dev if out_dev is None else out_dev)))

    def recon_frames(self, stack_dev, pos, dirs, n_frames, n_elements, n_rows, grid, out_dev, count_dev=None, stats_dev=None, row_mm=None, unit_mm=10.0,
                     **opts):
        """mcrt_recon_frames: the tracked stack [n_frames][n_elements][n_rows] binned into grid's voxels (a VolumeGrid in the WORLD frame, mm)
        by the pose tables pos / dirs [F][E][3] it was traced with (numpy arrays, CUDA torch tensors or raw device pointers) -> out_dev float
        [nw][nv][nu], count_dev uint32 the same, stats_dev uint32 [2].  row_mm None: depth_mm_f / n_rows, the row pitch of mcrt_volume_maps.
        opts: the keywords of recon_opts_struct (mode, value_max, fill_radius, fill_min, empty)"""
        o = recon_opts_struct(**opts)
        if row_mm is None:
            row_mm = _depth_mm_f(self.params.depth_cm, self.params.speed_of_sound) / n_rows
        pos, dirs, n_frames = _pose_tables("recon_frames", pos, dirs, n_frames, n_elements)
        check(self.L.mcrt_recon_frames(self.h, ptr(stack_dev), n_frames, n_elements, n_rows, ptr(pos), ptr(dirs), float(row_mm), float(unit_mm), C.byref(grid),
                                       C.byref(o), ptr(out_dev), ptr(count_dev), ptr(stats_dev)))

    def recon_label_frames(self, tissue_dev, pos, dirs, n_frames, n_elements, n_rows, grid, n_labels, out_dev=None, count_dev=None, votes_dev=None,
                           stats_dev=None, row_mm=None, unit_mm=10.0, **opts):
        """mcrt_recon_label_frames: the tissue stack uint8 [n_frames][n_elements][n_rows] that label_frames wrote for the pose tables pos / dirs
        voted into grid's voxels (a VolumeGrid in the WORLD frame, mm) -> out_dev uint8 [nw][nv][nu] (the label with the most votes, holes
        filled from their sampled neighbours, LABEL_NONE where nothing is near), count_dev uint32 the same (votes per voxel), votes_dev uint32
        the same (the winner's), stats_dev uint32 [2]; at least one of them.  row_mm None: as recon_frames.  opts: fill_radius, fill_min"""
        o = recon_label_opts_struct(n_labels, **opts)
        if row_mm is None:
            row_mm = _depth_mm_f(self.params.depth_cm, self.params.speed_of_sound) / n_rows
        pos, dirs, n_frames = _pose_tables("recon_label_frames", pos, dirs, n_frames, n_elements)
        check(self.L.mcrt_recon_label_frames(self.h, ptr(tissue_dev), n_frames, n_elements, n_rows, ptr(pos), ptr(dirs), float(row_mm), float(unit_mm), C.byref(grid),
                                             C.byref(o), ptr(out_dev), ptr(count_dev), ptr(votes_dev), ptr(stats_dev)))

    def render_label_frames(self, label_dev, n_frames, shape, view, depth_dev, out_dev):
        """mcrt_render_label_frames: the label blocks uint8 [n_frames][nw][nv][nu] (shape = (nw, nv, nu)) read where render_frames' depth_dev
        [n_frames][ny][nx] says the rays of view saw something -> out_dev uint8 [n_frames][ny][nx], LABEL_NONE where nothing was seen"""
        nw, nv, nu = shape
        check(self.L.mcrt_render_label_frames(self.h, ptr(label_dev), n_frames, nu, nv, nw, C.byref(view), ptr(depth_dev), ptr(out_dev)))

    def noise_frames(self, rf_dev, n_frames, n_images, n_elements, n_rows, first_image_id=0, element_gain=None, sigma_dev=None, **opts):
        """mcrt_noise_frames: receiver noise over the RF stack [n_frames][n_images][n_elements][n_rows], in place -- a Gaussian noise floor
        (image j of the stack draws from the streams of id first_image_id + j) and a gain per scan-line (element_gain: host floats
        [n_elements] or None).  sigma_dev: [n_frames] floats on the device that receive each frame's sigma, or None.  opts: the keywords of
        noise_opts_struct (snr_db or sigma, seed)"""
        o = noise_opts_struct(**opts)
        g = None
        if element_gain is not None:
            g = np.ascontiguousarray(element_gain, np.float32)
            if g.shape != (n_elements,):
                raise ValueError("element_gain takes one gain per scan-line: %d, got shape %s" % (n_elements, g.shape))
        check(self.L.mcrt_noise_frames(self.h, ptr(rf_dev), n_frames, n_images, n_elements, n_rows, first_image_id, C.byref(o), ptr(g), ptr(sigma_dev)))

    def autogain_frames(self, rf_dev, n_frames, n_images, n_elements, n_rows, floor_dev=None, gain_dev=None, band_bin_dev=None, pen_dev=None, **opts):
        """mcrt_autogain_frames: automatic gain over the float stack [n_frames][n_images][n_elements][n_rows], in place -- a depth gain
        curve per frame from its own amplitude histograms.  floor_dev: [n_frames] floats on the device, each frame's noise floor (the
        sigma_dev of noise_frames), or None: opts' floor.  gain_dev [n_frames][n_rows] floats, band_bin_dev [n_frames][n_bands] int32 and
        pen_dev [n_frames] uint32 on the device receive the row gains, the band levels and the penetration depths [rows], or None.
        opts: the keywords of autogain_opts_struct"""
        o = autogain_opts_struct(**opts)
        check(self.L.mcrt_autogain_frames(self.h, ptr(rf_dev), n_frames, n_images, n_elements, n_rows, C.byref(o), ptr(floor_dev), ptr(gain_dev),
                                          ptr(band_bin_dev), ptr(pen_dev)))

    def label_frames(self, pos=None, dirs=None, *, rule="traced", start_offset=None, e_begin=0, e_end=None, n_frames=None, tissue_dev=None,
                     interface_dev=None, crossings_dev=None):
        """mcrt_label_frames: the central beam of every scan-line walked through the scene.  pos / dirs None: the context's transducer (one
        frame); else pose tables [F][E][3] as trace_frames_poses takes them (raw device pointers need n_frames).  Each output is a device pointer or None: tissue uint8
        [F][ne][R], interface int32 [F][ne][R], crossings uint32 [F][ne]"""
        e_end = self.params.n_elements if e_end is None else e_end
        if pos is None:
            n_frames = 1 if n_frames is None else n_frames
        else:
            pos, dirs, n_frames = _pose_tables("label_frames", pos, dirs, n_frames, self.params.n_elements)
        o = label_opts_struct(rule, start_offset)
        check(self.L.mcrt_label_frames(self.h, n_frames, e_begin, e_end, ptr(pos), ptr(dirs), C.byref(o), ptr(tissue_dev), ptr(interface_dev), ptr(crossings_dev)))

    def transmit_frames(self, pos=None, dirs=None, *, mode="total", rule="traced", start_offset=None, e_begin=0, e_end=None, n_frames=None, transmit_dev=None,
                        reflect_dev=None, crossings_dev=None):
        """mcrt_transmit_frames: the tracer's intensity carried along the central beam of every scan-line.  pos / dirs and the scan-line
        range as label_frames.  Each output is a device pointer or None: transmit float32 [F][ne][R] (the fraction of the emitted
        intensity that arrives at a row), reflect float32 [F][ne][R] (what the boundary in a row turns back, 0 elsewhere), crossings
        uint32 [F][ne] (label_frames' own)"""
        e_end = self.params.n_elements if e_end is None else e_end
        if pos is None:
            n_frames = 1 if n_frames is None else n_frames
        else:
            pos, dirs, n_frames = _pose_tables("transmit_frames", pos, dirs, n_frames, self.params.n_elements)
        o = transmit_opts_struct(mode, rule, start_offset)
        check(self.L.mcrt_transmit_frames(self.h, n_frames, e_begin, e_end, ptr(pos), ptr(dirs), C.byref(o), ptr(transmit_dev), ptr(reflect_dev), ptr(crossings_dev)))

    def label_scan_convert_frames(self, tissue_dev, n_frames, n_elements, n_rows, out_dev, radius_mm=30.0, total_angle=DEFAULT_ANGLE, out_rows=400, out_cols=500):
        """mcrt_label_scan_convert_frames: tissue maps [n_frames][E][R] -> bytes [n_frames][out_rows][out_cols], nearest neighbour through
        scan_convert_frames' own maps; LABEL_NONE outside the sector"""
        check(self.L.mcrt_label_scan_convert_frames(self.h, ptr(tissue_dev), n_frames, n_elements, n_rows, radius_mm, total_angle, ptr(out_dev), out_rows, out_cols))

    def label_volume_frames(self, tissue_dev, n_frames, n_elements, n_rows, sweep, grid, out_dev, radius_mm=30.0, total_angle=DEFAULT_ANGLE):
        """mcrt_label_volume_frames: the tissue maps [n_frames][K][E][R] of a sweep -> bytes [n_frames][nw][nv][nu] at grid's points, nearest
        neighbour through volume_frames' own maps; LABEL_NONE outside the sweep"""
        sw = _as_sweep(sweep)
        check(self.L.mcrt_label_volume_frames(self.h, ptr(tissue_dev), n_frames, n_elements, n_rows, radius_mm, total_angle, C.byref(sw), C.byref(grid), ptr(out_dev)))

    def export_rf(self, rf_dev, n_elements, n_rows):
        out = np.empty((n_rows, n_elements), np.float32)
        check(self.L.mcrt_export_rf(self.h, ptr(rf_dev), n_elements, n_rows, ptr(out)))
        return out

    # instrumentation
    def enable_stats(self, on=True):
        check(self.L.mcrt_enable_stats(self.h, int(on)))

    def get_stats(self, reset=True):
        s = Stats()
        check(self.L.mcrt_get_stats(self.h, C.byref(s), int(reset)))
        return s.as_dict()

    def enable_timing(self, on=True):
        check(self.L.mcrt_enable_timing(self.h, int(on)))

    def kernel_times(self, reset=True):
        """{"walk" | "shade" | "march": (average ms per launch, launches)} since the last reset (shade / march only under enable_timing(2))"""
        ms = (C.c_double * 3)(); n = (C.c_uint32 * 3)()
        check(self.L.mcrt_get_kernel_times(self.h, ms, n, int(reset)))
        return {k: (ms[i], n[i]) for i, k in enumerate(("walk", "shade", "march"))}

    def kernel_time(self, reset=True):
        ms = C.c_double(); n = C.c_uint32()
        check(self.L.mcrt_get_kernel_time(self.h, C.byref(ms), C.byref(n), int(reset)))
        return ms.value, n.value

    def debug_math(self, op, x, y=None):
        x = np.ascontiguousarray(x, np.float64); out = np.empty_like(x)
        if y is not None:
            y = np.ascontiguousarray(y, np.float64)
        check(self.L.mcrt_debug_math(self.h, op, ptr(x), ptr(y), ptr(out), x.size))
        return out

    def debug_philox(self, ctr, key):
        c = np.asarray(ctr, np.uint32); k = np.asarray(key, np.uint32); o = np.zeros(4, np.uint32)
        check(self.L.mcrt_debug_philox(self.h, ptr(c), ptr(k), ptr(o)))
        return o


# ------------------------------------------------------------------ several GPUs behind one call (mcrt_group_*)
def shard_range(rank, n_ranks, n_elements):
    """the contiguous scan-line block of `rank` (mcrt_group_shard; dist.shard_range is the same rule in Python)"""
    b = C.c_uint32(); e = C.c_uint32()
    check(load_library().mcrt_group_shard(rank, n_ranks, n_elements, C.byref(b), C.byref(e)))
    return int(b.value), int(e.value)


class Group(_SceneCalls):
    """mcrt_group: one tracing context per listed device (a device may repeat), scan-lines cut into contiguous shards, the blocks
    gathered on devices[0].  `root` is the context that owns the gathered frames (post-processing, alloc, exports)."""
    PREFIX = "mcrt_group_"

    def __init__(self, devices):
        self.L = load_library()
        devs = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        check(self.L.mcrt_group_create(C.cast(devs, C.c_void_p), len(devices), C.byref(h)))
        self.h = h
        self.size = int(self.L.mcrt_group_size(self.h))
        self.root = Context(_borrowed=self.L.mcrt_group_root(self.h))
        self.members = [Context(_borrowed=self.L.mcrt_group_member(self.h, r)) for r in range(self.size)]
        self.params = Params()
        check(self.L.mcrt_default_params(C.byref(self.params)))

    def close(self):
        if getattr(self, "h", None):
            self.L.mcrt_group_destroy(self.h)
            self.h = None
            self.root.h = None
            for m in self.members:
                m.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_params(self, **kw):
        self._assign_params(kw)
        try:
            check(self.L.mcrt_group_set_params(self.h, C.byref(self.params)))
        finally:       # (refused parameters leave every context on the old ones: read back what the group really holds)
            for c in [self.root] + self.members:
                check(self.L.mcrt_get_params(c.h, C.byref(c.params)))
            check(self.L.mcrt_get_params(self.root.h, C.byref(self.params)))

    def update_triangles(self, tri):
        tri = np.ascontiguousarray(tri, np.float32).reshape(-1, 9)
        check(self.L.mcrt_group_update_triangles(self.h, ptr(tri), tri.shape[0]))

    def refit_triangles(self, tri):
        tri = np.ascontiguousarray(tri, np.float32).reshape(-1, 9)
        check(self.L.mcrt_group_refit_triangles(self.h, ptr(tri), tri.shape[0]))

    def trace_frames(self, frame_id, n_frames, rf_dev):
        """rf_dev: [n_frames][E][R] on devices[0]; complete on the root context's stream"""
        check(self.L.mcrt_group_trace_frames(self.h, frame_id, n_frames, ptr(rf_dev)))

    def trace_frames_poses(self, frame_id, pos, dirs, rf_dev):
        pos = np.ascontiguousarray(pos, np.float32); dirs = np.ascontiguousarray(dirs, np.float32)
        assert tuple(pos.shape) == (pos.shape[0], self.params.n_elements, 3) and tuple(dirs.shape) == tuple(pos.shape)
        check(self.L.mcrt_group_trace_frames_poses(self.h, frame_id, pos.shape[0], ptr(pos), ptr(dirs), ptr(rf_dev)))

    def synchronize(self):
        check(self.L.mcrt_group_synchronize(self.h))

    def last_scene_seconds(self):
        """(host SAH build -- once, on the calling thread --, the ranks' concurrent uploads) of the last upload_scene / update_triangles"""
        b, u = C.c_double(), C.c_double()
        check(self.L.mcrt_group_last_scene_seconds(self.h, C.byref(b), C.byref(u)))
        return b.value, u.value

    def last_pass_ms(self):
        t = np.zeros(self.size, np.float32); c = np.zeros(self.size, np.float32)
        check(self.L.mcrt_group_last_pass_ms(self.h, ptr(t), ptr(c)))
        return t, c


# ------------------------------------------------------------------ frame-level mirror of main.cpp:92-152
# the device images a stage acts on: `images` of them from dev on, as `frames` frames of `per_frame` each, the first with the id first_id
_Images = collections.namedtuple("_Images", "dev images frames per_frame first_id")


class _GrowOnly:
    """a device buffer of a context that is made on first use and only grows"""

    def __init__(self, ctx):
        self.ctx, self.dev, self.nbytes = ctx, None, 0

    def reserve(self, nbytes):
        if self.dev is None or self.nbytes < nbytes:
            self.release()
            self.dev, self.nbytes = self.ctx.alloc(nbytes), nbytes
        return self.dev

    def release(self):
        if self.dev is not None:
            self.ctx.free(self.dev)
        self.dev, self.nbytes = None, 0


def _option(value, other=lambda v: {} if v is True else dict(v)):
    """an option keyword of Simulator -> None (off: None or False) or the dict of its keywords: a dict is copied, anything else goes through
    `other` (True: the defaults)"""
    if value is None or value is False:
        return None
    return dict(value) if isinstance(value, dict) else other(value)


def _detect_word(detect):
    if isinstance(detect, str) and detect != "quadrature":
        raise ValueError("detect takes None, \"quadrature\" or a dict of n_taps=, got %r" % (detect,))
    return {} if isinstance(detect, str) else dict(detect)


def _grid_shape(grid):
    """(the shape of grid's output [nw][nv][nu], its points)"""
    return (grid.nw, grid.nv, grid.nu), grid.nw * grid.nv * grid.nu


class Simulator:
    """scene + transducer + rf_image of the reference, driven frame by frame.

        sim = Simulator(scene_data, transducer, n_samples=5)
        rf = sim.frame(0)                 # clear -> cast_rays -> accumulate -> convolve, returns [R][E] host image
    """

    def __init__(self, scene_data, transducer, n_samples=5, n_rows=None, device=0, seed=0x5EED, psf=None, texture=None,
                 max_depth=10, sanitize_tir=0, tex_n=256, bvh_builder="sah", elevation=False, compound=None, compound_mode="mean", compound_weights=None,
                 compound_feather=0.0, sweep=None, sweep_pivot_mm=0.0, speckle=None, noise=None, speckle3d=None, autogain=None, detect=None, flow=None, strain=None, shear=None, motion=None):
        """elevation=True: slice thickness.  trace() then traces the psf's elevation_size planes of the frame as one pose pass -- plane k of
        frame f with frame id f * K + k, the frame-id rule of include/mcrt.h -- and folds them into rf_dev with psf.elevation_rows();
        everything after (convolve, bmode, frame) is unchanged.
        compound=(steer_rad, ...): spatial compounding.  trace() then traces the N steered views of the frame as one pose pass -- view n of
        frame f with frame id f * N + n, with elevation its plane k with (f * N + n) * K + k -- into views_dev [N][E][R] (folded per view
        with elevation=True); convolve() and the envelope run over the N views, bmode() ends in mcrt_bmode_compound_frames and
        compound_image() in mcrt_compound_frames.  frame() returns RF, which a compounded frame does not have: it raises.
        compound_mode ("mean" / "max" / "median"), compound_weights (one weight per view) and compound_feather (a lateral edge ramp in
        scan-lines) are carried into compound_image() and bmode(): the keywords of Context.compound_frames.
        sweep=(K, step_rad): volume imaging with a probe swept in elevation about the axis through (0, sweep_pivot_mm, 0).  trace() then traces
        the K tilted planes as one pose pass -- plane k of volume f with frame id f * K + k -- into sweep_dev [K][E][R]; convolve() and the
        envelope run over the K planes; volume() and bmode_volume() gather them at a grid's points.  frame(), bmode() and compound_image()
        raise.  It does not combine with compound= or elevation=.
        speckle=True, or a dict of the keywords of speckle_opts_struct (n_iter, q0, rho, lambda): speckle reduction.  Every picture that
        runs the envelope (bmode, compound_image, volume, bmode_volume, render) then passes the enveloped stack through
        mcrt_speckle_frames in place (despeckle()) before anything reads it.  frame() returns RF and is left alone.
        noise=X (an snr_db), or a dict of snr_db= or sigma=, seed=, element_gain= (one gain per scan-line) and dead_elements= (scan-lines
        whose gain is 0): receiver noise.  Every run then passes the image stack through mcrt_noise_frames in place (add_noise()) after the
        convolution step -- whether or not convolve ran -- and before the envelope, with first_image_id = frame_id * (images in the stack):
        the ids the images were traced with, so a frame carries the same noise whatever pass it is part of.  frame() therefore returns
        noisy RF, and everything downstream (bmode, compound_image, volume, render, freehand) sees it.  The stage sits after the lateral PSF
        because receive noise is uncorrelated between scan-lines, which the PSF's lateral blur would undo; that is a modelling choice
        that no measurement backs.
        speckle3d=True, or a dict of the keywords of speckle3d_opts_struct (n_iter, q0, rho, lambda, weights): 3-D speckle reduction over
        voxel blocks.  volume() and freehand() then pass their float block through mcrt_speckle_volume_frames in place on the device before
        it is copied out, with the weights of the grid's pitches (host_speckle3d_weights(grid)) unless the dict gives weights.
        bmode_volume() and render() gather bytes straight from the planes and have no float block to filter: under speckle3d= they
        raise.  Without the keyword no call changes.
        autogain=True, or a dict of the keywords of autogain_opts_struct (band_rows, min_permille, floor, floor_scale, max_gain or
        max_gain_db, apply): automatic gain.  Every picture that runs the envelope then passes the enveloped (and despeckled) stack through
        mcrt_autogain_frames in place (auto_gain()) before anything gathers it: the views of a compounded frame and the planes of a sweep
        share one curve, the tracked frames of freehand() have one each.  With noise= the noise stage's sigma of every frame is the floor;
        without it the options' floor.  gain_curve() and penetration_mm() return the last run's by-products.  frame() returns RF and is
        left alone.  Without the keyword no call changes.
        A psf with bands (Psf(bands=...) or a downshift): frequency compounding.  convolve() then writes the stack's n images as n * B band
        images into a band stack of its own [n][B][E][R] (mcrt_convolve_bands_frames); add_noise() acts on those, as the n * B images of one
        frame -- one receiver, one peak, image i's band b with the id (frame_id * n + i) * B + b; envelope() detects every band image and
        folds them back into the usual stack (mcrt_band_fold_frames), so everything downstream -- the speckle filter, auto gain, every gather,
        compound=, sweep=, elevation=, freehand() -- sees the stack it always saw.  Without the envelope (frame(), envelope=False) the fold
        runs alone where the envelope would have: a coherent sum of the band images, the same as one pulse that is the weighted sum of the
        bands' -- it changes the pulse and reduces no speckle.  Without bands no call and no bit changes.
        detect="quadrature", or a dict of the keywords of detect_opts_struct (n_taps): quadrature detection.  envelope() then calls
        mcrt_detect_frames in place where it calls mcrt_envelope_frames -- with bands over the band stack's n * B images, then fold_bands(),
        as before -- so everything downstream sees the stack it always saw.  The detector is flat within 1 % only for carriers between
        0.05 and 0.45 cycles per row at 31 taps (host_psf_carrier, host_detect_gain); a band near Nyquist comes out darker.  iq() returns the
        analytic pair of frame()'s RF whether or not the keyword is given.  Without the keyword no call and no bit changes.
        flow={"BLOOD": (vx, vy, vz)} -- a velocity vector [mm/s] per material name of the scene --, or a dict of velocity_mm_s= (that
        mapping) and the keywords of flow_opts_struct (n_packets, wall, avg_rows, avg_lines, prf_hz, freq_mhz, sigma, seed), of the label pass
        (rule, start_offset) and of the display (power_scale, vel_thr_mm_s, grey_max): colour Doppler.  colour_flow() and flow_velocity()
        then synthesise a slow-time ensemble from ONE traced frame, split by tissue label into what stands still and what moves, and
        estimate the axial velocity with the Kasai autocorrelator; with noise= the noise stage's sigma is the ensemble's, else the
        dict's.  The displayed power threshold is power_scale * 2 * N * sigma^2 (default scale 4): a modelling choice that no
        measurement backs.  spectral_doppler() runs the same chain up to the detected pairs and then synthesises the slow-time series of
        ONE sample gate under a speed waveform and a velocity profile (its own keywords; of flow= it reads the material's direction, prf_hz,
        sigma and the label rule).  Every other method is left alone: without the keyword no call and no bit changes.
        strain={"LIVER": 1.0, "TUMOR": 5.0} -- a Young's modulus per material name of the scene (any unit; 0: rigid) --, or a dict of
        modulus= (that mapping), applied= (the strain of a material of the reference modulus, 0.01), ref_modulus= (1.0; a material that
        is not named takes it), the keywords of strain_opts_struct (window_rows, search_rows, lsq_rows, seed), noise= (the receiver noise
        per I/Q component of the post-compression frame, 0) and of the label pass (rule, start_offset): strain elastography.  strain()
        and elastogram() then synthesise the post-compression frame from ONE traced frame's analytic signal and its tissue labels, and
        track the speckle between the two.  Every other method is left alone: without the keyword no call and no bit changes."""
        self.strain_opts = _option(strain)
        if self.strain_opts is not None:
            sd = self.strain_opts if "modulus" in self.strain_opts else dict(modulus=self.strain_opts)
            names = list(scene_data.material_names)
            ref_modulus = float(sd.pop("ref_modulus", 1.0))
            modulus = np.full(len(names), ref_modulus, np.float64)
            for name, v in dict(sd.pop("modulus")).items():
                if name not in names:
                    raise ValueError("strain: the scene has no material %r (it has %s)" % (name, ", ".join(names)))
                modulus[names.index(name)] = float(v)
            applied = float(sd.pop("applied", 0.01))
            label = dict(rule=sd.pop("rule", "traced"), start_offset=sd.pop("start_offset", None))
            label_opts_struct(**label)                      # (an unknown rule ends it here)
            opts = strain_opts_struct(sigma=sd.pop("noise", None), **sd)       # (unknown keywords end it here)
            self.strain_opts = dict(modulus=modulus, applied=applied, ref_modulus=ref_modulus, eps=host_strain_table(modulus, applied, ref_modulus),
                                    opts=opts, label=label)         # (a strain above the cap ends it here)
        # shear={"LIVER": 1.5, "TUMOR": 3.0} -- a shear speed per material name of the scene [m/s] (0: a fluid, the wave does not pass) --, or a
        # dict of speed_m_s= (that mapping), ref_speed_m_s= (2.0; a material that is not named takes it), push=(scan-line, depth_mm of the
        # push's centre, length_mm) (None: push_line / push_row0 / push_rows as they are), width_pulses= (12) and decay_lines= (8.0) of the
        # default time profile and decay, radius_mm= and total_angle= of the sector the pitch is taken from, ref_kpa= (the elastogram's
        # middle; None: 3 density ref_speed^2), the keywords of shear_opts_struct (n_pulses, window_rows, prf_hz, seed, peak_q24,
        # speed_lines, avg_rows, density, ...), noise= (the receiver noise per I/Q component of every tracking line, 0) and of the label
        # pass (rule, start_offset): shear-wave elastography.  shear_wave() and shear_elastogram() then trace the frame ONCE, synthesise
        # the tracked wave from that frame and estimate its speed.  Every other method is left alone.
        self.shear_opts = _option(shear)
        if self.shear_opts is not None:
            sd = self.shear_opts if "speed_m_s" in self.shear_opts else dict(speed_m_s=self.shear_opts)
            names = list(scene_data.material_names)
            ref_speed = float(sd.pop("ref_speed_m_s", 2.0))
            speeds = np.full(len(names), ref_speed, np.float64)
            for name, v in dict(sd.pop("speed_m_s")).items():
                if name not in names:
                    raise ValueError("shear: the scene has no material %r (it has %s)" % (name, ", ".join(names)))
                speeds[names.index(name)] = float(v)
            label = dict(rule=sd.pop("rule", "traced"), start_offset=sd.pop("start_offset", None))
            label_opts_struct(**label)                      # (an unknown rule ends it here)
            push, ref_kpa = sd.pop("push", None), sd.pop("ref_kpa", None)
            geometry = dict(radius_mm=float(sd.pop("radius_mm", 30.0)), total_angle=float(sd.pop("total_angle", DEFAULT_ANGLE)))
            shape, decay = host_shear_shape(int(sd.pop("width_pulses", 12))), float(sd.pop("decay_lines", 8.0))
            opts = shear_opts_struct(sigma=sd.pop("noise", None), **sd)        # (unknown keywords end it here)
            slow, speed_f = host_shear_table(speeds, opts.prf_hz)             # (a speed out of range ends it here)
            self.shear_opts = dict(speeds=speeds, slow=slow, speed_f=speed_f, shape=shape, decay=decay, push=push, geometry=geometry, opts=opts, label=label,
                                   ref_kpa=3.0 * opts.density * ref_speed * ref_speed if ref_kpa is None else float(ref_kpa))
        # motion={"BLOOD": -0.05} -- a dilation per material name of the scene: the peak axial strain of that material over the cycle,
        # positive: compression, so a lumen that widens in systole has a negative one; at most 25 % --, or a dict of dilation= (that
        # mapping), prf_hz= (1000), beats_per_min= (72; the default waveform, host_mmode_waveform), n_pulses= (1024), bulk_mm= and
        # bulk_per_min= (a rigid sinusoidal shift of the whole line, host_mmode_bulk; 0 and 15), noise= (the receiver noise per I/Q
        # component of every pulse, 0), seed= and of the label pass (rule, start_offset): M-mode.  m_mode() then traces the frame ONCE and
        # synthesises the pulses of one scan-line from that frame.  Every other method is left alone.
        self.motion = _option(motion)
        if self.motion is not None:
            md = self.motion if "dilation" in self.motion else dict(dilation=self.motion)
            names = list(scene_data.material_names)
            dilation = np.zeros(len(names), np.float64)
            for name, v in dict(md.pop("dilation")).items():
                if name not in names:
                    raise ValueError("motion: the scene has no material %r (it has %s)" % (name, ", ".join(names)))
                dilation[names.index(name)] = float(v)
            label = dict(rule=md.pop("rule", "traced"), start_offset=md.pop("start_offset", None))
            label_opts_struct(**label)                      # (an unknown rule ends it here)
            timing = dict(prf_hz=float(md.pop("prf_hz", 1000.0)), beats_per_min=float(md.pop("beats_per_min", 72.0)), bulk_mm=float(md.pop("bulk_mm", 0.0)),
                          bulk_per_min=float(md.pop("bulk_per_min", 15.0)))
            opts = mmode_opts_struct(sigma=md.pop("noise", None), **md)        # (unknown keywords end it here)
            host_mmode_waveform(timing["prf_hz"], timing["beats_per_min"], opts.n_pulses)      # (a rate or a pulse count out of range ends it here)
            self.motion = dict(dilation=dilation, dil=host_mmode_table(dilation), opts=opts, label=label, **timing)     # (a dilation above the cap ends it here)
        self.flow = _option(flow)
        if self.flow is not None:
            fd = self.flow if "velocity_mm_s" in self.flow else dict(velocity_mm_s=self.flow)
            names = list(scene_data.material_names)
            vel = np.zeros((len(names), 3), np.float32)
            for name, v in dict(fd.pop("velocity_mm_s")).items():
                if name not in names:
                    raise ValueError("flow: the scene has no material %r (it has %s)" % (name, ", ".join(names)))
                vel[names.index(name)] = np.asarray(v, np.float32).reshape(3)
            label = dict(rule=fd.pop("rule", "traced"), start_offset=fd.pop("start_offset", None))
            label_opts_struct(**label)                      # (an unknown rule ends it here)
            display = dict(power_scale=float(fd.pop("power_scale", 4.0)), vel_thr_mm_s=fd.pop("vel_thr_mm_s", None), grey_max=fd.pop("grey_max", None))
            colour_opts_struct(vel_thr_mm_s=display["vel_thr_mm_s"], grey_max=display["grey_max"])
            opts = flow_opts_struct(**fd)                   # (unknown keywords end it here)
            v_nyq = host_flow_nyquist(transducer.frequency, opts=opts)      # (options out of range end it here; the speed of sound is set below)
            self.flow = dict(vel=vel, moving=(vel != 0).any(axis=1).astype(np.uint8), opts=opts, label=label, display=display, v_nyq=v_nyq)
        self.detect = _option(detect, _detect_word)
        if self.detect is not None:
            host_detect_taps(detect_opts_struct(**self.detect).n_taps)   # (unknown keywords and a bad n_taps end it here)
        self.autogain = _option(autogain)
        if self.autogain is not None:
            autogain_opts_struct(**self.autogain)           # (unknown keywords end it here)
        self._ag_gain, self._ag_pen = None, None
        self.speckle3d = _option(speckle3d)
        if self.speckle3d is not None:
            speckle3d_opts_struct(**self.speckle3d)         # (unknown keywords and a wrong number of weights end it here)
        if sweep is not None and (compound is not None or elevation):
            raise ValueError("sweep= does not combine with compound= or elevation=")
        if compound is not None and not 1 <= len(tuple(compound)) <= 16:
            raise ValueError("compound takes 1..16 steering angles, got %d" % len(tuple(compound)))
        self.speckle = None if _option(speckle) is None else speckle_opts_struct(**_option(speckle))
        E = transducer.n_elements
        self.noise, self.noise_gain = None, None
        nd = _option(noise, lambda snr_db: dict(snr_db=snr_db))
        if nd is not None:
            gain, dead = nd.pop("element_gain", None), nd.pop("dead_elements", None)
            self.noise = noise_opts_struct(**nd)
            if gain is not None or dead is not None:
                self.noise_gain = np.ones(E, np.float32) if gain is None else np.array(gain, np.float32)
                if self.noise_gain.shape != (E,):
                    raise ValueError("noise: element_gain takes one gain per scan-line (%d)" % E)
                for e in (dead or ()):
                    if not 0 <= int(e) < E:
                        raise ValueError("noise: dead_elements: scan-line %d is not in 0..%d" % (int(e), E - 1))
                    self.noise_gain[int(e)] = 0.0
        self.ctx = Context(device)
        self.ctx.set_bvh_builder(bvh_builder)
        self.tr = transducer
        self.ctx.set_params(n_elements=E, n_samples=n_samples, frequency=transducer.frequency, seed=seed, max_depth=max_depth,
                            sanitize_tir=sanitize_tir, tex_n=tex_n, **({"n_rows": n_rows} if n_rows else {}))
        self.E, self.R, self.S = E, self.ctx.params.n_rows, n_samples
        if self.flow is not None:
            self.flow["v_nyq"] = host_flow_nyquist(transducer.frequency, self.ctx.params.speed_of_sound, opts=self.flow["opts"])
            self.flow["phasor"], self.flow["truth"] = host_flow_phasors(self.flow["v_nyq"], self.flow["vel"], transducer.dir)
        self.n_materials = int(scene_data.materials.shape[0])
        self.material_names = list(getattr(scene_data, "material_names", ()))   # (flow= resolves its names through them)
        self.ctx.upload_scene(scene_data)
        self.ctx.upload_texture(texture, tex_n)
        self.ctx.set_transducer(transducer.pos, transducer.dir)
        self.psf = psf or Psf(freq=transducer.frequency)
        self.rf_dev = self.ctx.alloc(E * self.R * 4)
        # the band stack [n][B][E][R] of a psf with bands, auto gain's (sigma [F], pen [F], gain [F][R]), and whether band images of the own stack
        # wait in the first (between convolve() and envelope() / fold_bands())
        self._band_buf, self._gain_buf, self._held = _GrowOnly(self.ctx), _GrowOnly(self.ctx), False
        self.elevation, self.planes_dev, self.views_dev, self.sweep, self.sweep_dev = bool(elevation), None, None, None, None
        self.steers = tuple(float(x) for x in compound) if compound is not None else None
        self.N = len(self.steers) if self.steers is not None else 1
        if compound_weights is not None and (self.steers is None or len(tuple(compound_weights)) != len(self.steers)):
            raise ValueError("compound_weights takes one weight per steering angle of compound=")
        if self.steers is None and not _compound_defaults(compound_mode, None, compound_feather):
            raise ValueError("compound_mode and compound_feather need compound=")
        self.compound_opts = dict(mode=compound_mode, view_weights=tuple(float(x) for x in compound_weights) if compound_weights is not None else None,
                                  feather_lines=float(compound_feather))
        # decided here, once: the image stack (device buffer, images) that convolve(), envelope() and the pictures read, and the pose pass
        # (pos, dirs, destination, images per frame) that trace() fills it with -- None: the context's own transducer, mcrt_trace_frame
        self._stack, self._pass = (self.rf_dev, 1), None
        if self.steers is not None:
            self.view_pos, self.view_dir = transducer.steered(self.steers)
            self.views_dev = self.ctx.alloc(self.N * E * self.R * 4)
            self._stack, self._pass = (self.views_dev, self.N), (self.view_pos, self.view_dir, self.views_dev, self.N)
        if sweep is not None:
            self.sweep = sweep_struct(sweep[0], sweep[1], sweep_pivot_mm)
            self.sweep_pos, self.sweep_dir = transducer.swept(self.sweep.n_planes, self.sweep.step_rad, self.sweep.pivot_mm)
            self.sweep_dev = self.ctx.alloc(self.sweep.n_planes * E * self.R * 4)
            self._stack, self._pass = (self.sweep_dev, self.sweep.n_planes), (self.sweep_pos, self.sweep_dir, self.sweep_dev, self.sweep.n_planes)
        if self.elevation:                              # the pose pass goes to the plane stacks, which trace() folds into the image stack
            self.K = self.psf.elevation_size
            self.plane_pos, self.plane_dir, self.plane_z_mm = transducer.planes(self.K, self.psf.elevation_pitch_um)
            if self.steers is not None:                 # the views are outer: [N][K][E][3]
                axis = host_elevation_axis(transducer.angles)
                tabs = [host_elevation_planes(self.view_pos[n], self.view_dir[n], axis, self.K, self.psf.elevation_pitch_um) for n in range(self.N)]
                self.plane_pos = np.concatenate([t[0] for t in tabs]); self.plane_dir = np.concatenate([t[1] for t in tabs])
            self.planes_dev = self.ctx.alloc(self.N * self.K * E * self.R * 4)
            self._pass = (self.plane_pos, self.plane_dir, self.planes_dev, self.N * self.K)

    def close(self):
        if self.ctx.h:
            for d in (self.rf_dev, self.planes_dev, self.views_dev, self.sweep_dev):
                if d:
                    self.ctx.free(d)
            self._gain_buf.release(); self._band_buf.release()
            self.ctx.close()

    def trace(self, frame_id=0):
        self._held = False
        if self._pass is None:
            self.ctx.trace_frame(frame_id, self.rf_dev)
            return
        pos, dirs, dest, per_frame = self._pass
        self.ctx.trace_frames_poses(frame_id * per_frame, pos, dirs, dest)
        if self.elevation:
            self.ctx.elevation_frames(self.planes_dev, self._stack[1], self.K, self.E, self.R, self.psf.elevation_rows(self.R, self.row_mm), self._stack[0])

    @property
    def row_mm(self):
        """the RF row pitch [mm]: the depth of row r is r * row_mm (path length, as the reference's row index)"""
        return row_pitch_mm(self.ctx.params.frequency)

    # ---- the images a stage acts on, and the stages over any of them
    def _images(self, frame_id=0, own_frames=False, stack=None):
        """the n images of a traced pass -- this simulator's stack, or `stack` = (device buffer, n) -- as the views or planes of ONE frame (one
        receiver, one peak, one curve); own_frames=True: so many frames of one image each (the tracked frames of freehand()).  Image i was
        traced with the id frame_id * n + i"""
        dev, n = stack or self._stack
        return _Images(dev, n, n if own_frames else 1, 1 if own_frames else n, frame_id * n)

    def _band_images(self, s):
        """the band images of s in the band stack: B per image of the same frame, image i's band b with the id (first id + i) * B + b"""
        B = self.psf.bands.n_bands
        return _Images(self._band_buf.reserve(s.images * B * self.E * self.R * 4), s.images * B, s.frames, s.per_frame * B, s.first_id * B)

    def _convolve(self, s):
        """-> the images that wait for the envelope: s, or with a psf that has bands its band images"""
        if not self.psf.has_bands:
            if self.psf.has_focus:
                self.ctx.convolve_frames_depth(s.dev, s.images, self.E, self.R, self.psf.axial_kernel, self.psf.lateral_rows(self.R, self.row_mm))
            else:
                self.ctx.convolve_frames(s.dev, s.images, self.E, self.R, self.psf.axial_kernel, self.psf.lateral_kernel)
            return s
        p = self._band_images(s)
        lat = dict(lat_rows=self.psf.lateral_rows(self.R, self.row_mm)) if self.psf.has_focus else dict(lateral=self.psf.lateral_kernel)
        self.ctx.convolve_bands_frames(s.dev, s.images, self.E, self.R, self.psf.axial_rows(self.R, self.row_mm), p.dev, **lat)
        return p

    def _noise(self, p):
        o = self.noise if self.noise is not None else noise_opts_struct()
        kw = dict(sigma=o.sigma) if o.mode == NOISE_ABS else dict(snr_db=o.snr_db)
        sigma_dev = self._gain_bufs(p.frames)[0] if self.autogain is not None or self.flow is not None else None   # (auto_gain()'s floor, the colour ensemble's sigma)
        self.ctx.noise_frames(p.dev, p.frames, p.per_frame, self.E, self.R, first_image_id=p.first_id, element_gain=self.noise_gain, sigma_dev=sigma_dev,
                              seed=o.seed, **kw)

    def _detect(self, p, s):
        if self.detect is not None:                     # quadrature detection in the place of the reference's envelope
            self.ctx.detect_frames(p.dev, p.images, self.E, self.R, env_dev=p.dev, **self.detect)
        else:
            self.ctx.envelope_frames(p.dev, p.images, self.E, self.R)
        self._fold(p, s)                                # every band image is detected on its own, then they are averaged (nothing to do without bands)

    def _fold(self, p, s):
        if p != s:
            self.ctx.band_fold_frames(p.dev, s.images, self.psf.bands.n_bands, self.E, self.R, self.psf.band_weights(self.R, self.row_mm), s.dev)

    def _despeckle(self, s):
        o = self.speckle if self.speckle is not None else speckle_opts_struct()
        self.ctx.speckle_frames(s.dev, s.images, self.E, self.R, n_iter=o.n_iter, q0=o.q0, rho=o.rho, lambda_=o.lambda_)

    def _gain_bufs(self, F):
        """the device side of auto_gain() for F frames: (sigma [F], pen [F], gain [F][R])"""
        dev = self._gain_buf.reserve(F * (2 + self.R) * 4)
        return dev, dev + 4 * F, dev + 8 * F

    def _autogain(self, s):
        sigma_dev, pen_dev, gain_dev = self._gain_bufs(s.frames)
        self.ctx.autogain_frames(s.dev, s.frames, s.per_frame, self.E, self.R, floor_dev=sigma_dev if self.noise is not None else None, gain_dev=gain_dev,
                                 pen_dev=pen_dev, **(self.autogain or {}))
        self._ag_gain = self.ctx.d2h(gain_dev, (s.frames, self.R), np.float32)
        self._ag_pen = self.ctx.d2h(pen_dev, (s.frames,), np.uint32)

    def _stages(self, images, frame_id, convolve=True, envelope=True, own_frames=False):
        """convolve (-> add_noise with noise=) -> envelope (-> despeckle with speckle=) (-> auto_gain with autogain=), or without the envelope the
        fold alone, over images = (device buffer, n).  p is what waits for the envelope: the images, or their band images"""
        s = self._images(frame_id, own_frames, images)
        p = self._convolve(s) if convolve else s
        if self.noise is not None:
            self._noise(p)
        if not envelope:
            self._fold(p, s)
            return
        self._detect(p, s)
        if self.speckle is not None:
            self._despeckle(s)
        if self.autogain is not None:
            self._autogain(s)

    # ---- the same stages one by one, over this simulator's own stack
    def _pending(self, s):
        return self._band_images(s) if self._held else s

    def convolve(self):
        """over the stack's images as so many frames (mcrt_convolve is mcrt_convolve_frames of one); with a psf that has bands into the band
        stack, where the images stay until envelope() or fold_bands() brings them back"""
        self._held = self._convolve(self._images()) != self._images()

    def envelope(self):
        self._detect(self._pending(self._images()), self._images())
        self._held = False

    def fold_bands(self):
        """mcrt_band_fold_frames: the band images that convolve() left, folded back into the stack with the bands' weights (nothing to do
        when there are none).  After envelope() that is frequency compounding; on RF it is a coherent sum"""
        self._fold(self._pending(self._images()), self._images())
        self._held = False

    def despeckle(self):
        """mcrt_speckle_frames over the stack's images, in place, with the options of speckle= (the defaults without one)"""
        self._despeckle(self._images())

    def despeckle_volume(self, vox_dev, grid):
        """mcrt_speckle_volume_frames over the float block of grid on the device, in place, with the options of speckle3d= (the defaults
        without one); the weights are the grid's pitches' unless the options give them"""
        o = dict(self.speckle3d or {})
        if o.get("weights") is None:
            o["weights"] = host_speckle3d_weights(grid)
        self.ctx.speckle_volume_frames(vox_dev, 1, _grid_shape(grid)[0], **o)

    def add_noise(self, frame_id=0, own_peaks=False):
        """mcrt_noise_frames over the stack's images, in place, with the options of noise= (the defaults without one): the images are the
        views or planes of ONE frame (one receiver, one peak) with the ids frame_id * (images in the stack) onwards; own_peaks=True: so many
        frames of one image each (the tracked frames of freehand()).  After a convolve() with bands it acts on the band images"""
        self._noise(self._pending(self._images(frame_id, own_peaks)))

    def auto_gain(self, own_frames=False):
        """mcrt_autogain_frames over the stack's images, in place, with the options of autogain= (the defaults without one): the images are
        the views or planes of ONE frame (one receiver, one curve); own_frames=True: so many frames of one image each (the tracked frames
        of freehand()).  The floor is the sigma that add_noise() left on the device when noise= is on.  It keeps the row gains and the
        penetration depths for gain_curve() and penetration_mm()"""
        self._autogain(self._images(own_frames=own_frames))

    def gain_curve(self):
        """the row gains of the last run under autogain=: float32 [R], or [F][R] after freehand(); None before any"""
        g = self._ag_gain
        return None if g is None else (g[0].copy() if g.shape[0] == 1 else g.copy())

    def penetration_mm(self):
        """the penetration depth of the last run under autogain= [mm]: the rows of mcrt_autogain_frames times the row pitch -- a float, or
        an array [F] after freehand(); None before any"""
        p = self._ag_pen
        return None if p is None else (float(p[0]) * self.row_mm if p.shape[0] == 1 else p.astype(np.float64) * self.row_mm)

    def _run(self, frame_id, convolve=True, envelope=True):
        self.trace(frame_id)
        self._stages(self._stack, frame_id, convolve, envelope)

    def compound_image(self, frame_id=0, convolve=True, envelope=True, radius_mm=30.0, total_angle=DEFAULT_ANGLE, out_rows=400, out_cols=500):
        """trace -> convolve -> envelope -> mcrt_compound_frames -> host: the compounded float picture [out_rows][out_cols] (compound= only)"""
        if self.steers is None:
            raise RuntimeError("compound_image() needs Simulator(compound=...)")
        self._run(frame_id, convolve, envelope)
        with self.ctx.temp(out_rows * out_cols * 4) as out:
            self.ctx.compound_frames(self.views_dev, 1, self.E, self.R, self.steers, out, radius_mm=radius_mm, total_angle=total_angle, out_rows=out_rows,
                                     out_cols=out_cols, **self.compound_opts)
            return self.ctx.d2h(out, (out_rows, out_cols), np.float32)

    def volume(self, frame_id, grid, convolve=True, envelope=True, radius_mm=30.0, total_angle=DEFAULT_ANGLE):
        """trace -> convolve -> envelope -> mcrt_volume_frames (-> despeckle_volume with speckle3d=) -> host: the float voxels [nw][nv][nu] of
        grid, a volume or any cut (sweep= only)"""
        if self.sweep is None:
            raise RuntimeError("volume() needs Simulator(sweep=...)")
        self._run(frame_id, convolve, envelope)
        shape, n = _grid_shape(grid)
        with self.ctx.temp(n * 4) as out:
            self.ctx.volume_frames(self.sweep_dev, 1, self.E, self.R, self.sweep, grid, out, radius_mm=radius_mm, total_angle=total_angle)
            if self.speckle3d is not None:
                self.despeckle_volume(out, grid)
            return self.ctx.d2h(out, shape, np.float32)

    def bmode_volume(self, frame_id, grid, **display):
        """trace -> convolve -> envelope -> mcrt_bmode_volume_frames -> host: the displayed 8-bit voxels, uint8 [nw][nv][nu] (sweep= only).
        display: the keywords of Context.bmode_volume_frames (mode, dynamic_range_db, gain_db, ref, tgc_db, radius_mm, total_angle)"""
        if self.sweep is None:
            raise RuntimeError("bmode_volume() needs Simulator(sweep=...)")
        if self.speckle3d is not None:
            raise RuntimeError("bmode_volume() gathers bytes straight from the planes: there is no float block for speckle3d= to filter (use volume())")
        self._run(frame_id)
        shape, n = _grid_shape(grid)
        with self.ctx.temp(n) as out:
            self.ctx.bmode_volume_frames(self.sweep_dev, 1, self.E, self.R, self.sweep, grid, out, **display)
            return self.ctx.d2h(out, shape, np.uint8)

    def render(self, frame_id, grid, direction, up=(0, 0, 1), size=(500, 400), pixel_mm=0.25, step_mm=0.25, mode="surface", labels=False, label_rule="traced",
               label_offset=None, **opts):
        """trace -> convolve -> envelope -> mcrt_bmode_volume_frames -> mcrt_render_frames -> host: grid's displayed voxels seen along
        `direction`, uint8 [ny][nx] with size = (nx, ny) (sweep= only).  opts: the display keywords of Context.bmode_volume_frames
        (dynamic_range_db, gain_db, ref, tgc_db, radius_mm, total_angle; bmode_mode for its grey curve) and the render keywords of
        Context.render_frames (lo, hi, threshold, ramp, opacity, depth_cue, t_cut).
        labels=True: (picture, labels) -- the tissue of what every pixel shows, uint8 [ny][nx]: the label block of label_volume() on the
        same grid (label_rule, label_offset: its rule and start_offset) read through the depth buffer of the same render call; LABEL_NONE
        where the ray saw nothing (every pixel of mode "mean") or saw it outside the sweep"""
        if self.sweep is None:
            raise RuntimeError("render() needs Simulator(sweep=...)")
        if self.speckle3d is not None:
            raise RuntimeError("render() gathers bytes straight from the planes: there is no float block for speckle3d= to filter "
                               "(Context.volume_frames -> speckle_volume_frames -> render_frames(in_u8=False) renders a filtered block)")
        ropts = {k: opts.pop(k) for k in ("lo", "hi", "threshold", "ramp", "opacity", "depth_cue", "t_cut") if k in opts}
        if "bmode_mode" in opts:
            opts["mode"] = opts.pop("bmode_mode")
        view = render_view(grid, direction, up, pixel_mm, step_mm, size[0], size[1])
        self._run(frame_id)
        shape, n = _grid_shape(grid)
        with self.ctx.temp(n) as vox, self.ctx.temp(size[0] * size[1]) as out:
            self.ctx.bmode_volume_frames(self.sweep_dev, 1, self.E, self.R, self.sweep, grid, vox, **opts)
            if not labels:
                self.ctx.render_frames(vox, 1, shape, view, out8_dev=out, in_u8=True, mode=mode, **ropts)
                return self.ctx.d2h(out, (size[1], size[0]), np.uint8)
            geometry = {k: opts[k] for k in ("radius_mm", "total_angle") if k in opts}
            with self.ctx.temp(size[0] * size[1] * 4) as depth, self._label_pass(label_rule, label_offset, want_rows=False) as (F, bufs):
                self.ctx.render_frames(vox, 1, shape, view, out8_dev=out, depth_dev=depth, in_u8=True, mode=mode, **ropts)
                picture = self.ctx.d2h(out, (size[1], size[0]), np.uint8)
                self.ctx.label_volume_frames(bufs[0], 1, self.E, self.R, self.sweep, grid, vox, **geometry)      # (the voxels are rendered: the block is free)
                self.ctx.render_label_frames(vox, 1, shape, view, depth, out)
                return picture, self.ctx.d2h(out, (size[1], size[0]), np.uint8)

    def freehand(self, frame_id, pos, dirs, grid, convolve=True, envelope=True, counts=False, row_mm=None, unit_mm=10.0, **opts):
        """a freehand sweep and its volume: the F poses pos / dirs [F][E][3] (Transducer.poses) traced as one pose pass into a temporary stack
        -- pose f with frame id frame_id * F + f -- -> convolve (-> add_noise with noise=) -> envelope (-> despeckle with speckle=) (-> auto_gain with autogain=) -> mcrt_recon_frames -> host: the float
        voxels [nw][nv][nu] of grid (a VolumeGrid in the WORLD frame, mm); with counts=True (voxels, sample counts uint32 of the same shape).
        opts: the keywords of recon_opts_struct.  It raises under compound=, sweep= or elevation=.
        With speckle3d= the block is filtered on the device (despeckle_volume) before it is copied out.  A hole's `empty` value is then a
        value like any other -- step 0 of the rule applies to it (|empty|, or 0 when it is not finite) and it diffuses into its
        neighbours; counts=True still tells which voxels were empty."""
        if self.steers is not None or self.sweep is not None or self.elevation:
            raise RuntimeError("freehand() does not combine with compound=, sweep= or elevation=")
        pos, dirs, F = _pose_tables("freehand", np.asarray(pos), np.asarray(dirs), None, self.E)
        shape, n = _grid_shape(grid)
        with self.ctx.temp(F * self.E * self.R * 4) as stack_dev, self.ctx.temp(n * 4) as out, self.ctx.temp(n * 4) as cnt:
            self.ctx.trace_frames_poses(frame_id * F, pos, dirs, stack_dev)
            self._stages((stack_dev, F), frame_id, convolve, envelope, own_frames=True)       # (every tracked frame is a frame of its own)
            self.ctx.recon_frames(stack_dev, pos, dirs, F, self.E, self.R, grid, out, count_dev=cnt if counts else None, row_mm=row_mm, unit_mm=unit_mm, **opts)
            if self.speckle3d is not None:
                self.despeckle_volume(out, grid)
            vox = self.ctx.d2h(out, shape, np.float32)
            return (vox, self.ctx.d2h(cnt, shape, np.uint32)) if counts else vox

    def freehand_labels(self, pos, dirs, grid, rule="traced", start_offset=None, fill_radius=1, fill_min=1, counts=False, votes=False):
        """the ground truth of freehand()'s volume: the label pass over the F poses pos / dirs [F][E][3] (mcrt_label_frames: the central beam
        of every scan-line), then mcrt_recon_label_frames with the scene's material count as n_labels -> host: the tissue of every voxel of
        grid, uint8 [nw][nv][nu] -- the label most of a voxel's samples carry, a hole filled from its sampled neighbours, LABEL_NONE where
        nothing is near; with counts=True and / or votes=True a tuple (labels[, samples per voxel uint32][, the winner's votes uint32]).
        Labels depend on neither seed nor frame: there is no frame_id.  row_mm and unit_mm are freehand()'s defaults, fill_radius and
        fill_min its defaults too, so the two volumes fill the same holes.  It raises under compound=, sweep= or elevation= as freehand()
        does, and mcrt_label_frames takes at most 1024 poses per pass."""
        if self.steers is not None or self.sweep is not None or self.elevation:
            raise RuntimeError("freehand_labels() does not combine with compound=, sweep= or elevation=")
        pos, dirs, F = _pose_tables("freehand_labels", np.asarray(pos), np.asarray(dirs), None, self.E)
        shape, n = _grid_shape(grid)
        with self.ctx.temp(F * self.E * self.R) as tissue, self.ctx.temp(n) as out, self.ctx.temp(n * 4) as cnt, self.ctx.temp(n * 4) as win:
            self.ctx.label_frames(pos, dirs, rule=rule, start_offset=start_offset, tissue_dev=tissue)
            self.ctx.recon_label_frames(tissue, pos, dirs, F, self.E, self.R, grid, self.n_materials, out, count_dev=cnt if counts else None,
                                        votes_dev=win if votes else None, fill_radius=fill_radius, fill_min=fill_min)
            got = (self.ctx.d2h(out, shape, np.uint8),) + ((self.ctx.d2h(cnt, shape, np.uint32),) if counts else ()) + ((self.ctx.d2h(win, shape, np.uint32),) if votes else ())
            return got if len(got) > 1 else got[0]

    @contextlib.contextmanager
    def _beam_pass(self, call, tables, want_rows, **opts):
        """a central-beam pass of this probe (call: Context.label_frames or transmit_frames, with opts) into device buffers that live as long as the
        block -> (F, [the two row tables named in `tables` = ((keyword, bytes per sample), ...), crossings_dev]; only the first unless want_rows): the K
        planes of a sweep, else the unsteered probe in its own plane, whatever compound= and elevation= are"""
        F = self.sweep.n_planes if self.sweep is not None else 1
        n = F * self.E * self.R
        with contextlib.ExitStack() as held:
            sizes = (tables[0][1] * n, tables[1][1] * n, 4 * F * self.E) if want_rows else (tables[0][1] * n, 0, 0)
            bufs = [held.enter_context(self.ctx.temp(size)) if size else None for size in sizes]
            pos, dirs = (self.sweep_pos, self.sweep_dir) if self.sweep is not None else (None, None)
            call(pos, dirs, **opts, **{tables[0][0]: bufs[0], tables[1][0]: bufs[1], "crossings_dev": bufs[2]})
            yield F, bufs

    def _label_pass(self, rule, start_offset, want_rows=True):
        """-> (F, [tissue_dev, interface_dev, crossings_dev])"""
        return self._beam_pass(self.ctx.label_frames, (("tissue_dev", 1), ("interface_dev", 4)), want_rows, rule=rule, start_offset=start_offset)

    def _transmit_pass(self, mode, rule, start_offset, want_rows=True):
        """-> (F, [transmit_dev, reflect_dev, crossings_dev])"""
        return self._beam_pass(self.ctx.transmit_frames, (("transmit_dev", 4), ("reflect_dev", 4)), want_rows, mode=mode, rule=rule, start_offset=start_offset)

    def labels(self, rule="traced", start_offset=None, picture=True, radius_mm=30.0, total_angle=DEFAULT_ANGLE, out_rows=400, out_cols=500):
        """the ground truth of this probe's pictures -> dict(tissue uint8 [E][R], interface int32 [E][R], crossings uint32 [E], picture uint8
        [out_rows][out_cols] or None): material index per scan-line sample, mesh id of the boundary in it (-1: none), boundaries per
        scan-line (bit 31: LABEL_CAPPED), and the tissue map scan-converted like the B-mode picture (LABEL_NONE outside the sector).  It is
        the unsteered probe's central beam per scan-line, whatever compound= is; with elevation= the probe's own plane.  With sweep= the
        arrays gain a leading axis of the K planes and there is no sector picture: use label_volume()."""
        with self._label_pass(rule, start_offset) as (F, bufs):
            lead = (F,) if self.sweep is not None else ()
            out = dict(tissue=self.ctx.d2h(bufs[0], lead + (self.E, self.R), np.uint8), interface=self.ctx.d2h(bufs[1], lead + (self.E, self.R), np.int32),
                       crossings=self.ctx.d2h(bufs[2], lead + (self.E,), np.uint32), picture=None)
            if picture and self.sweep is None:
                with self.ctx.temp(out_rows * out_cols) as pic_dev:
                    self.ctx.label_scan_convert_frames(bufs[0], 1, self.E, self.R, pic_dev, radius_mm=radius_mm, total_angle=total_angle, out_rows=out_rows, out_cols=out_cols)
                    out["picture"] = self.ctx.d2h(pic_dev, (out_rows, out_cols), np.uint8)
            return out

    def label_volume(self, grid, rule="traced", start_offset=None, radius_mm=30.0, total_angle=DEFAULT_ANGLE):
        """the tissue of every point of grid, uint8 [nw][nv][nu]: the labels of volume() / bmode_volume() (sweep= only; LABEL_NONE outside the sweep)"""
        if self.sweep is None:
            raise RuntimeError("label_volume() needs Simulator(sweep=...)")
        shape, n = _grid_shape(grid)
        with self._label_pass(rule, start_offset, want_rows=False) as (F, bufs), self.ctx.temp(n) as out:
            self.ctx.label_volume_frames(bufs[0], 1, self.E, self.R, self.sweep, grid, out, radius_mm=radius_mm, total_angle=total_angle)
            return self.ctx.d2h(out, shape, np.uint8)

    def transmission(self, mode="total", rule="traced", start_offset=None, picture=True, radius_mm=30.0, total_angle=DEFAULT_ANGLE, out_rows=400, out_cols=500):
        """the acoustic ground truth of this probe's pictures -> dict(transmit float32 [E][R], reflect float32 [E][R], crossings uint32 [E],
        picture float32 [out_rows][out_cols] or None): the fraction of the emitted intensity that arrives at every scan-line sample (the
        shadow behind bone, the enhancement behind fluid), the fraction the boundary in a sample turns back, boundaries per scan-line as
        labels(), and `transmit` scan-converted like the float picture (mcrt_scan_convert_frames: 0 outside the sector;
        labels()["picture"] == LABEL_NONE is the mask).  Deterministic: it depends on neither seed, samples nor texture.  The probe is
        labels()' own; with sweep= the arrays gain a leading axis of the K planes and there is no sector picture: use
        transmission_volume()."""
        with self._transmit_pass(mode, rule, start_offset) as (F, bufs):
            lead = (F,) if self.sweep is not None else ()
            out = dict(transmit=self.ctx.d2h(bufs[0], lead + (self.E, self.R), np.float32), reflect=self.ctx.d2h(bufs[1], lead + (self.E, self.R), np.float32),
                       crossings=self.ctx.d2h(bufs[2], lead + (self.E,), np.uint32), picture=None)
            if picture and self.sweep is None:
                with self.ctx.temp(out_rows * out_cols * 4) as pic_dev:
                    self.ctx.scan_convert_frames(bufs[0], 1, self.E, self.R, pic_dev, radius_mm=radius_mm, total_angle=total_angle, out_rows=out_rows, out_cols=out_cols)
                    out["picture"] = self.ctx.d2h(pic_dev, (out_rows, out_cols), np.float32)
            return out

    def transmission_volume(self, grid, mode="total", rule="traced", start_offset=None, radius_mm=30.0, total_angle=DEFAULT_ANGLE):
        """`transmit` at every point of grid, float32 [nw][nv][nu]: the transmission of volume()'s voxels, through mcrt_volume_frames (sweep= only)"""
        if self.sweep is None:
            raise RuntimeError("transmission_volume() needs Simulator(sweep=...)")
        shape, n = _grid_shape(grid)
        with self._transmit_pass(mode, rule, start_offset, want_rows=False) as (F, bufs), self.ctx.temp(n * 4) as out:
            self.ctx.volume_frames(bufs[0], 1, self.E, self.R, self.sweep, grid, out, radius_mm=radius_mm, total_angle=total_angle)
            return self.ctx.d2h(out, shape, np.float32)

    def freehand_transmission(self, pos, dirs, grid, mode="total", rule="traced", start_offset=None, counts=False, row_mm=None, unit_mm=10.0, **opts):
        """the transmission of freehand()'s volume: the transmission pass over the F poses pos / dirs [F][E][3], then mcrt_recon_frames in its
        mean mode with freehand()'s defaults -> host: float32 [nw][nv][nu]; with counts=True (voxels, sample counts uint32).  opts: the
        keywords of recon_opts_struct.  There is no frame_id (nothing is random); it raises under compound=, sweep= or elevation= as
        freehand_labels() does, and takes at most 1024 poses per pass."""
        if self.steers is not None or self.sweep is not None or self.elevation:
            raise RuntimeError("freehand_transmission() does not combine with compound=, sweep= or elevation=")
        pos, dirs, F = _pose_tables("freehand_transmission", np.asarray(pos), np.asarray(dirs), None, self.E)
        shape, n = _grid_shape(grid)
        with self.ctx.temp(F * self.E * self.R * 4) as stack_dev, self.ctx.temp(n * 4) as out, self.ctx.temp(n * 4) as cnt:
            self.ctx.transmit_frames(pos, dirs, mode=mode, rule=rule, start_offset=start_offset, transmit_dev=stack_dev)
            self.ctx.recon_frames(stack_dev, pos, dirs, F, self.E, self.R, grid, out, count_dev=cnt if counts else None, row_mm=row_mm, unit_mm=unit_mm, **opts)
            vox = self.ctx.d2h(out, shape, np.float32)
            return (vox, self.ctx.d2h(cnt, shape, np.uint32)) if counts else vox

    def bmode(self, frame_id=0, **display):
        """trace -> convolve -> envelope -> mcrt_bmode_frames -> host: the displayed 8-bit frame, uint8 [out_rows][out_cols].
        display: the keywords of Context.bmode_frames (mode, dynamic_range_db, gain_db, ref, tgc_db, ...)"""
        if self.sweep is not None:
            raise RuntimeError("a swept probe has K planes and meets only at a grid's points: use volume() or bmode_volume()")
        rows, cols = display.get("out_rows", 400), display.get("out_cols", 500)
        self._run(frame_id)
        with self.ctx.temp(rows * cols) as out:
            if self.steers is not None:
                o = self.compound_opts
                self.ctx.bmode_compound_frames(self.views_dev, 1, self.E, self.R, self.steers, out, compound_mode=o["mode"], view_weights=o["view_weights"],
                                               feather_lines=o["feather_lines"], **display)
            else:
                self.ctx.bmode_frames(self.rf_dev, 1, self.E, self.R, out, **display)
            return self.ctx.d2h(out, (rows, cols), np.uint8)

    def frame(self, frame_id=0, convolve=True):
        if self.sweep is not None:
            raise RuntimeError("a swept probe has K planes and meets only at a grid's points: use volume() or bmode_volume()")
        if self.steers is not None:
            raise RuntimeError("frame() returns one RF image; a compounded frame has N views and meets only as a picture: use compound_image() or bmode()")
        self._run(frame_id, convolve, envelope=False)
        return self.ctx.export_rf(self.rf_dev, self.E, self.R)

    def iq(self, frame_id=0, convolve=True):
        """frame()'s stages -> mcrt_detect_frames with iq_dev -> host: the analytic signal of the frame's RF at the RF rate, complex64 of
        frame()'s shape [R][E] -- the real part frame()'s own bits, the imaginary part the FIR Hilbert transform along the scan-line
        (n_taps of detect=, else 31).  It raises where frame() raises, and with a psf that has bands: the coherent sum of the band images
        has no one carrier"""
        if self.psf.has_bands:
            raise RuntimeError("iq() returns the analytic pair of one RF image; with bands there is one image per band: give a psf without bands")
        if self.sweep is not None or self.steers is not None:
            return self.frame(frame_id, convolve)       # (it raises, and says what to use)
        self._run(frame_id, convolve, envelope=False)
        with self.ctx.temp(self.E * self.R * 8) as out:
            self.ctx.detect_frames(self.rf_dev, 1, self.E, self.R, iq_dev=out, **(self.detect or {}))
            pair = self.ctx.d2h(out, (self.E, self.R, 2), np.float32)
        return np.ascontiguousarray(pair.transpose(1, 0, 2)).view(np.complex64)[..., 0]

    # ---- colour Doppler (flow=)
    @contextlib.contextmanager
    def _flow_pass(self, frame_id, want):
        """ONE trace of the frame -> the label pass -> the raw RF split by label (its device copy: rf_dev goes on through bmode()'s own
        stages in place, noise= included, which leaves sigma on the device) -> the two parts through the PSF and the detector's I/Q ->
        mcrt_flow_frames.  Yields dict(tissue, corr, vel, var, truth: device buffers that live as long as the block, those in `want`;
        iq_static, iq_moving: the detected pairs [E][R][2] the ensemble was made of; sigma: the ensemble's, on the host)"""
        if self.flow is None:
            raise RuntimeError("colour flow needs Simulator(flow=...)")
        for on, what in ((self.sweep is not None, "sweep="), (self.steers is not None, "compound="), (self.elevation, "elevation="), (self.psf.has_bands, "a psf with bands")):
            if on:
                raise RuntimeError("colour flow is one plane of one pulse: it does not combine with %s" % what)
        fl, n = self.flow, self.E * self.R
        sizes = dict(corr=12 * n, vel=4 * n, var=4 * n, truth=4 * n)
        with contextlib.ExitStack() as held:
            tissue, parts, iq = (held.enter_context(self.ctx.temp(size)) for size in (n, 8 * n, 16 * n))
            out = {k: held.enter_context(self.ctx.temp(sizes[k])) for k in want}
            self.trace(frame_id)
            self.ctx.label_frames(tissue_dev=tissue, **fl["label"])
            self.ctx.flow_split_frames(self.rf_dev, tissue, 1, self.E, self.R, fl["moving"], parts)
            self._stages(self._stack, frame_id)
            self._convolve(_Images(parts, 2, 2, 1, 0))
            self.ctx.detect_frames(parts, 2, self.E, self.R, iq_dev=iq, **(self.detect or {}))
            sigma_dev = self._gain_bufs(1)[0] if self.noise is not None else None
            self.ctx.flow_frames(iq, iq + 8 * n, tissue, 1, self.E, self.R, fl["v_nyq"], fl["phasor"], fl["truth"], first_image_id=frame_id, sigma_dev=sigma_dev,
                                 opts=fl["opts"], **{k + "_dev": p for k, p in out.items()})
            sigma = float(self.ctx.d2h(sigma_dev, (1,), np.float32)[0]) if sigma_dev is not None else float(fl["opts"].sigma)
            yield dict(out, tissue=tissue, sigma=sigma, iq_static=iq, iq_moving=iq + 8 * n)

    def flow_velocity(self, frame_id=0):
        """the colour processor's estimates in beam space -> dict(vel, var, truth: float32 [E][R]): the Kasai velocity [mm/s, towards the
        probe positive, aliased beyond the Nyquist velocity], the variance estimate in 0..1, and the true axial velocity of every
        sample's material (flow= only)"""
        with self._flow_pass(frame_id, ("vel", "var", "truth")) as b:
            return {k: self.ctx.d2h(b[k], (self.E, self.R), np.float32) for k in ("vel", "var", "truth")}

    def spectral_doppler(self, frame_id=0, gate=(0, 0.0, 2.0), material="BLOOD", waveform=None, profile=2.0, window="hann", **kw):
        """the sonogram of one sample gate -> dict(power float32 [n_cols][N] in velocity order, grey uint8 [N][n_cols] as displayed (row 0
        the highest velocity towards the probe), mean float32 [n_cols], series complex64 [T], truth float32 [n_cols], velocity_axis float64
        [N] in mm/s, time_axis float64 [n_cols] in seconds (the windows' centres)).  It traces ONCE and runs colour flow's chain up to the
        detected pairs (flow= only; it refuses what colour_flow() refuses), reads the gate line's tissue labels for the velocity profile
        and synthesises the slow-time series of the gate.  gate: (scan-line, depth_mm of the gate's centre, length_mm); material: the
        scene's material whose velocity vector (flow=) gives the direction of the flow -- its length is not used: waveform is the
        centre-line speed [mm/s] per pulse, an array or dict(beats_per_min=, v_peak=, v_min=) for host_pulse_waveform at the flow's
        prf_hz (n_pulses pulses, default 2048); profile: the exponent of host_spectral_profile (0: plug flow, 2: a parabola).  truth is
        the true axial centre-line velocity averaged over each window.  kw: n_pulses, n_fft, hop, wall, wall_bins, sigma (default: the
        ensemble's), seed, and the sonogram's dynamic_range_db, gain_db, ref"""
        if self.flow is None:
            raise RuntimeError("spectral Doppler needs Simulator(flow=...)")
        fl = self.flow
        if material not in self.material_names:
            raise ValueError("spectral_doppler: the scene has no material %r (it has %s)" % (material, ", ".join(self.material_names)))
        label = self.material_names.index(material)
        vel = fl["vel"][label].astype(np.float64)
        if not vel.any():
            raise ValueError("spectral_doppler: flow= gives material %r no velocity, so the flow has no direction" % material)
        norm = float(np.sqrt((vel[0] * vel[0] + vel[1] * vel[1]) + vel[2] * vel[2]))
        display = {k: kw.pop(k) for k in ("dynamic_range_db", "gain_db", "ref") if k in kw}
        line, depth_mm, length_mm = int(gate[0]), float(gate[1]), float(gate[2])
        pitch = row_pitch_mm(self.tr.frequency)
        G = min(max(int(round(length_mm / pitch)), 1), 64, self.R)
        row0 = min(max(int(round(depth_mm / pitch - G / 2.0)), 0), self.R - G)
        if not 0 <= line < self.E:
            raise ValueError("spectral_doppler: scan-line %d is not in 0..%d" % (line, self.E - 1))
        prf = float(fl["opts"].prf_hz)
        if waveform is None or isinstance(waveform, dict):
            w = dict(beats_per_min=72.0, v_peak=norm, v_min=0.0)
            w.update(waveform or {})
            speed = host_pulse_waveform(prf, w["beats_per_min"], w["v_peak"], w["v_min"], kw.get("n_pulses", 2048))
        else:
            speed = np.ascontiguousarray(waveform, np.float32).reshape(-1)
        kw["n_pulses"] = speed.size
        d = self.tr.dir[line].astype(np.float64)
        unit = (vel / norm).astype(np.float32).astype(np.float64)
        axial = min(max(0.0 - ((unit[0] * d[0] + unit[1] * d[1]) + unit[2] * d[2]), -1.0), 1.0)
        moving = np.zeros(len(self.material_names), np.uint8); moving[label] = 1
        with self._flow_pass(frame_id, ("truth",)) as b:
            kw.setdefault("sigma", b["sigma"])
            o = spectral_opts_struct(gate_rows=G, **kw)
            T, N, hop = o.n_pulses, o.n_fft, o.hop
            if T < N:
                raise ValueError("spectral_doppler: %d pulses are fewer than one window of %d" % (T, N))
            cols = (T - N) // hop + 1
            tissue_line = self.ctx.d2h(b["tissue"] + line * self.R, (self.R,), np.uint8)
            frac = host_spectral_profile(tissue_line, row0, G, moving, profile)
            rate = host_spectral_rates(frac, axial)
            phase = host_spectral_phase(fl["v_nyq"], speed)
            with self.ctx.temp(8 * T) as series, self.ctx.temp(4 * cols * N) as power, self.ctx.temp(4 * cols) as mean, self.ctx.temp(cols * N) as grey:
                self.ctx.spectral_series_frames(b["iq_static"], b["iq_moving"], 1, self.E, self.R, [[0, line, row0]], np.ones(G, np.float32), rate, phase, series,
                                                first_image_id=frame_id, opts=o)
                self.ctx.spectral_frames(series, 1, fl["v_nyq"], power_dev=power, mean_dev=mean, window=window, opts=o)
                self.ctx.sonogram_frames(power, 1, cols, N, grey, **display)
                z = self.ctx.d2h(series, (T, 2), np.float32)
                out = dict(power=self.ctx.d2h(power, (cols, N), np.float32), grey=self.ctx.d2h(grey, (N, cols), np.uint8),
                           mean=self.ctx.d2h(mean, (cols,), np.float32), series=np.ascontiguousarray(z).view(np.complex64)[:, 0])
        axial_speed = speed.astype(np.float64) * axial
        out["truth"] = np.array([axial_speed[c * hop:c * hop + N].mean() for c in range(cols)], np.float32)
        out["velocity_axis"] = (np.arange(N) - N // 2) * (2.0 * fl["v_nyq"] / N)
        out["time_axis"] = (np.arange(cols) * hop + N / 2.0) / prf
        out["gate"] = dict(line=line, row0=row0, rows=G, rate=rate, frac=frac, axial=axial)
        return out

    # ---- strain elastography (strain=)
    @contextlib.contextmanager
    def _strain_pass(self, frame_id):
        """ONE trace of the frame -> the label pass -> frame()'s stages -> the detector's I/Q -> mcrt_strain_compress_frames ->
        mcrt_strain_frames.  Yields dict(tissue, post, truth_disp, truth_strain, disp, rho, strain: device buffers that live as long as
        the block); rf_dev holds the frame's RF before the envelope"""
        if self.strain_opts is None:
            raise RuntimeError("strain imaging needs Simulator(strain=...)")
        for on, what in ((self.sweep is not None, "sweep="), (self.steers is not None, "compound="), (self.elevation, "elevation="), (self.psf.has_bands, "a psf with bands")):
            if on:
                raise RuntimeError("strain imaging is one plane of one pulse: it does not combine with %s" % what)
        st, n = self.strain_opts, self.E * self.R
        cycles = host_psf_carrier(self.tr.frequency, self.psf.resolution_um)
        with contextlib.ExitStack() as held:
            tissue, iq, post = (held.enter_context(self.ctx.temp(size)) for size in (n, 8 * n, 8 * n))
            out = {k: held.enter_context(self.ctx.temp(4 * n)) for k in ("truth_disp", "truth_strain", "disp", "rho", "strain")}
            self.trace(frame_id)
            self.ctx.label_frames(tissue_dev=tissue, **st["label"])
            self._stages(self._stack, frame_id, envelope=False)
            self.ctx.detect_frames(self.rf_dev, 1, self.E, self.R, iq_dev=iq, **(self.detect or {}))
            self.ctx.strain_compress_frames(iq, tissue, 1, self.E, self.R, st["eps"], cycles, first_image_id=frame_id, post_iq_dev=post,
                                            truth_disp_dev=out["truth_disp"], truth_strain_dev=out["truth_strain"], opts=st["opts"])
            self.ctx.strain_frames(iq, post, 1, self.E, self.R, cycles, disp_dev=out["disp"], rho_dev=out["rho"], strain_dev=out["strain"], opts=st["opts"])
            yield dict(out, tissue=tissue, iq=iq, post=post)

    def _strain_host(self, b):
        return {k: self.ctx.d2h(b[k], (self.E, self.R), np.float32) for k in ("strain", "rho", "disp", "truth_strain", "truth_disp")}

    def strain(self, frame_id=0):
        """the tracker's estimates in beam space -> dict(strain, rho, disp, truth_strain, truth_disp: float32 [E][R]): the estimated strain
        (positive: compression), the correlation coefficient of the winning lag, the displacement in rows, and the true strain and
        displacement of every sample, registered sample for sample (strain= only)"""
        with self._strain_pass(frame_id) as b:
            return self._strain_host(b)

    def elastogram(self, frame_id=0, ref_strain=None, rho_min=None, grey_min=None, alpha=None, lut=None, **display):
        """the elastogram of a frame -> dict(rgb uint8 [out_rows][out_cols][3], grey uint8 [out_rows][out_cols], strain_img and rho_img
        float32 [out_rows][out_cols], and strain()'s beam-space outputs).  It traces ONCE; grey is bmode()'s own picture of that trace
        (display: the keywords of Context.bmode_frames), the strain and the correlation coefficient are gathered through
        mcrt_scan_convert_frames and laid over it by mcrt_elastogram_frames; ref_strain defaults to the applied strain (strain= only)"""
        if display.get("persistence", 0.0) != 0.0:
            raise ValueError("elastogram() shows one frame: persistence is left out")
        rows, cols = display.get("out_rows", 400), display.get("out_cols", 500)
        geometry = {k: display[k] for k in ("radius_mm", "total_angle", "out_rows", "out_cols") if k in display}
        n = rows * cols
        with self._strain_pass(frame_id) as b, self.ctx.temp(n) as grey, self.ctx.temp(8 * n) as img, self.ctx.temp(3 * n) as rgb:
            s = self._images(frame_id)
            self._detect(s, s)                              # bmode()'s remaining stages over the same trace
            if self.speckle is not None:
                self._despeckle(s)
            if self.autogain is not None:
                self._autogain(s)
            self.ctx.bmode_frames(self.rf_dev, 1, self.E, self.R, grey, **display)
            self.ctx.scan_convert_frames(b["strain"], 1, self.E, self.R, img, **geometry)
            self.ctx.scan_convert_frames(b["rho"], 1, self.E, self.R, img + 4 * n, **geometry)
            self.ctx.elastogram_frames(img, img + 4 * n, grey, 1, rows, cols, rgb, lut=lut, rho_min=rho_min, grey_min=grey_min, alpha=alpha,
                                       ref_strain=self.strain_opts["applied"] if ref_strain is None else ref_strain)
            return dict(self._strain_host(b), rgb=self.ctx.d2h(rgb, (rows, cols, 3), np.uint8), grey=self.ctx.d2h(grey, (rows, cols), np.uint8),
                        strain_img=self.ctx.d2h(img, (rows, cols), np.float32), rho_img=self.ctx.d2h(img + 4 * n, (rows, cols), np.float32))

    # ---- shear-wave elastography (shear=)
    SHEAR_MAPS = ("speed", "modulus", "quality", "peak_time", "peak_disp", "truth_arrival", "truth_speed")

    @contextlib.contextmanager
    def _shear_pass(self, frame_id):
        """ONE trace of the frame -> the label pass -> frame()'s stages -> the detector's I/Q -> mcrt_shear_wave_frames ->
        mcrt_shear_speed_frames.  Yields dict(tissue, iq and SHEAR_MAPS: device buffers that live as long as the block); rf_dev holds the
        frame's RF before the envelope"""
        if self.shear_opts is None:
            raise RuntimeError("shear-wave imaging needs Simulator(shear=...)")
        for on, what in ((self.sweep is not None, "sweep="), (self.steers is not None, "compound="), (self.elevation, "elevation="), (self.psf.has_bands, "a psf with bands")):
            if on:
                raise RuntimeError("shear-wave imaging is one plane of one pulse: it does not combine with %s" % what)
        sh, n, o = self.shear_opts, self.E * self.R, self.shear_opts["opts"]
        if sh["push"] is not None:
            line, depth_mm, length_mm = int(sh["push"][0]), float(sh["push"][1]), float(sh["push"][2])
            if not 0 <= line < self.E:
                raise ValueError("shear: scan-line %d is not in 0..%d" % (line, self.E - 1))
            pitch = row_pitch_mm(self.tr.frequency)
            rows = min(max(int(round(length_mm / pitch)), 1), self.R)
            o.push_line, o.push_rows = line, rows
            o.push_row0 = min(max(int(round(depth_mm / pitch - rows / 2.0)), 0), self.R - rows)
        prm = self.ctx.params
        travel = int((prm.depth_cm / float(prm.speed_of_sound)) * 10000.0)
        pitch_q8, pitch_mm = host_shear_pitch(self.E, self.R, max_travel_us=travel, speed_of_sound=int(prm.speed_of_sound), **sh["geometry"])
        cycles = host_psf_carrier(self.tr.frequency, self.psf.resolution_um)
        with contextlib.ExitStack() as held:
            tissue, iq = (held.enter_context(self.ctx.temp(size)) for size in (n, 8 * n))
            out = {k: held.enter_context(self.ctx.temp(4 * n)) for k in self.SHEAR_MAPS}
            self.trace(frame_id)
            self.ctx.label_frames(tissue_dev=tissue, **sh["label"])
            self._stages(self._stack, frame_id, envelope=False)
            self.ctx.detect_frames(self.rf_dev, 1, self.E, self.R, iq_dev=iq, **(self.detect or {}))
            self.ctx.shear_wave_frames(iq, tissue, 1, self.E, self.R, sh["slow"], sh["speed_f"], pitch_q8, sh["shape"], host_shear_decay(self.E, sh["decay"]), cycles,
                                       first_image_id=frame_id, peak_time_dev=out["peak_time"], peak_disp_dev=out["peak_disp"],
                                       truth_arrival_dev=out["truth_arrival"], truth_speed_dev=out["truth_speed"], opts=o)
            self.ctx.shear_speed_frames(out["peak_time"], 1, self.E, self.R, pitch_mm, speed_dev=out["speed"], modulus_dev=out["modulus"],
                                        quality_dev=out["quality"], opts=o)
            yield dict(out, tissue=tissue, iq=iq)

    def _shear_host(self, b):
        return {k: self.ctx.d2h(b[k], (self.E, self.R), np.float32) for k in self.SHEAR_MAPS}

    def shear_wave(self, frame_id=0):
        """the shear wave of a push in beam space -> dict(speed [m/s], modulus [kPa], quality (the r^2 of the fit), peak_time [pulses],
        peak_disp [rows], truth_arrival [pulses, +inf: never] and truth_speed [m/s]: float32 [E][R]), the truths registered sample for
        sample (shear= only)"""
        with self._shear_pass(frame_id) as b:
            return self._shear_host(b)

    def shear_elastogram(self, frame_id=0, ref_kpa=None, quality_min=None, grey_min=None, alpha=None, lut=None, **display):
        """the shear-wave elastogram of a frame -> dict(rgb uint8 [out_rows][out_cols][3], grey uint8 [out_rows][out_cols], modulus_img and
        quality_img float32 [out_rows][out_cols], and shear_wave()'s beam-space outputs).  It traces ONCE; grey is bmode()'s own picture of
        that trace (display: the keywords of Context.bmode_frames), the modulus and the quality are gathered through
        mcrt_scan_convert_frames and laid over it by mcrt_elastogram_frames as they are, with host_shear_map()'s table (soft blue, stiff
        red); ref_kpa defaults to shear=...'s; a radius_mm or total_angle other than shear=...'s, the sector the pitch was taken from, is
        refused (shear= only)"""
        if display.get("persistence", 0.0) != 0.0:
            raise ValueError("shear_elastogram() shows one frame: persistence is left out")
        for k, v in (self.shear_opts or {}).get("geometry", {}).items():
            if float(display.get(k, v)) != v:               # the speed is scaled by the pitch of one sector: the picture is drawn in the same
                raise ValueError("shear_elastogram(): %s=%r differs from shear=...'s %r, the sector the scan-line pitch was taken from" % (k, display[k], v))
        rows, cols = display.get("out_rows", 400), display.get("out_cols", 500)
        geometry = {k: display[k] for k in ("radius_mm", "total_angle", "out_rows", "out_cols") if k in display}
        n = rows * cols
        with self._shear_pass(frame_id) as b, self.ctx.temp(n) as grey, self.ctx.temp(8 * n) as img, self.ctx.temp(3 * n) as rgb:
            s = self._images(frame_id)
            self._detect(s, s)                              # bmode()'s remaining stages over the same trace
            if self.speckle is not None:
                self._despeckle(s)
            if self.autogain is not None:
                self._autogain(s)
            self.ctx.bmode_frames(self.rf_dev, 1, self.E, self.R, grey, **display)
            self.ctx.scan_convert_frames(b["modulus"], 1, self.E, self.R, img, **geometry)
            self.ctx.scan_convert_frames(b["quality"], 1, self.E, self.R, img + 4 * n, **geometry)
            self.ctx.elastogram_frames(img, img + 4 * n, grey, 1, rows, cols, rgb, lut=host_shear_map() if lut is None else lut, rho_min=quality_min,
                                       grey_min=grey_min, alpha=alpha, ref_strain=self.shear_opts["ref_kpa"] if ref_kpa is None else ref_kpa)
            return dict(self._shear_host(b), rgb=self.ctx.d2h(rgb, (rows, cols, 3), np.uint8), grey=self.ctx.d2h(grey, (rows, cols), np.uint8),
                        modulus_img=self.ctx.d2h(img, (rows, cols), np.float32), quality_img=self.ctx.d2h(img + 4 * n, (rows, cols), np.float32))

    # ---- M-mode (motion=)
    def m_mode(self, frame_id=0, line=None, depth_mm=None, hop=None, height=None, waveform=None, bulk=None, **display):
        """the M-mode sweep of one scan-line -> dict(picture uint8 [H][W] (a column is a time, a row a depth), labels uint8 [H][W] and
        truth_disp float32 [H][W] (rows; positive: read from deeper down) registered with it pixel for pixel, env float32 [T][R] (the
        M-line of every pulse), time_s float64 [W] (each column's first pulse) and depth_mm float64 [H]).  It makes ONE trace of the frame,
        one label pass and frame()'s stages before the envelope, detects the analytic lines, then mcrt_mmode_lines_frames and
        mcrt_mmode_picture_frames (motion= only).  line: the scan-line (default: the middle one); depth_mm: (lo, hi), the depths shown
        (default: the whole line); hop: pulses per column (4); height: H (400); waveform: int32 [n_pulses] in Q16 (default:
        host_mmode_waveform at motion='s prf_hz and beats_per_min); bulk: int32 [n_pulses] in Q24 rows (default: host_mmode_bulk of
        motion='s bulk_mm and bulk_per_min); display: dynamic_range_db, gain_db, ref of mmode_display_opts_struct"""
        if self.motion is None:
            raise RuntimeError("M-mode needs Simulator(motion=...)")
        for on, what in ((self.sweep is not None, "sweep="), (self.steers is not None, "compound="), (self.elevation, "elevation="), (self.psf.has_bands, "a psf with bands")):
            if on:
                raise RuntimeError("M-mode is one scan-line of one plane and one pulse shape: it does not combine with %s" % what)
        mo, E, R = self.motion, self.E, self.R
        line = E // 2 if line is None else int(line)
        if not 0 <= line < E:
            raise ValueError("m_mode: scan-line %d is not in 0..%d" % (line, E - 1))
        T, prf, pitch = int(mo["opts"].n_pulses), mo["prf_hz"], row_pitch_mm(self.tr.frequency)
        w = host_mmode_waveform(prf, mo["beats_per_min"], T) if waveform is None else np.ascontiguousarray(waveform, np.int32).reshape(-1)
        b = host_mmode_bulk(prf, mo["bulk_per_min"], mo["bulk_mm"] / pitch, T) if bulk is None else np.ascontiguousarray(bulk, np.int32).reshape(-1)
        if w.size != T or b.size != T:
            raise ValueError("m_mode: waveform and bulk take one entry per pulse (%d), got %d and %d" % (T, w.size, b.size))
        o = mmode_display_opts_struct(hop=hop, height=height, **display)
        if depth_mm is not None:
            o.row_lo = min(max(int(round(float(depth_mm[0]) / pitch)), 0), R - 1)
            o.row_hi = min(max(int(round(float(depth_mm[1]) / pitch)), o.row_lo + 1), R)
        if o.hop == 0 or o.hop > T:
            raise ValueError("m_mode: a hop of %d pulses leaves no column of %d pulses" % (o.hop, T))
        W, H, n, m = T // o.hop, int(o.height), E * R, T * R
        row_lo, row_hi = int(o.row_lo), int(o.row_hi) if o.row_hi else R
        cycles = host_psf_carrier(self.tr.frequency, self.psf.resolution_um)
        with contextlib.ExitStack() as held:
            tissue, iq, env, lab, disp, pic, lab_pic, disp_pic = (held.enter_context(self.ctx.temp(size)) for size in (n, 8 * n, 4 * m, m, 4 * m, H * W, H * W, 4 * H * W))
            self.trace(frame_id)
            self.ctx.label_frames(tissue_dev=tissue, **mo["label"])
            self._stages(self._stack, frame_id, envelope=False)
            self.ctx.detect_frames(self.rf_dev, 1, E, R, iq_dev=iq, **(self.detect or {}))
            self.ctx.mmode_lines_frames(iq, tissue, 1, E, R, [[0, line]], mo["dil"], w, b, cycles, first_image_id=frame_id, env_dev=env, truth_disp_dev=disp,
                                        truth_label_dev=lab, opts=mo["opts"])
            self.ctx.mmode_picture_frames(env, 1, T, R, pic, truth_label_dev=lab, truth_disp_dev=disp, label_out_dev=lab_pic, disp_out_dev=disp_pic, opts=o)
            rows = np.clip(row_lo + (np.arange(H) + 0.5) * (row_hi - row_lo) / H - 0.5, row_lo, row_hi - 1)
            return dict(picture=self.ctx.d2h(pic, (H, W), np.uint8), labels=self.ctx.d2h(lab_pic, (H, W), np.uint8), truth_disp=self.ctx.d2h(disp_pic, (H, W), np.float32),
                        env=self.ctx.d2h(env, (T, R), np.float32), time_s=np.arange(W) * int(o.hop) / prf, depth_mm=rows * pitch,
                        lines=dict(line=line, row_lo=row_lo, row_hi=row_hi, hop=int(o.hop), w_q16=w, bulk_q24=b))

    def colour_flow(self, frame_id=0, **display):
        """the colour-flow picture of a frame -> dict(rgb uint8 [out_rows][out_cols][3], grey uint8 [out_rows][out_cols], velocity float32
        [out_rows][out_cols] (0 where nothing is shown), truth float32 [E][R], corr float32 [3][E][R]).  It traces ONCE; grey is bmode()'s
        own picture of that trace (display: the keywords of Context.bmode_frames), the autocorrelation is gathered through
        mcrt_scan_convert_frames and coloured by mcrt_colour_frames with power_thr = power_scale * 2 * N * sigma^2 (flow= only)"""
        if display.get("persistence", 0.0) != 0.0:
            raise ValueError("colour_flow() shows one frame: persistence is left out")
        rows, cols = display.get("out_rows", 400), display.get("out_cols", 500)
        geometry = {k: display[k] for k in ("radius_mm", "total_angle", "out_rows", "out_cols") if k in display}
        n = rows * cols
        with self._flow_pass(frame_id, ("corr", "truth")) as b, self.ctx.temp(n) as grey, self.ctx.temp(12 * n) as img, self.ctx.temp(3 * n) as rgb, \
                self.ctx.temp(4 * n) as vel:
            self.ctx.bmode_frames(self.rf_dev, 1, self.E, self.R, grey, **display)
            self.ctx.scan_convert_frames(b["corr"], 3, self.E, self.R, img, **geometry)
            fl = self.flow
            power_thr = fl["display"]["power_scale"] * 2.0 * fl["opts"].n_packets * b["sigma"] * b["sigma"]
            self.ctx.colour_frames(img, grey, 1, rows, cols, fl["v_nyq"], rgb, vel_img_dev=vel, power_thr=power_thr, vel_thr_mm_s=fl["display"]["vel_thr_mm_s"],
                                   grey_max=fl["display"]["grey_max"])
            return dict(rgb=self.ctx.d2h(rgb, (rows, cols, 3), np.uint8), grey=self.ctx.d2h(grey, (rows, cols), np.uint8),
                        velocity=self.ctx.d2h(vel, (rows, cols), np.float32), truth=self.ctx.d2h(b["truth"], (self.E, self.R), np.float32),
                        corr=self.ctx.d2h(b["corr"], (3, self.E, self.R), np.float32))
