// mattausch_hip -- the reference's program (main.cpp:42-161) on the MI355X library:
//     mattausch_hip <scene.json> [frames] [samples] [out.pgm] [rf.bin] [--gpus N | --devices 0,1,...]
//                   [--db DR] [--gain G] [--ref-log] [--persistence A] [--focus-mm F1[,F2,...]] [--focal-range-mm R]
//                   [--elevation K] [--elevation-pitch-um P] [--var-z V] [--compound N] [--compound-step-deg D]
//                   [--compound-mode mean|max|median] [--compound-feather LINES] [--compound-weights w0,w1,...]
//                   [--sweep K --sweep-step-deg D [--sweep-pivot-mm P] (--cplane-mm Y | --sagittal-mm X | --render DX,DY,DZ ...)]
//                   [--render DX,DY,DZ --render-box-mm X0,Y0,Z0,X1,Y1,Z1 --render-voxel-mm P [--render-mode mip|mean|surface] [--render-size NX,NY]]
//                   [--labels FILE.pgm [--label-rule traced|geometric] [--label-offset X]] [--render-labels FILE.pgm] [--freehand-labels FILE.raw]
//                   [--transmission FILE.pgm [--transmission-mode total|boundaries] [--transmission-db X]]
//                   [--speckle N [--speckle-q0 X] [--speckle-rho X] [--speckle-lambda X]]
//                   [--speckle3d N [--speckle3d-q0 X] [--speckle3d-rho X] [--speckle3d-lambda X]]
//                   [--noise-db X | --noise-sigma X [--noise-seed N] [--dead-elements a,b,c]]
//                   [--freq-compound N [--freq-span-mhz X]] [--freq-var-x V] [--downshift-mhz-per-mm X [--downshift-min-mhz X]]
//                   [--autogain [--autogain-band N] [--autogain-floor-scale X] [--autogain-max-db X] [--autogain-curve FILE.txt]]
//                   [--freehand N --freehand-step-mm D [--freehand-fan-deg A] --freehand-box-mm X0,Y0,Z0,X1,Y1,Z1 --freehand-voxel-mm P --freehand-out FILE.raw
//                    [--freehand-mode mean|max] [--freehand-fill H]]
// --gpus N: the first N GPUs of the node, the frame's scan-lines sharded over them (mcrt_group_*: one tracing context and host thread per
// GPU, the blocks gathered on GPU 0); --devices lists them explicitly, and may repeat one (two ranks sharing a GPU: the one-GPU test).
// Same constants (main.cpp:23-37), same frame loop body; instead of blocking on imshow/waitKey every frame it
// runs `frames` frames, prints rays/s and frames/s, and writes the last B-mode image as a PGM.
// Without display options the PGM is the linear float scan conversion times 255 (rf_image::save).  With any of them every frame is
// log-compressed to 8-bit grey on the GPU (mcrt_bmode_frames) and the PGM holds those bytes: --db DR decibels of dynamic range below each
// frame's peak (60 when only another option is given), --gain G dB, --ref-log the reference's log10(v+1)/log10(max+1) instead of
// decibels, --persistence A temporal smoothing y = A y_prev + (1-A) s across the frames of the run.
// --focus-mm 40 (or 30,60,90: up to 8, ascending) places focal zones: every RF row gets its own lateral PSF, narrowest at the nearest
// focus and widening with the distance to it over --focal-range-mm R (20 mm, a display choice; mcrt_psf_focus_kernels).  Without
// --focus-mm the reference's one lateral kernel is used and --focal-range-mm has no effect.
// --elevation K (odd, 1..31) gives the picture its slice thickness (psf.h:16-18,42,77): every frame is traced in K parallel planes
// --elevation-pitch-um P apart (145) around the probe's own, as one pass, and folded with the elevation PSF of variance --var-z V (0.1 mm^2,
// main.cpp:54; mcrt_elevation_frames) before the convolution.  Without --elevation the frame is the reference's thin sheet and the other
// two options have no effect; --elevation 1 is that sheet again.
// --compound N (odd, 1..15) compounds every frame from N views steered in the image plane, --compound-step-deg D apart (5) and centred on
// the unsteered one: the views are traced as one pass, convolved and enveloped as N frames and averaged where they cover a pixel
// (mcrt_compound_frames, or mcrt_bmode_compound_frames with a display option).  rf.bin then holds the unsteered view.  Without --compound
// nothing changes and --compound-step-deg has no effect; --compound 1 is the plain run again.  It does not combine with --elevation here
// (the Python Simulator does both).
// --compound-mode max or median takes the largest or the middle look of every pixel in place of their mean; --compound-feather LINES ramps
// every view's weight up over its first and last LINES scan-lines, which hides where a steered view's coverage ends; --compound-weights
// gives each of the N views a weight (mcrt_compound_opts).  Each of the three needs --compound; at their defaults (mean, 0, all 1) the
// picture is the plain compound's byte for byte.
// --sweep K (1..256) makes the probe a volume probe: the array wobbles in elevation about the line parallel to the lateral axis through the
// point --sweep-pivot-mm P (0: the arc's centre) on the arc's axis, and every frame is traced in K planes --sweep-step-deg D apart, centred
// on tilt 0, as one pass; the planes are convolved and enveloped as K frames.  The picture is then a cut through the volume no 2-D probe
// shows (mcrt_volume_frames, or mcrt_bmode_volume_frames with a display option), written as the PGM: --cplane-mm Y, the x-z picture at axial
// position Y mm from the arc's centre (500 columns along x, 400 rows along z, 0.25 mm apart, centred on the arc's axis), or --sagittal-mm X,
// the y-z picture at lateral position X mm (400 columns along z centred on the probe's plane, 500 rows along y from the arc's apex down,
// 0.25 mm apart).  rf.bin then holds plane K / 2.  --sweep needs one of the two cuts and --sweep-step-deg; it does not combine with
// --compound or --elevation, and --persistence has no volume form.
// --render DX,DY,DZ, with --sweep, writes a rendered view in place of a cut: the box --render-box-mm X0,Y0,Z0,X1,Y1,Z1 of the probe-local frame
// (mm: x lateral, y the arc's axis from its centre, z elevation) is gathered into cubic voxels --render-voxel-mm P apart, log-compressed to
// 8-bit grey (mcrt_bmode_volume_frames with the display options, 60 dB without one) and seen along the direction DX,DY,DZ by an orthographic
// camera that looks at the box's centre with the z axis up (the y axis when the direction is along z): pixels and steps P apart, --render-size
// NX,NY pixels (500,400), --render-mode mip (the brightest voxel on each ray), mean, or surface (the default: front-to-back compositing with
// depth cueing; mcrt_render_frames).  It needs --sweep, the box and the voxel size, and takes the place of --cplane-mm / --sagittal-mm;
// --labels does not combine with it.
// --labels FILE.pgm writes the ground truth of the picture as a PGM of material indices (their order in the scene file; 255 outside the
// sector or the sweep): the tissue under every pixel, from the central beam of every scan-line of the unsteered probe walked through the
// scene (mcrt_label_frames) and scan-converted nearest neighbour (mcrt_label_scan_convert_frames) -- with --sweep the cut of --cplane-mm /
// --sagittal-mm through the K planes' labels (mcrt_label_volume_frames).  --label-rule traced (the default) names the medium the tracer's
// rays carry, its quirks included -- the map that explains the picture --, geometric the anatomy of closed, nested meshes; --label-offset X
// restarts the beam X scene units behind every boundary (default: the tracer's 0.1; geometric wants a small one such as 1e-3, which does
// not step over thin walls).  Both need --labels.
// --speckle N runs N iterations (0..256) of speckle-reducing anisotropic diffusion over every enveloped image before the picture is made
// (mcrt_speckle_frames: the despeckle filter of a scanner), on every path above -- the plain picture, the display options, the views of
// --compound, the planes of --sweep, --render; rf.bin holds the filtered image too.  --speckle-q0 X is the speckle scale (0.5227232, fully
// developed speckle), --speckle-rho X its decay per iteration (1/6), --speckle-lambda X the time step in (0, 1] (0.5); the three need
// --speckle.  Without --speckle nothing changes.
// --speckle3d N, with --freehand, runs N iterations (0..256) of the same diffusion with six neighbours over the --freehand-out block on the
// device before it is written (mcrt_speckle_volume_frames), with the weights of the freehand grid's pitches (mcrt_speckle3d_weights: cubic
// voxels, so 1 along every axis that has more than one voxel); a hole's value diffuses like any other.  --speckle3d-q0, --speckle3d-rho and
// --speckle3d-lambda are --speckle's, for this filter; the three need --speckle3d.  Without --speckle3d nothing changes.
// --noise-db X adds receiver noise to every RF image between the convolution and the envelope (mcrt_noise_frames): a Gaussian noise floor
// X dB below the frame's own peak -- the views of --compound and the planes of --sweep share one receiver, hence one peak; the frames of
// --freehand have one each --, drawn from the streams of the frame ids the images were traced with; --noise-sigma X gives the floor's
// standard deviation in RF units instead (0: no noise).  --noise-seed N is the seed of the noise streams; --dead-elements a,b,c silences
// those scan-lines (0..511: a gain of 0, the dark radial streak of a dead element).  The last two need one of the first two, which exclude
// each other.  rf.bin holds the noisy image.  Without these options nothing changes.
// --autogain is the scanner's auto-optimise key (mcrt_autogain_frames): after the envelope (and --speckle) every frame's own amplitude
// histograms, taken in depth bands of --autogain-band N rows (4..256; 16), give a gain curve over depth that flattens the tissue brightness and
// stops amplifying where only noise is left -- the views of --compound and the planes of --sweep share one curve; the frames of --freehand
// have one each.  With --noise-db / --noise-sigma the floor is that frame's noise sigma times --autogain-floor-scale X (3), otherwise there is
// no floor; a band's gain stays within +- --autogain-max-db X (60).  The penetration depth of the last frame is printed, and
// --autogain-curve FILE.txt writes its row gains, one "row depth_mm gain" line per RF row.  The three need --autogain.  rf.bin holds the
// gained image.  Without --autogain nothing changes.
// --freq-compound N (1..8) is receive-side frequency compounding (mcrt_convolve_bands_frames, mcrt_band_fold_frames): the received band is split
// into N sub-bands, evenly spaced over the probe's 4.5 MHz +- --freq-span-mhz X / 2 (2 MHz) with equal weights; every image is convolved with each
// band's pulse, every band image is detected on its own and the detected images are averaged -- speckle falls at the price of axial resolution,
// and no second trace is needed.  It combines with every path above (the views of --compound, the planes of --sweep, --freehand, --noise-db: the
// noise is then added to the band images).  --freq-var-x V is the axial variance of the bands' pulses in mm^2 (0.05, the reference's; a sub-band's
// pulse is longer).  --downshift-mhz-per-mm X lets every band's centre frequency fall with depth, down to --downshift-min-mhz X (0): the pulse
// loses its high frequencies on the way down; alone it is one band at 4.5 MHz.  It has no default that the reference backs: a value is the
// caller's choice.  --freq-compound 1 alone is the plain run byte for byte.
// --freehand N (1..1024) adds a freehand 3-D acquisition after the frames of the run: the probe is moved by hand, here along its elevation axis
// in N steps of --freehand-step-mm D centred on the scene's pose, step k tilted by (k - (N-1)/2) x --freehand-fan-deg A (0) about the line through
// the arc's apex; the N frames are traced as one pass with the last frame's number, convolved, enveloped (and despeckled with --speckle) and
// binned into the cubic voxels --freehand-voxel-mm P of the box --freehand-box-mm X0,Y0,Z0,X1,Y1,Z1 of the WORLD frame (mm: scene units are cm)
// from their poses, holes filled from sampled voxels up to --freehand-fill H voxels away (0..3, default 1), every voxel the mean of its
// samples or with --freehand-mode max the largest (mcrt_recon_frames).  --freehand-out FILE.raw receives the block as little-endian float32,
// [nw][nv][nu] with x fastest; its sizes are printed.  The picture of the positional arguments is written as without the option.
// --freehand-labels FILE.raw, with --freehand, writes that block's ground truth beside it: nu x nv x nw bytes, x fastest, the material most of
// a voxel's samples lie in (the central beams of the N poses, mcrt_label_frames, voted voxel by voxel: mcrt_recon_label_frames), holes filled
// up to --freehand-fill voxels away as the float block's, 255 where nothing is near.  --render-labels FILE.pgm, with --sweep ... --render,
// writes the ground truth of the rendered view: the material of the voxel every pixel shows (mcrt_render_label_frames through the
// rendering's depth buffer and the label block of the box), 255 where the ray saw nothing -- every pixel of --render-mode mean.
// --label-rule and --label-offset are taken with either as with --labels.
// --transmission FILE.pgm writes the acoustic ground truth of the picture: how much of the emitted intensity ARRIVES under every pixel -- the
// shadow behind bone and gas, the enhancement behind fluid --, the tracer's own attenuation and impedance rule carried along the central beam
// of every scan-line (mcrt_transmit_frames) and scan-converted like the float picture (mcrt_scan_convert_frames; 0 outside the sector).  The
// 8-bit grey is made here: min(max(T, 0), 1) * 255 + 0.5, or with --transmission-db X the decibels 10 log10 T over a range of X dB,
// T > 0 ? clamp((10 log10 T + X) / X) * 255 + 0.5 : 0.  --transmission-mode boundaries leaves the attenuation out (the losses at the
// boundaries alone); --label-rule and --label-offset are taken as with --labels.  It does not combine with --sweep.
// --detect quadrature replaces the reference's envelope -- straight lines between the local maxima of the samples, which beat against a carrier
// of fewer than three rows per cycle -- by quadrature detection (mcrt_detect_frames): an FIR Hilbert transformer of --detect-taps N taps (3, 7,
// 11, ..., 63; 31) along every scan-line, the envelope the magnitude of the analytic signal.  It runs wherever the envelope ran: the plain
// picture, the views of --compound, the planes of --sweep, the band images of --freq-compound, --freehand; rf.bin holds the detected image.
// The detector is flat within 1 % between 0.05 and 0.45 cycles per row at 31 taps: a band near Nyquist (3.5 MHz: 0.4925) comes out darker.
// --iq FILE.raw writes the last frame's analytic pair before detection, float32 [512][465][2] scan-line-major: the RF's own bits and its Hilbert
// transform (the I/Q data at the RF rate), with --detect-taps' taps whether or not --detect is given.  It does not combine with --compound,
// --sweep or the band options.  --detect-taps needs --detect or --iq.  Without these options nothing changes.
// --colour-flow FILE.ppm writes the last frame's colour-flow picture, a binary PPM of the B-mode size: the frame's ONE trace is split by tissue
// label into what stands still and what moves, a slow-time ensemble of --flow-packets N pulses (2..16; 8) at --flow-prf-hz X (4000) is
// synthesised from the two parts, filtered (--flow-wall none|mean|linear; mean), and the Kasai autocorrelator's velocity is laid over the 8-bit
// B-mode frame (the display options apply; the picture is log-compressed whether or not one is given), red towards the probe.
// --flow-velocity NAME:vx,vy,vz [mm/s] gives a material its velocity vector and may be repeated; at least one is needed.  --flow-avg A,B is the
// averaging half-window in rows and scan-lines (2,1); --flow-vel-thr X [mm/s] and --flow-grey-max G are the display thresholds (0, 255); with
// --noise the ensemble carries the receiver's sigma and power below 4 * 2 N sigma^2 is not shown.  --flow-truth FILE.raw writes the true axial
// velocity of every scan-line sample, float32 [512][465].  It does not combine with --compound, --sweep, --elevation or the band options.
// --spectral FILE.pgm writes the last frame's sonogram (pulsed-wave spectral Doppler), a binary PGM of N rows (velocities, row 0 the highest towards
// the probe) by (T - N) / H + 1 columns (times): --gate LINE,DEPTH_MM,LEN_MM is the sample gate -- a scan-line, the depth of its centre and its
// length --, whose slow-time series of --spectral-pulses T pulses (1..16384; 2048) is synthesised from that frame's ONE trace (colour flow's chain
// up to the detected pairs) under a parabolic velocity profile across the lumen and the pulsatile centre-line speed --flow-waveform BPM,PEAK,MIN
// [1/min, mm/s, mm/s] (72, the speed of --flow-velocity, 0) along the FIRST --flow-velocity's direction; a Hann-windowed FFT of --spectral-fft N
// pulses (32, 64, 128, 256, 512; 128) every --spectral-hop H pulses (32) is shown over --spectral-db X dB (40).  --spectral-iq FILE.raw writes the
// series itself, float32 [T][2].  --flow-prf-hz applies; it does not combine with --compound, --sweep, --elevation or the band options.
// --elastogram FILE.ppm writes the last frame's elastogram (quasi-static strain imaging), a binary PPM of the B-mode size: every scan-line of the
// frame's ONE trace is compressed as a column of springs -- --stiffness NAME:E[,NAME:E...] gives materials their Young's modulus (any unit; the
// others have 1; 0 is rigid), --compress X (0.01) is the strain of modulus 1 --, the speckle is tracked between the two analytic frames over
// --strain-window N rows (0..32; 16) and lags up to --strain-search N (0..16; 8), and the least-squares strain over --strain-lsq N rows (1..32; 12)
// is laid over the 8-bit B-mode frame: stiff blue, the applied strain green, soft red.  --strain-truth FILE.raw writes the true strain of every
// scan-line sample, float32 [512][465].  It does not combine with --compound, --sweep, --elevation or the band options.
// --shear-elastogram FILE.ppm writes the last frame's shear-wave elastogram, a binary PPM of the B-mode size: a push on scan-line LINE over
// LEN_MM about DEPTH_MM (--push LINE,DEPTH_MM,LEN_MM) launches a shear wave along every RF row of the frame's ONE trace, --shear-speed
// NAME:c[,NAME:c...] gives materials their shear speed [m/s] (the others have 2; 0 is a fluid, the wave does not pass), the wave is tracked over
// --shear-pulses N pulses (4..256; 64) at --shear-prf HZ (10000), and the modulus 3 rho c^2 of the time-to-peak speed is laid over the 8-bit
// B-mode frame: soft blue, 12 kPa (2 m/s) green, stiff red.  --shear-truth FILE.raw writes the true shear speed of every scan-line sample,
// float32 [512][465].  It does not combine with --compound, --sweep, --elevation or the band options.
// --m-mode FILE.pgm writes the M-mode sweep of scan-line --m-line LINE of the last frame, a binary PGM of --m-height H (400) rows and
// T / N columns: --motion NAME:e[,NAME:e...] gives materials their dilation (the peak axial strain over the cycle, positive: compression, at
// most 0.25; the others have 0), the frame's ONE trace is moved over --m-pulses T pulses (1..16384; 1024) at --m-prf HZ (1000) under the default
// waveform of --m-bpm X beats per minute (72) and a rigid sinusoidal shift of --m-bulk-mm A,PER_MIN (0,15), --m-hop N (4) pulses make a
// column, and --m-depth-mm LO,HI shows those depths (the whole line).  --m-labels FILE.pgm writes the material and --m-truth FILE.raw the true
// displacement [rows] of every pixel, float32 [H][T / N].  It does not combine with --compound, --sweep, --elevation or the band options.
#include "mcrt_host.hpp"
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <iostream>
#include <type_traits>

using namespace mcrt_host;

constexpr float transducer_frequency = 4.5f;                  // [MHz]
constexpr size_t transducer_elements = 512;
constexpr double transducer_amplitude = 60.0 * 3.14159265358979323846264338327950288419716939937510 / 180.0;   // 60_deg -> rad
constexpr double transducer_radius_cm = 3.0;
constexpr unsigned int resolution = 145;                      // [um]
using psf_ = psf<7, 13, 7, resolution>;
using rf_image_ = rf_image<transducer_elements, 100, 322>;    // max_travel_time 100 us, axial resolution 322 um (main.cpp:31,36)
using transducer_ = transducer<transducer_elements>;

template <typename T> static std::vector<T> comma_list(const char *q)   // "a,b,...": atoi (an integer T) or atof of every item
{
    std::vector<T> v;
    while (*q) { v.push_back(std::is_integral<T>::value ? (T)std::atoi(q) : (T)std::atof(q)); while (*q && *q != ',') q++; if (*q == ',') q++; }
    return v;
}

int main(int argc, char **argv)
{
    std::vector<int> devices{ 0 };
    mcrt_bmode_params display; mcrt_default_bmode(&display);
    display.reset_state = 0;                          // the persistence state runs on from frame to frame
    bool bmode = false;
    std::vector<float> focus_mm; float focal_range_mm = 20.0f;
    int elevation = 0; long elevation_pitch_um = 145; float var_z = 0.1f;      // elevation 0: off
    bool elevation_given = false;
    int compound = 0; double compound_step_deg = 5.0;                         // compound 0: off
    bool compound_given = false;
    mcrt_compound_opts copts; mcrt_default_compound_opts(&copts);
    const char *compound_mode = nullptr, *compound_feather = nullptr, *compound_weights = nullptr;   // the options as given
    int sweep_planes = 0; double sweep_step_deg = 0.0, sweep_pivot_mm = 0.0, cut_mm = 0.0;   // sweep_planes 0: off
    bool sweep_given = false, sweep_step_given = false, cplane_given = false, sagittal_given = false;
    const char *render_dir = nullptr, *render_box = nullptr, *render_voxel = nullptr, *render_mode = nullptr, *render_size = nullptr;   // the options as given
    const char *labels_file = nullptr, *label_rule = nullptr, *label_offset = nullptr, *render_labels = nullptr, *freehand_labels = nullptr;
    mcrt_label_opts lopts; mcrt_default_label_opts(&lopts);
    const char *transmission_file = nullptr, *transmission_mode = nullptr, *transmission_db = nullptr;   // the options as given
    mcrt_transmit_opts topts; mcrt_default_transmit_opts(&topts);
    float transmission_range_db = 0.0f;               // 0: the linear grey
    const char *speckle_n = nullptr, *speckle_q0 = nullptr, *speckle_rho = nullptr, *speckle_lambda = nullptr;   // the options as given
    mcrt_speckle_opts sopts; mcrt_default_speckle_opts(&sopts);
    const char *speckle3d_n = nullptr, *speckle3d_q0 = nullptr, *speckle3d_rho = nullptr, *speckle3d_lambda = nullptr;   // the options as given
    mcrt_speckle3d_opts s3opts; mcrt_default_speckle3d_opts(&s3opts);
    const char *noise_db = nullptr, *noise_sigma = nullptr, *noise_seed = nullptr, *dead_elements = nullptr;   // the options as given
    mcrt_noise_opts nopts; mcrt_default_noise_opts(&nopts);
    std::vector<float> element_gain;                  // empty: no gain table
    bool autogain = false;
    const char *autogain_band = nullptr, *autogain_scale = nullptr, *autogain_max_db = nullptr, *autogain_curve = nullptr;   // the options as given
    mcrt_autogain_opts aopts; mcrt_default_autogain_opts(&aopts);
    const char *freq_compound = nullptr, *freq_span = nullptr, *freq_var_x = nullptr, *downshift = nullptr, *downshift_min = nullptr;   // the options as given
    const char *detect = nullptr, *detect_taps = nullptr, *iq_file = nullptr;   // the options as given
    const char *colour_flow = nullptr, *flow_packets = nullptr, *flow_prf = nullptr, *flow_wall = nullptr, *flow_avg = nullptr, *flow_vel_thr = nullptr,
               *flow_grey_max = nullptr, *flow_truth = nullptr;   // the options as given
    std::vector<std::string> flow_velocity;
    const char *elastogram = nullptr, *stiffness = nullptr, *compress = nullptr, *strain_window = nullptr, *strain_search = nullptr, *strain_lsq = nullptr,
               *strain_truth = nullptr;   // the options as given
    const char *shear_elastogram = nullptr, *shear_speed = nullptr, *shear_push = nullptr, *shear_pulses = nullptr, *shear_prf = nullptr, *shear_truth = nullptr;
    mcrt_shear_opts shopts; mcrt_default_shear_opts(&shopts);
    const char *m_mode = nullptr, *m_line = nullptr, *motion = nullptr, *m_prf = nullptr, *m_bpm = nullptr, *m_pulses = nullptr, *m_hop = nullptr, *m_height = nullptr,
               *m_depth = nullptr, *m_bulk = nullptr, *m_labels = nullptr, *m_truth = nullptr;
    mcrt_mmode_opts mmopts; mcrt_default_mmode_opts(&mmopts);
    mcrt_mmode_display_opts mdopts; mcrt_default_mmode_display_opts(&mdopts);
    double m_prf_hz = 1000.0, m_beats = 72.0, m_bulk_mm = 0.0, m_bulk_per_min = 15.0, m_depth_lo = 0.0, m_depth_hi = 0.0;
    uint32_t m_scan_line = 0;
    mcrt_elastogram_opts shelopts; mcrt_default_elastogram_opts(&shelopts);
    double push_depth_mm = 0.0, push_len_mm = 0.0;
    double applied = 0.01;
    mcrt_strain_opts stopts; mcrt_default_strain_opts(&stopts);
    mcrt_elastogram_opts elopts; mcrt_default_elastogram_opts(&elopts);
    const char *spectral = nullptr, *spectral_gate = nullptr, *spectral_pulses = nullptr, *spectral_fft = nullptr, *spectral_hop = nullptr, *spectral_db = nullptr,
               *flow_waveform = nullptr, *spectral_iq = nullptr;   // the options as given
    mcrt_spectral_opts spopts; mcrt_default_spectral_opts(&spopts);
    mcrt_sonogram_opts sgopts; mcrt_default_sonogram_opts(&sgopts);
    double gate_depth_mm = 0.0, gate_len_mm = 0.0, wave_bpm = 72.0, wave_peak = -1.0, wave_min = 0.0;   // wave_peak < 0: the speed of --flow-velocity
    uint32_t gate_line = 0;
    mcrt_flow_opts flopts; mcrt_default_flow_opts(&flopts);
    mcrt_colour_opts flcol; mcrt_default_colour_opts(&flcol);
    mcrt_detect_opts dopts; mcrt_default_detect_opts(&dopts);
    const char *freehand_n = nullptr, *freehand_step = nullptr, *freehand_fan = nullptr, *freehand_box = nullptr, *freehand_voxel = nullptr, *freehand_out = nullptr,
               *freehand_mode = nullptr, *freehand_fill = nullptr;   // the options as given
    mcrt_recon_opts fopts; mcrt_default_recon_opts(&fopts);
    {   // the options, taken out of the positional arguments
        int keep = 1;
        for (int i = 1; i < argc; i++) {
            if (!std::strcmp(argv[i], "--db") && i + 1 < argc) { display.dynamic_range_db = (float)std::atof(argv[++i]); bmode = true; }
            else if (!std::strcmp(argv[i], "--gain") && i + 1 < argc) { display.gain_db = (float)std::atof(argv[++i]); bmode = true; }
            else if (!std::strcmp(argv[i], "--ref-log")) { display.mode = MCRT_BMODE_REF_LOG; bmode = true; }
            else if (!std::strcmp(argv[i], "--persistence") && i + 1 < argc) { display.persistence = (float)std::atof(argv[++i]); bmode = true; }
            else if (!std::strcmp(argv[i], "--focus-mm") && i + 1 < argc) focus_mm = comma_list<float>(argv[++i]);
            else if (!std::strcmp(argv[i], "--focal-range-mm") && i + 1 < argc) focal_range_mm = (float)std::atof(argv[++i]);
            else if (!std::strcmp(argv[i], "--elevation") && i + 1 < argc) { elevation = std::atoi(argv[++i]); elevation_given = true; }
            else if (!std::strcmp(argv[i], "--elevation-pitch-um") && i + 1 < argc) elevation_pitch_um = std::atol(argv[++i]);
            else if (!std::strcmp(argv[i], "--var-z") && i + 1 < argc) var_z = (float)std::atof(argv[++i]);
            else if (!std::strcmp(argv[i], "--compound") && i + 1 < argc) { compound = std::atoi(argv[++i]); compound_given = true; }
            else if (!std::strcmp(argv[i], "--compound-step-deg") && i + 1 < argc) compound_step_deg = std::atof(argv[++i]);
            else if (!std::strcmp(argv[i], "--compound-mode") && i + 1 < argc) compound_mode = argv[++i];
            else if (!std::strcmp(argv[i], "--compound-feather") && i + 1 < argc) compound_feather = argv[++i];
            else if (!std::strcmp(argv[i], "--compound-weights") && i + 1 < argc) compound_weights = argv[++i];
            else if (!std::strcmp(argv[i], "--sweep") && i + 1 < argc) { sweep_planes = std::atoi(argv[++i]); sweep_given = true; }
            else if (!std::strcmp(argv[i], "--sweep-step-deg") && i + 1 < argc) { sweep_step_deg = std::atof(argv[++i]); sweep_step_given = true; }
            else if (!std::strcmp(argv[i], "--sweep-pivot-mm") && i + 1 < argc) sweep_pivot_mm = std::atof(argv[++i]);
            else if (!std::strcmp(argv[i], "--cplane-mm") && i + 1 < argc) { cut_mm = std::atof(argv[++i]); cplane_given = true; }
            else if (!std::strcmp(argv[i], "--sagittal-mm") && i + 1 < argc) { cut_mm = std::atof(argv[++i]); sagittal_given = true; }
            else if (!std::strcmp(argv[i], "--render") && i + 1 < argc) render_dir = argv[++i];
            else if (!std::strcmp(argv[i], "--render-box-mm") && i + 1 < argc) render_box = argv[++i];
            else if (!std::strcmp(argv[i], "--render-voxel-mm") && i + 1 < argc) render_voxel = argv[++i];
            else if (!std::strcmp(argv[i], "--render-mode") && i + 1 < argc) render_mode = argv[++i];
            else if (!std::strcmp(argv[i], "--render-size") && i + 1 < argc) render_size = argv[++i];
            else if (!std::strcmp(argv[i], "--labels") && i + 1 < argc) labels_file = argv[++i];
            else if (!std::strcmp(argv[i], "--render-labels") && i + 1 < argc) render_labels = argv[++i];
            else if (!std::strcmp(argv[i], "--freehand-labels") && i + 1 < argc) freehand_labels = argv[++i];
            else if (!std::strcmp(argv[i], "--transmission") && i + 1 < argc) transmission_file = argv[++i];
            else if (!std::strcmp(argv[i], "--transmission-mode") && i + 1 < argc) transmission_mode = argv[++i];
            else if (!std::strcmp(argv[i], "--transmission-db") && i + 1 < argc) transmission_db = argv[++i];
            else if (!std::strcmp(argv[i], "--label-rule") && i + 1 < argc) label_rule = argv[++i];
            else if (!std::strcmp(argv[i], "--label-offset") && i + 1 < argc) label_offset = argv[++i];
            else if (!std::strcmp(argv[i], "--speckle") && i + 1 < argc) speckle_n = argv[++i];
            else if (!std::strcmp(argv[i], "--speckle-q0") && i + 1 < argc) speckle_q0 = argv[++i];
            else if (!std::strcmp(argv[i], "--speckle-rho") && i + 1 < argc) speckle_rho = argv[++i];
            else if (!std::strcmp(argv[i], "--speckle-lambda") && i + 1 < argc) speckle_lambda = argv[++i];
            else if (!std::strcmp(argv[i], "--speckle3d") && i + 1 < argc) speckle3d_n = argv[++i];
            else if (!std::strcmp(argv[i], "--speckle3d-q0") && i + 1 < argc) speckle3d_q0 = argv[++i];
            else if (!std::strcmp(argv[i], "--speckle3d-rho") && i + 1 < argc) speckle3d_rho = argv[++i];
            else if (!std::strcmp(argv[i], "--speckle3d-lambda") && i + 1 < argc) speckle3d_lambda = argv[++i];
            else if (!std::strcmp(argv[i], "--noise-db") && i + 1 < argc) noise_db = argv[++i];
            else if (!std::strcmp(argv[i], "--noise-sigma") && i + 1 < argc) noise_sigma = argv[++i];
            else if (!std::strcmp(argv[i], "--noise-seed") && i + 1 < argc) noise_seed = argv[++i];
            else if (!std::strcmp(argv[i], "--dead-elements") && i + 1 < argc) dead_elements = argv[++i];
            else if (!std::strcmp(argv[i], "--autogain")) autogain = true;
            else if (!std::strcmp(argv[i], "--autogain-band") && i + 1 < argc) autogain_band = argv[++i];
            else if (!std::strcmp(argv[i], "--autogain-floor-scale") && i + 1 < argc) autogain_scale = argv[++i];
            else if (!std::strcmp(argv[i], "--autogain-max-db") && i + 1 < argc) autogain_max_db = argv[++i];
            else if (!std::strcmp(argv[i], "--autogain-curve") && i + 1 < argc) autogain_curve = argv[++i];
            else if (!std::strcmp(argv[i], "--freq-compound") && i + 1 < argc) freq_compound = argv[++i];
            else if (!std::strcmp(argv[i], "--freq-span-mhz") && i + 1 < argc) freq_span = argv[++i];
            else if (!std::strcmp(argv[i], "--freq-var-x") && i + 1 < argc) freq_var_x = argv[++i];
            else if (!std::strcmp(argv[i], "--downshift-mhz-per-mm") && i + 1 < argc) downshift = argv[++i];
            else if (!std::strcmp(argv[i], "--downshift-min-mhz") && i + 1 < argc) downshift_min = argv[++i];
            else if (!std::strcmp(argv[i], "--detect") && i + 1 < argc) detect = argv[++i];
            else if (!std::strcmp(argv[i], "--detect-taps") && i + 1 < argc) detect_taps = argv[++i];
            else if (!std::strcmp(argv[i], "--iq") && i + 1 < argc) iq_file = argv[++i];
            else if (!std::strcmp(argv[i], "--colour-flow") && i + 1 < argc) colour_flow = argv[++i];
            else if (!std::strcmp(argv[i], "--flow-velocity") && i + 1 < argc) flow_velocity.push_back(argv[++i]);
            else if (!std::strcmp(argv[i], "--flow-packets") && i + 1 < argc) flow_packets = argv[++i];
            else if (!std::strcmp(argv[i], "--flow-prf-hz") && i + 1 < argc) flow_prf = argv[++i];
            else if (!std::strcmp(argv[i], "--flow-wall") && i + 1 < argc) flow_wall = argv[++i];
            else if (!std::strcmp(argv[i], "--flow-avg") && i + 1 < argc) flow_avg = argv[++i];
            else if (!std::strcmp(argv[i], "--flow-vel-thr") && i + 1 < argc) flow_vel_thr = argv[++i];
            else if (!std::strcmp(argv[i], "--flow-grey-max") && i + 1 < argc) flow_grey_max = argv[++i];
            else if (!std::strcmp(argv[i], "--flow-truth") && i + 1 < argc) flow_truth = argv[++i];
            else if (!std::strcmp(argv[i], "--elastogram") && i + 1 < argc) elastogram = argv[++i];
            else if (!std::strcmp(argv[i], "--stiffness") && i + 1 < argc) stiffness = argv[++i];
            else if (!std::strcmp(argv[i], "--compress") && i + 1 < argc) compress = argv[++i];
            else if (!std::strcmp(argv[i], "--strain-window") && i + 1 < argc) strain_window = argv[++i];
            else if (!std::strcmp(argv[i], "--strain-search") && i + 1 < argc) strain_search = argv[++i];
            else if (!std::strcmp(argv[i], "--strain-lsq") && i + 1 < argc) strain_lsq = argv[++i];
            else if (!std::strcmp(argv[i], "--strain-truth") && i + 1 < argc) strain_truth = argv[++i];
            else if (!std::strcmp(argv[i], "--shear-elastogram") && i + 1 < argc) shear_elastogram = argv[++i];
            else if (!std::strcmp(argv[i], "--shear-speed") && i + 1 < argc) shear_speed = argv[++i];
            else if (!std::strcmp(argv[i], "--push") && i + 1 < argc) shear_push = argv[++i];
            else if (!std::strcmp(argv[i], "--shear-pulses") && i + 1 < argc) shear_pulses = argv[++i];
            else if (!std::strcmp(argv[i], "--shear-prf") && i + 1 < argc) shear_prf = argv[++i];
            else if (!std::strcmp(argv[i], "--shear-truth") && i + 1 < argc) shear_truth = argv[++i];
            else if (!std::strcmp(argv[i], "--m-mode") && i + 1 < argc) m_mode = argv[++i];
            else if (!std::strcmp(argv[i], "--m-line") && i + 1 < argc) m_line = argv[++i];
            else if (!std::strcmp(argv[i], "--motion") && i + 1 < argc) motion = argv[++i];
            else if (!std::strcmp(argv[i], "--m-prf") && i + 1 < argc) m_prf = argv[++i];
            else if (!std::strcmp(argv[i], "--m-bpm") && i + 1 < argc) m_bpm = argv[++i];
            else if (!std::strcmp(argv[i], "--m-pulses") && i + 1 < argc) m_pulses = argv[++i];
            else if (!std::strcmp(argv[i], "--m-hop") && i + 1 < argc) m_hop = argv[++i];
            else if (!std::strcmp(argv[i], "--m-height") && i + 1 < argc) m_height = argv[++i];
            else if (!std::strcmp(argv[i], "--m-depth-mm") && i + 1 < argc) m_depth = argv[++i];
            else if (!std::strcmp(argv[i], "--m-bulk-mm") && i + 1 < argc) m_bulk = argv[++i];
            else if (!std::strcmp(argv[i], "--m-labels") && i + 1 < argc) m_labels = argv[++i];
            else if (!std::strcmp(argv[i], "--m-truth") && i + 1 < argc) m_truth = argv[++i];
            else if (!std::strcmp(argv[i], "--spectral") && i + 1 < argc) spectral = argv[++i];
            else if (!std::strcmp(argv[i], "--gate") && i + 1 < argc) spectral_gate = argv[++i];
            else if (!std::strcmp(argv[i], "--spectral-pulses") && i + 1 < argc) spectral_pulses = argv[++i];
            else if (!std::strcmp(argv[i], "--spectral-fft") && i + 1 < argc) spectral_fft = argv[++i];
            else if (!std::strcmp(argv[i], "--spectral-hop") && i + 1 < argc) spectral_hop = argv[++i];
            else if (!std::strcmp(argv[i], "--spectral-db") && i + 1 < argc) spectral_db = argv[++i];
            else if (!std::strcmp(argv[i], "--flow-waveform") && i + 1 < argc) flow_waveform = argv[++i];
            else if (!std::strcmp(argv[i], "--spectral-iq") && i + 1 < argc) spectral_iq = argv[++i];
            else if (!std::strcmp(argv[i], "--freehand") && i + 1 < argc) freehand_n = argv[++i];
            else if (!std::strcmp(argv[i], "--freehand-step-mm") && i + 1 < argc) freehand_step = argv[++i];
            else if (!std::strcmp(argv[i], "--freehand-fan-deg") && i + 1 < argc) freehand_fan = argv[++i];
            else if (!std::strcmp(argv[i], "--freehand-box-mm") && i + 1 < argc) freehand_box = argv[++i];
            else if (!std::strcmp(argv[i], "--freehand-voxel-mm") && i + 1 < argc) freehand_voxel = argv[++i];
            else if (!std::strcmp(argv[i], "--freehand-out") && i + 1 < argc) freehand_out = argv[++i];
            else if (!std::strcmp(argv[i], "--freehand-mode") && i + 1 < argc) freehand_mode = argv[++i];
            else if (!std::strcmp(argv[i], "--freehand-fill") && i + 1 < argc) freehand_fill = argv[++i];
            else if (!std::strcmp(argv[i], "--gpus") && i + 1 < argc) { devices.clear(); for (int d = 0; d < std::max(1, std::atoi(argv[i + 1])); d++) devices.push_back(d); i++; }
            else if (!std::strcmp(argv[i], "--devices") && i + 1 < argc) {
                devices = comma_list<int>(argv[++i]);
                if (devices.empty()) devices.push_back(0);
            }
            else argv[keep++] = argv[i];
        }
        argc = keep;
    }
    if (argc < 2) { std::cout << "Incorrect argument list." << std::endl; return 0; }
    const int frames = argc > 2 ? std::atoi(argv[2]) : 10;
    const unsigned samples = argc > 3 ? (unsigned)std::atoi(argv[3]) : 5;   // samples_te (main.cpp:27)
    try {
        if (elevation_given && (elevation < 1 || elevation > 31 || elevation % 2 == 0))
            throw std::invalid_argument("--elevation takes an odd number of planes, 1..31");
        if (elevation_given && (elevation_pitch_um < 1 || elevation_pitch_um > 0xffffffffl))
            throw std::invalid_argument("--elevation-pitch-um must be a positive number of micrometres");
        if (compound_given && (compound < 1 || compound > 15 || compound % 2 == 0))
            throw std::invalid_argument("--compound takes an odd number of views, 1..15");
        if (compound_given && elevation_given) throw std::invalid_argument("--compound and --elevation do not combine in this program");
        if (!compound_given && (compound_mode || compound_feather || compound_weights))
            throw std::invalid_argument(std::string(compound_mode ? "--compound-mode" : compound_feather ? "--compound-feather" : "--compound-weights") + " needs --compound");
        if (compound_mode) {
            if (!std::strcmp(compound_mode, "mean")) copts.mode = MCRT_COMPOUND_MEAN;
            else if (!std::strcmp(compound_mode, "max")) copts.mode = MCRT_COMPOUND_MAX;
            else if (!std::strcmp(compound_mode, "median")) copts.mode = MCRT_COMPOUND_MEDIAN;
            else throw std::invalid_argument("--compound-mode takes mean, max or median");
        }
        if (compound_feather) {
            copts.feather_lines = (float)std::atof(compound_feather);
            if (!(std::isfinite(copts.feather_lines) && copts.feather_lines >= 0.0f)) throw std::invalid_argument("--compound-feather takes a number of scan-lines >= 0");
        }
        if (compound_weights) {
            const std::vector<float> w = comma_list<float>(compound_weights);
            if ((int)w.size() != compound) throw std::invalid_argument("--compound-weights takes one weight per view of --compound (" + std::to_string(compound) + ")");
            for (size_t n = 0; n < w.size(); n++) copts.view_weight[n] = w[n];
        }
        if (sweep_given && (compound_given || elevation_given)) throw std::invalid_argument("--sweep does not combine with --compound or --elevation");
        if (!sweep_given && (sweep_step_given || cplane_given || sagittal_given)) throw std::invalid_argument("--sweep-step-deg, --cplane-mm and --sagittal-mm need --sweep");
        if (!sweep_given && (render_dir || render_box || render_voxel || render_mode || render_size)) throw std::invalid_argument("--render and its options need --sweep");
        if (render_labels && !render_dir) throw std::invalid_argument("--render-labels needs --render (with --sweep)");
        if (freehand_labels && !freehand_n) throw std::invalid_argument("--freehand-labels needs --freehand");
        if (!render_dir && (render_box || render_voxel || render_mode || render_size)) throw std::invalid_argument("--render-box-mm, --render-voxel-mm, --render-mode and --render-size need --render (with --sweep)");
        mcrt_sweep sweep{ 0, 0.0f, 0.0f };
        mcrt_volume_grid cut{};
        mcrt_render_view view{};
        mcrt_render_opts ropts; mcrt_default_render_opts(&ropts, 1);
        if (sweep_given) {
            if (sweep_planes < 1 || sweep_planes > 256) throw std::invalid_argument("--sweep takes 1..256 planes");
            if (!sweep_step_given) throw std::invalid_argument("--sweep needs --sweep-step-deg");
            if ((int)cplane_given + (int)sagittal_given + (render_dir ? 1 : 0) != 1) throw std::invalid_argument("--sweep needs one of --cplane-mm, --sagittal-mm and --render");
            sweep.n_planes = (uint32_t)sweep_planes; sweep.step_rad = (float)(sweep_step_deg * 3.14159265358979323846 / 180.0); sweep.pivot_mm = (float)sweep_pivot_mm;
            if (!(std::isfinite(sweep.step_rad) && sweep.step_rad > 0.0f && (double)(sweep_planes - 1) / 2.0 * (double)sweep.step_rad < 1.5707963267948966))
                throw std::invalid_argument("--sweep-step-deg must be > 0 and keep every plane's tilt below 90 degrees");
            if (!std::isfinite(sweep.pivot_mm) || !std::isfinite(cut_mm)) throw std::invalid_argument("--sweep-pivot-mm and the cut's position must be finite");
            if (display.persistence != 0.0f) throw std::invalid_argument("--persistence has no volume form: it does not combine with --sweep");
            const double pitch = 0.25;
            if (render_dir) {
                if (!render_box || !render_voxel) throw std::invalid_argument("--render (with --sweep) needs --render-box-mm and --render-voxel-mm");
                if (labels_file) throw std::invalid_argument("--labels does not combine with --render (with --sweep): a rendered view has no label picture");
                const std::vector<double> dir = comma_list<double>(render_dir), box = comma_list<double>(render_box);
                const std::vector<int> size = render_size ? comma_list<int>(render_size) : std::vector<int>{ 500, 400 };
                const double voxel = std::atof(render_voxel);
                if (dir.size() != 3 || box.size() != 6 || size.size() != 2) throw std::invalid_argument("--render (with --sweep) takes DX,DY,DZ, --render-box-mm six numbers, --render-size NX,NY");
                if (!(std::isfinite(voxel) && voxel > 0.0)) throw std::invalid_argument("--render-voxel-mm (with --sweep --render) must be > 0");
                if (size[0] < 1 || size[1] < 1) throw std::invalid_argument("--render-size (with --sweep --render) takes two positive numbers");
                uint32_t n[3];
                for (int k = 0; k < 3; k++) {
                    const double cells = std::floor((box[3 + k] - box[k]) / voxel);
                    if (!(cells >= 0.0 && cells < 16777215.0)) throw std::invalid_argument("--render-box-mm (with --sweep --render): X1 >= X0, Y1 >= Y0, Z1 >= Z0, and fewer than 2^24 voxels along an axis");
                    n[k] = (uint32_t)cells + 1u; cut.origin_mm[k] = box[k];
                }
                cut.du_mm[0] = cut.dv_mm[1] = cut.dw_mm[2] = voxel; cut.nu = n[0]; cut.nv = n[1]; cut.nw = n[2];
                if (render_mode) {
                    if (!std::strcmp(render_mode, "mip")) ropts.mode = MCRT_RENDER_MIP;
                    else if (!std::strcmp(render_mode, "mean")) ropts.mode = MCRT_RENDER_MEAN;
                    else if (!std::strcmp(render_mode, "surface")) ropts.mode = MCRT_RENDER_SURFACE;
                    else throw std::invalid_argument("--render-mode (with --sweep --render) takes mip, mean or surface");
                }
                const double along_z[3] = { 0.0, 0.0, 1.0 }, along_y[3] = { 0.0, 1.0, 0.0 };
                const bool dir_is_z = dir[0] == 0.0 && dir[1] == 0.0;
                if (mcrt_render_view_for_grid(&cut, dir.data(), dir_is_z ? along_y : along_z, voxel, voxel, (uint32_t)size[0], (uint32_t)size[1], &view) != MCRT_OK)
                    throw std::invalid_argument(std::string("--render (with --sweep): ") + mcrt_last_error());
            }
            else if (cplane_given) { cut.origin_mm[0] = -(500 - 1) * pitch / 2.0; cut.origin_mm[1] = cut_mm; cut.origin_mm[2] = -(400 - 1) * pitch / 2.0; cut.du_mm[0] = pitch; cut.dv_mm[2] = pitch; cut.nu = 500; cut.nv = 400; }
            else { cut.origin_mm[0] = cut_mm; cut.origin_mm[1] = transducer_radius_cm * 10.0; cut.origin_mm[2] = -(400 - 1) * pitch / 2.0; cut.du_mm[2] = pitch; cut.dv_mm[1] = pitch; cut.nu = 400; cut.nv = 500; }
            if (!render_dir) cut.nw = 1;
        }
        if (!transmission_file && (transmission_mode || transmission_db)) throw std::invalid_argument(std::string(transmission_mode ? "--transmission-mode" : "--transmission-db") + " needs --transmission");
        if (transmission_file && sweep_given) throw std::invalid_argument("--transmission does not combine with --sweep: it is the sector's picture");
        if (transmission_mode) {
            if (!std::strcmp(transmission_mode, "total")) topts.mode = MCRT_TRANSMIT_TOTAL;
            else if (!std::strcmp(transmission_mode, "boundaries")) topts.mode = MCRT_TRANSMIT_BOUNDARIES;
            else throw std::invalid_argument("--transmission-mode takes total or boundaries");
        }
        if (transmission_db) {
            transmission_range_db = (float)std::atof(transmission_db);
            if (!(std::isfinite(transmission_range_db) && transmission_range_db > 0.0f)) throw std::invalid_argument("--transmission-db takes a finite range > 0");
        }
        if (!labels_file && !render_labels && !freehand_labels && !transmission_file && (label_rule || label_offset)) throw std::invalid_argument(std::string(label_rule ? "--label-rule" : "--label-offset") + " needs --labels");
        if (label_rule) {
            if (!std::strcmp(label_rule, "traced")) lopts.rule = MCRT_LABEL_TRACED;
            else if (!std::strcmp(label_rule, "geometric")) lopts.rule = MCRT_LABEL_GEOMETRIC;
            else throw std::invalid_argument("--label-rule takes traced or geometric");
        }
        if (label_offset) {
            lopts.start_offset = (float)std::atof(label_offset);
            if (!(std::isfinite(lopts.start_offset) && lopts.start_offset > 0.0f)) throw std::invalid_argument("--label-offset takes a finite offset > 0");
        }
        if (!speckle_n && (speckle_q0 || speckle_rho || speckle_lambda)) throw std::invalid_argument("--speckle-q0, --speckle-rho and --speckle-lambda need --speckle");
        if (speckle_n) {
            const long n = std::atol(speckle_n);
            if (n < 0 || n > 256) throw std::invalid_argument("--speckle takes 0..256 iterations");
            sopts.n_iter = (uint32_t)n;
            if (speckle_q0) sopts.q0 = (float)std::atof(speckle_q0);
            if (speckle_rho) sopts.rho = (float)std::atof(speckle_rho);
            if (speckle_lambda) sopts.lambda = (float)std::atof(speckle_lambda);
            float q0sq[256], kq[256], lam4;
            if (mcrt_speckle_tables(&sopts, q0sq, kq, &lam4) != MCRT_OK) throw std::invalid_argument(std::string("--speckle: ") + mcrt_last_error());
        }
        if (noise_db && noise_sigma) throw std::invalid_argument("--noise-db and --noise-sigma exclude each other");
        if (!noise_db && !noise_sigma && (noise_seed || dead_elements)) throw std::invalid_argument("--noise-seed and --dead-elements need --noise-db or --noise-sigma");
        const bool noise = noise_db || noise_sigma;
        if (noise_db) {
            nopts.mode = MCRT_NOISE_SNR_DB; nopts.snr_db = (float)std::atof(noise_db);
            if (!std::isfinite(nopts.snr_db)) throw std::invalid_argument("--noise-db takes a finite number of dB");
        }
        if (noise_sigma) {
            nopts.mode = MCRT_NOISE_ABS; nopts.sigma = (float)std::atof(noise_sigma);
            if (!(std::isfinite(nopts.sigma) && nopts.sigma >= 0.0f)) throw std::invalid_argument("--noise-sigma takes a finite standard deviation >= 0");
        }
        if (noise_seed) nopts.seed = (uint32_t)std::strtoul(noise_seed, nullptr, 0);
        if (dead_elements) {
            element_gain.assign(transducer_elements, 1.0f);
            const std::vector<int> dead = comma_list<int>(dead_elements);
            if (dead.empty()) throw std::invalid_argument("--dead-elements takes a list of scan-lines a,b,c");
            for (int e : dead) {
                if (e < 0 || e >= (int)transducer_elements) throw std::invalid_argument("--dead-elements takes scan-lines 0.." + std::to_string(transducer_elements - 1));
                element_gain[(size_t)e] = 0.0f;
            }
        }
        const float *gain = element_gain.empty() ? nullptr : element_gain.data();
        if (!autogain && (autogain_band || autogain_scale || autogain_max_db || autogain_curve))
            throw std::invalid_argument("--autogain-band, --autogain-floor-scale, --autogain-max-db and --autogain-curve need --autogain");
        if (autogain_band) {
            const long n = std::atol(autogain_band);
            if (n < 4 || n > 256) throw std::invalid_argument("--autogain-band takes 4..256 rows");
            aopts.band_rows = (uint32_t)n;
        }
        if (autogain_scale) {
            aopts.floor_scale = (float)std::atof(autogain_scale);
            if (!(std::isfinite(aopts.floor_scale) && aopts.floor_scale >= 0.0f)) throw std::invalid_argument("--autogain-floor-scale takes a finite factor >= 0");
        }
        if (autogain_max_db) {
            const double db = std::atof(autogain_max_db);
            aopts.max_gain = (float)std::pow(10.0, db / 20.0);
            if (!(std::isfinite(db) && db >= 0.0 && std::isfinite(aopts.max_gain))) throw std::invalid_argument("--autogain-max-db takes a finite number of dB >= 0");
        }
        if (!freq_compound && freq_span) throw std::invalid_argument("--freq-span-mhz needs --freq-compound");
        if (!downshift && downshift_min) throw std::invalid_argument("--downshift-min-mhz needs --downshift-mhz-per-mm");
        mcrt_bands bands; mcrt_default_bands(&bands, transducer_frequency, 0.05f);
        // (--freq-compound 1 alone leaves the plain run as it is; a pulse or a downshift of its own is one band through the band path)
        const bool with_bands = (freq_compound && std::atol(freq_compound) != 1) || freq_var_x || downshift;
        if (freq_compound) {
            const long n = std::atol(freq_compound);
            if (n < 1 || n > 8) throw std::invalid_argument("--freq-compound takes 1..8 bands");
            const double span = freq_span ? std::atof(freq_span) : 2.0;
            if (!(std::isfinite(span) && span >= 0.0)) throw std::invalid_argument("--freq-span-mhz takes a finite span >= 0");
            bands.n_bands = (uint32_t)n;
            for (long b = 0; b < n; b++) {
                bands.band_mhz[b] = n > 1 ? (float)((double)transducer_frequency - span / 2.0 + span * (double)b / (double)(n - 1)) : transducer_frequency;
                bands.band_weight[b] = 1.0f;
            }
        }
        if (freq_var_x) bands.var_x = (float)std::atof(freq_var_x);
        if (downshift) bands.downshift_mhz_per_mm = (float)std::atof(downshift);
        if (downshift_min) bands.min_mhz = (float)std::atof(downshift_min);
        if (with_bands) {   // the model's own checks, before anything is traced
            float taps[8 * 7];
            if (mcrt_psf_band_kernels(&bands, resolution, 1, rf_image_::row_mm(), taps, 7, nullptr) != MCRT_OK) throw std::invalid_argument(std::string("--freq-compound: ") + mcrt_last_error());
        }
        if (detect && std::strcmp(detect, "quadrature")) throw std::invalid_argument("--detect takes quadrature");
        if (detect_taps && !detect && !iq_file) throw std::invalid_argument("--detect-taps needs --detect or --iq");
        if (detect_taps) {
            dopts.n_taps = (uint32_t)std::max(std::atol(detect_taps), 0l);
            float taps[63];
            if (dopts.n_taps > 63u || mcrt_detect_taps(&dopts, taps) != MCRT_OK) throw std::invalid_argument("--detect-taps takes 3, 7, 11, ..., 63 taps");
        }
        if (iq_file && (compound_given || sweep_given || with_bands)) throw std::invalid_argument("--iq does not combine with --compound, --sweep or the band options");
        if (!spectral && (spectral_gate || spectral_pulses || spectral_fft || spectral_hop || spectral_db || flow_waveform || spectral_iq))
            throw std::invalid_argument("--gate, --spectral-pulses, --spectral-fft, --spectral-hop, --spectral-db, --flow-waveform and --spectral-iq need --spectral");
        if (spectral) {
            if (compound_given || sweep_given || elevation_given || with_bands) throw std::invalid_argument("--spectral does not combine with --compound, --sweep, --elevation or the band options");
            if (!spectral_gate) throw std::invalid_argument("--spectral needs --gate LINE,DEPTH_MM,LEN_MM");
            if (flow_velocity.empty()) throw std::invalid_argument("--spectral needs --flow-velocity NAME:vx,vy,vz");
            const auto g = comma_list<double>(spectral_gate);
            if (g.size() != 3 || !(g[0] >= 0.0 && g[0] < (double)transducer_elements) || !(g[1] >= 0.0) || !(g[2] > 0.0))
                throw std::invalid_argument("--gate takes LINE,DEPTH_MM,LEN_MM: a scan-line of the probe, a depth >= 0 and a length > 0");
            gate_line = (uint32_t)g[0]; gate_depth_mm = g[1]; gate_len_mm = g[2];
            if (spectral_pulses) spopts.n_pulses = (uint32_t)std::max(std::atol(spectral_pulses), 0l);
            if (spectral_fft) spopts.n_fft = (uint32_t)std::max(std::atol(spectral_fft), 0l);
            if (spectral_hop) spopts.hop = (uint32_t)std::max(std::atol(spectral_hop), 0l);
            if (spectral_db) sgopts.dynamic_range_db = (float)std::atof(spectral_db);
            float h[512];
            if (spopts.n_fft > 512u || mcrt_spectral_window(1, spopts.n_fft, h) != MCRT_OK) throw std::invalid_argument("--spectral-fft: n_fft takes 32, 64, 128, 256 or 512");
            if (spopts.n_pulses < spopts.n_fft || spopts.n_pulses > 16384u) throw std::invalid_argument("--spectral-pulses takes n_fft .. 16384 pulses");
            if (spopts.hop < 1u || spopts.hop > spopts.n_fft) throw std::invalid_argument("--spectral-hop takes 1 .. n_fft pulses");
            if (!(sgopts.dynamic_range_db > 0.0f)) throw std::invalid_argument("--spectral-db takes a dynamic range > 0");
            if (flow_waveform) {
                const auto w = comma_list<double>(flow_waveform);
                if (w.size() != 3 || !(w[0] > 0.0)) throw std::invalid_argument("--flow-waveform takes BPM,PEAK,MIN: beats per minute > 0 and two speeds in mm/s");
                wave_bpm = w[0]; wave_peak = w[1]; wave_min = w[2];
            }
            if (flow_prf) flopts.prf_hz = (float)std::atof(flow_prf);
            double v_nyq = 0.0;
            if (mcrt_flow_nyquist(&flopts, transducer_frequency, 1500.0, &v_nyq) != MCRT_OK) throw std::invalid_argument(std::string("--spectral: ") + mcrt_last_error());
        }
        if (!colour_flow && ((!spectral && (!flow_velocity.empty() || flow_prf)) || flow_packets || flow_wall || flow_avg || flow_vel_thr || flow_grey_max || flow_truth))
            throw std::invalid_argument("--flow-velocity, --flow-packets, --flow-prf-hz, --flow-wall, --flow-avg, --flow-vel-thr, --flow-grey-max and --flow-truth need --colour-flow");
        if (!elastogram && (stiffness || compress || strain_window || strain_search || strain_lsq || strain_truth))
            throw std::invalid_argument("--stiffness, --compress, --strain-window, --strain-search, --strain-lsq and --strain-truth need --elastogram");
        if (elastogram) {
            if (compound_given || sweep_given || elevation_given || with_bands) throw std::invalid_argument("--elastogram does not combine with --compound, --sweep, --elevation or the band options");
            if (!stiffness) throw std::invalid_argument("--elastogram needs --stiffness NAME:E[,NAME:E...]");
            if (compress) applied = std::atof(compress);
            if (strain_window) stopts.window_rows = (uint32_t)std::max(std::atol(strain_window), 0l);
            if (strain_search) stopts.search_rows = (uint32_t)std::max(std::atol(strain_search), 0l);
            if (strain_lsq) stopts.lsq_rows = (uint32_t)std::max(std::atol(strain_lsq), 0l);
            if (stopts.window_rows > 32u || stopts.search_rows > 16u || stopts.lsq_rows < 1u || stopts.lsq_rows > 32u)
                throw std::invalid_argument("--strain-window takes 0..32, --strain-search 0..16 and --strain-lsq 1..32");
            if (!(std::fabs(applied) > 0.0 && std::fabs(applied) <= 0.03125)) throw std::invalid_argument("--compress takes a strain that is not 0, up to 1/32");
            elopts.ref_strain = (float)applied;
            bmode = true;                               // the colour lies over the 8-bit frame
        }
        if (!shear_elastogram && (shear_speed || shear_push || shear_pulses || shear_prf || shear_truth))
            throw std::invalid_argument("--shear-speed, --push, --shear-pulses, --shear-prf and --shear-truth need --shear-elastogram");
        if (shear_elastogram) {
            if (compound_given || sweep_given || elevation_given || with_bands) throw std::invalid_argument("--shear-elastogram does not combine with --compound, --sweep, --elevation or the band options");
            if (!shear_speed) throw std::invalid_argument("--shear-elastogram needs --shear-speed NAME:c[,NAME:c...]");
            if (!shear_push) throw std::invalid_argument("--shear-elastogram needs --push LINE,DEPTH_MM,LEN_MM");
            const auto push = comma_list<double>(shear_push);
            if (push.size() != 3 || !(push[0] >= 0.0 && push[0] == std::floor(push[0])) || !(push[1] >= 0.0) || !(push[2] > 0.0))
                throw std::invalid_argument("--push takes LINE,DEPTH_MM,LEN_MM: a scan-line, a depth >= 0 and a length > 0");
            if (push[0] >= (double)transducer_elements) throw std::invalid_argument("--push: the scan-line is not one of the transducer's");
            shopts.push_line = (uint32_t)push[0]; push_depth_mm = push[1]; push_len_mm = push[2];
            if (shear_pulses) shopts.n_pulses = (uint32_t)std::max(std::atol(shear_pulses), 0l);
            if (shear_prf) shopts.prf_hz = (float)std::atof(shear_prf);
            if (shopts.n_pulses < 4u || shopts.n_pulses > 256u) throw std::invalid_argument("--shear-pulses takes 4..256");
            if (!(std::isfinite(shopts.prf_hz) && shopts.prf_hz > 0.0f)) throw std::invalid_argument("--shear-prf takes a pulse rate > 0");
            shelopts.ref_strain = 3.0f * shopts.density * 2.0f * 2.0f;      // the modulus of the speed a material has that is not named
            bmode = true;                               // the colour lies over the 8-bit frame
        }
        if (!m_mode && (m_line || motion || m_prf || m_bpm || m_pulses || m_hop || m_height || m_depth || m_bulk || m_labels || m_truth))
            throw std::invalid_argument("--m-line, --motion, --m-prf, --m-bpm, --m-pulses, --m-hop, --m-height, --m-depth-mm, --m-bulk-mm, --m-labels and --m-truth need --m-mode");
        if (m_mode) {
            if (compound_given || sweep_given || elevation_given || with_bands) throw std::invalid_argument("--m-mode does not combine with --compound, --sweep, --elevation or the band options");
            if (!motion) throw std::invalid_argument("--m-mode needs --motion NAME:e[,NAME:e...]");
            if (!m_line) throw std::invalid_argument("--m-mode needs --m-line LINE");
            const long line = std::atol(m_line);
            if (line < 0 || line >= (long)transducer_elements) throw std::invalid_argument("--m-line: the scan-line is not one of the transducer's");
            m_scan_line = (uint32_t)line;
            if (m_prf) m_prf_hz = std::atof(m_prf);
            if (m_bpm) m_beats = std::atof(m_bpm);
            if (!(std::isfinite(m_prf_hz) && m_prf_hz > 0.0) || !(std::isfinite(m_beats) && m_beats > 0.0)) throw std::invalid_argument("--m-prf and --m-bpm take rates > 0");
            if (m_pulses) mmopts.n_pulses = (uint32_t)std::max(std::atol(m_pulses), 0l);
            if (mmopts.n_pulses < 1u || mmopts.n_pulses > 16384u) throw std::invalid_argument("--m-pulses takes 1..16384");
            if (m_hop) mdopts.hop = (uint32_t)std::max(std::atol(m_hop), 0l);
            if (mdopts.hop < 1u || mdopts.hop > mmopts.n_pulses) throw std::invalid_argument("--m-hop takes 1..the pulses");
            if (m_height) mdopts.height = (uint32_t)std::max(std::atol(m_height), 0l);
            if (mdopts.height < 1u || mdopts.height > 4096u) throw std::invalid_argument("--m-height takes 1..4096");
            if (m_depth) {
                const auto d = comma_list<double>(m_depth);
                if (d.size() != 2 || !(d[0] >= 0.0) || !(d[1] > d[0])) throw std::invalid_argument("--m-depth-mm takes LO,HI: two depths, 0 <= LO < HI");
                m_depth_lo = d[0]; m_depth_hi = d[1];
            }
            if (m_bulk) {
                const auto b = comma_list<double>(m_bulk);
                if (b.size() != 2 || !std::isfinite(b[0]) || !std::isfinite(b[1])) throw std::invalid_argument("--m-bulk-mm takes A,PER_MIN: an amplitude [mm] and cycles per minute");
                m_bulk_mm = b[0]; m_bulk_per_min = b[1];
            }
        }
        if (colour_flow) {
            if (compound_given || sweep_given || elevation_given || with_bands) throw std::invalid_argument("--colour-flow does not combine with --compound, --sweep, --elevation or the band options");
            if (flow_velocity.empty()) throw std::invalid_argument("--colour-flow needs --flow-velocity NAME:vx,vy,vz");
            if (flow_packets) flopts.n_packets = (uint32_t)std::max(std::atol(flow_packets), 0l);
            if (flow_prf) flopts.prf_hz = (float)std::atof(flow_prf);
            if (flow_wall) {
                if (!std::strcmp(flow_wall, "none")) flopts.wall = MCRT_FLOW_WALL_NONE;
                else if (!std::strcmp(flow_wall, "mean")) flopts.wall = MCRT_FLOW_WALL_MEAN;
                else if (!std::strcmp(flow_wall, "linear")) flopts.wall = MCRT_FLOW_WALL_LINEAR;
                else throw std::invalid_argument("--flow-wall takes none, mean or linear");
            }
            if (flow_avg) {
                const auto ab = comma_list<int>(flow_avg);
                if (ab.size() != 2 || ab[0] < 0 || ab[1] < 0) throw std::invalid_argument("--flow-avg takes A,B: the half-window in rows and scan-lines");
                flopts.avg_rows = (uint32_t)ab[0]; flopts.avg_lines = (uint32_t)ab[1];
            }
            if (flow_vel_thr) flcol.vel_thr_mm_s = (float)std::atof(flow_vel_thr);
            if (flow_grey_max) flcol.grey_max = (uint32_t)std::max(std::atol(flow_grey_max), 0l);
            double v_nyq = 0.0;
            if (mcrt_flow_nyquist(&flopts, transducer_frequency, 1500.0, &v_nyq) != MCRT_OK) throw std::invalid_argument(std::string("--colour-flow: ") + mcrt_last_error());
            if (!(flcol.vel_thr_mm_s >= 0.0f) || flcol.grey_max > 255u) throw std::invalid_argument("--flow-vel-thr takes a velocity >= 0 and --flow-grey-max 0..255");
            bmode = true;                               // the colour lies over the 8-bit frame
        }
        if (!freehand_n && (freehand_step || freehand_fan || freehand_box || freehand_voxel || freehand_out || freehand_mode || freehand_fill))
            throw std::invalid_argument("--freehand-step-mm, --freehand-fan-deg, --freehand-box-mm, --freehand-voxel-mm, --freehand-out, --freehand-mode and --freehand-fill need --freehand");
        long freehand_frames = 0; double freehand_step_mm = 0.0, freehand_fan_deg = 0.0;
        mcrt_volume_grid fgrid{};
        if (freehand_n) {
            freehand_frames = std::atol(freehand_n);
            if (freehand_frames < 1 || freehand_frames > 1024) throw std::invalid_argument("--freehand takes 1..1024 frames");
            if (!freehand_step || !freehand_box || !freehand_voxel || !freehand_out)
                throw std::invalid_argument("--freehand needs --freehand-step-mm, --freehand-box-mm, --freehand-voxel-mm and --freehand-out");
            freehand_step_mm = std::atof(freehand_step); freehand_fan_deg = freehand_fan ? std::atof(freehand_fan) : 0.0;
            if (!std::isfinite(freehand_step_mm)) throw std::invalid_argument("--freehand-step-mm must be finite");
            if (!(std::isfinite(freehand_fan_deg) && std::fabs((double)(freehand_frames - 1) / 2.0 * freehand_fan_deg) < 90.0))
                throw std::invalid_argument("--freehand-fan-deg must keep every frame's tilt below 90 degrees");
            const std::vector<double> box = comma_list<double>(freehand_box);
            const double voxel = std::atof(freehand_voxel);
            if (box.size() != 6) throw std::invalid_argument("--freehand-box-mm takes six numbers");
            if (!(std::isfinite(voxel) && voxel > 0.0)) throw std::invalid_argument("--freehand-voxel-mm must be > 0");
            uint32_t n[3];
            for (int k = 0; k < 3; k++) {
                const double cells = std::floor((box[3 + k] - box[k]) / voxel);
                if (!(cells >= 0.0 && cells < 16777215.0)) throw std::invalid_argument("--freehand-box-mm: X1 >= X0, Y1 >= Y0, Z1 >= Z0, and fewer than 2^24 voxels along an axis");
                n[k] = (uint32_t)cells + 1u; fgrid.origin_mm[k] = box[k];
            }
            fgrid.du_mm[0] = fgrid.dv_mm[1] = fgrid.dw_mm[2] = voxel; fgrid.nu = n[0]; fgrid.nv = n[1]; fgrid.nw = n[2];
            if (freehand_mode) {
                if (!std::strcmp(freehand_mode, "mean")) fopts.mode = MCRT_RECON_MEAN;
                else if (!std::strcmp(freehand_mode, "max")) fopts.mode = MCRT_RECON_MAX;
                else throw std::invalid_argument("--freehand-mode takes mean or max");
            }
            if (freehand_fill) {
                const long h = std::atol(freehand_fill);
                if (h < 0 || h > 3) throw std::invalid_argument("--freehand-fill takes 0..3 voxels");
                fopts.fill_radius = (uint32_t)h;
            }
            float A[9], b[3];
            if (mcrt_recon_transform(&fgrid, 10.0, A, b) != MCRT_OK) throw std::invalid_argument(std::string("--freehand: ") + mcrt_last_error());
            if ((double)fgrid.nu * fgrid.nv * fgrid.nw >= 2147483648.0) throw std::invalid_argument("--freehand-box-mm: 2^31 voxels or more");
        }
        if (!speckle3d_n && (speckle3d_q0 || speckle3d_rho || speckle3d_lambda)) throw std::invalid_argument("--speckle3d-q0, --speckle3d-rho and --speckle3d-lambda need --speckle3d");
        if (speckle3d_n) {
            if (!freehand_n) throw std::invalid_argument("--speckle3d needs --freehand");
            const long n = std::atol(speckle3d_n);
            if (n < 0 || n > 256) throw std::invalid_argument("--speckle3d takes 0..256 iterations");
            s3opts.n_iter = (uint32_t)n;
            if (speckle3d_q0) s3opts.q0 = (float)std::atof(speckle3d_q0);
            if (speckle3d_rho) s3opts.rho = (float)std::atof(speckle3d_rho);
            if (speckle3d_lambda) s3opts.lambda = (float)std::atof(speckle3d_lambda);
            if (mcrt_speckle3d_weights(&fgrid, s3opts.weight) != MCRT_OK) throw std::invalid_argument(std::string("--speckle3d: ") + mcrt_last_error());
            float q0sq[256], kq[256], k[4];
            if (mcrt_speckle3d_tables(&s3opts, q0sq, kq, k) != MCRT_OK) throw std::invalid_argument(std::string("--speckle3d: ") + mcrt_last_error());
        }
        std::vector<unsigned char> cut_bytes;         // the last frame's cut, as the PGM holds it
        const mcrt_compound_opts *opts = compound_mode || compound_feather || compound_weights ? &copts : nullptr;
        std::vector<float> steers;                    // centred on the unsteered view, ascending
        for (int n = 0; n < compound; n++) steers.push_back((float)((double)(n - (compound - 1) / 2) * compound_step_deg * 3.14159265358979323846 / 180.0));
        for (float s : steers)
            if (!(std::isfinite(s) && std::fabs((double)s) < 1.5707963267948966)) throw std::invalid_argument("--compound-step-deg: every view must be steered by less than 90 degrees");
        const json cfg = load_json(argv[1]);
        const psf_ psf = [&] {
            psf_ p{ transducer_frequency, 0.05f, 0.2f, var_z };
            if (!focus_mm.empty()) p.set_focus(focus_mm.data(), (uint32_t)focus_mm.size(), focal_range_mm);
            if (elevation_given) p.set_elevation((uint32_t)elevation_pitch_um);
            if (with_bands) p.set_bands(bands);
            return p;
        }();
        const auto &t_pos = cfg.at("transducerPosition");
        const auto &t_dir = cfg.at("transducerAngles");
        // millimeter_t sep = amplitude.to<float>() * radius / elements (main.cpp:66): float * cm -> cm, then -> mm
        const double separation_mm = (((double)(float)transducer_amplitude * transducer_radius_cm) / (double)transducer_elements) * 10.0;
        transducer_ transducer(transducer_frequency, transducer_radius_cm, separation_mm, vec3((float)t_pos[0], (float)t_pos[1], (float)t_pos[2]),
                               std::array<float, 3>{ (float)t_dir[0], (float)t_dir[1], (float)t_dir[2] });
        auto dev = std::make_shared<device>(devices);
        scene scene{ cfg, transducer, dev, samples };
        scene.step(1000.0f);
        rf_image_ rf_image{ dev, transducer_radius_cm * 10.0, transducer_amplitude };
        std::vector<float> flow_vel;                    // --flow-velocity: a vector per material of the scene
        uint32_t spectral_material = 0;                 // --spectral: the material of the first --flow-velocity
        if (colour_flow || spectral) {
            spectral_material = scene.material_index(flow_velocity.front().substr(0, flow_velocity.front().find(':')));
            flow_vel.assign(3 * scene.material_names.size(), 0.0f);
            for (const std::string &item : flow_velocity) {
                const size_t colon = item.find(':');
                const auto v = colon == std::string::npos ? std::vector<float>{} : comma_list<float>(item.c_str() + colon + 1);
                if (v.size() != 3) throw std::invalid_argument("--flow-velocity takes NAME:vx,vy,vz");
                const uint32_t m = scene.material_index(item.substr(0, colon));
                for (int k = 0; k < 3; k++) flow_vel[3 * m + k] = v[k];
            }
        }
        std::vector<double> modulus;                    // --stiffness: a Young's modulus per material of the scene
        if (elastogram) {
            modulus.assign(scene.material_names.size(), 1.0);
            std::string list = stiffness;
            for (size_t at = 0; at <= list.size();) {
                const size_t comma = std::min(list.find(',', at), list.size());
                const std::string item = list.substr(at, comma - at);
                const size_t colon = item.find(':');
                if (colon == std::string::npos || colon + 1 >= item.size()) throw std::invalid_argument("--stiffness takes NAME:E[,NAME:E...]");
                modulus[scene.material_index(item.substr(0, colon))] = std::atof(item.c_str() + colon + 1);
                at = comma + 1;
            }
        }
        std::vector<double> shear_c;                    // --shear-speed: a shear speed per material of the scene
        if (shear_elastogram) {
            shear_c.assign(scene.material_names.size(), 2.0);
            std::string list = shear_speed;
            for (size_t at = 0; at <= list.size();) {
                const size_t comma = std::min(list.find(',', at), list.size());
                const std::string item = list.substr(at, comma - at);
                const size_t colon = item.find(':');
                if (colon == std::string::npos || colon + 1 >= item.size()) throw std::invalid_argument("--shear-speed takes NAME:c[,NAME:c...]");
                shear_c[scene.material_index(item.substr(0, colon))] = std::atof(item.c_str() + colon + 1);
                at = comma + 1;
            }
            const double pitch = rf_image_::row_mm(), R = (double)rf_image_::max_rows;
            const double rows = std::min(std::max(std::nearbyint(push_len_mm / pitch), 1.0), R);
            shopts.push_rows = (uint32_t)rows;
            shopts.push_row0 = (uint32_t)std::min(std::max(std::nearbyint(push_depth_mm / pitch - rows / 2.0), 0.0), R - rows);
        }
        std::vector<double> dilation;                   // --motion: a dilation per material of the scene
        std::vector<int32_t> m_wave, m_shift;           // ... the waveform and the bulk motion of every pulse
        if (m_mode) {
            dilation.assign(scene.material_names.size(), 0.0);
            std::string list = motion;
            for (size_t at = 0; at <= list.size();) {
                const size_t comma = std::min(list.find(',', at), list.size());
                const std::string item = list.substr(at, comma - at);
                const size_t colon = item.find(':');
                if (colon == std::string::npos || colon + 1 >= item.size()) throw std::invalid_argument("--motion takes NAME:e[,NAME:e...]");
                dilation[scene.material_index(item.substr(0, colon))] = std::atof(item.c_str() + colon + 1);
                at = comma + 1;
            }
            const double pitch = rf_image_::row_mm();
            const long R = (long)rf_image_::max_rows;
            m_wave.assign(mmopts.n_pulses, 0); m_shift.assign(mmopts.n_pulses, 0);
            check(mcrt_mmode_waveform(m_prf_hz, m_beats, mmopts.n_pulses, m_wave.data()), "mcrt_mmode_waveform");
            check(mcrt_mmode_bulk(m_prf_hz, m_bulk_per_min, m_bulk_mm / pitch, mmopts.n_pulses, m_shift.data()), "mcrt_mmode_bulk");
            if (m_depth) {
                mdopts.row_lo = (uint32_t)std::min(std::max((long)std::nearbyint(m_depth_lo / pitch), 0l), R - 1);
                mdopts.row_hi = (uint32_t)std::min(std::max((long)std::nearbyint(m_depth_hi / pitch), (long)mdopts.row_lo + 1), R);
            }
        }

        const auto t0 = std::chrono::high_resolution_clock::now();
        for (int f = 0; f < frames; f++) {
            if (sweep_given) rf_image.trace((uint32_t)f, transducer, sweep);                        // ... in K tilted planes
            else if (compound_given) rf_image.trace((uint32_t)f, transducer, steers);               // ... in N steered views
            else if (elevation_given) rf_image.trace((uint32_t)f, transducer, psf, (uint32_t)elevation);   // ... in K elevation planes, folded
            else rf_image.trace((uint32_t)f);      // clear + cast_rays + accumulation (main.cpp:102-144)
            if ((colour_flow || spectral) && f == frames - 1) rf_image.flow_split(transducer, flow_vel);   // the raw trace split by label, before the PSF
            rf_image.convolve(psf);           // main.cpp:146
            if (noise) rf_image.add_noise(nopts, gain);   // the receiver's noise floor and dead elements, on whatever the convolution ran over
            if (iq_file && f == frames - 1) {            // the analytic pair of the last frame's RF, before it is detected
                std::vector<float> pair;
                rf_image.iq(dopts, pair);
                std::ofstream out(iq_file, std::ios::binary);
                out.write((const char *)pair.data(), (std::streamsize)(pair.size() * sizeof(float)));
                if (!out) throw std::runtime_error(std::string("cannot write ") + iq_file);
            }
            rf_image_::strain_truth strain_true;
            if (elastogram && f == frames - 1) {         // the labels, the analytic pair and the post-compression pair of the RF, before it is detected
                double cycles = 0.0;
                check(mcrt_psf_carrier(transducer_frequency, resolution, &cycles), "mcrt_psf_carrier");
                strain_true = rf_image.compress(transducer, modulus, applied, 1.0, stopts, cycles, nullptr, detect ? &dopts : nullptr);
            }
            rf_image_::shear_wave_maps shear_true;
            if (shear_elastogram && f == frames - 1) {   // the labels, the analytic pair, the push and its tracked wave, before the RF is detected
                double cycles = 0.0;
                check(mcrt_psf_carrier(transducer_frequency, resolution, &cycles), "mcrt_psf_carrier");
                shear_true = rf_image.shear_wave(transducer, shear_c, shopts, cycles, 12, 8.0, nullptr, detect ? &dopts : nullptr);
            }
            if (m_mode && f == frames - 1) {             // the labels, the analytic pair and the pulses of one scan-line, before the RF is detected; then their sweep
                double cycles = 0.0;
                check(mcrt_psf_carrier(transducer_frequency, resolution, &cycles), "mcrt_psf_carrier");
                rf_image.m_lines(transducer, m_scan_line, dilation, m_wave, m_shift, mmopts, cycles, nullptr, detect ? &dopts : nullptr);
                const auto sweep_pic = rf_image.m_mode(mdopts);
                write_pgm(m_mode, sweep_pic.width, sweep_pic.height, sweep_pic.picture);
                if (m_labels) write_pgm(m_labels, sweep_pic.width, sweep_pic.height, sweep_pic.labels);
                if (m_truth) {
                    std::ofstream out(m_truth, std::ios::binary);
                    out.write((const char *)sweep_pic.truth_disp.data(), (std::streamsize)(sweep_pic.truth_disp.size() * sizeof(float)));
                    if (!out) throw std::runtime_error(std::string("cannot write ") + m_truth);
                }
            }
            if (detect) rf_image.detect(dopts);          // quadrature detection in the place of ...
            else rf_image.envelope();         // main.cpp:147
            if (speckle_n) rf_image.despeckle(sopts);   // the despeckle filter, on whatever the envelope ran over
            if (autogain) rf_image.autogain(aopts, noise);   // the gain curve over depth, before anything gathers a picture; the floor is the noise stage's
            if (render_dir && render_labels && f == frames - 1) {                                   // the box seen from a direction, and what is seen
                rf_image.labels(transducer, &lopts);
                write_pgm(render_labels, view.nx, view.ny, rf_image.render_labels(cut, view, &ropts, &display, nullptr, &cut_bytes));
            }
            else if (render_dir) cut_bytes = rf_image.render(cut, view, &ropts, &display);          // the box seen from a direction
            else if (sweep_given)             // the cut through the swept volume
                cut_bytes = bmode ? rf_image.volume(display, cut) : to_bytes(rf_image.volume(cut));   // (as rf_image::save)
            else if (compound_given) { if (bmode) rf_image.postprocess(display, steers, nullptr, opts); else rf_image.postprocess(steers, opts); }   // the views averaged (or opts' mode)
            else if (bmode) rf_image.postprocess(display);   // main.cpp:148, log-compressed to 8-bit grey
            else rf_image.postprocess();      // main.cpp:148
            if (colour_flow && f == frames - 1) {        // the colour processor and the overlay over the frame just made
                std::vector<unsigned char> rgb;
                const auto maps = rf_image.colour_flow(psf, flopts, flcol, rgb, noise, 4.0, detect ? &dopts : nullptr);
                write_ppm(colour_flow, display.out_cols, display.out_rows, rgb);
                if (flow_truth) {
                    std::ofstream out(flow_truth, std::ios::binary);
                    out.write((const char *)maps.truth.data(), (std::streamsize)(maps.truth.size() * sizeof(float)));
                    if (!out) throw std::runtime_error(std::string("cannot write ") + flow_truth);
                }
            }
            if (elastogram && f == frames - 1) {         // the tracker and the overlay over the frame just made
                std::vector<unsigned char> rgb;
                rf_image.track(stopts);
                rf_image.elastogram(elopts, rgb);
                write_ppm(elastogram, display.out_cols, display.out_rows, rgb);
                if (strain_truth) {
                    std::ofstream out(strain_truth, std::ios::binary);
                    out.write((const char *)strain_true.strain.data(), (std::streamsize)(strain_true.strain.size() * sizeof(float)));
                    if (!out) throw std::runtime_error(std::string("cannot write ") + strain_truth);
                }
            }
            if (shear_elastogram && f == frames - 1) {   // the fit across scan-lines and the overlay over the frame just made
                std::vector<unsigned char> rgb;
                rf_image.shear_speed(shopts);
                rf_image.shear_elastogram(shelopts, rgb);
                write_ppm(shear_elastogram, display.out_cols, display.out_rows, rgb);
                if (shear_truth) {
                    std::ofstream out(shear_truth, std::ios::binary);
                    out.write((const char *)shear_true.truth_speed.data(), (std::streamsize)(shear_true.truth_speed.size() * sizeof(float)));
                    if (!out) throw std::runtime_error(std::string("cannot write ") + shear_truth);
                }
            }
            if (spectral && f == frames - 1) {           // the sample gate's series, its spectra and the sonogram
                double v_nyq = 0.0;
                check(mcrt_flow_nyquist(&flopts, transducer_frequency, 1500.0, &v_nyq), "mcrt_flow_nyquist");
                if (!colour_flow) rf_image.flow(psf, flopts, noise, detect ? &dopts : nullptr);     // (colour_flow() has detected the two parts already)
                const uint32_t L = (uint32_t)scene.material_names.size(), R = (uint32_t)rf_image_::max_rows, m = spectral_material;
                const double pitch = rf_image_::row_mm();
                const uint32_t G = (uint32_t)std::min(std::max(std::nearbyint(gate_len_mm / pitch), 1.0), 64.0);
                const uint32_t row0 = (uint32_t)std::min(std::max(std::nearbyint(gate_depth_mm / pitch - G / 2.0), 0.0), (double)(R - G));
                spopts.gate_rows = G;
                const double vx = flow_vel[3 * m], vy = flow_vel[3 * m + 1], vz = flow_vel[3 * m + 2], norm = std::sqrt((vx * vx + vy * vy) + vz * vz);
                if (!(norm > 0.0)) throw std::invalid_argument("--spectral: the first --flow-velocity gives its material no velocity, so the flow has no direction");
                const double ux = (float)(vx / norm), uy = (float)(vy / norm), uz = (float)(vz / norm);
                const double dx = transducer.dir[3 * gate_line], dy = transducer.dir[3 * gate_line + 1], dz = transducer.dir[3 * gate_line + 2];
                const double axial = std::min(std::max(0.0 - ((ux * dx + uy * dy) + uz * dz), -1.0), 1.0);
                std::vector<uint8_t> moving(L, 0); moving[m] = 1;
                const std::vector<uint8_t> line_labels = rf_image.tissue_line(gate_line);
                std::vector<float> frac(G), speed(spopts.n_pulses);
                std::vector<int32_t> rate(G);
                std::vector<int64_t> phase(spopts.n_pulses);
                check(mcrt_spectral_profile(line_labels.data(), R, row0, G, moving.data(), L, 2.0, frac.data()), "mcrt_spectral_profile");
                check(mcrt_spectral_rates(frac.data(), G, axial, rate.data()), "mcrt_spectral_rates");
                check(mcrt_pulse_waveform((double)flopts.prf_hz, wave_bpm, wave_peak < 0.0 ? norm : wave_peak, wave_min, spopts.n_pulses, speed.data()), "mcrt_pulse_waveform");
                check(mcrt_spectral_phase(v_nyq, speed.data(), spopts.n_pulses, phase.data()), "mcrt_spectral_phase");
                const std::vector<float> series = rf_image.spectral_series(gate_line, row0, spopts, rate, phase, noise);
                const auto sp = rf_image.spectrum(spopts, v_nyq);
                write_pgm(spectral, sp.n_cols, sp.n_fft, rf_image.sonogram(sgopts));
                if (spectral_iq) {
                    std::ofstream out(spectral_iq, std::ios::binary);
                    out.write((const char *)series.data(), (std::streamsize)(series.size() * sizeof(float)));
                    if (!out) throw std::runtime_error(std::string("cannot write ") + spectral_iq);
                }
            }
        }
        check(dev->synchronize(), "mcrt_synchronize");
        const double dt = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - t0).count();
        std::cout << frames / dt << " frames/s, " << (double)frames * transducer_elements * samples / dt << " rays/s on " << devices.size() << " GPU context(s)" << std::endl;
        if (autogain && frames > 0) {   // the last frame's penetration depth and gain curve
            const std::vector<float> &k = rf_image.gain_curve();
            const std::vector<uint32_t> &pen = rf_image.penetration_rows();
            std::cout << "autogain: penetration depth " << rf_image.penetration_mm() << " mm (" << pen.at(0) << " of " << k.size() << " rows), gain "
                      << *std::min_element(k.begin(), k.end()) << " .. " << *std::max_element(k.begin(), k.end()) << std::endl;
            if (autogain_curve) {
                std::ofstream f(autogain_curve);
                f.precision(9);
                for (size_t r = 0; r < k.size(); r++) f << r << " " << (double)r * rf_image_::row_mm() << " " << k[r] << "\n";
                if (!f) throw std::runtime_error(std::string("cannot write ") + autogain_curve);
            }
        }
        if (freehand_n) {   // the freehand sweep and its volume, in an image of its own: the picture below is the run's
            rf_image_ tracked{ dev, transducer_radius_cm * 10.0, transducer_amplitude };
            const auto poses = transducer.freehand((uint32_t)freehand_frames, freehand_step_mm, freehand_fan_deg);
            tracked.trace((uint32_t)std::max(frames - 1, 0), poses.pos, poses.dir);
            tracked.convolve(psf);
            if (noise) tracked.add_noise(nopts, gain);
            if (detect) tracked.detect(dopts); else tracked.envelope();
            if (speckle_n) tracked.despeckle(sopts);
            if (autogain) tracked.autogain(aopts, noise);
            const std::vector<float> vox = tracked.reconstruct(fgrid, &fopts, nullptr, speckle3d_n ? &s3opts : nullptr);
            std::ofstream f(freehand_out, std::ios::binary);
            for (float v : vox) {
                uint32_t w; std::memcpy(&w, &v, 4);
                const unsigned char le[4] = { (unsigned char)w, (unsigned char)(w >> 8), (unsigned char)(w >> 16), (unsigned char)(w >> 24) };
                f.write((const char *)le, 4);
            }
            if (!f) throw std::runtime_error(std::string("cannot write ") + freehand_out);
            if (freehand_labels) {   // what tissue every voxel is
                mcrt_recon_label_opts flopts; mcrt_default_recon_label_opts(&flopts, (uint32_t)scene.materials.size());
                flopts.fill_radius = fopts.fill_radius; flopts.fill_min = fopts.fill_min;
                const std::vector<unsigned char> lab = tracked.reconstruct_labels(fgrid, flopts, &lopts);
                std::ofstream fl(freehand_labels, std::ios::binary);
                fl.write((const char *)lab.data(), (std::streamsize)lab.size());
                if (!fl) throw std::runtime_error(std::string("cannot write ") + freehand_labels);
            }
            std::cout << "freehand volume: " << fgrid.nu << " x " << fgrid.nv << " x " << fgrid.nw << " voxels (x, y, z), float32 [nw][nv][nu], " << freehand_frames << " frames" << std::endl;
        }
        if (argc > 4 && render_dir) write_pgm(argv[4], view.nx, view.ny, cut_bytes);
        else if (argc > 4 && sweep_given) write_pgm(argv[4], cut.nu, cut.nv, cut_bytes);
        else if (argc > 4) { if (bmode) rf_image.save_bmode(argv[4]); else rf_image.save(argv[4]); }
        if (labels_file) {   // what is in that picture: the tissue under every pixel
            rf_image.labels(transducer, &lopts);
            if (sweep_given) write_pgm(labels_file, cut.nu, cut.nv, rf_image.label_volume(cut));
            else write_pgm(labels_file, 500, 400, rf_image.label_picture());
        }
        if (transmission_file) {   // how much sound gets to every pixel of that picture
            topts.rule = lopts.rule; topts.start_offset = lopts.start_offset;
            rf_image.transmission(transducer, &topts);
            const std::vector<float> T = rf_image.transmission_picture();
            std::vector<unsigned char> grey(T.size());
            for (size_t i = 0; i < T.size(); i++) {
                float g = T[i] > 0.0f ? std::min(T[i], 1.0f) : 0.0f;      // min(max(T, 0), 1), a NaN black
                if (transmission_db) g = T[i] > 0.0f ? std::min(std::max((10.0f * std::log10(T[i]) + transmission_range_db) / transmission_range_db, 0.0f), 1.0f) : 0.0f;
                grey[i] = (unsigned char)(g * 255.0f + 0.5f);
            }
            write_pgm(transmission_file, 500, 400, grey);
        }
        if (argc > 5) {   // the last frame's RF image after main.cpp:146-147, row-major [465][512] float32 (for the parity test)
            const auto img = sweep_given ? rf_image.view_intensities((uint32_t)sweep_planes / 2u)
                             : compound_given ? rf_image.view_intensities((uint32_t)(compound - 1) / 2u) : rf_image.intensities();
            std::ofstream f(argv[5], std::ios::binary);
            f.write((const char *)img.data(), (std::streamsize)(img.size() * sizeof(float)));
        }
    } catch (const std::exception &ex) {
        std::cout << "The program found an error and will terminate.\n" << "Reason:\n" << ex.what() << std::endl;
        return 1;
    }
    return 0;
}
