"""The calls Simulator makes on its Context, pinned: every mode (plain, compound=, sweep=, elevation=, compound= with elevation=) with and without a
two-band Psf and with noise=, speckle=, autogain= and detect= all on, through a recording stand-in for api.Context -- no device.  The expected logs
are literals: which buffer every stage acts on, how many images, split into how many frames, from which image id on.  E = 64, 465 rows, frame id 3
(not 0, so that frame_id * n and frame_id * n * B show)."""
import contextlib
import ctypes as C
import hashlib
import types
import numpy as np
import pytest

E, R, S, FID = 64, 465, 2, 3
STEERS, SWEEP, BANDS = (-0.1, 0.1), (2, 0.02), (4.0, 5.0)
ALL_ON = dict(noise=40, speckle=True, autogain=True, detect="quadrature")
MODES = {"plain": {}, "compound": dict(compound=STEERS), "sweep": dict(sweep=SWEEP), "elevation": dict(elevation=True),
         "compound+elevation": dict(compound=STEERS, elevation=True)}
# the calls a mode allows (iq() also needs a psf without bands)
CALLS = {"plain": ("bmode", "frame", "iq", "freehand", "labels", "transmission"), "compound": ("bmode", "compound_image", "labels", "transmission"),
         "sweep": ("volume", "labels", "transmission"), "elevation": ("bmode", "frame", "iq", "labels", "transmission"),
         "compound+elevation": ("bmode", "compound_image", "labels", "transmission")}


class Handle:
    """device memory of the stand-in: the allocation's ordinal and a byte offset into it"""

    def __init__(self, ordinal, offset=0):
        self.ordinal, self.offset = ordinal, offset

    def __add__(self, nbytes):
        return Handle(self.ordinal, self.offset + int(nbytes))

    def __eq__(self, other):
        return isinstance(other, Handle) and (self.ordinal, self.offset) == (other.ordinal, other.offset)

    def __hash__(self):
        return hash((self.ordinal, self.offset))


def shown(v, arrays):
    """a value of a call as the log keeps it: handles as h<ordinal>+<offset>, arrays by their name in `arrays` (shape, dtype, sha1 of bytes -> name; one
    the table does not know is given a name when the table may grow, else shown in full), structs by their fields"""
    if isinstance(v, Handle):
        return "h%d+%d" % (v.ordinal, v.offset)
    if isinstance(v, np.ndarray):
        key = (tuple(v.shape), str(v.dtype), hashlib.sha1(np.ascontiguousarray(v).tobytes()).hexdigest())
        if key not in arrays and getattr(arrays, "grows", False):
            arrays[key] = "a%d" % len(arrays)
        return arrays.get(key, repr(key))
    if isinstance(v, C.Structure):
        return "%s(%s)" % (type(v).__name__, " ".join("%s=%s" % (f[0], shown(getattr(v, f[0]), arrays)) for f in v._fields_ if not f[0].startswith("_")))
    if isinstance(v, C.Array):
        return shown(tuple(v), arrays)
    if isinstance(v, (tuple, list)):
        return "(" + ",".join(shown(x, arrays) for x in v) + ")"
    if isinstance(v, (np.floating, np.integer)):
        v = v.item()
    return repr(v) if v is None or isinstance(v, (bool, int, float, str)) else "<%s>" % type(v).__name__       # (the scene, at set-up)


def recorder(arrays):
    """the stand-in for api.Context, as a class: alloc and temp hand out handles, d2h zeros, every other method is logged as one line"""

    class Recorder:
        def __init__(self, device=0):
            self.h, self.log, self.sizes = 1, [], []                      # sizes[ordinal] = (bytes, whether ctx.temp made it)
            self.params = types.SimpleNamespace(n_rows=R, frequency=4.5)

        def alloc(self, nbytes, temp=False):
            self.sizes.append((int(nbytes), temp))
            return Handle(len(self.sizes) - 1)

        @contextlib.contextmanager
        def temp(self, nbytes):
            yield self.alloc(nbytes, temp=True)

        def d2h(self, dev, shape, dtype=np.float32):
            assert isinstance(dev, Handle)
            return np.zeros(shape, dtype)

        def __getattr__(self, name):
            if name.startswith("_"):
                raise AttributeError(name)

            def call(*args, **kw):
                self.log.append(" ".join([name] + [shown(a, arrays) for a in args] + ["%s=%s" % (k, shown(x, arrays)) for k, x in kw.items()]))
            return call

    return Recorder


def run_case(mcrt, monkeypatch, arrays, mode, bands, options=ALL_ON):
    """one Simulator through the calls its mode allows -> ({call: its log}, the stand-in's allocations at the end)"""
    monkeypatch.setattr(mcrt.api, "Context", recorder(arrays))
    tr = mcrt.Transducer(E)
    psf = mcrt.Psf(freq=tr.frequency, bands=BANDS if bands else None)
    sim = mcrt.Simulator(types.SimpleNamespace(materials=np.zeros((3, 8), np.float32)), tr, n_samples=S, psf=psf, **MODES[mode], **options)
    grid = mcrt.volume_grid((-4, 30, -2), (2, 0, 0), (0, 2, 0), (0, 0, 2), 4, 3, 2)
    pos, dirs = tr.poses([(0, 0, -0.1), (0, 0, 0.1)], [(0, 0, 0), (0, 0, 0)])
    args = dict(bmode=(FID,), frame=(FID,), iq=(FID,), compound_image=(FID,), volume=(FID, grid), freehand=(FID, pos, dirs, grid), labels=(), transmission=())
    logs = {}
    for call in CALLS[mode]:
        if call == "iq" and bands:
            continue
        sim.ctx.log.clear()
        getattr(sim, call)(*args[call])
        logs[call] = list(sim.ctx.log)
    sizes = list(sim.ctx.sizes)
    sim.close()
    return logs, sizes


CASES = [(mode, bands) for mode in MODES for bands in (False, True)]


def case_name(mode, bands):
    return mode + ("/bands" if bands else "")


@pytest.mark.parametrize("mode,bands", CASES, ids=[case_name(*c) for c in CASES])
def test_every_stage_on(mcrt, monkeypatch, mode, bands):
    logs, sizes = run_case(mcrt, monkeypatch, dict(ARRAYS), mode, bands)
    want = EXPECTED[case_name(mode, bands)]
    assert sorted(logs) == sorted(want)
    for call, log in logs.items():
        assert log == want[call].split("\n"), "%s: %s() logged\n%s" % (case_name(mode, bands), call, "\n".join(log))
    # the buffers that outlive a call, in the order they were made: the RF image, the stack, the plane stacks; then what the first run needs, and
    # what freehand()'s two tracked frames need on top -- a band stack of exactly n * B * E * R * 4 bytes with bands and none without
    n, img, B = 2 if mode in ("compound", "sweep", "compound+elevation") else 1, E * R * 4, len(BANDS)
    kept = [img] + ([n * img] if n > 1 else []) + ([n * 7 * img] if "elevation" in mode else [])
    for frames, images in [(1, n)] + ([(2, 2)] if mode == "plain" else []):
        kept += ([images * B * img] if bands else []) + [frames * (2 + R) * 4]
    assert [nbytes for nbytes, temp in sizes if not temp] == kept
    # after a run nothing is left waiting in the band stack: the last call that names it is the fold
    for call, log in logs.items():
        stacks = {ln.split()[6] for ln in log if ln.startswith("convolve_bands_frames ")}
        assert len(stacks) == (1 if bands and call not in ("labels", "transmission") else 0)
        for h in stacks:
            assert sizes[int(h[1:].split("+")[0])] == ((2 if call == "freehand" else n) * B * img, False)
            assert [ln.split()[0] for ln in log if h in ln.split()][-1] == "band_fold_frames"


def test_every_option_off(mcrt, monkeypatch):
    """only trace, convolve, envelope and the gather"""
    logs, sizes = run_case(mcrt, monkeypatch, dict(ARRAYS), "plain", False, options={})
    assert logs["bmode"] == EXPECTED["plain/off"]["bmode"].split("\n")
    assert [ln.split()[0] for ln in logs["bmode"]] == ["trace_frame", "convolve_frames", "envelope_frames", "bmode_frames"]
    assert [ln.split()[0] for ln in logs["freehand"]] == ["trace_frames_poses", "convolve_frames", "envelope_frames", "recon_frames"]
    assert [nbytes for nbytes, temp in sizes if not temp] == [E * R * 4]


# the host tables the calls are given: (shape, dtype, sha1 of the bytes) -> the name the logs below use
ARRAYS = {
    ((7,), 'float32', '27c16db31bd380be1ba00d3be41aa7cf75c4d6bd'): 'a2',              # the psf's axial kernel
    ((13,), 'float32', '36b978b606915cde11f0d82116a624eafbbf4535'): 'a3',             # ... and lateral kernel
    ((2, 64, 3), 'float32', '5ca440c040f9caa566330e2d8109f656bd12bb3c'): 'a4',        # freehand()'s two poses: positions
    ((2, 64, 3), 'float32', 'a9c5fe841c4f573c934de187d2fb0f329edb23f0'): 'a5',        # ... and directions
    ((2, 465, 7), 'float32', '1848a1046b60dc9aadc07626b24bd8bed38f71ad'): 'a6',       # the two bands' axial rows
    ((465, 2), 'float32', 'bc80b15130375c4d83a15964adb7854c89b234bb'): 'a7',          # ... and weights
    ((2, 64, 3), 'float32', '84b17e7bb23b4acff00d469cd307af4d4078b7f4'): 'a8',        # the steered views: positions
    ((2, 64, 3), 'float32', '7c6545cadecb5355f5b59045e71854173f3e3cab'): 'a9',        # ... and directions
    ((2, 64, 3), 'float32', 'e92115ea2a55d3400d8ebb5b63130ae2ca555017'): 'a10',       # the swept planes: positions
    ((2, 64, 3), 'float32', '504b22fea33e6cd401f4fcfe5f72c52d21269c2b'): 'a11',       # ... and directions
    ((7, 64, 3), 'float32', '1c4b723c91f1bb71a976dd2f088498291cc7f76f'): 'a12',       # the elevation planes: positions
    ((7, 64, 3), 'float32', '9bb7c1307ef88a94dc1b3e5d23a5298ce337c6eb'): 'a13',       # ... and directions
    ((465, 7), 'float32', '7fbbed92c0d93e1cd8354b0eecd17205c4f389cf'): 'a14',         # the elevation weights of every row
    ((14, 64, 3), 'float32', 'ad8dc1473a69631b890edc3d63dd3b47f90cc42d'): 'a15',      # the elevation planes of the two views: positions
    ((14, 64, 3), 'float32', '0d604bcb312762f4ec0b4c7f105e029b8c70af55'): 'a16',      # ... and directions
}

# {case: {call: its log, one call per line}}, as the parent of the commit that added this file made them
EXPECTED = {
    'plain': {
        'bmode': """trace_frame 3 h0+0
convolve_frames h0+0 1 64 465 a2 a3
noise_frames h0+0 1 1 64 465 first_image_id=3 element_gain=None sigma_dev=h1+0 seed=1313818963 snr_db=40.0
detect_frames h0+0 1 64 465 env_dev=h0+0
speckle_frames h0+0 1 64 465 n_iter=20 q0=0.5227231979370117 rho=0.1666666716337204 lambda_=0.5
autogain_frames h0+0 1 1 64 465 floor_dev=h1+0 gain_dev=h1+8 pen_dev=h1+4
bmode_frames h0+0 1 64 465 h2+0""",
        'frame': """trace_frame 3 h0+0
convolve_frames h0+0 1 64 465 a2 a3
noise_frames h0+0 1 1 64 465 first_image_id=3 element_gain=None sigma_dev=h1+0 seed=1313818963 snr_db=40.0
export_rf h0+0 64 465""",
        'iq': """trace_frame 3 h0+0
convolve_frames h0+0 1 64 465 a2 a3
noise_frames h0+0 1 1 64 465 first_image_id=3 element_gain=None sigma_dev=h1+0 seed=1313818963 snr_db=40.0
detect_frames h0+0 1 64 465 iq_dev=h3+0""",
        'freehand': """trace_frames_poses 6 a4 a5 h4+0
convolve_frames h4+0 2 64 465 a2 a3
free h1+0
noise_frames h4+0 2 1 64 465 first_image_id=6 element_gain=None sigma_dev=h7+0 seed=1313818963 snr_db=40.0
detect_frames h4+0 2 64 465 env_dev=h4+0
speckle_frames h4+0 2 64 465 n_iter=20 q0=0.5227231979370117 rho=0.1666666716337204 lambda_=0.5
autogain_frames h4+0 2 1 64 465 floor_dev=h7+0 gain_dev=h7+16 pen_dev=h7+8
recon_frames h4+0 a4 a5 2 64 465 VolumeGrid(origin_mm=(-4.0,30.0,-2.0) du_mm=(2.0,0.0,0.0) dv_mm=(0.0,2.0,0.0) dw_mm=(0.0,0.0,2.0) nu=4 nv=3 nw=2) h5+0 count_dev=None row_mm=None unit_mm=10.0""",
        'labels': """label_frames None None rule='traced' start_offset=None tissue_dev=h8+0 interface_dev=h9+0 crossings_dev=h10+0
label_scan_convert_frames h8+0 1 64 465 h11+0 radius_mm=30.0 total_angle=1.0471975511965976 out_rows=400 out_cols=500""",
        'transmission': """transmit_frames None None mode='total' rule='traced' start_offset=None transmit_dev=h12+0 reflect_dev=h13+0 crossings_dev=h14+0
scan_convert_frames h12+0 1 64 465 h15+0 radius_mm=30.0 total_angle=1.0471975511965976 out_rows=400 out_cols=500""",
    },
    'plain/bands': {
        'bmode': """trace_frame 3 h0+0
convolve_bands_frames h0+0 1 64 465 a6 h1+0 lateral=a3
noise_frames h1+0 1 2 64 465 first_image_id=6 element_gain=None sigma_dev=h2+0 seed=1313818963 snr_db=40.0
detect_frames h1+0 2 64 465 env_dev=h1+0
band_fold_frames h1+0 1 2 64 465 a7 h0+0
speckle_frames h0+0 1 64 465 n_iter=20 q0=0.5227231979370117 rho=0.1666666716337204 lambda_=0.5
autogain_frames h0+0 1 1 64 465 floor_dev=h2+0 gain_dev=h2+8 pen_dev=h2+4
bmode_frames h0+0 1 64 465 h3+0""",
        'frame': """trace_frame 3 h0+0
convolve_bands_frames h0+0 1 64 465 a6 h1+0 lateral=a3
noise_frames h1+0 1 2 64 465 first_image_id=6 element_gain=None sigma_dev=h2+0 seed=1313818963 snr_db=40.0
band_fold_frames h1+0 1 2 64 465 a7 h0+0
export_rf h0+0 64 465""",
        'freehand': """trace_frames_poses 6 a4 a5 h4+0
free h1+0
convolve_bands_frames h4+0 2 64 465 a6 h7+0 lateral=a3
free h2+0
noise_frames h7+0 2 2 64 465 first_image_id=12 element_gain=None sigma_dev=h8+0 seed=1313818963 snr_db=40.0
detect_frames h7+0 4 64 465 env_dev=h7+0
band_fold_frames h7+0 2 2 64 465 a7 h4+0
speckle_frames h4+0 2 64 465 n_iter=20 q0=0.5227231979370117 rho=0.1666666716337204 lambda_=0.5
autogain_frames h4+0 2 1 64 465 floor_dev=h8+0 gain_dev=h8+16 pen_dev=h8+8
recon_frames h4+0 a4 a5 2 64 465 VolumeGrid(origin_mm=(-4.0,30.0,-2.0) du_mm=(2.0,0.0,0.0) dv_mm=(0.0,2.0,0.0) dw_mm=(0.0,0.0,2.0) nu=4 nv=3 nw=2) h5+0 count_dev=None row_mm=None unit_mm=10.0""",
        'labels': """label_frames None None rule='traced' start_offset=None tissue_dev=h9+0 interface_dev=h10+0 crossings_dev=h11+0
label_scan_convert_frames h9+0 1 64 465 h12+0 radius_mm=30.0 total_angle=1.0471975511965976 out_rows=400 out_cols=500""",
        'transmission': """transmit_frames None None mode='total' rule='traced' start_offset=None transmit_dev=h13+0 reflect_dev=h14+0 crossings_dev=h15+0
scan_convert_frames h13+0 1 64 465 h16+0 radius_mm=30.0 total_angle=1.0471975511965976 out_rows=400 out_cols=500""",
    },
    'compound': {
        'bmode': """trace_frames_poses 6 a8 a9 h1+0
convolve_frames h1+0 2 64 465 a2 a3
noise_frames h1+0 1 2 64 465 first_image_id=6 element_gain=None sigma_dev=h2+0 seed=1313818963 snr_db=40.0
detect_frames h1+0 2 64 465 env_dev=h1+0
speckle_frames h1+0 2 64 465 n_iter=20 q0=0.5227231979370117 rho=0.1666666716337204 lambda_=0.5
autogain_frames h1+0 1 2 64 465 floor_dev=h2+0 gain_dev=h2+8 pen_dev=h2+4
bmode_compound_frames h1+0 1 64 465 (-0.1,0.1) h3+0 compound_mode='mean' view_weights=None feather_lines=0.0""",
        'compound_image': """trace_frames_poses 6 a8 a9 h1+0
convolve_frames h1+0 2 64 465 a2 a3
noise_frames h1+0 1 2 64 465 first_image_id=6 element_gain=None sigma_dev=h2+0 seed=1313818963 snr_db=40.0
detect_frames h1+0 2 64 465 env_dev=h1+0
speckle_frames h1+0 2 64 465 n_iter=20 q0=0.5227231979370117 rho=0.1666666716337204 lambda_=0.5
autogain_frames h1+0 1 2 64 465 floor_dev=h2+0 gain_dev=h2+8 pen_dev=h2+4
compound_frames h1+0 1 64 465 (-0.1,0.1) h4+0 radius_mm=30.0 total_angle=1.0471975511965976 out_rows=400 out_cols=500 mode='mean' view_weights=None feather_lines=0.0""",
        'labels': """label_frames None None rule='traced' start_offset=None tissue_dev=h5+0 interface_dev=h6+0 crossings_dev=h7+0
label_scan_convert_frames h5+0 1 64 465 h8+0 radius_mm=30.0 total_angle=1.0471975511965976 out_rows=400 out_cols=500""",
        'transmission': """transmit_frames None None mode='total' rule='traced' start_offset=None transmit_dev=h9+0 reflect_dev=h10+0 crossings_dev=h11+0
scan_convert_frames h9+0 1 64 465 h12+0 radius_mm=30.0 total_angle=1.0471975511965976 out_rows=400 out_cols=500""",
    },
    'compound/bands': {
        'bmode': """trace_frames_poses 6 a8 a9 h1+0
convolve_bands_frames h1+0 2 64 465 a6 h2+0 lateral=a3
noise_frames h2+0 1 4 64 465 first_image_id=12 element_gain=None sigma_dev=h3+0 seed=1313818963 snr_db=40.0
detect_frames h2+0 4 64 465 env_dev=h2+0
band_fold_frames h2+0 2 2 64 465 a7 h1+0
speckle_frames h1+0 2 64 465 n_iter=20 q0=0.5227231979370117 rho=0.1666666716337204 lambda_=0.5
autogain_frames h1+0 1 2 64 465 floor_dev=h3+0 gain_dev=h3+8 pen_dev=h3+4
bmode_compound_frames h1+0 1 64 465 (-0.1,0.1) h4+0 compound_mode='mean' view_weights=None feather_lines=0.0""",
        'compound_image': """trace_frames_poses 6 a8 a9 h1+0
convolve_bands_frames h1+0 2 64 465 a6 h2+0 lateral=a3
noise_frames h2+0 1 4 64 465 first_image_id=12 element_gain=None sigma_dev=h3+0 seed=1313818963 snr_db=40.0
detect_frames h2+0 4 64 465 env_dev=h2+0
band_fold_frames h2+0 2 2 64 465 a7 h1+0
speckle_frames h1+0 2 64 465 n_iter=20 q0=0.5227231979370117 rho=0.1666666716337204 lambda_=0.5
autogain_frames h1+0 1 2 64 465 floor_dev=h3+0 gain_dev=h3+8 pen_dev=h3+4
compound_frames h1+0 1 64 465 (-0.1,0.1) h5+0 radius_mm=30.0 total_angle=1.0471975511965976 out_rows=400 out_cols=500 mode='mean' view_weights=None feather_lines=0.0""",
        'labels': """label_frames None None rule='traced' start_offset=None tissue_dev=h6+0 interface_dev=h7+0 crossings_dev=h8+0
label_scan_convert_frames h6+0 1 64 465 h9+0 radius_mm=30.0 total_angle=1.0471975511965976 out_rows=400 out_cols=500""",
        'transmission': """transmit_frames None None mode='total' rule='traced' start_offset=None transmit_dev=h10+0 reflect_dev=h11+0 crossings_dev=h12+0
scan_convert_frames h10+0 1 64 465 h13+0 radius_mm=30.0 total_angle=1.0471975511965976 out_rows=400 out_cols=500""",
    },
    'sweep': {
        'volume': """trace_frames_poses 6 a10 a11 h1+0
convolve_frames h1+0 2 64 465 a2 a3
noise_frames h1+0 1 2 64 465 first_image_id=6 element_gain=None sigma_dev=h2+0 seed=1313818963 snr_db=40.0
detect_frames h1+0 2 64 465 env_dev=h1+0
speckle_frames h1+0 2 64 465 n_iter=20 q0=0.5227231979370117 rho=0.1666666716337204 lambda_=0.5
autogain_frames h1+0 1 2 64 465 floor_dev=h2+0 gain_dev=h2+8 pen_dev=h2+4
volume_frames h1+0 1 64 465 Sweep(n_planes=2 step_rad=0.019999999552965164 pivot_mm=0.0) VolumeGrid(origin_mm=(-4.0,30.0,-2.0) du_mm=(2.0,0.0,0.0) dv_mm=(0.0,2.0,0.0) dw_mm=(0.0,0.0,2.0) nu=4 nv=3 nw=2) h3+0 radius_mm=30.0 total_angle=1.0471975511965976""",
        'labels': """label_frames a10 a11 rule='traced' start_offset=None tissue_dev=h4+0 interface_dev=h5+0 crossings_dev=h6+0""",
        'transmission': """transmit_frames a10 a11 mode='total' rule='traced' start_offset=None transmit_dev=h7+0 reflect_dev=h8+0 crossings_dev=h9+0""",
    },
    'sweep/bands': {
        'volume': """trace_frames_poses 6 a10 a11 h1+0
convolve_bands_frames h1+0 2 64 465 a6 h2+0 lateral=a3
noise_frames h2+0 1 4 64 465 first_image_id=12 element_gain=None sigma_dev=h3+0 seed=1313818963 snr_db=40.0
detect_frames h2+0 4 64 465 env_dev=h2+0
band_fold_frames h2+0 2 2 64 465 a7 h1+0
speckle_frames h1+0 2 64 465 n_iter=20 q0=0.5227231979370117 rho=0.1666666716337204 lambda_=0.5
autogain_frames h1+0 1 2 64 465 floor_dev=h3+0 gain_dev=h3+8 pen_dev=h3+4
volume_frames h1+0 1 64 465 Sweep(n_planes=2 step_rad=0.019999999552965164 pivot_mm=0.0) VolumeGrid(origin_mm=(-4.0,30.0,-2.0) du_mm=(2.0,0.0,0.0) dv_mm=(0.0,2.0,0.0) dw_mm=(0.0,0.0,2.0) nu=4 nv=3 nw=2) h4+0 radius_mm=30.0 total_angle=1.0471975511965976""",
        'labels': """label_frames a10 a11 rule='traced' start_offset=None tissue_dev=h5+0 interface_dev=h6+0 crossings_dev=h7+0""",
        'transmission': """transmit_frames a10 a11 mode='total' rule='traced' start_offset=None transmit_dev=h8+0 reflect_dev=h9+0 crossings_dev=h10+0""",
    },
    'elevation': {
        'bmode': """trace_frames_poses 21 a12 a13 h1+0
elevation_frames h1+0 1 7 64 465 a14 h0+0
convolve_frames h0+0 1 64 465 a2 a3
noise_frames h0+0 1 1 64 465 first_image_id=3 element_gain=None sigma_dev=h2+0 seed=1313818963 snr_db=40.0
detect_frames h0+0 1 64 465 env_dev=h0+0
speckle_frames h0+0 1 64 465 n_iter=20 q0=0.5227231979370117 rho=0.1666666716337204 lambda_=0.5
autogain_frames h0+0 1 1 64 465 floor_dev=h2+0 gain_dev=h2+8 pen_dev=h2+4
bmode_frames h0+0 1 64 465 h3+0""",
        'frame': """trace_frames_poses 21 a12 a13 h1+0
elevation_frames h1+0 1 7 64 465 a14 h0+0
convolve_frames h0+0 1 64 465 a2 a3
noise_frames h0+0 1 1 64 465 first_image_id=3 element_gain=None sigma_dev=h2+0 seed=1313818963 snr_db=40.0
export_rf h0+0 64 465""",
        'iq': """trace_frames_poses 21 a12 a13 h1+0
elevation_frames h1+0 1 7 64 465 a14 h0+0
convolve_frames h0+0 1 64 465 a2 a3
noise_frames h0+0 1 1 64 465 first_image_id=3 element_gain=None sigma_dev=h2+0 seed=1313818963 snr_db=40.0
detect_frames h0+0 1 64 465 iq_dev=h4+0""",
        'labels': """label_frames None None rule='traced' start_offset=None tissue_dev=h5+0 interface_dev=h6+0 crossings_dev=h7+0
label_scan_convert_frames h5+0 1 64 465 h8+0 radius_mm=30.0 total_angle=1.0471975511965976 out_rows=400 out_cols=500""",
        'transmission': """transmit_frames None None mode='total' rule='traced' start_offset=None transmit_dev=h9+0 reflect_dev=h10+0 crossings_dev=h11+0
scan_convert_frames h9+0 1 64 465 h12+0 radius_mm=30.0 total_angle=1.0471975511965976 out_rows=400 out_cols=500""",
    },
    'elevation/bands': {
        'bmode': """trace_frames_poses 21 a12 a13 h1+0
elevation_frames h1+0 1 7 64 465 a14 h0+0
convolve_bands_frames h0+0 1 64 465 a6 h2+0 lateral=a3
noise_frames h2+0 1 2 64 465 first_image_id=6 element_gain=None sigma_dev=h3+0 seed=1313818963 snr_db=40.0
detect_frames h2+0 2 64 465 env_dev=h2+0
band_fold_frames h2+0 1 2 64 465 a7 h0+0
speckle_frames h0+0 1 64 465 n_iter=20 q0=0.5227231979370117 rho=0.1666666716337204 lambda_=0.5
autogain_frames h0+0 1 1 64 465 floor_dev=h3+0 gain_dev=h3+8 pen_dev=h3+4
bmode_frames h0+0 1 64 465 h4+0""",
        'frame': """trace_frames_poses 21 a12 a13 h1+0
elevation_frames h1+0 1 7 64 465 a14 h0+0
convolve_bands_frames h0+0 1 64 465 a6 h2+0 lateral=a3
noise_frames h2+0 1 2 64 465 first_image_id=6 element_gain=None sigma_dev=h3+0 seed=1313818963 snr_db=40.0
band_fold_frames h2+0 1 2 64 465 a7 h0+0
export_rf h0+0 64 465""",
        'labels': """label_frames None None rule='traced' start_offset=None tissue_dev=h5+0 interface_dev=h6+0 crossings_dev=h7+0
label_scan_convert_frames h5+0 1 64 465 h8+0 radius_mm=30.0 total_angle=1.0471975511965976 out_rows=400 out_cols=500""",
        'transmission': """transmit_frames None None mode='total' rule='traced' start_offset=None transmit_dev=h9+0 reflect_dev=h10+0 crossings_dev=h11+0
scan_convert_frames h9+0 1 64 465 h12+0 radius_mm=30.0 total_angle=1.0471975511965976 out_rows=400 out_cols=500""",
    },
    'compound+elevation': {
        'bmode': """trace_frames_poses 42 a15 a16 h2+0
elevation_frames h2+0 2 7 64 465 a14 h1+0
convolve_frames h1+0 2 64 465 a2 a3
noise_frames h1+0 1 2 64 465 first_image_id=6 element_gain=None sigma_dev=h3+0 seed=1313818963 snr_db=40.0
detect_frames h1+0 2 64 465 env_dev=h1+0
speckle_frames h1+0 2 64 465 n_iter=20 q0=0.5227231979370117 rho=0.1666666716337204 lambda_=0.5
autogain_frames h1+0 1 2 64 465 floor_dev=h3+0 gain_dev=h3+8 pen_dev=h3+4
bmode_compound_frames h1+0 1 64 465 (-0.1,0.1) h4+0 compound_mode='mean' view_weights=None feather_lines=0.0""",
        'compound_image': """trace_frames_poses 42 a15 a16 h2+0
elevation_frames h2+0 2 7 64 465 a14 h1+0
convolve_frames h1+0 2 64 465 a2 a3
noise_frames h1+0 1 2 64 465 first_image_id=6 element_gain=None sigma_dev=h3+0 seed=1313818963 snr_db=40.0
detect_frames h1+0 2 64 465 env_dev=h1+0
speckle_frames h1+0 2 64 465 n_iter=20 q0=0.5227231979370117 rho=0.1666666716337204 lambda_=0.5
autogain_frames h1+0 1 2 64 465 floor_dev=h3+0 gain_dev=h3+8 pen_dev=h3+4
compound_frames h1+0 1 64 465 (-0.1,0.1) h5+0 radius_mm=30.0 total_angle=1.0471975511965976 out_rows=400 out_cols=500 mode='mean' view_weights=None feather_lines=0.0""",
        'labels': """label_frames None None rule='traced' start_offset=None tissue_dev=h6+0 interface_dev=h7+0 crossings_dev=h8+0
label_scan_convert_frames h6+0 1 64 465 h9+0 radius_mm=30.0 total_angle=1.0471975511965976 out_rows=400 out_cols=500""",
        'transmission': """transmit_frames None None mode='total' rule='traced' start_offset=None transmit_dev=h10+0 reflect_dev=h11+0 crossings_dev=h12+0
scan_convert_frames h10+0 1 64 465 h13+0 radius_mm=30.0 total_angle=1.0471975511965976 out_rows=400 out_cols=500""",
    },
    'compound+elevation/bands': {
        'bmode': """trace_frames_poses 42 a15 a16 h2+0
elevation_frames h2+0 2 7 64 465 a14 h1+0
convolve_bands_frames h1+0 2 64 465 a6 h3+0 lateral=a3
noise_frames h3+0 1 4 64 465 first_image_id=12 element_gain=None sigma_dev=h4+0 seed=1313818963 snr_db=40.0
detect_frames h3+0 4 64 465 env_dev=h3+0
band_fold_frames h3+0 2 2 64 465 a7 h1+0
speckle_frames h1+0 2 64 465 n_iter=20 q0=0.5227231979370117 rho=0.1666666716337204 lambda_=0.5
autogain_frames h1+0 1 2 64 465 floor_dev=h4+0 gain_dev=h4+8 pen_dev=h4+4
bmode_compound_frames h1+0 1 64 465 (-0.1,0.1) h5+0 compound_mode='mean' view_weights=None feather_lines=0.0""",
        'compound_image': """trace_frames_poses 42 a15 a16 h2+0
elevation_frames h2+0 2 7 64 465 a14 h1+0
convolve_bands_frames h1+0 2 64 465 a6 h3+0 lateral=a3
noise_frames h3+0 1 4 64 465 first_image_id=12 element_gain=None sigma_dev=h4+0 seed=1313818963 snr_db=40.0
detect_frames h3+0 4 64 465 env_dev=h3+0
band_fold_frames h3+0 2 2 64 465 a7 h1+0
speckle_frames h1+0 2 64 465 n_iter=20 q0=0.5227231979370117 rho=0.1666666716337204 lambda_=0.5
autogain_frames h1+0 1 2 64 465 floor_dev=h4+0 gain_dev=h4+8 pen_dev=h4+4
compound_frames h1+0 1 64 465 (-0.1,0.1) h6+0 radius_mm=30.0 total_angle=1.0471975511965976 out_rows=400 out_cols=500 mode='mean' view_weights=None feather_lines=0.0""",
        'labels': """label_frames None None rule='traced' start_offset=None tissue_dev=h7+0 interface_dev=h8+0 crossings_dev=h9+0
label_scan_convert_frames h7+0 1 64 465 h10+0 radius_mm=30.0 total_angle=1.0471975511965976 out_rows=400 out_cols=500""",
        'transmission': """transmit_frames None None mode='total' rule='traced' start_offset=None transmit_dev=h11+0 reflect_dev=h12+0 crossings_dev=h13+0
scan_convert_frames h11+0 1 64 465 h14+0 radius_mm=30.0 total_angle=1.0471975511965976 out_rows=400 out_cols=500""",
    },
    'plain/off': {
        'bmode': """trace_frame 3 h0+0
convolve_frames h0+0 1 64 465 a2 a3
envelope_frames h0+0 1 64 465
bmode_frames h0+0 1 64 465 h1+0""",
    },
}

