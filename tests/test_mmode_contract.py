"""M-mode without a GPU (include/mcrt.h: mcrt_mline, mcrt_mmode_opts, mcrt_default_mmode_opts, mcrt_mmode_table, mcrt_mmode_waveform,
mcrt_mmode_bulk, mcrt_mmode_draws, mcrt_mmode_display_opts, mcrt_default_mmode_display_opts, mcrt_mmode_rows): the host helpers against
tests/mmode_mirror.py exactly, the structs and their defaults, every refusal that needs no device, and the properties of the model on the
float32 mirror: the zero-motion identity, a rigid shift by whole rows, the displacement against an independent integer sum (with its
saturation), and how well the far wall of a pulsating lumen can be followed.

THE MEASURED ACCURACY of the float32 mirror (a line of 465 rows of speckle at 0.3475 cycles per row, a lumen of 60 rows at a twentieth of
the speckle's amplitude dilated by up to 3 %, a wall echo of forty times the speckle's amplitude on either side, 64 pulses over one beat, no
noise; the energy centroid of the far wall's echo within +- 5 rows of its true position against that position, which moves by up to 1.8
rows): median error 0.0033 rows, largest 0.0191 rows (MEDIAN_ROWS and LARGEST_ROWS below; with walls of ten times the speckle the
speckle that interferes with the echo biases the centroid by 0.06 rows at rest).  The test asserts twice these figures.
(The four model tests read tests/mmode_mirror.py alone: they hold the model to its properties whatever the library does, and the model
is tied to the device by tests/test_gpu_mmode.py, bit for bit.  Every other test here calls the library's new symbols.)"""
import ctypes as C
import numpy as np
import pytest

import mmode_mirror as mm

f32 = np.float32
INVALID, LIMIT = -1, -5
CARRIER = 0.3475
p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)


def speckle(R, seed=0, E=1):
    """finite speckle-like pairs [1][E][R][2]: a carrier at CARRIER cycles per row under a smooth random envelope"""
    rng = np.random.default_rng(seed)
    b = rng.standard_normal((1, E, R + 6, 2))
    b = sum(b[:, :, i:i + R] for i in range(7)) / 7.0
    z = (b[..., 0] + 1j * b[..., 1]) * np.exp(2j * np.pi * CARRIER * np.arange(R))
    return np.stack([z.real, z.imag], axis=-1).astype(f32)


# ------------------------------------------------------------------ structs, defaults, the version
def test_structs_and_defaults(mcrt):
    L = mcrt.load_library()
    assert L.mcrt_version() == 109
    assert C.sizeof(mcrt.Mline) == 8 and (mcrt.Mline.image.offset, mcrt.Mline.line.offset) == (0, 4)
    o = mcrt.MmodeOpts()
    assert C.sizeof(o) == 12 and [getattr(mcrt.MmodeOpts, n).offset for n in ("n_pulses", "sigma", "seed")] == [0, 4, 8]
    assert L.mcrt_default_mmode_opts(C.byref(o)) == 0
    assert (o.n_pulses, o.sigma, o.seed) == (1024, 0.0, 0x4D4D4F44) and {n: getattr(o, n) for n in mm.DEFAULTS} == mm.DEFAULTS
    assert L.mcrt_default_mmode_opts(None) == INVALID
    d = mcrt.MmodeDisplayOpts()
    names = ("hop", "height", "row_lo", "row_hi", "dynamic_range_db", "gain_db", "ref")
    assert C.sizeof(d) == 28 and [getattr(mcrt.MmodeDisplayOpts, n).offset for n in names] == list(range(0, 28, 4))
    assert L.mcrt_default_mmode_display_opts(C.byref(d)) == 0
    assert tuple(getattr(d, n) for n in names) == (4, 400, 0, 0, 60.0, 0.0, 0.0) and {n: getattr(d, n) for n in names} == mm.DISPLAY_DEFAULTS
    assert L.mcrt_default_mmode_display_opts(None) == INVALID
    o = mcrt.mmode_opts_struct(n_pulses=16384, sigma=0.5, seed=9)
    assert (o.n_pulses, o.sigma, o.seed) == (16384, 0.5, 9)
    d = mcrt.mmode_display_opts_struct(hop=3, height=7, row_lo=2, row_hi=9, dynamic_range_db=40.0, gain_db=-3.0, ref=2.5)
    assert tuple(getattr(d, n) for n in names) == (3, 7, 2, 9, 40.0, -3.0, 2.5)


def test_the_counter_word_is_its_own():
    assert mm.COUNTER == 0x4D4D4F44 and mm.COUNTER not in (0x4E4F4953, 0x464C4F57, 0x53504543, 0x5354524E, 0x53484552) and mm.COUNTER >= 16


# ------------------------------------------------------------------ the tables
def test_table_equals_the_mirrors(mcrt):
    dil = [0.0, -0.05, 0.03, 0.25, -0.25, 1e-9, 0.0123456789, -3e-8]
    got = mcrt.host_mmode_table(dil)
    assert got.dtype == np.int32 and np.array_equal(got, mm.mmode_table(dil))
    assert list(mcrt.host_mmode_table([0.25, -0.25, 0.01])) == [4194304, -4194304, 167772]


def test_table_refuses(mcrt):
    L = mcrt.load_library()
    dil = np.array([0.01, -0.02], np.float64)
    out = np.full(2, -7, np.int32)
    call = lambda d=dil, n=2, o=out: L.mcrt_mmode_table(p(d), n, p(o))
    assert call(d=None) == INVALID and call(o=None) == INVALID and call(n=0) == INVALID
    assert L.mcrt_mmode_table(p(np.zeros(255)), 255, p(np.zeros(255, np.int32))) == LIMIT
    for bad in (np.nan, np.inf, -np.inf, 0.2500001, -0.2500001, 1e30):
        assert call(d=np.array([0.01, bad])) == INVALID, bad
    assert (out == -7).all()
    assert call() == 0 and list(out) == [167772, -335544]


@pytest.mark.parametrize("prf,bpm,T", [(1000.0, 72.0, 1024), (64.0, 60.0, 64), (5000.0, 140.0, 333), (123.456, 33.3, 1), (1000.0, 72.0, 16384)])
def test_waveform_equals_the_mirrors(mcrt, prf, bpm, T):
    w = mcrt.host_mmode_waveform(prf, bpm, T)
    assert w.dtype == np.int32 and w.shape == (T,) and np.array_equal(w, mm.waveform(prf, bpm, T))
    assert w.min() >= 0 and w.max() <= 65536 and w[0] == 0


def test_waveform_reaches_its_peak_and_rests():
    w = mm.waveform(1000.0, 60.0, 1000)                                  # one beat: the peak at x = 0.15, at rest from x = 0.3 on
    assert w[150] == 65536 and not w[300:].any() and (w[1:300] > 0).all()


@pytest.mark.parametrize("prf,cpm,amp,T", [(1000.0, 15.0, 3.0, 1024), (50.0, 12.0, -32.0, 500), (1000.0, 0.0, 5.0, 7), (777.0, -20.0, 0.001, 100), (100.0, 15.0, 32.0, 16384)])
def test_bulk_equals_the_mirrors(mcrt, prf, cpm, amp, T):
    b = mcrt.host_mmode_bulk(prf, cpm, amp, T)
    assert b.dtype == np.int32 and b.shape == (T,) and np.array_equal(b, mm.bulk(prf, cpm, amp, T))
    assert np.abs(b.astype(np.int64)).max() <= 32 << 24 and b[0] == 0


def test_waveform_and_bulk_refuse(mcrt):
    L = mcrt.load_library()
    w = np.full(8, -7, np.int32)
    wave = lambda prf=1000.0, bpm=72.0, n=8, o=w: L.mcrt_mmode_waveform(prf, bpm, n, p(o))
    bulk = lambda prf=1000.0, cpm=15.0, amp=2.0, n=8, o=w: L.mcrt_mmode_bulk(prf, cpm, amp, n, p(o))
    assert wave(o=None) == INVALID and wave(n=0) == INVALID and bulk(o=None) == INVALID and bulk(n=0) == INVALID
    big = np.zeros(16385, np.int32)
    assert wave(n=16385, o=big) == LIMIT and bulk(n=16385, o=big) == LIMIT
    for bad in (np.nan, np.inf, -np.inf, 0.0, -1.0):
        assert wave(prf=bad) == INVALID and wave(bpm=bad) == INVALID and bulk(prf=bad) == INVALID, bad
    for bad in (np.nan, np.inf, -np.inf):
        assert bulk(cpm=bad) == INVALID and bulk(amp=bad) == INVALID, bad
    assert bulk(amp=32.0000001) == INVALID and bulk(amp=-33.0) == INVALID
    assert (w == -7).all() and not big.any()
    assert wave() == 0 and (w != -7).all() and bulk(amp=32.0) == 0 and bulk(amp=-32.0) == 0


@pytest.mark.parametrize("seed,image,line,R,T", [(0x4D4D4F44, 0, 0, 1, 1), (7, 3, 5, 65, 9), (0xFFFFFFFF, 0xFFFFFFFF, 511, 130, 3), (1, 2, 0, 2048, 2)])
def test_draws_equal_the_mirrors(mcrt, seed, image, line, R, T):
    d = mcrt.host_mmode_draws(seed, image, line, R, T)
    assert d.dtype == np.int32 and d.shape == (T, R, 2) and np.array_equal(d, mm.draws(seed, image, line, R, T))


def test_draws_differ_from_the_other_stages(mcrt):
    """the same (line, row, pulse, key) under the strain and the shear stage's counter words gives other draws"""
    d = mcrt.host_mmode_draws(5, 1, 2, 40, 1)[0]
    assert not np.array_equal(d, mcrt.host_strain_draws(5, 1, 3, 40)[2]) and not np.array_equal(d, mcrt.host_shear_draws(5, 1, 3, 40, 0)[2])


def test_draws_refuse(mcrt):
    L = mcrt.load_library()
    d = np.full((2, 3, 2), -7, np.int32)
    call = lambda R=3, T=2, o=d: L.mcrt_mmode_draws(1, 2, 3, R, T, p(o))
    assert call(o=None) == INVALID and call(R=0) == INVALID and call(T=0) == INVALID
    assert call(R=2049) == LIMIT and call(T=16385) == LIMIT
    assert (d == -7).all() and call() == 0 and (d != -7).any()


@pytest.mark.parametrize("lo,hi,H", [(0, 465, 400), (0, 465, 465), (0, 465, 930), (0, 1, 1), (0, 1, 7), (17, 18, 400), (100, 131, 7), (3, 2048, 4096), (0, 2048, 1), (5, 12, 7)])
def test_rows_equal_the_mirrors(mcrt, lo, hi, H):
    idx, wt = mcrt.host_mmode_rows(lo, hi, H)
    mi, mw = mm.rows(lo, hi, H)
    assert idx.dtype == np.uint32 and wt.dtype == f32 and np.array_equal(idx, mi) and np.array_equal(wt.view(np.uint32), mw.view(np.uint32))
    assert idx.min() >= lo and idx.max() <= hi - 1 and wt.min() >= 0.0 and wt.max() <= 1.0 and (np.diff(idx.astype(np.int64)) >= 0).all()
    if H == hi - lo:                                                     # one picture row per line row: the rows themselves
        assert np.array_equal(idx, np.arange(lo, hi)) and not wt.any()


def test_rows_refuse(mcrt):
    L = mcrt.load_library()
    idx = np.full(4, 77, np.uint32); wt = np.full(4, -7.0, f32)
    call = lambda lo=0, hi=9, H=4, i=idx, w=wt: L.mcrt_mmode_rows(lo, hi, H, p(i), p(w))
    assert call(i=None) == INVALID and call(w=None) == INVALID and call(H=0) == INVALID and call(H=4097) == INVALID
    assert call(lo=9, hi=9) == INVALID and call(lo=10, hi=9) == INVALID and call(hi=0) == INVALID
    assert call(hi=2049) == LIMIT
    assert (idx == 77).all() and (wt == -7.0).all() and call() == 0 and (idx != 77).all()


# ------------------------------------------------------------------ the model, on the mirror
def anatomy(R, seed=0):
    """labels [1][1][R] in runs, with a label past a table of three and MCRT_LABEL_NONE among them"""
    rng = np.random.default_rng(seed)
    return np.repeat(rng.choice(np.array([0, 1, 2, 3, 255], np.uint8), size=R // 11 + 1), 11)[:R].reshape(1, 1, R)


def test_no_motion_is_the_envelope_of_the_line():
    """(a) all dilations 0, bulk 0, no noise: every pulse's env is sqrtf(re^2 + im^2) of the pre line, bit for bit, on finite input"""
    R, T = 300, 5
    iq = speckle(R, seed=1)
    for dil, w in (([0, 0, 0], mm.waveform(5.0, 60.0, T)), ([4194304, -4194304, 77], np.zeros(T, np.int32))):
        got = mm.lines(iq, anatomy(R), [[0, 0]], dil, w, np.zeros(T, np.int32), CARRIER)
        re, im = iq[0, 0, :, 0], iq[0, 0, :, 1]
        want = np.sqrt(((re * re).astype(f32) + (im * im).astype(f32)).astype(f32)).astype(f32)
        for t in range(T):
            assert np.array_equal(got["env"][0, t].view(np.uint32), want.view(np.uint32)), t
        assert not got["truth_disp"].any() and (got["truth_label"][0] == anatomy(R)[0, 0]).all()
        assert np.array_equal(got["iq_out"][0, 0], iq[0, 0])


@pytest.mark.parametrize("k", [1, -1, 7, -32, 32])
def test_a_bulk_of_whole_rows_shifts_the_line(k):
    """(b) bulk_q24[t] = k << 24: the pre line shifted by exactly k rows, zeros beyond its ends; the labels shifted, MCRT_LABEL_NONE beyond"""
    R, T = 100, 3
    iq = speckle(R, seed=2); tissue = anatomy(R, seed=2)
    b = np.array([0, k << 24, -(k << 24)], np.int32)
    got = mm.lines(iq, tissue, [[0, 0]], [0, 0, 0], np.full(T, 65536, np.int32), b, CARRIER)
    for t, s in ((0, 0), (1, k), (2, -k)):
        q = np.arange(R) + s
        ok = (q >= 0) & (q < R)
        want = np.where(ok[:, None], iq[0, 0][np.clip(q, 0, R - 1)], f32(0.0))
        assert np.array_equal(got["iq_out"][0, t], want), (t, s)
        assert np.array_equal(got["truth_label"][0, t], np.where(ok, tissue[0, 0][np.clip(q, 0, R - 1)], 255)), (t, s)
        assert (got["truth_disp"][0, t] == f32(s)).all()
        assert not got["env"][0, t][~ok].any()


def test_the_displacement_is_the_integer_sum_and_saturates():
    """(c) truth_disp is (D * w >> 16) + bulk of an independent int64 cumulative sum, clamped at +- 127 rows"""
    R, T = 2048, 6
    rng = np.random.default_rng(3)
    tissue = rng.choice(np.array([0, 1, 2, 3, 255], np.uint8), size=(1, 1, R))
    dil = np.array([4194304, -1000000, 4194304], np.int32)
    w = np.array([65536, -65536, 12345, 0, 1, -1], np.int32); b = np.array([0, 1 << 29, -(1 << 29), 5, -5, 1 << 24], np.int32)
    got = mm.lines(speckle(R, seed=3), tissue, [[0, 0]], dil, w, b, CARRIER)
    D = np.zeros(R, np.int64)
    for q in range(1, R):
        l = int(tissue[0, 0, q - 1])
        D[q] = D[q - 1] + (int(dil[l]) if l < 3 else 0)
    for t in range(T):
        u = [min(max(((int(D[q]) * int(w[t])) >> 16) + int(b[t]), -(127 << 24)), 127 << 24) for q in range(R)]
        want = (np.array(u, np.int32).astype(f32) * f32(2.0 ** -24)).astype(f32)
        assert np.array_equal(got["truth_disp"][0, t].view(np.uint32), want.view(np.uint32)), t
    assert got["truth_disp"][0, 0].max() == 127.0 and got["truth_disp"][0, 1].min() == -127.0      # the case saturates both ways


MEDIAN_ROWS, LARGEST_ROWS = 0.0033, 0.0191                # measured on the float32 mirror (the module's docstring)


def test_the_far_wall_of_a_pulsating_lumen_is_followed():
    """(d) the figure of merit: the energy centroid of the far wall's echo within +- 5 rows of its true position"""
    R, T, lo, hi = 465, 64, 200, 260
    iq = speckle(R, seed=4)
    iq[0, 0, lo:hi] *= f32(0.05)                                         # the lumen
    q = np.arange(R)
    for centre in (lo - 3, hi + 3):                                      # the walls, just outside it
        z = 40.0 * np.exp(-0.5 * ((q - centre) / 1.2) ** 2) * np.exp(2j * np.pi * CARRIER * q)
        iq[0, 0, :, 0] += z.real.astype(f32); iq[0, 0, :, 1] += z.imag.astype(f32)
    tissue = np.zeros((1, 1, R), np.uint8); tissue[0, 0, lo:hi] = 1
    got = mm.lines(iq, tissue, [[0, 0]], mm.mmode_table([0.0, -0.03]), mm.waveform(64.0, 60.0, T), np.zeros(T, np.int32), CARRIER)
    err = []
    for t in range(T):
        true = (hi + 3) - float(got["truth_disp"][0, t, hi + 3])        # the wall is read at q + U: it shows where q = centre - U
        win = np.abs(q - true) <= 5.0
        e = got["env"][0, t].astype(np.float64) ** 2
        err.append(abs(float((q[win] * e[win]).sum() / e[win].sum()) - true))
    moved = -float(got["truth_disp"][0, :, hi + 3].min())
    print("far wall: moved %.3f rows, median error %.4f rows, largest %.4f rows" % (moved, float(np.median(err)), max(err)))
    assert 1.79 < moved <= 1.8
    assert float(np.median(err)) <= 2.0 * MEDIAN_ROWS and max(err) <= 2.0 * LARGEST_ROWS
