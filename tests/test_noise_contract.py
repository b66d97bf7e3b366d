"""Receiver noise without a GPU (include/mcrt.h: mcrt_noise_opts, mcrt_default_noise_opts, mcrt_noise_draws, mcrt_noise_frames): the numpy
Philox of tests/noise_mirror.py against the Random123 known answers and the oracle's, the host's draws against the mirror's exactly, the
statistics of the draws at bounds of five standard errors, the struct and its defaults, every refusal that needs no device, and the
mirror's own identity cases, which hold tests/test_gpu_noise.py honest."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest

import noise_mirror as nm

f32 = np.float32
INVALID, LIMIT = -1, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONES = 0xFFFFFFFF


# ------------------------------------------------------------------ the Philox mirror
def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32_10"""
    zero = [int(x) for x in nm.philox((0, 0, 0, 0), (0, 0))]
    ones = [int(x) for x in nm.philox((ONES, ONES, ONES, ONES), (ONES, ONES))]
    assert zero == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert ones == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]


def test_philox_equals_the_oracles(orc):
    rng = np.random.default_rng(20)
    ctr = rng.integers(0, 1 << 32, (100, 4), dtype=np.uint64)
    key = rng.integers(0, 1 << 32, (100, 2), dtype=np.uint64)
    for c, k in zip(ctr, key):
        got = np.array([int(x) for x in nm.philox(tuple(int(v) for v in c), (int(k[0]), int(k[1])))], np.uint32)
        assert np.array_equal(got, orc.philox(c.astype(np.uint32), k.astype(np.uint32))), (c, k)
    # vectorised over the counters under one key: the same numbers
    o = nm.philox((ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3]), (7, 9))
    for i in (0, 57, 99):
        assert [int(x[i]) for x in o] == [int(v) for v in orc.philox(ctr[i].astype(np.uint32), np.array([7, 9], np.uint32))]


# ------------------------------------------------------------------ the draws
SHAPES = [(1, 1), (1, 5), (3, 1), (7, 257), (512, 465)]
SEEDS = (nm.STREAM, 0x5EED)
IDS = (0, 1, ONES)


@pytest.mark.parametrize("E,R", SHAPES)
def test_host_draws_equal_the_mirrors(mcrt, E, R):
    seen = []
    for seed in SEEDS:
        for image_id in IDS:
            d = mcrt.host_noise_draws(seed, image_id, E, R)
            assert d.dtype == np.int32 and d.shape == (E, R)
            assert np.array_equal(d, nm.draws(seed, image_id, E, R)), (seed, image_id)
            assert np.abs(d.astype(np.int64)).max() <= nm.OFFSET
            seen.append(d)
    if E * R >= 5:                                               # other ids or seeds give other arrays
        for i in range(len(seen)):
            for j in range(i):
                assert not np.array_equal(seen[i], seen[j]), (i, j)


def test_a_draw_by_hand(mcrt, orc):
    """one sample spelled out: the counter (e, r, 0x4E4F4953, 0), the key (seed, id), the eight halves summed"""
    e, r, seed, image_id = 5, 300, 0xABCDEF01, 77
    o = orc.philox(np.array([e, r, 0x4E4F4953, 0], np.uint32), np.array([seed, image_id], np.uint32))
    s = sum((int(w) & 0xFFFF) + (int(w) >> 16) for w in o)
    assert mcrt.host_noise_draws(seed, image_id, 8, 301)[e, r] == s - 262140
    assert nm.OFFSET == 4 * 65535 and nm.VARIANCE == 8 * (65536 ** 2 - 1) // 12 and 8 * (65536 ** 2 - 1) % 12 == 0


@pytest.mark.parametrize("image_id", [0, 1])
def test_statistics_of_the_draws(mcrt, image_id):
    """z = d / sqrt(2863311530) at 512 x 465 (n = 238 080), every bound five standard errors of its estimator under the rule's own
    distribution: the mean's is 1/sqrt(n), the variance's sqrt(2/n) and the excess kurtosis' sqrt(24/n) (the normal values; the
    Irwin-Hall sum of 8 has excess kurtosis -6/(5*8) = -0.15, which makes the true errors a little smaller), a lag-1 correlation's
    1/sqrt(n)"""
    E, R = 512, 465
    n = E * R
    z = mcrt.host_noise_draws(nm.STREAM, image_id, E, R).astype(np.float64) / np.sqrt(float(nm.VARIANCE))
    mean, var = z.mean(), z.var()
    kurt = ((z - mean) ** 4).mean() / var ** 2 - 3.0
    rows = np.corrcoef(z[:, :-1].ravel(), z[:, 1:].ravel())[0, 1]
    lines = np.corrcoef(z[:-1].ravel(), z[1:].ravel())[0, 1]
    print("id %d: mean %.4f variance %.4f lag-1 rows %.4f scan-lines %.4f excess kurtosis %.4f" % (image_id, mean, var, rows, lines, kurt))
    assert abs(mean) < 5.0 / np.sqrt(n)
    assert abs(var - 1.0) < 5.0 * np.sqrt(2.0 / n)
    assert abs(rows) < 5.0 / np.sqrt(n) and abs(lines) < 5.0 / np.sqrt(n)
    assert abs(kurt - (-0.15)) < 5.0 * np.sqrt(24.0 / n)
    assert np.abs(z).max() <= 262140.0 / np.sqrt(float(nm.VARIANCE)) < 4.9


# ------------------------------------------------------------------ struct, defaults, header, errors
def test_struct_defaults_and_header(mcrt):
    O = mcrt.NoiseOpts
    assert C.sizeof(O) == 16 and [getattr(O, n).offset for n in ("mode", "snr_db", "sigma", "seed")] == [0, 4, 8, 12]
    L = mcrt.load_library()
    o = O()
    C.memset(C.byref(o), 0xA5, 16)
    assert L.mcrt_default_noise_opts(C.byref(o)) == 0
    assert (o.mode, o.snr_db, o.sigma, o.seed) == (mcrt.NOISE_SNR_DB, 50.0, 0.0, 0x4E4F4953)
    assert nm.DEFAULTS == dict(snr_db=o.snr_db, seed=o.seed) and (mcrt.NOISE_SNR_DB, mcrt.NOISE_ABS) == (0, 1)
    assert L.mcrt_default_noise_opts(None) == INVALID and b"null" in L.mcrt_last_error()
    d = mcrt.noise_opts_struct()
    assert (d.mode, d.snr_db, d.sigma, d.seed) == (o.mode, o.snr_db, o.sigma, o.seed)
    a = mcrt.noise_opts_struct(sigma=0.25, seed=9)
    assert (a.mode, a.sigma, a.seed) == (mcrt.NOISE_ABS, 0.25, 9)
    s = mcrt.noise_opts_struct(snr_db=30)
    assert (s.mode, s.snr_db, s.seed) == (mcrt.NOISE_SNR_DB, 30.0, o.seed)
    with pytest.raises(ValueError):
        mcrt.noise_opts_struct(snr_db=30.0, sigma=0.25)
    with pytest.raises(TypeError):
        mcrt.noise_opts_struct(db=30.0)
    src = open(os.path.join(ROOT, "include", "mcrt.h")).read()
    assert "#define MCRT_VERSION 109 " in src
    block = src[src.index("#define MCRT_VERSION"):src.index("typedef enum")]
    added = block[block.index("mcrt_noise_opts"):]
    for name in ("mcrt_noise_opts", "mcrt_default_noise_opts", "mcrt_noise_draws", "mcrt_noise_frames", "receiver noise", "additive"):
        assert name in added, name
    for name in ("mcrt_default_noise_opts", "mcrt_noise_draws", "mcrt_noise_frames"):
        assert re.search(r"\bint " + name + r"\(", src) and hasattr(L, name) and name in mcrt._lib.SYMBOLS, name
    assert "MCRT_NOISE_SNR_DB = 0" in src and re.search(r"MCRT_NOISE_ABS\s+= 1", src)
    # the call without a context is refused before anything else is looked at
    assert L.mcrt_noise_frames(None, None, 1, 1, 1, 1, 0, None, None, None) == INVALID and b"null context" in L.mcrt_last_error()


def test_draws_errors_write_nothing(mcrt):
    L = mcrt.load_library()
    d = np.full((4, 2049), -12345, np.int32)
    p = d.ctypes.data_as(C.c_void_p)
    for args, code, word in (((1, 2, 3, 4, None), INVALID, b"null d"), ((1, 2, 0, 4, p), INVALID, b"n_elements"), ((1, 2, 3, 0, p), INVALID, b"n_rows"),
                             ((1, 2, 0, 0, p), INVALID, b"zero"), ((1, 2, 4, 2049, p), LIMIT, b"n_rows")):
        assert L.mcrt_noise_draws(*args) == code, args
        assert word in L.mcrt_last_error(), (args, L.mcrt_last_error())
    assert (d == -12345).all()
    assert L.mcrt_noise_draws(1, 2, 4, 2048, p) == 0                     # the limit itself is fine, and writes [E][R] and no more
    flat = d.reshape(-1)
    assert np.array_equal(flat[:4 * 2048].reshape(4, 2048), nm.draws(1, 2, 4, 2048)) and (flat[4 * 2048:] == -12345).all()


# ------------------------------------------------------------------ the kernel's resources
def test_k_noise_uses_no_scratch_and_no_lds():
    """the compiler's own report for k_noise (its translation unit alone): nothing spilled, no scratch, no LDS, full occupancy"""
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "mcray-tracing_amd"), "resources", "KERNELS=mcrt_noise"], capture_output=True, text=True).stderr
    blocks = [b for b in out.split("Function Name: ") if b.startswith("_ZN4mcrt7k_noiseE")]
    assert len(blocks) == 1, out[-2000:]
    val = lambda key: int(re.search(key + r": (\d+)", blocks[0]).group(1))
    assert val("VGPRs Spill") == 0 and val("SGPRs Spill") == 0 and val(r"ScratchSize \[bytes/lane\]") == 0, blocks[0][:900]
    assert val(r"LDS Size \[bytes/block\]") == 0 and val(r"Occupancy \[waves/SIMD\]") == 8, blocks[0][:900]


# ------------------------------------------------------------------ the mirror's identity cases
def _stack(F, N, E, R):
    rng = np.random.default_rng(E * 1000 + R)
    x = (rng.standard_normal((F, N, E, R)) * 3.0).astype(f32)
    flat = x.reshape(-1)
    flat[:6] = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-30], f32)
    return x


def test_mirror_identities():
    x = _stack(2, 3, 5, 9)
    out, sigma = nm.noise(x, 4, dict(sigma=0.0))
    assert np.array_equal(out.view(np.uint32), x.view(np.uint32)) and (sigma == 0).all()          # the input's bits, NaN and -0.0 included
    g = np.array([0.0, 1.0, 0.5, -2.0, 1.0], f32)
    z = np.zeros((2, 1, 5, 9), f32); z[0, 0, 2, 3] = -0.0
    out, sigma = nm.noise(z, 0, dict(snr_db=30.0), g)
    assert (sigma == 0).all() and np.array_equal(out.view(np.uint32), (z * g.reshape(1, 1, 5, 1)).view(np.uint32))   # a zero frame: u
    # SNR_DB: each frame's sigma is its own peak's, NaN and inf are no peak, and the noise has that deviation
    x = _stack(2, 1, 64, 465)
    x[1] *= f32(4.0)
    out, sigma = nm.noise(x, 0, dict(snr_db=20.0))
    for f in range(2):
        fin = np.isfinite(x[f])
        assert sigma[f] == f32(np.abs(x[f][fin]).max()) * nm.snr_factor(20.0)
        diff = (out[f][fin].astype(np.float64) - x[f][fin]) / float(sigma[f])
        assert abs(diff.std() - 1.0) < 0.02 and abs(diff.mean()) < 0.02
        assert np.array_equal(np.isnan(out[f]), np.isnan(x[f])) and np.array_equal(np.isinf(out[f]), np.isinf(x[f]))
    # image j of the stack has id first_id + j: a stack is its images one by one
    x = _stack(2, 3, 4, 7)
    whole, _ = nm.noise(x, 5, dict(sigma=0.5, seed=3))
    for j in range(6):
        one, _ = nm.noise(x.reshape(6, 1, 4, 7)[j:j + 1], 5 + j, dict(sigma=0.5, seed=3))
        assert np.array_equal(one.view(np.uint32), whole.reshape(6, 1, 4, 7)[j:j + 1].view(np.uint32))
