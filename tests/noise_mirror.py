"""A numpy mirror of the receiver-noise stage (include/mcrt.h: mcrt_noise_draws, mcrt_noise_frames): a vectorised Philox4x32-10, the
integer draws, and the rule in np.float32 operations, one rounding each.  The tests hold the library to it bit for bit."""
import math
import numpy as np

f32 = np.float32
u32, u64 = np.uint32, np.uint64
STREAM = 0x4E4F4953                     # the counter's third word, and the default seed
OFFSET = 262140                         # 4 * 65535: the mean of the sum of eight 16-bit halves
VARIANCE = 2863311530                   # 8 * (65536^2 - 1) / 12, exactly
INV_STD = f32(1.0 / math.sqrt(float(VARIANCE)))
DEFAULTS = dict(snr_db=50.0, seed=STREAM)
M0, M1, W0, W1 = u64(0xD2511F53), u64(0xCD9E8D57), 0x9E3779B9, 0xBB67AE85
LOW = u64(0xFFFFFFFF)


def philox(ctr, key):
    """Philox4x32-10 over arrays: ctr = (c0, c1, c2, c3), key = (k0, k1), each an integer or an array that broadcasts -> four uint32 arrays"""
    c = [np.asarray(x, u64) & LOW for x in np.broadcast_arrays(*[np.asarray(x, u64) for x in ctr])]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                       # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> u64(32)) ^ c[1] ^ u64(k0), p1 & LOW, (p0 >> u64(32)) ^ c[3] ^ u64(k1), p0 & LOW]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [x.astype(u32) for x in c]


def draws(seed, image_id, E, R):
    """the draws d of one image, int32 [E][R]: the eight 16-bit halves of philox((e, r, STREAM, 0), (seed, image_id)) summed, minus OFFSET"""
    e, r = np.meshgrid(np.arange(E, dtype=u64), np.arange(R, dtype=u64), indexing="ij")
    o = philox((e, r, STREAM, 0), (seed, image_id))
    s = sum((x & u32(0xFFFF)).astype(np.int64) + (x >> u32(16)).astype(np.int64) for x in o)
    return (s - OFFSET).astype(np.int32)


def snr_factor(snr_db):
    """c of the contract: (float)pow(10.0, -(double)snr_db / 20.0) with snr_db a float"""
    return f32(math.pow(10.0, -float(f32(snr_db)) / 20.0))


def noise(stack, first_id=0, opts=None, gain=None):
    """the rule over stack [F][N][E][R] -> (out, sigma [F]).  opts: a dict of snr_db= or sigma= (giving sigma selects the absolute mode) and
    seed=; None: the defaults.  gain: [E] or None"""
    o = dict(opts or {})
    seed = o.pop("seed", None)
    seed = STREAM if seed is None else seed
    absolute = o.get("sigma") is not None
    assert not (absolute and o.get("snr_db") is not None)
    x = np.ascontiguousarray(stack, f32)
    F, N, E, R = x.shape
    out = np.empty_like(x)
    sigma = np.empty(F, f32)
    g = None if gain is None else np.ascontiguousarray(gain, f32).reshape(1, E, 1)
    with np.errstate(all="ignore"):
        for f in range(F):
            if absolute:
                sigma[f] = f32(o["sigma"])
            else:
                a = np.abs(x[f])
                peak = f32(np.where(np.isfinite(a), a, f32(0.0)).max())
                snr = o.get("snr_db")
                sigma[f] = peak * snr_factor(DEFAULTS["snr_db"] if snr is None else snr)
            k = f32(sigma[f] * INV_STD)
            u = x[f] if g is None else (x[f] * g).astype(f32)
            if k == f32(0.0):
                out[f] = u
                continue
            d = np.stack([draws(seed, (first_id + f * N + i) & 0xFFFFFFFF, E, R) for i in range(N)])
            out[f] = u + (d.astype(f32) * k).astype(f32)
    return out, sigma
