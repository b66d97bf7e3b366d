"""numpy float32 mirror of mcrt_speckle_volume_frames (include/mcrt.h): the diffusion of speckle_mirror with six neighbours and a weight per
axis, over voxel blocks [..., nw, nv, nu].  Every multiply, add and divide is one float32 operation, in the contract's order.  The GPU tests
feed it the product's own table floats (mcrt_speckle3d_tables); tables() is the same double formulas in numpy."""
import numpy as np

import speckle_mirror as sm

f32 = np.float32
DEFAULTS = dict(sm.DEFAULTS, weights=(1.0, 1.0, 1.0))


def tables(n_iter=20, q0=DEFAULTS["q0"], rho=DEFAULTS["rho"], lambda_=0.5, weights=(1.0, 1.0, 1.0)):
    """q0sq [n_iter], kq [n_iter], k [4] = a, b, hs, lamw: double, each float rounded once (q0, rho, lambda_ and the weights are the struct's floats)"""
    q0sq, kq, _ = sm.tables(n_iter, q0, rho, lambda_)
    wu, wv, ww = (np.float64(f32(w)) for w in weights)
    sw = (wu + wv) + ww
    return q0sq, kq, np.array([1.0 / sw, 1.0 / (4.0 * sw * sw), 1.0 / (2.0 * sw), np.float64(f32(lambda_)) / (2.0 * sw)], np.float64).astype(f32)


def _lo(X, axis):
    """the neighbour at index - 1 along axis, clamped"""
    n = X.shape[axis]
    return np.take(X, np.maximum(np.arange(n) - 1, 0), axis)


def _hi(X, axis):
    """the neighbour at index + 1 along axis, clamped"""
    n = X.shape[axis]
    return np.take(X, np.minimum(np.arange(n) + 1, n - 1), axis)


def step(X, q0sq, kq, k, weights):
    """one iteration on [..., nw, nv, nu]"""
    wu, wv, ww = (f32(w) for w in weights)
    a, b, hs, lamw = (f32(v) for v in k)
    with np.errstate(all="ignore"):
        dN, dS, dW, dE, dD, dU = _lo(X, -2) - X, _hi(X, -2) - X, _lo(X, -1) - X, _hi(X, -1) - X, _lo(X, -3) - X, _hi(X, -3) - X
        gN, gS, gW, gE, gD, gU = wv * dN, wv * dS, wu * dW, wu * dE, ww * dD, ww * dU
        S1 = ((((gN + gS) + gW) + gE) + gD) + gU
        S2 = ((((gN * dN + gS * dS) + gW * dW) + gE * dE) + gD * dD) + gU * dU
        m = X + hs * S1
        q2 = (a * S2 - b * (S1 * S1)) / (m * m)
        c = np.fmin(np.fmax(f32(1.0) / (f32(1.0) + (q2 - f32(q0sq)) * f32(kq)), f32(0.0)), f32(1.0))
        D = ((((c * gN + _hi(c, -2) * gS) + c * gW) + _hi(c, -1) * gE) + c * gD) + _hi(c, -3) * gU
        return (X + lamw * D).astype(f32)


def srad3(blocks, q0sq, kq, k, weights):
    """[..., nw, nv, nu] float32 -> the filtered stack; len(q0sq) iterations (none: the input's own bits)"""
    X = np.ascontiguousarray(blocks, f32)
    assert X.ndim >= 3
    if len(q0sq) == 0:
        return X.copy()
    X = np.where(np.isfinite(X), np.abs(X), f32(0.0)).astype(f32)
    for s, t in zip(q0sq, kq):
        X = step(X, s, t, k, weights)
    return X
