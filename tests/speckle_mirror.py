"""numpy float32 mirror of mcrt_speckle_frames (include/mcrt.h): Yu & Acton's speckle-reducing anisotropic diffusion in its conservative
4-neighbour form.  Every multiply, add and divide is one float32 operation, in the contract's order.  The GPU tests feed it the product's own
table floats (mcrt_speckle_tables), as render_mirror is fed the view floats; tables() is the same double formulas in numpy."""
import numpy as np

f32 = np.float32
DEFAULTS = dict(n_iter=20, q0=float(f32(0.5227232)), rho=float(f32(1.0 / 6.0)), lambda_=0.5)


def tables(n_iter=20, q0=DEFAULTS["q0"], rho=DEFAULTS["rho"], lambda_=0.5):
    """q0sq [n_iter], kq [n_iter], lam4: double, each float rounded once (q0, rho, lambda_ are the struct's floats)"""
    q = np.float64(f32(q0)) * np.exp(-np.float64(f32(rho)) * np.arange(n_iter, dtype=np.float64))
    q2 = q * q
    return q2.astype(f32), (1.0 / (q2 * (1.0 + q2))).astype(f32), f32(0.25 * np.float64(f32(lambda_)))


def step(X, q0sq, kq, lam4):
    """one iteration on [..., H, W]"""
    N = np.concatenate([X[..., :1, :], X[..., :-1, :]], -2); S = np.concatenate([X[..., 1:, :], X[..., -1:, :]], -2)
    W = np.concatenate([X[..., :, :1], X[..., :, :-1]], -1); E = np.concatenate([X[..., :, 1:], X[..., :, -1:]], -1)
    with np.errstate(all="ignore"):
        dN, dS, dW, dE = N - X, S - X, W - X, E - X
        S1 = ((dN + dS) + dW) + dE
        S2 = ((dN * dN + dS * dS) + dW * dW) + dE * dE
        m = X + f32(0.25) * S1
        q2 = (f32(0.5) * S2 - f32(0.0625) * (S1 * S1)) / (m * m)
        c = np.fmin(np.fmax(f32(1.0) / (f32(1.0) + (q2 - f32(q0sq)) * f32(kq)), f32(0.0)), f32(1.0))
        cS = np.concatenate([c[..., 1:, :], c[..., -1:, :]], -2); cE = np.concatenate([c[..., :, 1:], c[..., :, -1:]], -1)
        D = ((c * dN + cS * dS) + c * dW) + cE * dE
        return (X + f32(lam4) * D).astype(f32)


def srad(frames, q0sq, kq, lam4):
    """[..., H, W] float32 -> the filtered stack; len(q0sq) iterations (none: the input's own bits)"""
    X = np.ascontiguousarray(frames, f32)
    if len(q0sq) == 0:
        return X.copy()
    X = np.where(np.isfinite(X), np.abs(X), f32(0.0)).astype(f32)
    for a, b in zip(q0sq, kq):
        X = step(X, a, b, lam4)
    return X
