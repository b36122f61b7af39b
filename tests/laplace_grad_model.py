"""numpy restatement of `dkt_laplace_grad_f32` (include/dkt_abi.h): the Laplace approximation of the log marginal likelihood of a binary GP
classifier and its gradient with respect to the prior covariance (GPML algorithm 5.1 in matrix form), with a `dtype` argument like
tests/laplace_model.py, which supplies the mode.

Everything is evaluated AT the mode f_hat that is handed in (pi, W, g, L are recomputed from it), not from the Newton loop's temporaries:

    pi = sigma(f),  W = pi (1 - pi),  g = y - pi,  L = chol(I + W^1/2 K W^1/2)
    lml = -1/2 g^T f - sum log(1 + exp(-(2y - 1) f)) - sum log L_ii
    R  = W^1/2 (I + W^1/2 K W^1/2)^-1 W^1/2
    s2 = -1/2 (diag K - diag(K R K)) * pi (1 - pi) (1 - 2 pi)
    u  = s2 - R (K s2)
    G  = d lml / d K = 1/2 (g g^T - R) + 1/2 (u g^T + g u^T)

dtype=float64 is the reference; dtype=float32 models the kernel (every array and operation fp32): its distance from the float64 result is the fp32
floor the GPU tests scale their tolerances from."""
import numpy as np
from scipy.linalg import cholesky, solve_triangular
from scipy.special import expit

import laplace_model as lm


def polish(k, y, f, steps=50):
    """Newton steps on a float64 mode until it is a fixed point to rounding (the stopping test of `mode_one` leaves |f - K g| ~ 1e-6)."""
    k, y, f = np.asarray(k, np.float64), np.asarray(y, np.float64), np.asarray(f, np.float64).copy()
    n = y.shape[0]
    for _ in range(steps):
        pi = expit(f)
        w = pi * (1 - pi)
        w_sr = np.sqrt(w)
        b = w * f + (y - pi)
        bm = np.eye(n) + w_sr[:, None] * k * w_sr
        a = b - w_sr * np.linalg.solve(bm, w_sr * k.dot(b))
        f_new = k.dot(a)
        done = np.abs(f_new - f).max() < 1e-15 * max(1.0, np.abs(f).max())
        f = f_new
        if done:
            break
    return f


def mode_polished(k, y, max_iter=100):
    """The float64 mode of one binary problem, polished."""
    return polish(k, y, lm.mode_one(k, y, max_iter)["f"])


def lml_at(k, y, f, dtype=np.float64):
    """The approximate log marginal likelihood at f (the formula above)."""
    return grad_one(k, y, f, dtype)[0]


def grad_one(k, y, f, dtype=np.float64):
    """One binary problem with prior covariance k [N,N]: (lml, G [N,N])."""
    k, y, f = np.asarray(k, dtype), np.asarray(y, dtype), np.asarray(f, dtype)
    n = y.shape[0]
    half, one, two = dtype(0.5), dtype(1), dtype(2)
    pi = expit(f)
    w = pi * (one - pi)
    w_sr = np.sqrt(w)
    g = y - pi
    chol = cholesky(np.eye(n, dtype=dtype) + (w_sr[:, None] * k) * w_sr, lower=True)
    z = (y * two - one) * f
    lml = -half * g.dot(f) - (np.maximum(-z, 0) + np.log1p(np.exp(-np.abs(z)))).sum() - np.log(np.diag(chol)).sum()
    t = solve_triangular(chol, np.eye(n, dtype=dtype), lower=True)          # L^-1
    r = (w_sr[:, None] * (t.T.dot(t))) * w_sr
    krk = np.einsum("ij,ij->i", k.dot(r), k)
    s2 = -half * (np.diag(k) - krk) * (w * (one - two * pi))
    u = s2 - r.dot(k.dot(s2))
    gm = half * (np.outer(g, g) - r) + half * (np.outer(u, g) + np.outer(g, u))
    assert gm.dtype == dtype and lml.dtype == dtype
    return lml, gm


def laplace_grad(k, y, f_hat, cls_weight, scale=None, dtype=np.float64):
    """The call: k [B,N,N] (shared; class stride 0) or [B,C,N,N], y [C,N] or [B,C,N] in {0,1}, f_hat [B,C,N], cls_weight [C], scale [C] or None (the
    covariance of problem (b, c) is scale[c] * k) -> lml [B,C] (unweighted), dK ([B,N,N]: sum over the classes in index order; or [B,C,N,N]) =
    cls_weight[c] * scale[c] * G_c, dscale [B,C] = cls_weight[c] * <G_c, k>."""
    k, y, f_hat = np.asarray(k, dtype), np.asarray(y, dtype), np.asarray(f_hat, dtype)
    b_, c_, n = f_hat.shape
    cw = np.asarray(cls_weight, dtype)
    sc = np.ones(c_, dtype) if scale is None else np.asarray(scale, dtype)
    shared = k.ndim == 3
    lml = np.zeros((b_, c_), dtype)
    dscale = np.zeros((b_, c_), dtype)
    dk = np.zeros((b_, n, n) if shared else (b_, c_, n, n), dtype)
    for b in range(b_):
        for c in range(c_):
            kb = k[b] if shared else k[b, c]
            lml[b, c], gm = grad_one(sc[c] * kb, y[c] if y.ndim == 2 else y[b, c], f_hat[b, c], dtype)
            dscale[b, c] = cw[c] * (gm * kb).sum()
            if shared:
                dk[b] = dk[b] + (cw[c] * sc[c]) * gm
            else:
                dk[b, c] = (cw[c] * sc[c]) * gm
    assert dk.dtype == dtype and lml.dtype == dtype and dscale.dtype == dtype
    return lml, dk, dscale


def modes(k, y, scale=None, max_iter=100):
    """Polished float64 modes f [B,C,N] of the problems of a call (k, y, scale as in `laplace_grad`)."""
    k, y = np.asarray(k, np.float64), np.asarray(y, np.float64)
    b_, c_ = k.shape[0], y.shape[-2]
    sc = np.ones(c_) if scale is None else np.asarray(scale, np.float64)
    return np.array([[mode_polished(sc[c] * (k[b] if k.ndim == 3 else k[b, c]), y[c] if y.ndim == 2 else y[b, c], max_iter) for c in range(c_)]
                     for b in range(b_)])
