"""numpy restatement of libdkt_gpc.so's two calls (include/dkt_abi_gpc.h), i.e. of scikit-learn's binary Laplace GPC (`_gpc.py`: `_posterior_mode`,
`predict_proba`, and `OneVsRestClassifier.predict`), with a `dtype` argument, plus the clustered-feature generator of the Laplace tests.

dtype=float64 is the reference (equal to sklearn to 1e-12, tests/test_laplace_host.py).  dtype=float32 models the KERNEL: every array and every
operation fp32 except the five-term mixture, which is summed in float64 from the fp32 mean and variance.  Its distance from the float64 result
is the fp32 floor the GPU tests scale their tolerances from."""
import numpy as np
from scipy.linalg import cho_solve, cholesky, solve_triangular
from scipy.special import erf, expit

LAMBDAS = np.array([0.41, 0.4, 0.37, 0.44, 0.39])[:, np.newaxis]
COEFS = np.array([-1854.8214151, 3516.89893646, 221.29346712, 128.12323805, -2010.49422654])[:, np.newaxis]


def clustered(rng, c, shots, m, d, spread):
    """Unit-norm class centres + spread * N(0,1) / sqrt(D), renormalised: support [c * shots, d] (class-major), queries [m, d] (classes in turn), float64."""
    centres = rng.standard_normal((c, d))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)

    def draw(cls):
        z = centres[cls] + spread * rng.standard_normal((len(cls), d)) / np.sqrt(d)
        return z / np.linalg.norm(z, axis=1, keepdims=True)

    return draw(np.repeat(np.arange(c), shots)), draw(np.arange(m) % c)


def rbf(a, b, lengthscale):
    d2 = (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * a @ b.T
    return np.exp(-0.5 * np.maximum(d2, 0.0) / lengthscale ** 2)


def one_vs_rest(c, shots):
    """Targets [C, N] in {0,1}; C == 1 stands for the binary problem with class 1 positive."""
    cls = np.repeat(np.arange(max(c, 2)), shots)
    return (cls[None, :] == (np.arange(c)[:, None] if c > 1 else 1)).astype(np.float64)


def mode_one(k, y, max_iter=100, dtype=np.float64):
    """`_posterior_mode` for one binary problem: dict(f, g, w_sr, chol, lml, iters)."""
    k, y = np.asarray(k, dtype), np.asarray(y, dtype)
    n = y.shape[0]
    f = np.zeros(n, dtype)
    lml_prev = dtype(-np.inf)
    half, one, two, tol = dtype(0.5), dtype(1), dtype(2), dtype(1e-10)
    iters = 0
    for _ in range(max_iter):
        pi = expit(f)
        w = pi * (one - pi)
        w_sr = np.sqrt(w)
        w_sr_k = w_sr[:, None] * k
        chol = cholesky(np.eye(n, dtype=dtype) + w_sr_k * w_sr, lower=True)
        b = w * f + (y - pi)
        a = b - w_sr * cho_solve((chol, True), w_sr_k.dot(b))
        f = k.dot(a)
        z = (y * two - one) * f
        lml = -half * a.dot(f) - (np.maximum(-z, 0) + np.log1p(np.exp(-np.abs(z)))).sum() - np.log(np.diag(chol)).sum()
        assert lml.dtype == dtype and f.dtype == dtype and chol.dtype == dtype
        iters += 1
        if lml - lml_prev < tol:
            break
        lml_prev = lml
    return dict(f=f, g=y - pi, w_sr=w_sr, chol=np.tril(chol), lml=lml_prev, iters=iters)


def mode(k, y, max_iter=100, dtype=np.float64):
    """k [B,N,N] or [B,C,N,N], y [C,N] or [B,C,N] -> dict of arrays stacked [B,C,...]."""
    k, y = np.asarray(k), np.asarray(y)
    b_, c = k.shape[0], y.shape[-2]
    outs = [[mode_one(k[b] if k.ndim == 3 else k[b, ci], y[ci] if y.ndim == 2 else y[b, ci], max_iter, dtype) for ci in range(c)] for b in range(b_)]
    return {key: np.array([[o[key] for o in row] for row in outs]) for key in outs[0][0]}


def predict(ks, kss, md, dtype=np.float64):
    """ks [B,M,N] or [B,C,M,N], kss [B,M] or [B,C,M], md of mode() -> mu, var, prob [B,C,M], labels [B,M] (last maximum wins; C == 1: mu > 0)."""
    ks, kss = np.asarray(ks, dtype), np.asarray(kss, dtype)
    b_, c = md["g"].shape[:2]
    m = ks.shape[-2]
    mu, var = np.zeros((b_, c, m), dtype), np.zeros((b_, c, m), dtype)
    for b in range(b_):
        for ci in range(c):
            k_star = (ks[b] if ks.ndim == 3 else ks[b, ci]).T                                     # [N, M]
            mu[b, ci] = k_star.T.dot(md["g"][b, ci].astype(dtype))
            v = solve_triangular(md["chol"][b, ci].astype(dtype), md["w_sr"][b, ci].astype(dtype)[:, None] * k_star, lower=True)
            var[b, ci] = (kss[b] if kss.ndim == 2 else kss[b, ci]) - np.einsum("ij,ij->j", v, v)
    assert mu.dtype == dtype and var.dtype == dtype
    mu64, var64 = mu.astype(np.float64).reshape(1, -1), var.astype(np.float64).reshape(1, -1)
    alpha = 1 / (2 * var64)
    integrals = np.sqrt(np.pi / alpha) * erf(LAMBDAS * mu64 * np.sqrt(alpha / (alpha + LAMBDAS ** 2))) / (2 * np.sqrt(var64 * 2 * np.pi))
    prob = ((COEFS * integrals).sum(axis=0) + 0.5 * COEFS.sum()).reshape(b_, c, m)
    if c == 1:
        labels = (mu[:, 0] > 0).astype(np.int32)
    else:
        labels = np.zeros((b_, m), np.int32)
        best = np.full((b_, m), -np.inf)
        for ci in range(c):
            take = prob[:, ci] >= best
            best = np.where(take, prob[:, ci], best)
            labels[take] = ci
    return mu, var, prob.astype(dtype), labels          # (the labels come from the unrounded sum, as in the kernel)


# (B, C, N = C * shots, M, D, spread, lengthscale): the shapes of the baseline configurations' test-time support sets + a dense-K case
CASES = [(1, 5, 5, 80, 64, 0.08, 0.1), (3, 5, 25, 80, 64, 0.08, 0.1), (2, 5, 25, 80, 1600, 0.1, 0.1), (2, 20, 100, 100, 64, 0.1, 0.1),
         (2, 5, 125, 15, 64, 0.1, 0.1), (2, 5, 25, 80, 64, 0.5, 1.0)]
NEAR_IDENTITY_CASE = (2, 5, 25, 80, 64, 0.3, 0.1)          # top-two margins of 4e-7 .. 5e-5: a probability case, never a label case


def build_case(case, seed=0):
    """Episodes of a case: support / query features (float64) and the fp32-representable K [B,N,N], Ks [B,M,N], kss [B,M], Y [C,N] every
    implementation is given (so that the comparison is about the algorithm, not about the rounding of its input)."""
    b_, c, n, m, d, spread, ls = case
    rng = np.random.default_rng(seed + 1000 * n + m)
    zs, zq = zip(*(clustered(rng, c, n // c, m, d, spread) for _ in range(b_)))
    k = np.stack([rbf(z, z, ls) for z in zs]).astype(np.float32).astype(np.float64)
    ks = np.stack([rbf(q, z, ls) for z, q in zip(zs, zq)]).astype(np.float32).astype(np.float64)
    return dict(zs=np.stack(zs), zq=np.stack(zq), k=k, ks=ks, kss=np.ones((b_, m)), y=one_vs_rest(c, n // c))
