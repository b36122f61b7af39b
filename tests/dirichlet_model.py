"""numpy restatement of `dkt_mll_rownoise_f32` and `dkt_dirichlet_proba_f32` (include/dkt_abi.h; docs/DIRICHLET.md), written from the formulas of
Milios et al., "Dirichlet-based Gaussian Processes for Large-scale Calibrated Classification" (NeurIPS 2018), with a `dtype` argument like
tests/laplace_grad_model.py.

    a = alpha_eps + [y is the class],  sigma^2 = log(1 / a + 1),  ytilde = log a - sigma^2 / 2          (the log-normal match of a Gamma(a, 1) marginal)
    K = sv E + diag(sigma^2),  r = ytilde - mean,  L = chol(K),  alpha = K^-1 r
    logp = -1/2 r.alpha - sum log L_ii - N/2 log 2 pi
    G = d logp / d K = 1/2 (alpha alpha^T - K^-1);   d logp / d sv = <G, E>,   d logp / d mean = sum alpha
    prob[q, c] = 1/S sum_s softmax_c(mu[c, q] + sqrt(max(var[c, q], 0)) eps[s, c])

dtype=float64 is the reference; dtype=float32 models the kernels (every array and operation fp32): its distance from the float64 result is the fp32
floor the GPU tests scale their tolerances from."""
import numpy as np
from scipy.linalg import cholesky, solve_triangular


def dirichlet_targets(y_pm1, alpha_eps=0.01, dtype=np.float64):
    """+-1 one-vs-rest labels -> (ytilde, noise_rows), same shape."""
    a = dtype(alpha_eps) + (np.asarray(y_pm1) > 0).astype(dtype)
    noise = np.log(dtype(1) / a + dtype(1))
    return np.log(a) - noise * dtype(0.5), noise


def one(e, y, noise_rows, sv, mean, dtype=np.float64, want_grad=True):
    """One problem: E [N,N], y and noise_rows [N], scalars sv, mean -> dict(logp, alpha, chol, info[, g])."""
    e, y, nr = np.asarray(e, dtype), np.asarray(y, dtype), np.asarray(noise_rows, dtype)
    n = y.shape[0]
    k = dtype(sv) * e + np.diag(nr)
    r = y - dtype(mean)
    try:
        if not np.isfinite(k).all():
            raise np.linalg.LinAlgError
        chol = cholesky(k, lower=True)
    except np.linalg.LinAlgError:
        nan = np.full((n, n), np.nan, dtype)
        return dict(logp=dtype(np.nan), alpha=nan[0], chol=nan, g=nan, info=1)
    t = solve_triangular(chol, r, lower=True)
    alpha = solve_triangular(chol, t, lower=True, trans="T")
    logp = dtype(-0.5) * t.dot(t) - np.log(np.diag(chol)).sum() - dtype(n) * dtype(0.5 * np.log(2 * np.pi))
    out = dict(logp=logp, alpha=alpha, chol=chol, info=0)
    if want_grad:
        li = solve_triangular(chol, np.eye(n, dtype=dtype), lower=True)
        out["g"] = dtype(0.5) * (np.outer(alpha, alpha) - li.T.dot(li))
        assert out["g"].dtype == dtype
    assert logp.dtype == dtype and alpha.dtype == dtype and chol.dtype == dtype
    return out


def mll_rownoise(e, y, noise_rows, sv, mean, cls_weight=None, dtype=np.float64):
    """The call: e [B,N,N] (shared; class stride 0) or [B,C,N,N]; y, noise_rows [C,N] or [B,C,N]; sv, mean [C]; cls_weight [C] or None (= 1) ->
    dict(logp [B,C], alpha [B,C,N], de ([B,N,N]: summed over the classes in index order; or [B,C,N,N]), dsv, dmean [B,C], chol [B,C,N,N], info [B,C])."""
    e, y, nr = np.asarray(e, dtype), np.asarray(y, dtype), np.asarray(noise_rows, dtype)
    sv, mean = np.asarray(sv, dtype), np.asarray(mean, dtype)
    b_, n = e.shape[0], e.shape[-1]
    c_ = y.shape[-2]
    cw = np.ones(c_, dtype) if cls_weight is None else np.asarray(cls_weight, dtype)
    shared = e.ndim == 3
    o = dict(logp=np.zeros((b_, c_), dtype), alpha=np.zeros((b_, c_, n), dtype), de=np.zeros((b_, n, n) if shared else (b_, c_, n, n), dtype),
             dsv=np.zeros((b_, c_), dtype), dmean=np.zeros((b_, c_), dtype), chol=np.zeros((b_, c_, n, n), dtype), info=np.zeros((b_, c_), np.int32))
    for b in range(b_):
        for c in range(c_):
            eb = e[b] if shared else e[b, c]
            p = one(eb, y[c] if y.ndim == 2 else y[b, c], nr[c] if nr.ndim == 2 else nr[b, c], sv[c], mean[c], dtype)
            o["logp"][b, c], o["alpha"][b, c], o["chol"][b, c], o["info"][b, c] = p["logp"], p["alpha"], p["chol"], p["info"]
            o["dsv"][b, c] = cw[c] * (p["g"] * eb).sum()
            o["dmean"][b, c] = cw[c] * p["alpha"].sum()
            if shared:
                o["de"][b] = o["de"][b] + (cw[c] * sv[c]) * p["g"]
            else:
                o["de"][b, c] = (cw[c] * sv[c]) * p["g"]
    assert all(o[q].dtype == dtype for q in ("logp", "alpha", "de", "dsv", "dmean", "chol"))
    return o


def proba(mu, var, eps, dtype=np.float64):
    """mu, var [B,C,M], eps [S,C] -> (prob [B,M,C], labels [B,M]: argmax_c mu, the first maximum)."""
    mu, var, eps = np.asarray(mu, dtype), np.asarray(var, dtype), np.asarray(eps, dtype)
    sd = np.sqrt(np.maximum(var, dtype(0)))
    acc = np.zeros((mu.shape[0], mu.shape[2], mu.shape[1]), dtype)
    for s in range(eps.shape[0]):                                            # s in index order
        f = (mu + sd * eps[s][None, :, None]).transpose(0, 2, 1)
        ex = np.exp(f - f.max(-1, keepdims=True))
        acc = acc + ex / ex.sum(-1, keepdims=True)
    prob = acc / dtype(eps.shape[0])
    assert prob.dtype == dtype
    return prob, np.argmax(mu, 1).astype(np.int32)


def predict(e, ex, exx, y, noise_rows, sv, mean, dtype=np.float64):
    """Latent posterior at the queries: e [N,N], ex [M,N], exx [M] -> (mu [C,M], var [C,M]); y, noise_rows [C,N]; sv, mean [C]."""
    ex, exx = np.asarray(ex, dtype), np.asarray(exx, dtype)
    mu, var = [], []
    for c in range(len(sv)):
        p = one(e, y[c], noise_rows[c], sv[c], mean[c], dtype, want_grad=False)
        v = solve_triangular(p["chol"], (dtype(sv[c]) * ex).T, lower=True)
        mu.append(dtype(mean[c]) + dtype(sv[c]) * ex.dot(p["alpha"]))
        var.append(dtype(sv[c]) * exx - (v * v).sum(0))
    return np.stack(mu), np.stack(var)


# ---- the case list of tests/test_dirichlet_gpu.py (built here so that test_dirichlet_host.py can state its float32 floors and label margins on the CPU) ----
QUANTITIES = ("logp", "alpha", "de", "dsv", "dmean", "chol")
# (B, C, N): 1, the 16-lane / wave / two-rows-per-lane boundaries of the kernel (15 16 17, 33, 63 64 65), its largest size, the 5-way 5-shot episode
SHAPES = [(1, 1, 1), (2, 5, 15), (2, 5, 16), (2, 5, 17), (1, 5, 33), (1, 2, 63), (1, 2, 64), (1, 2, 65), (1, 3, 127), (3, 5, 25)]
PROBA_SHAPES = [(1, 1, 1, 1), (2, 5, 80, 256), (1, 20, 65, 33)]              # (B, C, M, S)


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def unit_rows(rng, c, shots, d=64, spread=0.6):
    """Unit-norm class centres + spread * N(0,1) / sqrt(D), renormalised, class-major [c * shots, d]."""
    centres = rng.standard_normal((c, d))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    z = centres[np.repeat(np.arange(c), shots)] + spread * rng.standard_normal((c * shots, d)) / np.sqrt(d)
    return z / np.linalg.norm(z, axis=1, keepdims=True)


def shape_case(b_, c, n, sv=None, per_class=False, batched_y=False):
    """fp32-representable inputs of one call: a cosine E per episode ([B,N,N]; per_class: E_c = exp(-(1 - E) (1 + c) / 2) [B,C,N,N], an RBF on unit rows per
    class), the Dirichlet targets of n rows drawn from max(c, 2) classes ([C,N]; batched_y: another draw per episode, [B,C,N]), sv, mean, cls_weight."""
    rng = np.random.default_rng(1000 * n + 10 * c + b_)
    cc = max(c, 2)
    shots = (n + cc - 1) // cc

    def rows():
        return np.sort(rng.permutation(cc * shots)[:n])
    picks = [rows() for _ in range(b_)]
    e = np.stack([(lambda z: z @ z.T)(unit_rows(rng, cc, shots)[pk]) for pk in picks])
    if per_class:
        e = np.stack([np.exp(-(1.0 - e) * (1.0 + ci) / 2.0) for ci in range(c)], 1)
    cls = [pk // shots for pk in (picks if batched_y else picks[:1])]
    pm1 = np.stack([np.where(np.stack([k == ci for ci in range(c)]), 1.0, -1.0) for k in cls])
    if not batched_y:                                   # (one target for every episode: the classes of episode 0's rows)
        pm1 = pm1[0]
    y, nr = dirichlet_targets(pm1, dtype=np.float32)
    return dict(e=_f32(e), y=_f32(y), nr=_f32(nr), sv=_f32(np.linspace(0.5, 2.0, c) if sv is None else sv), mean=_f32(np.linspace(-0.5, 0.5, c) - 2.0),
                cw=_f32(-np.linspace(0.5, 1.5, c) / n))


def cases():
    """{key: inputs}: the shape list, the 20-way shared case with sv alternating 0.5 / 5, a per-class-E case with per-episode targets."""
    out = {("shape",) + s: shape_case(*s) for s in SHAPES}
    out[("shared-scaled",)] = shape_case(2, 20, 100, sv=np.tile([0.5, 5.0], 10))
    out[("per-class",)] = shape_case(2, 5, 25, sv=np.array([0.5, 5.0, 1.0, 2.0, 0.5]), per_class=True, batched_y=True)
    out[("batched-y",)] = shape_case(2, 5, 17, batched_y=True)
    return out


def solve(d, dtype):
    return mll_rownoise(d["e"], d["y"], d["nr"], d["sv"], d["mean"], d["cw"], dtype)


def floors(cs, names=QUANTITIES, run=solve):
    """(float64 results, e32): e32[q] = the largest absolute error of the float32 run against the float64 run over the case list."""
    r64 = {k: run(d, np.float64) for k, d in cs.items()}
    r32 = {k: run(d, np.float32) for k, d in cs.items()}
    return r64, {q: max(float(np.abs(np.asarray(r32[k][q], np.float64) - r64[k][q]).max()) for k in cs) for q in names}


def proba_cases():
    """{key: dict(mu, var [B,C,M], eps [S,C])}: the shape list, a zero variance, a slightly negative one (rounding of sv exx - |v|^2: clamped at 0)."""
    out = {}
    for s in PROBA_SHAPES:
        b_, c, m, ns = s
        rng = np.random.default_rng(sum(s))
        out[("shape",) + s] = dict(mu=_f32(3.0 * rng.standard_normal((b_, c, m))), var=_f32(2.0 * rng.random((b_, c, m))), eps=_f32(rng.standard_normal((ns, c))))
    base = out[("shape", 2, 5, 80, 256)]
    out[("zero-var",)] = dict(base, var=np.zeros_like(base["var"]))
    out[("negative-var",)] = dict(base, var=_f32(np.where(base["var"] < 0.5, -1e-6, base["var"])))
    return out


def solve_proba(d, dtype):
    prob, labels = proba(d["mu"], d["var"], d["eps"], dtype)
    return dict(prob=prob, labels=labels)


def top_two_margin(mu):
    """Smallest gap between the largest and the second largest of mu [.., C, M] over the classes, per query; C == 1: inf."""
    if mu.shape[-2] < 2:
        return np.full(mu.shape[:-2] + mu.shape[-1:], np.inf)
    s = np.sort(mu, axis=-2)
    return s[..., -1, :] - s[..., -2, :]


def episode_case(b_=2, c=5, shots=5, m=80, seed=5, spread=0.6):
    """Test-time episodes: support rows zs [B,N,D], queries zq [B,M,D] (unit rows, the classes in turn), fp32-representable."""
    rng = np.random.default_rng(seed)
    zs, zq = [], []
    for _ in range(b_):
        centres = rng.standard_normal((c, 64))
        centres /= np.linalg.norm(centres, axis=1, keepdims=True)

        def draw(lab):
            z = centres[lab] + spread * rng.standard_normal((len(lab), 64)) / 8.0
            return z / np.linalg.norm(z, axis=1, keepdims=True)
        zs.append(draw(np.repeat(np.arange(c), shots)))
        zq.append(draw(np.arange(m) % c))
    return _f32(np.stack(zs)), _f32(np.stack(zq))
