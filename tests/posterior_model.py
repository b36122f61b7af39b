"""The joint posterior of exact GP regression at a set of query points (Rasmussen & Williams, GPML, section 2.2) restated twice, independent of dkt_amd (a
helper, not a test; docs/POSTERIOR.md):

  closed_form   numpy, any dtype: two Cholesky factorisations and the triangular solves, as include/dkt_abi_post.h writes them
  definition    float64: the joint (N + M)-dimensional Gaussian of support and query targets, conditioned by the generic block formula (no factor)

and the cases of the GPU comparison (tests/test_posterior_gpu.py) with the rule of its tolerance: the error of a float32 evaluation of `closed_form` against the
float64 one is the floor of a case group, the bound is 4 x that floor.  `closed_form(defect=...)` seeds the two defects that the bound has to catch
(tests/test_posterior_host.py): "vtv" -- V^T V lacking the sv factor of one operand; "noise" -- Sigma missing its with_noise term."""
import functools

import numpy as np

HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)
QUANTITIES = ("mu", "cov", "chol", "logp", "lpd", "samples")
BOUND = 4.0                                   # x the float32 floor of the case's group
MIN_EIG_RATIO = 1e-3                          # the conditioning cap: lambda_min(Sigma) >= this x lambda_max(Sigma), in float64, on every case


def _bc(E, c):
    """[B,R,S] | [B,C,R,S] -> [B,C,R,S] (broadcast view)"""
    return E if E.ndim == 4 else np.broadcast_to(E[:, None], (E.shape[0], c) + E.shape[1:])


def _operands(Ess, Eqs, Eqq, Y, sv, mean, noise, yq, eps, dtype):
    Ess, Eqs, Eqq, Y, sv, mean, noise = (np.asarray(x, dtype=dtype) for x in (Ess, Eqs, Eqq, Y, sv, mean, noise))
    c = len(sv)
    y3 = Y if Y.ndim == 3 else np.broadcast_to(Y[None], (Ess.shape[0],) + Y.shape)
    yq = None if yq is None else np.asarray(yq, dtype=dtype)
    eps = None if eps is None or eps.shape[2] == 0 else np.asarray(eps, dtype=dtype)
    s4 = sv[None, :, None, None]
    return _bc(Ess, c), _bc(Eqs, c), _bc(Eqq, c), y3, s4, mean[None, :, None], noise[None, :, None, None], yq, eps


def _cholesky(a, nan_on_failure):
    """Batched lower factor; a seeded defect may leave some Sigma indefinite: those factors (and what is read off them) are NaN, which no bound admits."""
    try:
        return np.linalg.cholesky(a)
    except np.linalg.LinAlgError:
        if not nan_on_failure:
            raise
    out = np.full_like(a, np.nan)
    for idx in np.ndindex(a.shape[:-2]):
        try:
            out[idx] = np.linalg.cholesky(a[idx])
        except np.linalg.LinAlgError:
            pass
    return out


def closed_form(Ess, Eqs, Eqq, Y, sv, mean, noise, yq=None, eps=None, with_noise=True, jitter_s=0.0, jitter_q=0.0, dtype=np.float64, defect=None):
    """dict(mu [B,C,M], cov, chol [B,C,M,M], logp, lpd [B,C] (with yq), samples [B,C,S,M] (with eps)), every operation in `dtype`."""
    ess, eqs, eqq, y3, s4, m3, n4, yq, eps = _operands(Ess, Eqs, Eqq, Y, sv, mean, noise, yq, eps, dtype)
    n, m = ess.shape[-1], eqq.shape[-1]
    K = s4 * ess + (n4 + dtype(jitter_s)) * np.eye(n, dtype=dtype)
    L = np.linalg.cholesky(K)
    t = np.linalg.solve(L, (y3 - m3)[..., None])                                  # [B,C,N,1]
    V = np.linalg.solve(L, s4 * np.swapaxes(eqs, -1, -2))                         # [B,C,N,M]
    mu = m3 + np.matmul(np.swapaxes(V, -1, -2), t)[..., 0]
    Vl = np.linalg.solve(L, np.swapaxes(eqs, -1, -2)) if defect == "vtv" else V          # (the seeded defect: one operand without its sv)
    cov = s4 * eqq - np.matmul(np.swapaxes(Vl, -1, -2), V)
    if with_noise and defect != "noise":
        cov = cov + n4 * np.eye(m, dtype=dtype)
    cov = dtype(0.5) * (cov + np.swapaxes(cov, -1, -2))
    R = _cholesky(cov + dtype(jitter_q) * np.eye(m, dtype=dtype), nan_on_failure=defect is not None)
    out = dict(mu=mu, cov=cov, chol=R)
    if yq is not None:
        r = yq - mu
        failed = np.isnan(R).any((-1, -2))                                        # (a seeded defect only)
        z = np.linalg.solve(np.where(failed[..., None, None], np.eye(m, dtype=dtype), R), r[..., None])[..., 0]
        d = np.einsum("bcii->bci", cov)
        with np.errstate(invalid="ignore"):                                       # (a defective Sigma's diagonal may be negative)
            out["logp"] = dtype(-0.5) * (z * z).sum(-1) - np.log(np.einsum("bcii->bci", R)).sum(-1) - dtype(m * HALF_LOG_2PI)
            out["lpd"] = (dtype(-0.5) * np.log(d) - dtype(0.5) * r * r / d).sum(-1) - dtype(m * HALF_LOG_2PI)
    if eps is not None:
        out["samples"] = mu[:, :, None, :] + np.matmul(eps, np.swapaxes(R, -1, -2))
    return {k: np.asarray(v, dtype=dtype) for k, v in out.items()}


def definition(Ess, Eqs, Eqq, Y, sv, mean, noise, yq=None, with_noise=True):
    """The definition, float64: support and query targets are jointly Gaussian with covariance J = sv [[E_ss, E_qs^T], [E_qs, E_qq]] + noise diag(I_N, with_noise
    I_M) and a constant mean; the conditional of the query block given the support block by the generic formula mu = m + J_qs J_ss^-1 (y - m),
    Sigma = J_qq - J_qs J_ss^-1 J_sq (a general solve, no Cholesky factor), logp by slogdet + solve.  dict(mu, cov, logp, lpd, joint [B,C,N+M,N+M])."""
    ess, eqs, eqq, y3, s4, m3, n4, yq, _ = _operands(Ess, Eqs, Eqq, Y, sv, mean, noise, yq, None, np.float64)
    n, m = ess.shape[-1], eqq.shape[-1]
    J = s4 * np.concatenate([np.concatenate([ess, np.swapaxes(eqs, -1, -2)], -1), np.concatenate([eqs, eqq], -1)], -2)
    J = J + n4 * np.diag(np.concatenate([np.ones(n), np.full(m, 1.0 if with_noise else 0.0)]))
    Jss, Jqs, Jqq = J[..., :n, :n], J[..., n:, :n], J[..., n:, n:]
    mu = m3 + np.matmul(Jqs, np.linalg.solve(Jss, (y3 - m3)[..., None]))[..., 0]
    cov = Jqq - np.matmul(Jqs, np.linalg.solve(Jss, np.swapaxes(Jqs, -1, -2)))
    out = dict(mu=mu, cov=cov, joint=J)
    if yq is not None:
        r = yq - mu
        sign, logdet = np.linalg.slogdet(cov)
        assert (sign > 0).all()
        out["logp"] = -0.5 * (r * np.linalg.solve(cov, r[..., None])[..., 0]).sum(-1) - 0.5 * logdet - m * HALF_LOG_2PI
        d = np.einsum("bcii->bci", cov)
        out["lpd"] = (-0.5 * np.log(2.0 * np.pi * d) - 0.5 * r * r / d).sum(-1)
    return out


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------
def unit_rows(seed, b, n, d):
    z = np.random.default_rng(seed).standard_normal((b, n, d))
    return z / np.linalg.norm(z, axis=-1, keepdims=True)


def base_matrix(za, zb, kernel, c=None):
    """E = k(za, zb) of unit rows [B,R,D], [B,S,D], rounded to float32: shared [B,R,S] (c None) or per class [B,C,R,S] (rbf: lengthscales 0.6 .. 1.5; linear:
    offsets 0 .. 1, scaled back to a unit diagonal).  zb None: za against itself, symmetric bit for bit."""
    g = za @ np.swapaxes(za if zb is None else zb, -1, -2)
    if zb is None:
        g = 0.5 * (g + np.swapaxes(g, -1, -2))
    if c is None:
        e = np.exp(-(1.0 - g)) if kernel == "rbf" else g              # |zi - zj|^2 / 2 = 1 - g
    elif kernel == "rbf":
        e = np.exp(-(1.0 - g)[:, None] / np.linspace(0.6, 1.5, c).reshape(1, c, 1, 1) ** 2)
    else:
        off = np.linspace(0.0, 1.0, c).reshape(1, c, 1, 1)
        e = (g[:, None] + off) / (1.0 + off)
    return np.ascontiguousarray(e.astype(np.float32))


def targets(seed, c, n, b=None):
    """smooth-ish targets in [-1.5, 1.5]: [C,N], or [B,C,N] with b"""
    rng = np.random.default_rng(seed)
    y = np.sin(1.3 * np.arange(n)[None] + np.arange(c)[:, None]) + 0.3 * rng.standard_normal((c, n))
    if b is not None:
        y = y[None] + 0.2 * rng.standard_normal((b, c, n))
    return np.ascontiguousarray(y.astype(np.float32))


def hypers(c, sv0, noise0):
    return ((sv0 * np.linspace(0.8, 1.0, c)).astype(np.float32), np.linspace(-0.2, 0.3, c).astype(np.float32),
            (noise0 * np.linspace(1.0, 1.2, c)).astype(np.float32))


GROUPS = {"1-2": 2, "15-17": 19, "33": 33, "63-65": 65, "127": 127}          # name -> the largest max(N, M) it holds ((5,19) and (19,19) ride with 15-17)


class Case:
    def __init__(self, n, m, c, b, per_class, y_per_episode, with_noise, s, has_yq, d, kernel, noise0, sv0):
        (self.n, self.m, self.c, self.b, self.per_class, self.y_per_episode, self.with_noise, self.s, self.has_yq, self.d, self.kernel, self.noise0,
         self.sv0) = n, m, c, b, per_class, y_per_episode, with_noise, s, has_yq, d, kernel, noise0, sv0

    def __repr__(self):
        return "N%d-M%d-C%d-B%d-%s-%s-%s-S%d-%s-D%d-%s-noise%g-sv%g" % (
            self.n, self.m, self.c, self.b, "perclass" if self.per_class else "shared", "yB" if self.y_per_episode else "y",
            "noisy" if self.with_noise else "latent", self.s, "yq" if self.has_yq else "noyq", self.d, self.kernel, self.noise0, self.sv0)

    @property
    def group(self):
        return next(g for g, top in GROUPS.items() if max(self.n, self.m) <= top)

    def quantities(self):
        return tuple(q for q in QUANTITIES if not (q in ("logp", "lpd") and not self.has_yq) and not (q == "samples" and self.s == 0))

    def inputs(self):
        seed = 100000 * self.n + 100 * self.m + self.c + self.b
        zs, zq = unit_rows(seed, self.b, self.n, self.d), unit_rows(seed + 7, self.b, self.m, self.d)      # the query rows are draws of their own
        cc = self.c if self.per_class else None
        sv, mean, noise = hypers(self.c, self.sv0, self.noise0)
        rng = np.random.default_rng(seed + 13)
        return dict(e_ss=base_matrix(zs, None, self.kernel, cc), e_qs=base_matrix(zq, zs, self.kernel, cc), e_qq=base_matrix(zq, None, self.kernel, cc),
                    y=targets(seed, self.c, self.n, self.b if self.y_per_episode else None), sv=sv, mean=mean, noise=noise,
                    yq=targets(seed + 1, self.c, self.m, self.b) if self.has_yq else None,
                    eps=rng.standard_normal((self.b, self.c, self.s, self.m)).astype(np.float32) if self.s else None)


# (N, M): the edges of a wave (64 rows), of the factorisation's 16-lane row groups and of the 4 x 4 tiles, the limits, and the QMUL shapes (5,19), (19,19)
NS = (1, 2, 15, 16, 17, 33, 63, 64, 65, 127)
MS = (1, 2, 15, 16, 17, 33, 64, 65, 127)
PAIRS = ((1, 1), (1, 2), (2, 1), (2, 2),
         (1, 15), (15, 1), (15, 15), (16, 16), (17, 17), (2, 16), (16, 2), (17, 15), (15, 17), (5, 19), (19, 19), (16, 17),
         (33, 33), (1, 33), (33, 2), (17, 33), (33, 16), (15, 33),
         (63, 64), (64, 64), (65, 65), (64, 1), (2, 65), (63, 17), (33, 64), (65, 33), (16, 65), (63, 15),
         (127, 127), (1, 127), (127, 1), (127, 64), (64, 127), (33, 127), (127, 17), (65, 127))
MAX_ELEMENTS = 3 << 20                        # B C (N + M)^2, the entries of a case's joint matrices: B = 70 becomes 3 beyond it


def _cases():
    out = []
    for i, (n, m) in enumerate(PAIRS):
        c = (1, 3, 32)[i % 3]
        b = (1, 3, 70)[(i + i // 3) % 3]
        if b == 70 and b * c * (n + m) ** 2 > MAX_ELEMENTS:
            b = 3
        with_noise = i % 4 in (0, 3)
        d, kernel = (8, 64)[(i // 2) % 2], ("rbf", "linear")[(i + i // 4) % 2]
        if not with_noise:
            # the conditioning cap on the LATENT covariance (nothing on its diagonal): the kernel has to be of full rank with a floor under its spectrum
            # -- the RBF of near-orthogonal rows, D = 64 -- once there are more than a few query rows
            d, kernel = (64, "rbf") if m > 2 else (d, kernel)
        out.append(Case(n, m, c, b, per_class=i % 2 == 1, y_per_episode=(i // 2) % 2 == 1, with_noise=with_noise, s=(0, 1, 7)[(i + i // 5) % 3],
                        has_yq=i % 5 != 2, d=d, kernel=kernel, noise0=(0.1, 1.0)[(i // 3) % 2], sv0=(0.3, 1.0)[(i + i // 6) % 2]))
    return out


CASES = _cases()


def errors(got, ref, keys):
    """max |got - ref| / max |ref| per quantity (element-wise, not a norm: docs/FRONTEND_BWD.md)"""
    out = {}
    for k in keys:
        g, r = np.asarray(got[k], np.float64), np.asarray(ref[k], np.float64)
        scale = np.abs(r).max()
        out[k] = float(np.abs(g - r).max() / scale) if scale > 0 else float(np.abs(g - r).max())
    return out


def _model_args(inp, with_noise):
    return (inp["e_ss"], inp["e_qs"], inp["e_qq"], inp["y"], inp["sv"], inp["mean"], inp["noise"]), dict(yq=inp["yq"], eps=inp["eps"], with_noise=with_noise)


@functools.lru_cache(maxsize=None)
def reference(index):
    """(float64 closed form, float32 errors against it) of CASES[index]: computed once, shared, never modified"""
    kase = CASES[index]
    args, kw = _model_args(kase.inputs(), kase.with_noise)
    ref = closed_form(*args, **kw)
    f32 = closed_form(*args, dtype=np.float32, **kw)
    return ref, errors(f32, ref, kase.quantities())


@functools.lru_cache(maxsize=None)
def floors(group):
    """The float32 floor of a case group: per quantity, the largest float32 error over the cases that have it"""
    errs = [reference(i)[1] for i, k in enumerate(CASES) if k.group == group]
    return {q: max(e[q] for e in errs if q in e) for q in QUANTITIES if any(q in e for e in errs)}
