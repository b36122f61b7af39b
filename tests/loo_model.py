"""The leave-one-out predictive log likelihood of exact GP regression (Rasmussen & Williams, GPML, section 5.4.2) restated twice, independent of dkt_amd
(a helper, not a test; docs/LOO.md):

  closed_form   numpy, any dtype: from A = K^-1, K = sv E + (noise + jitter) I -- values, leave-one-out predictions and the gradients
  refits        the definition, float64: N refits per problem, each leaving one row out; its gradients by float64 torch autograd

and the cases of the GPU comparison (tests/test_loo_gpu.py) with the rule of its tolerance: the error of a float32 evaluation of `closed_form` against the
float64 one is the floor of a case group, the bound is 4 x that floor.  `closed_form(defect=True)` drops the alpha r^T term of G: the seeded defect that the
bound has to catch (tests/test_loo_host.py)."""
import functools

import numpy as np
import torch

HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)
VALUES = ("loo", "alpha", "mu_loo", "var_loo")
GRADS = ("w", "dsv", "dmean", "dnoise")
BOUND = 4.0                                   # x the float32 floor of the case's group


def _bc(E, Y, sv):
    """E [B,N,N] | [B,C,N,N], Y [C,N] | [B,C,N] -> E [B,C,N,N] (broadcast view), Y [B,C,N], per_class"""
    per_class = E.ndim == 4
    c = len(sv)
    e4 = E if per_class else np.broadcast_to(E[:, None], (E.shape[0], c) + E.shape[1:])
    y3 = Y if Y.ndim == 3 else np.broadcast_to(Y[None], (E.shape[0],) + Y.shape)
    return e4, y3, per_class


def closed_form(E, Y, sv, mean, noise, cw=None, jitter=0.0, dtype=np.float64, defect=False):
    """dict(loo [B,C], alpha, mu_loo, var_loo [B,C,N], w ([B,N,N] summed over the classes for a shared E, else [B,C,N,N]) = cw_c sv_c G_c, dsv, dmean, dnoise
    [B,C] raw), every operation in `dtype`."""
    E, Y, sv, mean, noise = (np.asarray(x, dtype=dtype) for x in (E, Y, sv, mean, noise))
    cw = np.ones_like(sv) if cw is None else np.asarray(cw, dtype=dtype)
    e4, y3, per_class = _bc(E, Y, sv)
    n = E.shape[-1]
    eye = np.eye(n, dtype=dtype)
    K = sv[None, :, None, None] * e4 + (noise + dtype(jitter))[None, :, None, None] * eye
    A = np.linalg.inv(K).astype(dtype)
    A = dtype(0.5) * (A + np.swapaxes(A, -1, -2))
    r0 = y3 - mean[None, :, None]
    alpha = np.einsum("bcij,bcj->bci", A, r0)
    d = np.einsum("bcii->bci", A)
    q = alpha / d
    loo = (dtype(0.5) * np.log(d) - dtype(0.5) * alpha * q).sum(-1) - dtype(n * HALF_LOG_2PI)
    p = dtype(0.5) / d + dtype(0.5) * q * q
    r = np.einsum("bcij,bcj->bci", A, q)
    G = -np.matmul(A * p[..., None, :], A)
    ar = alpha[..., :, None] * r[..., None, :]
    G = G + (dtype(0.5) * np.swapaxes(ar, -1, -2) if defect else dtype(0.5) * (ar + np.swapaxes(ar, -1, -2)))
    w = (cw * sv)[None, :, None, None] * G
    out = dict(loo=loo, alpha=alpha, mu_loo=y3 - q, var_loo=dtype(1.0) / d, w=w if per_class else w.sum(1), dsv=(G * e4).sum((-1, -2)),
               dmean=r.sum(-1), dnoise=np.einsum("bcii->bc", G))
    return {k: np.asarray(v, dtype=dtype) for k, v in out.items()}


def _refit_loo_torch(e4, y3, sv, mean, noise):
    """loo [B,C], mu [B,C,N], var [B,C,N] by N explicit refits (torch float64, differentiable)"""
    b_, c_, n = y3.shape
    K = sv.view(1, -1, 1, 1) * e4 + noise.view(1, -1, 1, 1) * torch.eye(n, dtype=torch.float64)
    mus, vars_ = [], []
    for i in range(n):
        keep = [j for j in range(n) if j != i]
        if keep:
            Kk = K[:, :, keep][:, :, :, keep]
            ki = K[:, :, keep, i]
            sol = torch.linalg.solve(Kk, torch.stack([y3[:, :, keep] - mean.view(1, -1, 1), ki], -1))
            mu = mean.view(1, -1) + (ki * sol[..., 0]).sum(-1)
            var = K[:, :, i, i] - (ki * sol[..., 1]).sum(-1)
        else:
            mu, var = mean.view(1, -1).expand(b_, c_), K[:, :, 0, 0]
        mus.append(mu)
        vars_.append(var)
    mu, var = torch.stack(mus, -1), torch.stack(vars_, -1)
    loo = (-0.5 * torch.log(var) - 0.5 * (y3 - mu) ** 2 / var - HALF_LOG_2PI).sum(-1)
    return loo, mu, var


def refits(E, Y, sv, mean, noise, cw=None):
    """The definition: the same dict as `closed_form` (no alpha), the gradients by autograd of obj = sum_bc loo (w: of sum_bc cw_c loo, symmetrised -- E enters
    through the symmetric K only)."""
    e4, y3, per_class = _bc(np.asarray(E, np.float64), np.asarray(Y, np.float64), sv)
    t = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=torch.float64)      # noqa: E731
    Et = t(E).requires_grad_(True)
    svt, mt, nt = (t(x).requires_grad_(True) for x in (sv, mean, noise))
    e4t = Et if per_class else Et.unsqueeze(1).expand(-1, len(sv), -1, -1)
    loo, mu, var = _refit_loo_torch(e4t, t(y3), svt, mt, nt)
    # per-problem hyper-parameter parts: d loo[b,c] / d sv[c] -- one backward per episode row would do; C columns are independent, so sum over b per row b
    dsv, dmean, dnoise = (np.zeros(loo.shape) for _ in range(3))
    for b in range(loo.shape[0]):
        g = torch.autograd.grad(loo[b].sum(), (svt, mt, nt), retain_graph=True)
        dsv[b], dmean[b], dnoise[b] = (x.numpy() for x in g)
    cwt = torch.ones(len(sv), dtype=torch.float64) if cw is None else t(cw)
    gE, = torch.autograd.grad((loo * cwt.view(1, -1)).sum(), Et)
    w = 0.5 * (gE + gE.transpose(-1, -2)).numpy()
    return dict(loo=loo.detach().numpy(), mu_loo=mu.detach().numpy(), var_loo=var.detach().numpy(), w=w, dsv=dsv, dmean=dmean, dnoise=dnoise)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------
def unit_rows(seed, b, n, d):
    z = np.random.default_rng(seed).standard_normal((b, n, d))
    return z / np.linalg.norm(z, axis=-1, keepdims=True)


def base_matrix(z, kernel, c=None):
    """E of unit rows z [B,N,D], rounded to float32: shared [B,N,N] (c None) or per class [B,C,N,N] (rbf: lengthscales 0.6 .. 1.5; linear: offsets 0 .. 1,
    scaled back to a unit diagonal)."""
    g = z @ np.swapaxes(z, -1, -2)
    g = 0.5 * (g + np.swapaxes(g, -1, -2))
    if c is None:
        e = np.exp(-(1.0 - g)) if kernel == "rbf" else g              # |zi - zj|^2 / 2 = 1 - g
    elif kernel == "rbf":
        e = np.exp(-(1.0 - g)[:, None] / np.linspace(0.6, 1.5, c).reshape(1, c, 1, 1) ** 2)
    else:
        off = np.linspace(0.0, 1.0, c).reshape(1, c, 1, 1)
        e = (g[:, None] + off) / (1.0 + off)
    return np.ascontiguousarray(e.astype(np.float32))


def targets(c, n, b=None, seed=0):
    """+-1 one-vs-rest targets [C,N]; with b: [B,C,N], each episode's with its own small perturbation"""
    cls = np.arange(n) % max(c, 2)
    y = np.where(cls[None] == np.arange(c)[:, None], 1.0, -1.0)
    if b is not None:
        y = y[None] + 0.1 * np.random.default_rng(seed).standard_normal((b, c, n))
    return np.ascontiguousarray(y.astype(np.float32))


def class_weights(mode, c, n):
    if mode == "none":
        return None
    if mode == "mixed":
        return (np.linspace(-1.0, 1.5, c) / (c * n)).astype(np.float32)
    return np.where(np.arange(c) % 2 == 0, 0.0, 0.7).astype(np.float32)          # "zeros"


def hypers(c, sv0, noise0):
    return ((sv0 * np.linspace(0.8, 1.0, c)).astype(np.float32), np.linspace(-0.2, 0.3, c).astype(np.float32),
            (noise0 * np.linspace(1.0, 1.2, c)).astype(np.float32))


class Case:
    def __init__(self, n, c, b, per_class, y_per_episode, cw, d, kernel, noise0, sv0):
        self.n, self.c, self.b, self.per_class, self.y_per_episode, self.cw, self.d, self.kernel, self.noise0, self.sv0 = (
            n, c, b, per_class, y_per_episode, cw, d, kernel, noise0, sv0)

    def __repr__(self):
        return "N%d-C%d-B%d-%s-%s-cw_%s-D%d-%s-noise%g-sv%g" % (self.n, self.c, self.b, "perclass" if self.per_class else "shared",
                                                               "yB" if self.y_per_episode else "y", self.cw, self.d, self.kernel, self.noise0, self.sv0)

    @property
    def group(self):
        return next(g for g, ns in GROUPS.items() if self.n in ns)

    def inputs(self):
        seed = 1000 * self.n + 10 * self.c + self.b
        e = base_matrix(unit_rows(seed, self.b, self.n, self.d), self.kernel, self.c if self.per_class else None)
        sv, mean, noise = hypers(self.c, self.sv0, self.noise0)
        return dict(e=e, y=targets(self.c, self.n, self.b if self.y_per_episode else None, seed), sv=sv, mean=mean, noise=noise,
                    cw=class_weights(self.cw, self.c, self.n))


# the tile edges of the kernel's 4 x 4 tiles, of a wave (64 rows) and of the 16-lane row groups of the factorisation; 127 = the limit
NS = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 96, 105, 112, 127)
GROUPS = {"n1-2": (1, 2), "n15-17": (15, 16, 17), "n31-33": (31, 32, 33), "n63-65": (63, 64, 65), "n96-127": (96, 105, 112, 127)}
MAX_ELEMENTS = 3 << 20                        # B C N^2, the entries of all of a case's matrices: its float64 model stays quick


def _cases():
    out = []
    for i, n in enumerate(NS):
        for k in range(3):
            c = (1, 5, 32)[(i + k) % 3]
            b = (1, 3, 70)[(i + 2 * k + 1) % 3]
            per_class = (i + k) % 2 == 1
            if b * c * n * n > MAX_ELEMENTS:
                b = 3
            out.append(Case(n, c, b, per_class, (i + k // 2) % 2 == 1, ("none", "mixed", "zeros")[k], (8, 64)[(i + k) % 2], ("rbf", "linear")[(i // 2 + k) % 2],
                            (0.1, 1.0)[(i + (k + 1) // 2) % 2], (0.3, 1.0)[(i // 3 + k) % 2]))
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


@functools.lru_cache(maxsize=None)
def reference(index):
    """(float64 closed form, float32 errors against it) of CASES[index]: computed once, shared, never modified"""
    inp = CASES[index].inputs()
    ref = closed_form(inp["e"], inp["y"], inp["sv"], inp["mean"], inp["noise"], inp["cw"])
    f32 = closed_form(inp["e"], inp["y"], inp["sv"], inp["mean"], inp["noise"], inp["cw"], dtype=np.float32)
    return ref, errors(f32, ref, VALUES + GRADS)


@functools.lru_cache(maxsize=None)
def floors(group):
    """The float32 floor of a case group: per quantity, the largest float32 error over its cases"""
    errs = [reference(i)[1] for i, k in enumerate(CASES) if k.group == group]
    return {q: max(e[q] for e in errs) for q in VALUES + GRADS}


# ---- the whole training episode in torch (any dtype, differentiable): what ops.episode_loss_loo / _bn compute ---------------------------------------
def loo_torch(e4, y3, sv, mean, noise):
    """loo [B,C] of E [B,C,N,N] (a shared E broadcast), y [B,C,N]: the closed form above, differentiable"""
    n = e4.shape[-1]
    K = sv.view(1, -1, 1, 1) * e4 + noise.view(1, -1, 1, 1) * torch.eye(n, dtype=e4.dtype)
    A = torch.linalg.inv(K)
    alpha = (A @ (y3 - mean.view(1, -1, 1)).unsqueeze(-1)).squeeze(-1)
    d = torch.diagonal(A, dim1=-2, dim2=-1)
    return (0.5 * torch.log(d) - 0.5 * alpha * alpha / d).sum(-1) - n * HALF_LOG_2PI


def episode_loss_torch(front, inputs, y, sv, mean, noise, cw, dtype):
    """mean_b sum_c cw_c loo[b,c] and its gradients with respect to `inputs` + (sv, mean, noise).  front: "linear" (inputs: z; E = z z^T), "rbf" (z, lengthscale [C];
    E_c = exp(-|zi - zj|^2 / (2 l_c^2))) or "bn" (x, gamma, beta; BatchNorm1d in train mode per episode, eps 1e-5, F.normalize, E = zn zn^T)."""
    leaves = [torch.tensor(np.asarray(t), dtype=dtype, requires_grad=True) for t in list(inputs) + [sv, mean, noise]]
    *ins, svt, mt, nt = leaves
    c = len(sv)
    if front == "bn":
        x, gamma, beta = ins
        xh = (x - x.mean(1, keepdim=True)) / torch.sqrt(x.var(1, unbiased=False, keepdim=True) + 1e-5)
        z = torch.nn.functional.normalize(xh * gamma + beta, p=2, dim=2)
    else:
        z = ins[0]
    g = z @ z.transpose(1, 2)
    if front == "rbf":
        sq = torch.diagonal(g, dim1=-2, dim2=-1)
        d2 = (sq.unsqueeze(-1) + sq.unsqueeze(-2) - 2.0 * g).clamp_min(0.0)
        e4 = torch.exp(-0.5 * d2.unsqueeze(1) / ins[1].view(1, -1, 1, 1) ** 2)
    else:
        e4 = g.unsqueeze(1).expand(-1, c, -1, -1)
    yt = torch.tensor(np.asarray(y), dtype=dtype)
    y3 = yt if yt.dim() == 3 else yt.unsqueeze(0).expand(z.shape[0], -1, -1)
    loss = (loo_torch(e4, y3, svt, mt, nt) * torch.tensor(np.asarray(cw), dtype=dtype).view(1, -1)).sum(1).mean()
    grads = torch.autograd.grad(loss, leaves)
    return loss.detach().numpy(), [gr.numpy() for gr in grads]
