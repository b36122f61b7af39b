"""The leave-one-out predictive log likelihood of the linear kernels, K = sv Z Z^T + (noise + jitter) I, stated twice in float64, independent of dkt_amd
(a helper, not a test; docs/LOOFS.md):

  feature_form   numpy, any dtype: the feature-space closed form -- D x D matrices and passes over the rows, values, leave-one-out predictions, gradients
  dense          the definition of docs/LOO.md: tests/loo_model.py's closed form on E = Z Z^T, dZ = 2 W Z

and the cases of the GPU comparison (tests/test_loo_lowrank_gpu.py) with the rule of its tolerance: the error of a float32 evaluation of `feature_form` against
the float64 one is the floor of a case group, the bound is 4 x that floor.  `feature_form(defect=...)` seeds the two defects the bound has to catch
(tests/test_loo_lowrank_host.py): "q" drops the 2 Q z_i term of dZ, "k" forgets the division by s in k_i."""
import functools
import os
import re

import numpy as np

import loo_model as lm

HALF_LOG_2PI = lm.HALF_LOG_2PI
VALUES = ("loo", "alpha", "mu_loo", "var_loo")
GRADS = ("dz", "dsv", "dmean", "dnoise")
BOUND = 4.0                                   # x the float32 floor of the case's group
H_CAP = 0.95                                  # every case: max_i h_i <= H_CAP in float64, so that 1 - h_i is a full-precision remainder
_HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dkt_abi_loofs.h")


def header_rows():
    """R, the row block of the kernel, as the header states it"""
    with open(_HEADER) as fh:
        return int(re.search(r"#define\s+DKT_LOOFS_ROWS\s+(\d+)", fh.read()).group(1))


def _y3(Y, b):
    return Y if Y.ndim == 3 else np.broadcast_to(Y[None], (b,) + Y.shape)


def feature_form(Z, Y, sv, mean, noise, cw=None, jitter=0.0, dtype=np.float64, defect=None):
    """dict(loo [B,C], alpha, mu_loo, var_loo [B,C,N], dz [B,N,D] = sum_c cw_c d loo_c / dZ, dsv, dmean, dnoise [B,C] raw, h [B,C,N]), every operation in `dtype`."""
    Z, Y, sv, mean, noise = (np.asarray(x, dtype=dtype) for x in (Z, Y, sv, mean, noise))
    cw = np.ones_like(sv) if cw is None else np.asarray(cw, dtype=dtype)
    b_, n, d = Z.shape
    y3 = _y3(Y, b_)
    s = noise + dtype(jitter)
    v = sv
    lam = s / v
    S = np.einsum("bnd,bne->bde", Z, Z)
    A = S[:, None] + lam[None, :, None, None] * np.eye(d, dtype=dtype)
    G = np.linalg.inv(A).astype(dtype)
    G = dtype(0.5) * (G + np.swapaxes(G, -1, -2))
    r = y3 - mean[None, :, None]
    p = np.einsum("bnd,bcn->bcd", Z, r)
    w = np.einsum("bcde,bce->bcd", G, p)
    s3 = s[None, :, None]
    alpha = (r - np.einsum("bnd,bcd->bcn", Z, w)) / s3
    GZ = np.einsum("bcde,bne->bcnd", G, Z)
    h = np.einsum("bcnd,bnd->bcn", GZ, Z)
    k = (dtype(1.0) - h) if defect == "k" else (dtype(1.0) - h) / s3
    loo = (dtype(0.5) * np.log(k) - dtype(0.5) * alpha * alpha / k).sum(-1) - dtype(n * HALF_LOG_2PI)
    a = -alpha / k
    bq = dtype(0.5) / k + dtype(0.5) * alpha * alpha / (k * k)
    c_ = -bq / s3
    gw = -np.einsum("bnd,bcn->bcd", Z, a) / s[None, :, None]
    gp = np.einsum("bcde,bce->bcd", G, gw)
    M = np.einsum("bcnd,bne->bcde", Z[:, None] * c_[..., None], Z)
    gwp = gw[..., :, None] * p[..., None, :]
    Q = -np.matmul(np.matmul(G, M + dtype(0.5) * (gwp + np.swapaxes(gwp, -1, -2))), G)
    dzc = dtype(2.0) * c_[..., None] * GZ - (a / s3)[..., None] * w[:, :, None, :] + r[..., None] * gp[:, :, None, :]
    if defect != "q":
        dzc = dzc + dtype(2.0) * np.einsum("bcde,bne->bcnd", Q, Z)
    trq = np.einsum("bcdd->bc", Q)
    out = dict(loo=loo, alpha=alpha, mu_loo=y3 - alpha / k, var_loo=dtype(1.0) / k, dz=np.einsum("c,bcnd->bnd", cw, dzc),
               dsv=-trq * s[None] / (v * v)[None], dmean=-(a / s3 + np.einsum("bnd,bcd->bcn", Z, gp)).sum(-1),
               dnoise=-(a * alpha).sum(-1) / s[None] - (bq * k).sum(-1) / s[None] + trq / v[None], h=h)
    return {key: np.asarray(val, dtype=dtype) for key, val in out.items()}


def dense(Z, Y, sv, mean, noise, cw=None, jitter=0.0, dtype=np.float64):
    """The same dict (no h) from the N x N definition: loo_model.closed_form on E = Z Z^T, dZ = (W + W^T) Z = 2 W Z, every operation in `dtype`."""
    Z = np.asarray(Z, dtype)
    out = lm.closed_form(np.matmul(Z, np.swapaxes(Z, -1, -2)), np.asarray(Y, dtype), sv, mean, noise, cw, jitter=jitter, dtype=dtype)
    out["dz"] = dtype(2.0) * np.matmul(out.pop("w"), Z)
    return out


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------
def rows(seed, b, n, d, unit=True):
    """Z [B,N,D] float32: unit rows, or rows of norms in [0.5, 1.2] (h_i <= |z_i|^2 / (|z_i|^2 + lam) <= 0.935 at lam >= 0.1: the cap holds for every N)"""
    z = lm.unit_rows(seed, b, n, d)
    if not unit:
        z = z * np.random.default_rng(seed + 7).uniform(0.5, 1.2, (b, n, 1))
    return np.ascontiguousarray(z.astype(np.float32))


class Case:
    def __init__(self, n, d, c, b, y_per_episode, cw, unit, noise0, sv0):
        self.n, self.d, self.c, self.b, self.y_per_episode, self.cw, self.unit, self.noise0, self.sv0 = n, d, c, b, y_per_episode, cw, unit, noise0, sv0

    def __repr__(self):
        return "N%d-D%d-C%d-B%d-%s-cw_%s-%s-noise%g-sv%g" % (self.n, self.d, self.c, self.b, "yB" if self.y_per_episode else "y", self.cw,
                                                            "unit" if self.unit else "raw", self.noise0, self.sv0)

    @property
    def group(self):
        return next(g for g, ns in GROUPS.items() if self.n in ns)

    def inputs(self):
        seed = 1000 * self.n + 10 * self.c + self.b + self.d
        sv, mean, noise = lm.hypers(self.c, self.sv0, self.noise0)
        return dict(z=rows(seed, self.b, self.n, self.d, self.unit), y=lm.targets(self.c, self.n, self.b if self.y_per_episode else None, seed), sv=sv, mean=mean,
                    noise=noise, cw=lm.class_weights(self.cw, self.c, self.n))


R = header_rows()
# 1, 2; the edges of the row block R - 1, R, R + 1, 2 R + 1; the edges of the resident kernel and of the route 127, 128, 129; the 20-way shapes
NS = tuple(sorted({1, 2, R - 1, R, R + 1, 2 * R + 1, 63, 64, 65, 127, 128, 129, 257, 420}))
GROUPS = {"n1-2": (1, 2), "block": tuple(sorted({R - 1, R, R + 1, 63, 64, 65})), "n127-129": tuple(sorted({127, 128, 129, 2 * R + 1})), "n257-420": (257, 420)}
MAX_ELEMENTS = 3 << 20                        # B C N^2, the entries of the float64 dense model of a case


def _cases():
    out = []
    for i, n in enumerate(NS):
        for k in range(2):
            j = 2 * i + k
            c = (1, 5, 20, 32)[j % 4]
            b = (70, 1, 3)[(j + i) % 3]
            if b * c * n * n > MAX_ELEMENTS:
                b = 3
            out.append(Case(n, (4, 8, 60, 64)[(j + j // 4) % 4], c, b, (i + k) % 2 == 1, ("none", "mixed", "zeros")[j % 3], (j // 2 + k) % 2 == 0,
                            (0.1, 1.0)[(j // 3) % 2], (0.3, 1.0)[(j // 5 + k) % 2]))
    out.append(Case(420, 64, 20, 1, False, "mixed", True, 0.1, 1.0))          # the 20-way 5-shot + 16-query episode itself
    return out


CASES = _cases()


def errors(got, ref, keys):
    return lm.errors(got, ref, keys)


@functools.lru_cache(maxsize=None)
def reference(index):
    """(float64 feature-space closed form, float32 errors against it) of CASES[index]: computed once, shared, never modified"""
    inp = CASES[index].inputs()
    ref = feature_form(inp["z"], inp["y"], inp["sv"], inp["mean"], inp["noise"], inp["cw"])
    f32 = feature_form(inp["z"], inp["y"], inp["sv"], inp["mean"], inp["noise"], inp["cw"], dtype=np.float32)
    return ref, errors(f32, ref, VALUES + GRADS)


@functools.lru_cache(maxsize=None)
def floors(group):
    """The float32 floor of a case group: per quantity, the largest float32 error over its cases"""
    errs = [reference(i)[1] for i, k in enumerate(CASES) if k.group == group]
    return {q: max(e[q] for e in errs) for q in VALUES + GRADS}
