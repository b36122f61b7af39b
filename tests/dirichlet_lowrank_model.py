"""numpy restatement of `dkt_rownoise_lowrank_f32`, `dkt_rownoise_lowrank_bwd_f32` and `dkt_rownoise_lowrank_predict_f32` (include/dkt_abi.h;
docs/DIRICHLET.md "Above 127 rows"): the row-noise GP of the Dirichlet likelihood for a linear kernel, in FEATURE space, with a `dtype` argument.

    K = s Z Z^T + Lambda (N x N, never formed),  Lambda = diag(noise_rows),  r = ytilde - mean
    B = I + s Z^T Lambda^-1 Z (D x D),  u = Z^T Lambda^-1 r,  t = B^-1 u
    alpha = Lambda^-1 (r - s Z t),  logp = -1/2 (r.Lambda^-1 r - s u.t) - 1/2 (sum log noise_rows + log det B) - N/2 log 2 pi
    d logp / d s = 1/2 (|t|^2 - (D - tr B^-1) / s),  d logp / d mean = sum alpha
    d obj / d Z = sum_c cw_c s_c Lambda_c^-1 (r_c t_c^T - Z Q_c),  Q_c = s_c t_c t_c^T + B_c^-1
    latent posterior at z: mu = mean + s z.t,  var = s z^T B^-1 z

The REFERENCE of every test is not this file but the N x N float64 formulas of tests/dirichlet_model.py on E = Z Z^T (`reference`, `reference_predict`);
the float32 run of this restatement against that reference is the fp32 floor e32 the GPU tests scale their bounds from."""
import numpy as np
import torch
from scipy.linalg import cholesky, solve_triangular

import dirichlet_model as dm

QUANTITIES = ("logp", "alpha", "dsv", "dmean", "dz")
PREDICT_QUANTITIES = ("mu", "var")
# (B, C, N, D): N around the 4-row step; around the 64-row chunk and the 127 / 128 rows of the resident kernel, D padded (60, 36); 16 / 17 / 32 classes
SHAPES = [(1, 1, 1, 4), (2, 5, 3, 64), (2, 5, 4, 64), (2, 5, 5, 64), (1, 2, 63, 64), (1, 2, 64, 64), (1, 2, 65, 64), (1, 3, 127, 60), (1, 3, 128, 64),
          (2, 5, 129, 36), (1, 16, 130, 64), (1, 17, 130, 64), (1, 32, 131, 64)]
PREDICT_M = (1, 15, 16, 17, 300)


def one(z, y, noise_rows, sv, mean, dtype=np.float64):
    """One problem: Z [N,D], y and noise_rows [N], scalars sv, mean -> dict(logp, alpha, dsv, dmean, t [D], binv [D,D], r, w)."""
    z, y, nr = np.asarray(z, dtype), np.asarray(y, dtype), np.asarray(noise_rows, dtype)
    sv, mean = dtype(sv), dtype(mean)
    n, d = z.shape
    w = dtype(1) / nr
    r = y - mean
    zw = z * w[:, None]
    b = np.eye(d, dtype=dtype) + sv * z.T.dot(zw)
    u = zw.T.dot(r)
    chol = cholesky(b, lower=True)
    tl = solve_triangular(chol, u, lower=True)
    t = solve_triangular(chol, tl, lower=True, trans="T")
    li = solve_triangular(chol, np.eye(d, dtype=dtype), lower=True)
    binv = li.T.dot(li)
    alpha = w * (r - sv * z.dot(t))
    logp = (dtype(-0.5) * ((r * r * w).sum() - sv * tl.dot(tl)) - dtype(0.5) * np.log(nr).sum() - np.log(np.diag(chol)).sum()
            - dtype(n) * dtype(0.5 * np.log(2 * np.pi)))
    dsv = dtype(0.5) * (t.dot(t) - (dtype(1) - np.diag(binv)).sum() / sv)
    out = dict(logp=logp, alpha=alpha, dsv=dsv, dmean=alpha.sum(), t=t, binv=binv, r=r, w=w)
    assert all(np.asarray(v).dtype == dtype for v in out.values())
    return out


def call(z, y, noise_rows, sv, mean, cls_weight, gobj, dtype=np.float64):
    """The forward and the backward call: z [B,N,D]; y, noise_rows [C,N] or [B,C,N]; sv, mean, cls_weight [C]; gobj [B] ->
    dict(logp [B,C] unweighted, alpha [B,C,N], dsv, dmean [B,C] (carrying cls_weight), dz [B,N,D], t [B,C,D], binv [B,C,D,D])."""
    z, y, nr = np.asarray(z, dtype), np.asarray(y, dtype), np.asarray(noise_rows, dtype)
    sv, mean, cw, gobj = (np.asarray(a, dtype) for a in (sv, mean, cls_weight, gobj))
    b_, n, d = z.shape
    c_ = y.shape[-2]
    o = dict(logp=np.zeros((b_, c_), dtype), alpha=np.zeros((b_, c_, n), dtype), dsv=np.zeros((b_, c_), dtype), dmean=np.zeros((b_, c_), dtype),
             dz=np.zeros((b_, n, d), dtype), t=np.zeros((b_, c_, d), dtype), binv=np.zeros((b_, c_, d, d), dtype))
    for b in range(b_):
        for c in range(c_):                                                # the classes in index order
            p = one(z[b], y[c] if y.ndim == 2 else y[b, c], nr[c] if nr.ndim == 2 else nr[b, c], sv[c], mean[c], dtype)
            o["logp"][b, c], o["alpha"][b, c], o["t"][b, c], o["binv"][b, c] = p["logp"], p["alpha"], p["t"], p["binv"]
            o["dsv"][b, c], o["dmean"][b, c] = cw[c] * p["dsv"], cw[c] * p["dmean"]
            q = sv[c] * np.outer(p["t"], p["t"]) + p["binv"]
            o["dz"][b] = o["dz"][b] + ((cw[c] * sv[c]) * p["w"])[:, None] * (np.outer(p["r"], p["t"]) - z[b].dot(q))
        o["dz"][b] = gobj[b] * o["dz"][b]
    assert all(v.dtype == dtype for v in o.values())
    return o


def predict(zq, t, binv, sv, mean, dtype=np.float64):
    """zq [B,M,D], t [B,C,D], binv [B,C,D,D] -> (mu, var [B,C,M], labels [B,M]: argmax_c mu, the first maximum)."""
    zq, t, binv, sv, mean = (np.asarray(a, dtype) for a in (zq, t, binv, sv, mean))
    mu = mean[None, :, None] + sv[None, :, None] * np.matmul(t, zq.transpose(0, 2, 1))
    var = sv[None, :, None] * (np.matmul(zq[:, None], binv) * zq[:, None]).sum(-1)
    assert mu.dtype == dtype and var.dtype == dtype
    return mu, var, np.argmax(mu, 1).astype(np.int32)


def reference(d):
    """The N x N float64 formulas of tests/dirichlet_model.py on E = Z Z^T; the gradient of Z is gobj_b 2 dE Z."""
    z = d["z"]
    o = dm.mll_rownoise(np.einsum("bnd,bmd->bnm", z, z), d["y"], d["nr"], d["sv"], d["mean"], d["cw"], np.float64)
    return dict(logp=o["logp"], alpha=o["alpha"], dsv=o["dsv"], dmean=o["dmean"], dz=d["gobj"][:, None, None] * 2.0 * np.einsum("bnm,bmd->bnd", o["de"], z))


def reference_predict(d):
    """dirichlet_model.predict on E = Zs Zs^T, Ex = Zq Zs^T per episode -> (mu, var [B,C,M])."""
    mu, var = [], []
    for b in range(d["z"].shape[0]):
        zs, zq = d["z"][b], d["zq"][b]
        m, v = dm.predict(zs @ zs.T, zq @ zs.T, (zq * zq).sum(-1), d["y"] if d["y"].ndim == 2 else d["y"][b], d["nr"] if d["nr"].ndim == 2 else d["nr"][b],
                          d["sv"], d["mean"], np.float64)
        mu.append(m); var.append(v)
    return np.stack(mu), np.stack(var)


def solve(d, dtype):
    return call(d["z"], d["y"], d["nr"], d["sv"], d["mean"], d["cw"], d["gobj"], dtype)


def solve_predict(d, dtype):
    o = solve(d, dtype)
    mu, var, labels = predict(d["zq"], o["t"], o["binv"], d["sv"], d["mean"], dtype)
    return dict(mu=mu, var=var, labels=labels)


def shape_case(b_, c, n, d, sv=None, batched_y=False, random_noise=False, m=0, seed=None, spread=0.6):
    """fp32-representable inputs of one call: unit rows Z [B,N,D] drawn from max(c, 2) classes, their Dirichlet targets ([C,N]; batched_y: per episode,
    [B,C,N]), sv, mean, cls_weight, gobj.  random_noise: noise_rows uniform in [0.3, 5] and rows of norm 0.1 to 3.  m > 0: queries zq [B,m,D], the classes in turn."""
    rng = np.random.default_rng(100000 * d + 1000 * n + 10 * c + b_ if seed is None else seed)
    cc = max(c, 2)
    shots = (n + cc - 1) // cc
    picks, zs, zq = [], [], []
    for _ in range(b_):
        centres = rng.standard_normal((cc, d))
        centres /= np.linalg.norm(centres, axis=1, keepdims=True)

        def draw(lab):
            z = centres[lab] + spread * rng.standard_normal((len(lab), d)) / np.sqrt(d)
            return z / np.linalg.norm(z, axis=1, keepdims=True)
        pk = np.sort(rng.permutation(cc * shots)[:n])
        picks.append(pk)
        zs.append(draw(pk // shots))
        if m:
            zq.append(draw(np.arange(m) % cc))
    z = np.stack(zs)
    cls = [pk // shots for pk in (picks if batched_y else picks[:1])]
    pm1 = np.stack([np.where(np.stack([k == ci for ci in range(c)]), 1.0, -1.0) for k in cls])
    if not batched_y:
        pm1 = pm1[0]
    y, nr = dm.dirichlet_targets(pm1, dtype=np.float32)
    if random_noise:
        nr = rng.uniform(0.3, 5.0, size=nr.shape)
        z = z * rng.uniform(0.1, 3.0, size=z.shape[:2])[..., None]
    out = dict(z=dm._f32(z), y=dm._f32(y), nr=dm._f32(nr), sv=dm._f32(np.linspace(0.5, 2.0, c) if sv is None else sv),
               mean=dm._f32(np.linspace(-0.5, 0.5, c) - 2.0), cw=dm._f32(-np.linspace(0.5, 1.5, c) / n), gobj=dm._f32(np.linspace(0.7, 1.3, b_)))
    if m:
        out["zq"] = dm._f32(np.stack(zq))
    return out


def cases():
    """{key: inputs}: the shape list, the 20-way training episode with sv alternating 0.5 / 5, per-episode targets, random noise on rows that are not unit."""
    out = {("shape",) + s: shape_case(*s) for s in SHAPES}
    out[("20-way",)] = shape_case(2, 20, 420, 64, sv=np.tile([0.5, 5.0], 10))
    out[("batched-y",)] = shape_case(2, 5, 70, 64, batched_y=True)
    out[("random-noise",)] = shape_case(2, 5, 133, 64, random_noise=True, batched_y=True)
    return out


def predict_cases():
    """{key: inputs with zq}: M = 1, 15, 16, 17 on a 5-way 130-row set (D = 60: padded), M = 300 on two 20-way 8-shot sets (the label case)."""
    out = {("m", m): shape_case(1, 5, 130, 60, m=m, seed=7000 + m) for m in PREDICT_M[:-1]}
    out[("labels",)] = shape_case(2, 20, 160, 64, sv=np.tile([0.5, 5.0], 10), m=PREDICT_M[-1], seed=11)
    return out


def floors(cs, names=QUANTITIES, run=solve, ref=reference):
    """(reference results, float64 run, e32): e32[q] = the largest absolute error of the float32 run of the restatement against the N x N float64
    reference over the case list."""
    r = {k: ref(d) for k, d in cs.items()}
    r64 = {k: run(d, np.float64) for k, d in cs.items()}
    r32 = {k: run(d, np.float32) for k, d in cs.items()}
    return r, r64, {q: max(float(np.abs(np.asarray(r32[k][q], np.float64) - r[k][q]).max()) for k in cs) for q in names}


def ref_predict(d):
    mu, var = reference_predict(d)
    return dict(mu=mu, var=var)


_cache = {}


def all_floors():
    """Computed once per process: dict(cases, ref, r64, e32, pcases, pref, p64, p32)."""
    if not _cache:
        cs, pcs = cases(), predict_cases()
        ref, r64, e32 = floors(cs)
        pref, p64, p32 = floors(pcs, PREDICT_QUANTITIES, solve_predict, ref_predict)
        _cache.update(cases=cs, ref=ref, r64=r64, e32=e32, pcases=pcs, pref=pref, p64=p64, p32=p32)
    return _cache


# ---- end-to-end chains in torch autograd on the CPU (the N x N formulas), shared by the GPU tests ------------------------------------------------
def as_tensor(a, dev):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(dev)


def _obj_from_k(k, yt, nrt, mean, cwt):
    """obj [B] from k = sv_c E [B,C,N,N] (differentiable): K = k + diag(noise_rows), exact-GP logp, weighted class sum."""
    n = k.shape[-1]
    chol = torch.linalg.cholesky(k + torch.diag_embed(nrt).expand_as(k))
    t = torch.linalg.solve_triangular(chol, (yt - mean.view(-1, 1)).expand(k.shape[0], -1, -1).unsqueeze(-1), upper=False).squeeze(-1)
    logp = -0.5 * (t * t).sum(-1) - torch.log(torch.diagonal(chol, dim1=-2, dim2=-1)).sum(-1) - 0.5 * n * np.log(2 * np.pi)
    return (logp * cwt).sum(1)


def chain(z, sv, mean, yt, nr, cw, dtype):
    """Rows z [B,N,D] -> linear kernel -> objective; obj.sum() differentiated in z, sv, mean."""
    z, sv, mean = (torch.tensor(a, dtype=dtype, requires_grad=True) for a in (z, sv, mean))
    yt, nr, cw = (torch.tensor(a, dtype=dtype) for a in (yt, nr, cw))
    obj = _obj_from_k(sv.view(1, -1, 1, 1) * (z @ z.transpose(1, 2)).unsqueeze(1), yt, nr, mean, cw)
    obj.sum().backward()
    return dict(obj=obj.detach().double().numpy(), dz=z.grad.double().numpy(), dsv=sv.grad.double().numpy(), dmean=mean.grad.double().numpy())


def bn_chain(x, gamma, beta, sv, mean, yt, nr, cw, use_bn, dtype, eps=1e-5):
    """The trunk front end: [train-mode BatchNorm1d per episode +] F.normalize + linear kernel, then the chain above."""
    x, sv, mean, gamma, beta = (torch.tensor(a, dtype=dtype, requires_grad=True) for a in (x, sv, mean, gamma, beta))
    yt, nr, cw = (torch.tensor(a, dtype=dtype) for a in (yt, nr, cw))
    h = x
    if use_bn:
        h = (x - x.mean(1, keepdim=True)) / torch.sqrt(x.var(1, unbiased=False, keepdim=True) + eps) * gamma + beta
    z = torch.nn.functional.normalize(h, p=2, dim=2)
    obj = _obj_from_k(sv.view(1, -1, 1, 1) * (z @ z.transpose(1, 2)).unsqueeze(1), yt, nr, mean, cw)
    obj.sum().backward()
    out = dict(obj=obj.detach().double().numpy(), dx=x.grad.double().numpy(), dsv=sv.grad.double().numpy(), dmean=mean.grad.double().numpy())
    if use_bn:
        out.update(dgamma=gamma.grad.double().numpy(), dbeta=beta.grad.double().numpy())
    return out


def chain_floors(run):
    """{name: f(dtype)} -> dict(r64, e32): the float64 results and, per quantity, the largest float32 error over the list."""
    r64 = {k: f(torch.float64) for k, f in run.items()}
    r32 = {k: f(torch.float32) for k, f in run.items()}
    e32 = {}
    for k in r64:
        for q in r64[k]:
            e32[q] = max(e32.get(q, 0.0), float(np.abs(r32[k][q] - r64[k][q]).max()))
    return dict(r64=r64, e32=e32)


def compare(tag, got, chains, factor=4.0):
    """Every quantity of the chain `tag` against float64, within factor x e32 of that quantity."""
    r64 = chains["r64"][tag]
    for q in r64:
        e32 = chains["e32"][q]
        err = float(np.abs(got[q].detach().double().cpu().numpy() - r64[q]).max())
        print(tag, q, "err %.3g, e32 %.3g (%.2f x)" % (err, e32, err / e32))
        assert err <= factor * e32, (tag, q, err, e32)
