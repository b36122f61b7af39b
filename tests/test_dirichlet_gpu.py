"""dkt_mll_rownoise_f32 / dkt_dirichlet_proba_f32 / ops.dirichlet_objective / DKT(likelihood="dirichlet") on the GPU against the float64 restatement
(tests/dirichlet_model.py; test_dirichlet_host.py checks that one against scipy and finite differences).

Tolerances follow docs/LAPLACE.md, as docs/DIRICHLET.md restates: e32 is the largest absolute error of the float32 run of the restatement against its
float64 run over the whole case list, per quantity, computed here on the CPU; the kernel is allowed 4 x e32.  The end-to-end tests do the same with their
own case list (four chains in torch on the CPU).  Inputs are fp32-representable."""
import ctypes

import numpy as np
import pytest
import torch

import dirichlet_model as dm
import dkt_amd

pytestmark = pytest.mark.gpu
ops, L = dkt_amd.ops, dkt_amd._lib
Q = dm.QUANTITIES


@pytest.fixture(scope="module")
def ref():
    cases = dm.cases()
    r64, e32 = dm.floors(cases)
    print("e32:", {q: "%.3g" % v for q, v in e32.items()})
    return dict(cases=cases, r64=r64, e32=e32)


@pytest.fixture(scope="module")
def pref():
    cases = dm.proba_cases()
    r64, e32 = dm.floors(cases, ("prob",), dm.solve_proba)
    print("e32(prob): %.3g" % e32["prob"])
    return dict(cases=cases, r64=r64, e32=e32)


def _t(a, cuda):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(cuda)


def _gpu(d, cuda):
    return ops.mll_rownoise(_t(d["e"], cuda), _t(d["y"], cuda), _t(d["nr"], cuda), _t(d["sv"], cuda), _t(d["mean"], cuda), want_grad=True, want_chol=True,
                            cls_weight=_t(d["cw"], cuda))


def _check(key, ref, cuda):
    got = _gpu(ref["cases"][key], cuda)
    err = {q: float(np.abs(got[q].double().cpu().numpy() - ref["r64"][key][q]).max()) for q in Q}
    print(key, {q: "%.3g (%.2f x e32)" % (err[q], err[q] / ref["e32"][q]) for q in Q})
    assert int(got["info"].abs().max()) == 0
    assert torch.equal(got["de"], got["de"].transpose(-1, -2))
    assert float(got["chol"].triu(1).abs().max()) == 0.0
    for q in Q:
        assert err[q] <= 4 * ref["e32"][q], (key, q, err[q], ref["e32"][q])
    return got


@pytest.mark.parametrize("shape", dm.SHAPES, ids=str)
def test_kernel_matches_float64_at_its_edges(shape, ref, cuda):
    _check(("shape",) + shape, ref, cuda)


@pytest.mark.parametrize("key", [("shared-scaled",), ("per-class",), ("batched-y",)], ids=str)
def test_kernel_matches_float64_scaled_per_class_and_batched_targets(key, ref, cuda):
    _check(key, ref, cuda)


@pytest.mark.parametrize("key", [("shape", 3, 5, 25), ("shared-scaled",), ("shape", 2, 5, 17)], ids=str)
def test_two_runs_and_both_forms_agree_bitwise(key, ref, cuda):
    d = ref["cases"][key]
    b_, c = d["e"].shape[0], d["y"].shape[0]
    shared, again = _gpu(d, cuda), _gpu(d, cuda)
    per_class = _gpu(dict(d, e=np.repeat(d["e"][:, None], c, 1), y=np.repeat(d["y"][None], b_, 0), nr=np.repeat(d["nr"][None], b_, 0)), cuda)
    for q in Q:
        assert torch.equal(shared[q], again[q]), q
    for q in ("logp", "alpha", "dsv", "dmean", "chol"):
        assert torch.equal(shared[q], per_class[q]), q
    acc = per_class["de"][:, 0].clone()
    for ci in range(1, c):                                 # the classes in index order
        acc = acc + per_class["de"][:, ci]
    assert torch.equal(shared["de"], acc)


def test_forward_only_call_gives_the_same_bits_and_touches_nothing_else(ref, cuda):
    d = ref["cases"][("shape", 2, 5, 17)]
    full = _gpu(d, cuda)
    fwd = ops.mll_rownoise(_t(d["e"], cuda), _t(d["y"], cuda), _t(d["nr"], cuda), _t(d["sv"], cuda), _t(d["mean"], cuda))
    assert fwd["de"] is None and fwd["chol"] is None
    assert torch.equal(fwd["logp"], full["logp"]) and torch.equal(fwd["alpha"], full["alpha"])


def test_a_negative_noise_fails_its_own_problem_only(ref, cuda):
    d = ref["cases"][("per-class",)]
    good = _gpu(d, cuda)
    nr = d["nr"].copy()
    nr[1, 3, 7] = -50.0                                    # K_77 < 0: the pivot of row 7 at the latest
    got = _gpu(dict(d, nr=nr), cuda)
    info = got["info"].cpu().numpy()
    assert 1 <= info[1, 3] <= 8 and (np.delete(info.reshape(-1), 1 * 5 + 3) == 0).all()
    assert bool(torch.isnan(got["logp"][1, 3])) and bool(torch.isnan(got["alpha"][1, 3]).all()) and bool(torch.isnan(got["de"][1, 3]).all())
    keep = torch.ones(2, 5, dtype=torch.bool, device=cuda)
    keep[1, 3] = False
    for q in Q:
        assert torch.equal(got[q][keep], good[q][keep]), q


def test_shape_limits_and_null_pointers_do_not_launch(cuda):
    lib = L.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def run(c, n, null=None, flags=3):
        e, y, nr = torch.eye(n, device=cuda)[None].contiguous(), torch.zeros(c, n, device=cuda), torch.ones(c, n, device=cuda)
        sv, mean = torch.ones(c, device=cuda), torch.zeros(c, device=cuda)
        outs = [torch.full(s, -7.0, device=cuda) for s in ((1, c), (1, c, n), (1, n, n), (1, c), (1, c), (1, c, n, n))]
        info = torch.full((1, c), -7, device=cuda, dtype=torch.int32)
        nbytes = int(lib.dkt_mll_rownoise_workspace_bytes(1, c, n))
        ws = torch.empty(nbytes // 4, device=cuda)
        a = dict(E=p(e), Y=p(y), nr=p(nr), sv=p(sv), mean=p(mean), logp=p(outs[0]), alpha=p(outs[1]), dE=p(outs[2]), chol=p(outs[5]), info=p(info), ws=p(ws))
        if null:
            a[null] = None
        st = lib.dkt_mll_rownoise_f32(a["E"], n * n, 0, a["Y"], 0, a["nr"], 0, a["sv"], a["mean"], None, a["logp"], a["alpha"], a["dE"], p(outs[3]), p(outs[4]),
                                      a["chol"], a["info"], 1, c, n, flags, a["ws"], nbytes, None)
        torch.cuda.synchronize()
        return st, all(bool((o == -7).all()) for o in outs + [info])

    assert run(5, 128) == (-5, True) and run(33, 10) == (-5, True)
    for null in ("E", "Y", "nr", "sv", "mean", "logp", "alpha", "dE", "chol", "info"):
        assert run(5, 10, null) == (-1, True), null
    assert run(5, 10, "ws") == (-3, True)                  # a shared E with gradients needs the workspace
    assert run(5, 10, flags=4) == (-1, True)               # no other flag of dkt_mll_f32 applies
    assert run(32, 127) == (0, False)
    with pytest.raises(RuntimeError, match="DKT_ERR_SHAPE"):
        ops.mll_rownoise(torch.eye(128, device=cuda)[None], torch.zeros(2, 128, device=cuda), torch.ones(2, 128, device=cuda), torch.ones(2, device=cuda),
                         torch.zeros(2, device=cuda))


def test_dirichlet_targets_match_the_restatement(cuda):
    y = torch.tensor([[1.0, -1.0, -1.0], [-1.0, 1.0, 1.0]], device=cuda)
    yt, nr = ops.dirichlet_targets(y)
    y64, n64 = dm.dirichlet_targets(y.cpu().numpy())
    assert np.abs(yt.cpu().numpy() - y64).max() < 1e-6 and np.abs(nr.cpu().numpy() - n64).max() < 1e-6       # a few ulps of 6.9


# ---- class probabilities ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [("shape",) + s for s in dm.PROBA_SHAPES] + [("zero-var",), ("negative-var",)], ids=str)
def test_proba_matches_the_restatement_on_the_same_eps(key, pref, cuda):
    d = pref["cases"][key]
    prob, labels = ops.dirichlet_proba(_t(d["mu"], cuda), _t(d["var"], cuda), _t(d["eps"], cuda))
    again = ops.dirichlet_proba(_t(d["mu"], cuda), _t(d["var"], cuda), _t(d["eps"], cuda))[0]
    got = prob.double().cpu().numpy()
    err = float(np.abs(got - pref["r64"][key]["prob"]).max())
    print(key, "prob err %.3g (%.2f x e32), rows sum to 1 within %.3g" % (err, err / pref["e32"]["prob"], np.abs(got.sum(-1) - 1).max()))
    assert err <= 4 * pref["e32"]["prob"]
    assert np.abs(got.sum(-1) - 1).max() <= 1e-6 and torch.equal(prob, again)
    assert (labels.cpu().numpy() == pref["r64"][key]["labels"]).all()               # (mu is the input: exact)
    if key == ("zero-var",):                                                       # no spread: the softmax of mu itself
        assert np.abs(got - torch.softmax(_t(d["mu"], cuda).double().transpose(1, 2), -1).cpu().numpy()).max() < 1e-6


def test_proba_first_maximum_wins_and_limits(cuda):
    mu = torch.tensor([[[1.0, 2.0], [3.0, 2.0], [3.0, 2.0]]], device=cuda)         # [1, 3, 2]
    prob, labels = ops.dirichlet_proba(mu, torch.zeros_like(mu), torch.zeros(2, 3, device=cuda))
    assert labels.cpu().tolist() == [[1, 0]]
    with pytest.raises(RuntimeError, match="DKT_ERR_SHAPE"):
        ops.dirichlet_proba(torch.zeros(1, 33, 2, device=cuda), torch.zeros(1, 33, 2, device=cuda), torch.zeros(1, 33, device=cuda))


# ---- end to end: features -> kernel -> objective, against float64 autograd of the same chain ---------------------------------------------------
def _obj_from_k(k, yt, nrt, mean, cwt):
    """obj [B] from the base matrices times sv, k [B,C,N,N] (torch, differentiable): K = k + diag(noise_rows), exact-GP logp, weighted class sum."""
    n = k.shape[-1]
    chol = torch.linalg.cholesky(k + torch.diag_embed(nrt).expand_as(k))
    t = torch.linalg.solve_triangular(chol, (yt - mean.view(-1, 1)).expand(k.shape[0], -1, -1).unsqueeze(-1), upper=False).squeeze(-1)
    logp = -0.5 * (t * t).sum(-1) - torch.log(torch.diagonal(chol, dim1=-2, dim2=-1)).sum(-1) - 0.5 * n * np.log(2 * np.pi)
    return (logp * cwt).sum(1)


def _chain(z, sv, mean, ls, yt, nr, cw, kind, dtype):
    z, sv, mean, ls = (torch.tensor(a, dtype=dtype, requires_grad=True) for a in (z, sv, mean, ls))
    yt, nr, cw = (torch.tensor(a, dtype=dtype) for a in (yt, nr, cw))
    if kind == "linear":
        k = sv.view(1, -1, 1, 1) * (z @ z.transpose(1, 2)).unsqueeze(1)
    else:
        d2 = ((z.unsqueeze(2) - z.unsqueeze(1)) ** 2).sum(-1)
        k = sv.view(1, -1, 1, 1) * torch.exp(-0.5 * d2.unsqueeze(1) / ls.view(1, -1, 1, 1) ** 2)
    obj = _obj_from_k(k, yt, nr, mean, cw)
    obj.sum().backward()
    return dict(obj=obj.detach().double().numpy(), dz=z.grad.double().numpy(), dsv=sv.grad.double().numpy(), dmean=mean.grad.double().numpy(),
                dls=None if ls.grad is None else ls.grad.double().numpy())


def _episode_inputs():
    rng = np.random.default_rng(3)
    z = np.stack([dm.unit_rows(rng, 5, 5, spread=0.6) for _ in range(2)]).astype(np.float32).astype(np.float64)          # [2, 25, 64], unit rows
    yt, nr = dm.dirichlet_targets(np.where(np.repeat(np.eye(5), 5, 1) > 0, 1.0, -1.0), dtype=np.float32)
    return z, yt.astype(np.float64), nr.astype(np.float64), np.array([0.5, 2.0, 1.0, 3.0, 0.75]), np.array([-2.0, -1.5, -2.5, -1.0, -3.0]), np.full(5, -1.0 / 125)


def _compare(tag, got, chains):
    """Every quantity of the chain `tag` against float64, within 4 x e32 of that quantity: the largest float32-chain error over the end-to-end case list."""
    r64 = chains["r64"][tag]
    for q in r64:
        e32 = chains["e32"][q]
        err = float(np.abs(got[q].detach().double().cpu().numpy() - r64[q]).max())
        print(tag, q, "err %.3g, e32 %.3g (%.2f x)" % (err, e32, err / e32))
        assert err <= 4 * e32, (tag, q, err, e32)


LS = np.array([0.75, 1.0, 1.25, 1.5, 0.875])


def _bn_inputs():
    rng = np.random.default_rng(5)
    centres = rng.standard_normal((5, 64))
    x = np.stack([np.repeat(centres, 5, 0) + 0.7 * rng.standard_normal((25, 64)) for _ in range(2)]).astype(np.float32).astype(np.float64)
    return x, (1.0 + 0.2 * rng.standard_normal(64)).astype(np.float32).astype(np.float64), (0.1 * rng.standard_normal(64)).astype(np.float32).astype(np.float64)


@pytest.fixture(scope="module")
def chains():
    """The end-to-end case list -- linear-unit and rbf from the features, the BN trunk front end with BatchNorm on and off -- in float64 and float32 torch on the
    CPU, once; e32[q] = the largest float32 error of quantity q over the list (dz, dsv, dmean, obj; dls, dx, dgamma, dbeta where a chain has them)."""
    z, yt, nr, sv, mean, cw = _episode_inputs()
    x, gamma, beta = _bn_inputs()
    run = {"linear": lambda dt: _chain(z, sv, mean, LS, yt, nr, cw, "linear", dt), "rbf": lambda dt: _chain(z, sv, mean, LS, yt, nr, cw, "rbf", dt),
           "bn": lambda dt: _bn_chain(x, gamma, beta, sv, mean, yt, nr, cw, True, dt), "no bn": lambda dt: _bn_chain(x, gamma, beta, sv, mean, yt, nr, cw, False, dt)}
    r64 = {k: {q: v for q, v in f(torch.float64).items() if v is not None} for k, f in run.items()}
    r32 = {k: f(torch.float32) for k, f in run.items()}
    e32 = {}
    for k in r64:
        for q in r64[k]:
            e32[q] = max(e32.get(q, 0.0), float(np.abs(r32[k][q] - r64[k][q]).max()))
    print("end-to-end e32:", {q: "%.3g" % v for q, v in e32.items()})
    return dict(r64=r64, e32=e32)


@pytest.mark.parametrize("kind", ["linear", "rbf"])
def test_objective_end_to_end_matches_float64_autograd(kind, chains, cuda):
    z, yt, nr, sv, mean, cw = _episode_inputs()
    zt, svt, mt, lst = (torch.tensor(a, dtype=torch.float32, device=cuda, requires_grad=True) for a in (z, sv, mean, LS))
    obj, logp, alpha, info, e = ops.episode_loss_dirichlet(zt, _t(yt, cuda), _t(nr, cuda), svt, mt, _t(cw, cuda), "bncossim" if kind == "linear" else "rbf",
                                                           lengthscale=lst, unit_rows=kind == "linear")
    obj.sum().backward()
    assert int(info.abs().max()) == 0 and e.dim() == (3 if kind == "linear" else 4) and (lst.grad is None) == (kind == "linear")
    _compare(kind, dict(obj=obj, dz=zt.grad, dsv=svt.grad, dmean=mt.grad, dls=lst.grad), chains)


def _bn_chain(x, gamma, beta, sv, mean, yt, nr, cw, use_bn, dtype, eps=1e-5):
    """The fused front end in torch on the CPU: [train-mode BatchNorm1d per episode +] F.normalize + linear kernel, then the chain above."""
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


@pytest.mark.parametrize("use_bn", [True, False])
def test_fused_front_end_gradients_match_float64_autograd(use_bn, chains, cuda):
    _, yt, nr, sv, mean, cw = _episode_inputs()
    x, gamma, beta = _bn_inputs()
    xt, gt, bt, svt, mt = (torch.tensor(a, dtype=torch.float32, device=cuda, requires_grad=True) for a in (x, gamma, beta, sv, mean))
    out = ops.episode_loss_dirichlet_bn(xt, gt if use_bn else None, bt if use_bn else None, _t(yt, cuda), _t(nr, cuda), svt, mt, _t(cw, cuda), use_bn=use_bn)
    out[0].sum().backward()
    _compare("bn" if use_bn else "no bn", dict(obj=out[0], dx=xt.grad, dsv=svt.grad, dmean=mt.grad, dgamma=gt.grad, dbeta=bt.grad), chains)


def test_dirichlet_objective_is_the_raw_call_and_differentiable(cuda, ref):
    d = ref["cases"][("shape", 3, 5, 25)]
    e, sv, mean = (_t(d[k], cuda).requires_grad_(True) for k in ("e", "sv", "mean"))
    y, nr, cw = _t(d["y"], cuda), _t(d["nr"], cuda), _t(d["cw"], cuda)
    obj, logp, alpha, info = ops.dirichlet_objective(e, y, nr, sv, mean, cw)
    raw = ops.mll_rownoise(e.detach(), y, nr, sv.detach(), mean.detach(), want_grad=True, cls_weight=cw)
    gout = torch.tensor([1.0, -2.0, 0.5], device=cuda)
    (obj * gout).sum().backward()
    assert torch.equal(logp, raw["logp"]) and torch.equal(alpha, raw["alpha"]) and torch.equal(obj, ops.objective(raw["logp"], cw))
    assert torch.equal(e.grad, raw["de"] * gout.view(-1, 1, 1))
    assert torch.allclose(sv.grad, (gout.view(-1, 1) * raw["dsv"]).sum(0), rtol=1e-6, atol=0)
    assert torch.allclose(mean.grad, (gout.view(-1, 1) * raw["dmean"]).sum(0), rtol=1e-6, atol=0)


# ---- test time: latent posterior, labels, probabilities ----------------------------------------------------------------------------------------
def test_latent_posterior_and_labels_match_float64(cuda):
    """Support set -> alpha, L (dkt_mll_rownoise_f32) -> mu (dkt_predict_f32), latent var (dkt_predict_var_f32, zero noise) -> labels.  Queries whose float64
    top-two margin of mu is under 100 x e32(mu) are left out of the label comparison (none is: test_dirichlet_host.py records the smallest margin)."""
    zs, zq = dm.episode_case()
    sv, mean = np.array([0.5, 2.0, 1.0, 3.0, 0.75]), np.array([-2.0, -1.5, -2.5, -1.0, -3.0])
    yt, nr = (a.astype(np.float64) for a in dm.dirichlet_targets(np.where(np.repeat(np.eye(5), 5, 1) > 0, 1.0, -1.0), dtype=np.float32))
    e, ex = dm._f32(zs @ zs.transpose(0, 2, 1)), dm._f32(zq @ zs.transpose(0, 2, 1))
    exx = dm._f32((zq * zq).sum(-1))
    r = {dt: [dm.predict(e[b], ex[b], exx[b], yt, nr, sv, mean, dt) for b in range(2)] for dt in (np.float64, np.float32)}
    mu64, var64 = (np.stack([r[np.float64][b][i] for b in range(2)]) for i in (0, 1))
    e32 = [max(float(np.abs(r[np.float32][b][i] - r[np.float64][b][i]).max()) for b in range(2)) for i in (0, 1)]
    out = ops.mll_rownoise(_t(e, cuda), _t(yt, cuda), _t(nr, cuda), _t(sv, cuda), _t(mean, cuda), want_chol=True)
    mu, labels = ops.predict(_t(ex, cuda), out["alpha"], _t(sv, cuda), _t(mean, cuda))
    var = ops.predict_var(_t(ex, cuda), _t(exx, cuda), out["chol"], _t(sv, cuda), torch.zeros(5, device=cuda))
    err = [float(np.abs(g.double().cpu().numpy() - w).max()) for g, w in ((mu, mu64), (var, var64))]
    print("mu err %.3g (%.2f x e32 = %.3g), var err %.3g (%.2f x e32 = %.3g)" % (err[0], err[0] / e32[0], e32[0], err[1], err[1] / e32[1], e32[1]))
    assert err[0] <= 4 * e32[0] and err[1] <= 4 * e32[1]
    keep = dm.top_two_margin(mu64) >= 100 * e32[0]
    print("smallest float64 margin %.3g, left out %d of %d" % (dm.top_two_margin(mu64).min(), (~keep).sum(), keep.size))
    assert (~keep).mean() <= 0.10
    assert (labels.cpu().numpy() == mu64.argmax(1))[keep].all()
    prob, plabels = ops.dirichlet_proba(mu, var, torch.randn(64, 5, generator=torch.Generator().manual_seed(0)).to(cuda))
    assert torch.equal(plabels, labels) and float((prob.sum(-1) - 1).abs().max()) <= 1e-6


# ---- the DKT surface --------------------------------------------------------------------------------------------------------------------------
def _episode(seed, n_way=5, per_class=5):
    return torch.rand(n_way, per_class, 3, 28, 28, generator=torch.Generator().manual_seed(seed))


def _model(cuda, **kw):
    torch.manual_seed(0)
    m = dkt_amd.DKT(dkt_amd.backbone.Conv4S, n_way=5, n_support=1, likelihood="dirichlet", **kw).to(cuda)
    m.train()
    return m


@pytest.mark.parametrize("kernel_type", ["bncossim", "rbf"])
def test_train_loop_step_calls_the_new_op_once_and_trains_scale_and_mean(cuda, capsys, monkeypatch, kernel_type):
    """Three episodes, print_freq 1000: every step is ONE gradient call of ops.mll_rownoise; the in-loop evaluation (first and last iteration) conditions on
    the transformed labels with one forward-only call each.  No Gaussian marginal-likelihood call at all."""
    calls = []
    real = ops.mll_rownoise
    monkeypatch.setattr(ops, "mll_rownoise", lambda *a, **k: (calls.append(bool(k.get("want_grad"))), real(*a, **k))[1])
    monkeypatch.setattr(ops, "mll", lambda *a, **k: pytest.fail("the Gaussian marginal likelihood was called"))
    monkeypatch.setenv("DKT_TRAIN_GRAPH", "0")
    m = _model(cuda, kernel_type=kernel_type)
    before = {k: v.clone() for k, v in m.model.state_dict().items()}
    m.train_loop(0, [(_episode(s), None) for s in (1, 2, 3)], None, print_freq=1000)
    assert calls.count(True) == 3 and calls.count(False) == 2, calls
    assert torch.isfinite(m._last["loss"]) and 0.0 <= float(m._last["acc_query"]) <= 100.0
    after = m.model.state_dict()
    assert not torch.equal(after["raw_outputscale"], before["raw_outputscale"]) and not torch.equal(after["mean_constant"], before["mean_constant"])
    assert torch.equal(after["raw_noise"], before["raw_noise"]) and m.model.raw_noise.requires_grad is False
    capsys.readouterr()


def test_meta_batch_step_and_loss_decreases(cuda, capsys, monkeypatch):
    monkeypatch.setenv("DKT_TRAIN_GRAPH", "0")
    m = _model(cuda)
    ep = _episode(7)
    m.train_loop(0, [(ep, None)], None, print_freq=1000)
    loss0 = float(m._last["loss"])
    m.train_loop(1, [(ep, None)] * 19, None, print_freq=1000)
    loss20 = float(m._last["loss"])
    print("loss step 1: %.6f, step 20: %.6f" % (loss0, loss20))
    assert np.isfinite(loss0) and loss20 < loss0
    m.meta_batch = 2
    m.train_loop(2, [(_episode(s), None) for s in (1, 2, 3, 4)], None, print_freq=1000)
    assert torch.isfinite(m._last["loss"])
    capsys.readouterr()


def test_graph_replay_is_bit_equal_to_an_eager_forward_on_the_same_state(cuda):
    """The captured step, replayed: three warm-up steps, a snapshot of the whole state, then capture + replay of step four; an eager `_train_forward` of a
    second model loaded with that snapshot gives the same loss bits, and the replay did move the weights."""
    import copy
    from dkt_amd.dkt import _GraphedTrainStep
    m = _model(cuda)
    opt = m._adam(capturable=True)
    xs = [_episode(s).view(25, 3, 28, 28).to(cuda) for s in (1, 2, 3, 4)]
    y = m._targets(5, 5, cuda)
    step = _GraphedTrainStep(m, opt, xs[0], y, 1, 25, "key")
    for x in xs[:3]:
        step.run(x)
    torch.cuda.synchronize()
    assert step.graph is None
    snap = copy.deepcopy(m.state_dict())
    loss_graph = step.run(xs[3])[0].clone()
    torch.cuda.synchronize()
    assert step.graph is not None and float(step.bad) == 0.0
    moved = [k for k, v in m.state_dict().items() if v.dtype.is_floating_point and not torch.equal(v, snap[k])]
    assert "model.raw_outputscale" in moved and "model.mean_constant" in moved and len(moved) > 10
    m2 = dkt_amd.DKT(dkt_amd.backbone.Conv4S, n_way=5, n_support=1, likelihood="dirichlet").to(cuda)
    m2.load_state_dict(snap)
    loss_eager = m2._train_forward(xs[3], y, 1, 25, True)[0].detach()
    print("step 4: graph replay %.9g, eager on the same state %.9g" % (float(loss_graph), float(loss_eager)))
    assert torch.isfinite(loss_eager) and torch.equal(loss_graph, loss_eager)


@pytest.mark.parametrize("kernel_type", ["bncossim", "rbf"])
def test_correct_adapts_and_proba_batched_equals_single(cuda, kernel_type):
    m = _model(cuda, kernel_type=kernel_type)
    m.eval()
    m.n_query = 4
    top1, count, avg = m.correct(_episode(8), N=2)
    assert count == 20 and 0.0 <= top1 <= 20.0 and np.isfinite(avg) and avg != 0.0
    top1, count, avg = m.correct(_episode(8))
    assert count == 20 and avg == 0.0
    logits = m.get_logits(_episode(8))
    assert tuple(logits.shape) == (20, 5) and bool(torch.isfinite(logits).all())
    xs = torch.stack([_episode(8), _episode(9)])
    single = [m.dirichlet_proba(x) for x in xs]
    batched = m.dirichlet_proba(xs, batched=True)
    assert tuple(batched.shape) == (2, 20, 5) and torch.equal(batched[0], single[0]) and torch.equal(batched[1], single[1])
    assert float((batched.sum(-1) - 1).abs().max()) <= 1e-6 and float(batched.min()) >= 0.0
    assert not torch.equal(m.dirichlet_proba(xs[0], seed=1), single[0]) and torch.equal(m.dirichlet_proba(xs[0], seed=0), single[0])


def test_dirichlet_takes_up_to_127_rows(cuda):
    m = dkt_amd.DKT(dkt_amd.backbone.Conv4S, n_way=5, n_support=5, likelihood="dirichlet", kernel_type="rbf").to(cuda)
    with pytest.raises(ValueError, match="127"):
        m._episode_loss(torch.randn(130, 64, device=cuda), m._targets(5, 26, cuda))


def test_calibration_driver_evaluates_the_dirichlet_model(cuda, capsys, monkeypatch, tmp_path):
    """`test_uncertainty.py --likelihood dirichlet` builds its DKT without passing the flag on: io_utils.parse_args('test') makes it the default likelihood
    (configs.likelihood), so the logits are the latent means conditioned on the transformed labels -- the row-noise call runs, the Gaussian one never."""
    import test_uncertainty
    from dkt_amd import configs
    monkeypatch.setattr(configs, "likelihood", None)
    monkeypatch.setattr(configs, "amp", None)
    monkeypatch.setattr(configs, "kernel_type", configs.kernel_type)
    monkeypatch.chdir(tmp_path)
    calls = []
    real = ops.mll_rownoise
    monkeypatch.setattr(ops, "mll_rownoise", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    monkeypatch.setattr(ops, "mll", lambda *a, **k: pytest.fail("the Gaussian posterior was evaluated for a Dirichlet model"))
    ece, temperature = test_uncertainty.main(["--model", "Conv4S", "--n_episode", "2", "--repeat", "1", "--likelihood", "dirichlet"])
    assert configs.likelihood == "dirichlet" and len(calls) == 4 and len(ece) == 1 and 0.0 <= ece[0] <= 1.0          # 2 episodes x (calibration + ECE)
    capsys.readouterr()
