"""dkt_laplace_grad_f32 / ops.laplace_objective / DKT(likelihood="bernoulli") on the GPU against the float64 restatement (tests/laplace_grad_model.py;
test_laplace_grad_host.py checks that one against finite differences and scikit-learn).

Tolerances follow docs/LAPLACE.md: e32 is the largest absolute error of the float32 run of the restatement against its float64 run over the whole
case list, per quantity (lml, dK, dscale), computed here on the CPU; the kernel is allowed 4 x e32.  Inputs are fp32-representable K, and f_hat is the
polished float64 mode rounded to fp32 (both runs and the kernel get the same f_hat)."""
import ctypes

import numpy as np
import pytest
import torch

import dkt_amd
import laplace_grad_model as gm
import laplace_model as lm

pytestmark = pytest.mark.gpu
ops, L = dkt_amd.ops, dkt_amd._lib
QUANTITIES = ("lml", "dk", "dscale")
# (B, C, N): 1, the 16-lane / wave / two-rows-per-lane boundaries of the kernel (15 16 17, 33, 63 64 65), its largest size, the 5-way 5-shot episode
SHAPES = [(1, 1, 1), (2, 5, 15), (2, 5, 16), (2, 5, 17), (1, 5, 33), (1, 2, 63), (1, 2, 64), (1, 2, 65), (1, 3, 127), (3, 5, 25)]


def _shape_case(b_, c, n, ls=0.1, spread=0.1, scale=None, per_class=False):
    rng = np.random.default_rng(1000 * n + 10 * c + b_)
    cc = max(c, 2)
    shots = (n + cc - 1) // cc
    rows = np.sort(rng.permutation(cc * shots)[:n])
    cls = rows // shots
    k = np.stack([lm.rbf(z, z, ls) for z in (lm.clustered(rng, cc, shots, 1, 64, spread)[0][rows] for _ in range(b_))])
    k = k.astype(np.float32).astype(np.float64)
    if per_class:                                         # every class its own matrix: K_c = K ** (1 + c / 4) (element-wise powers of an RBF matrix are RBF matrices)
        k = np.stack([k ** (1.0 + ci / 4.0) for ci in range(c)], 1).astype(np.float32).astype(np.float64)
    y = np.stack([cls == ci for ci in range(c)]).astype(np.float64)
    return dict(k=k, y=y, scale=scale, cw=np.linspace(0.5, 1.5, c) * -1.0 / n)


def _solve(d, dtype):
    lml, dk, dscale = gm.laplace_grad(d["k"], d["y"], d["f"], d["cw"], d["scale"], dtype=dtype)
    return dict(lml=lml, dk=dk, dscale=dscale)


@pytest.fixture(scope="module")
def ref():
    cases = {("shape",) + s: _shape_case(*s) for s in SHAPES}
    cases[("shared-scaled",)] = _shape_case(2, 20, 100, scale=np.tile([0.5, 5.0], 10))
    cases[("per-class",)] = _shape_case(2, 5, 25, ls=0.3, scale=np.array([0.5, 5.0, 1.0, 2.0, 0.5]), per_class=True)
    ni = lm.build_case(lm.NEAR_IDENTITY_CASE)
    cases[("near-identity",)] = dict(k=ni["k"], y=ni["y"], scale=None, cw=np.full(5, -1.0 / 125))
    for d in cases.values():
        d["f"] = gm.modes(d["k"], d["y"], d["scale"]).astype(np.float32).astype(np.float64)
    r64 = {k: _solve(d, np.float64) for k, d in cases.items()}
    r32 = {k: _solve(d, np.float32) for k, d in cases.items()}
    e32 = {q: max(float(np.abs(r32[k][q].astype(np.float64) - r64[k][q]).max()) for k in cases) for q in QUANTITIES}
    print("e32:", {q: "%.3g" % v for q, v in e32.items()})
    return dict(cases=cases, r64=r64, e32=e32)


def _t(a, cuda):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(cuda)


def _gpu(d, cuda):
    lml, dk, dscale = ops.laplace_grad(_t(d["k"], cuda), _t(d["y"], cuda), _t(d["f"], cuda), _t(d["cw"], cuda), _t(d["scale"], cuda))
    return dict(lml=lml, dk=dk, dscale=dscale)


def _check(key, ref, cuda):
    got = _gpu(ref["cases"][key], cuda)
    err = {q: float(np.abs(got[q].double().cpu().numpy() - ref["r64"][key][q]).max()) for q in QUANTITIES}
    print(key, {q: "%.3g (%.2f x e32)" % (err[q], err[q] / ref["e32"][q]) for q in QUANTITIES})
    for q in QUANTITIES:
        assert err[q] <= 4 * ref["e32"][q], (key, q, err[q], ref["e32"][q])
    return got


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_kernel_matches_float64_at_its_edges(shape, ref, cuda):
    _check(("shape",) + shape, ref, cuda)


@pytest.mark.parametrize("key", [("shared-scaled",), ("per-class",), ("near-identity",)], ids=str)
def test_kernel_matches_float64_scaled_per_class_and_near_identity(key, ref, cuda):
    _check(key, ref, cuda)


@pytest.mark.parametrize("key", [("shape", 3, 5, 25), ("shared-scaled",), ("shape", 2, 5, 17)], ids=str)
def test_two_runs_and_both_forms_agree_bitwise(key, ref, cuda):
    d = ref["cases"][key]
    b_, c = d["k"].shape[0], d["y"].shape[0]
    shared, again = _gpu(d, cuda), _gpu(d, cuda)
    per_class = _gpu(dict(d, k=np.repeat(d["k"][:, None], c, 1), y=np.repeat(d["y"][None], b_, 0)), cuda)
    for q in QUANTITIES:
        assert torch.equal(shared[q], again[q]), q
    assert torch.equal(shared["lml"], per_class["lml"]) and torch.equal(shared["dscale"], per_class["dscale"])
    acc = per_class["dk"][:, 0].clone()
    for ci in range(1, c):                                 # the classes in index order
        acc = acc + per_class["dk"][:, ci]
    assert torch.equal(shared["dk"], acc)


def test_shape_limits_and_null_pointers_do_not_launch(cuda):
    lib = L.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def run(c, n, null=None):
        k, y, f, cw = torch.eye(n, device=cuda)[None].contiguous(), torch.zeros(c, n, device=cuda), torch.zeros(1, c, n, device=cuda), torch.ones(c, device=cuda)
        lml, dk, ds = (torch.full(s, -7.0, device=cuda) for s in ((1, c), (1, n, n), (1, c)))
        nbytes = int(lib.dkt_laplace_grad_workspace_bytes(1, c, n))
        ws = torch.empty(nbytes // 4, device=cuda)
        args = dict(K=p(k), Y=p(y), f=p(f), lml=p(lml), dK=p(dk), ws=p(ws))
        if null:
            args[null] = None
        st = lib.dkt_laplace_grad_f32(args["K"], n * n, 0, None, args["Y"], 0, args["f"], p(cw), args["lml"], args["dK"], p(ds), 1, c, n, args["ws"], nbytes, None)
        torch.cuda.synchronize()
        return st, all(bool((o == -7).all()) for o in (lml, dk, ds))

    assert run(5, 128) == (-5, True) and run(33, 10) == (-5, True)
    for null in ("K", "Y", "f", "lml", "dK"):
        assert run(5, 10, null) == (-1, True), null
    assert run(5, 10, "ws") == (-3, True)                  # a shared K needs the workspace
    assert run(32, 127) == (0, False)
    assert lib.dkt_laplace_grad_f32(None, 0, 0, None, None, 0, None, None, None, None, None, 1, 5, 0, None, 0, None) == -1
    with pytest.raises(RuntimeError, match="DKT_ERR_SHAPE"):
        ops.laplace_grad(torch.eye(128, device=cuda)[None], torch.zeros(2, 128, device=cuda), torch.zeros(1, 2, 128, device=cuda), None)


# ---- end to end: features -> kernel -> objective, against float64 autograd through the fixed point ------------------------------------------
def _obj_from_k(k, yt, cwt, y, dtype):
    """obj [B] from the covariances k [B,C,N,N] (torch, differentiable): the mode by numpy, one differentiable Newton step from it, lml there."""
    f0 = torch.tensor(gm.modes(k.detach().double().numpy()[:, :, :, :], y), dtype=dtype)
    eye = torch.eye(k.shape[-1], dtype=dtype)
    pi = torch.sigmoid(f0)
    w = pi * (1 - pi)
    b = w * f0 + (yt - pi)
    bm = eye + w.sqrt().unsqueeze(-1) * k * w.sqrt().unsqueeze(-2)
    a = b - w.sqrt() * torch.linalg.solve(bm, (w.sqrt() * (k @ b.unsqueeze(-1)).squeeze(-1)).unsqueeze(-1)).squeeze(-1)
    f = (k @ a.unsqueeze(-1)).squeeze(-1)
    pi = torch.sigmoid(f)
    w = pi * (1 - pi)
    bm = eye + w.sqrt().unsqueeze(-1) * k * w.sqrt().unsqueeze(-2)
    lml = (-0.5 * ((yt - pi) * f).sum(-1) - torch.nn.functional.softplus(-(2 * yt - 1) * f).sum(-1)
           - torch.log(torch.diagonal(torch.linalg.cholesky(bm), dim1=-2, dim2=-1)).sum(-1))
    obj = (lml * cwt).sum(1)
    return obj


def _chain(z, sv, ls, y, cw, kind, dtype):
    """Float64 (or float32) torch on the CPU: K_c(z) -> the mode (numpy, no autograd) -> ONE differentiable Newton step from it (the Newton map's derivative
    with respect to f vanishes at its fixed point, so the step carries the exact d f_hat / d K) -> lml at that f -> obj, and autograd back to z, sv, ls."""
    z = torch.tensor(z, dtype=dtype, requires_grad=True)
    sv = torch.tensor(sv, dtype=dtype, requires_grad=True)
    ls = torch.tensor(ls, dtype=dtype, requires_grad=True)
    yt, cwt = torch.tensor(y, dtype=dtype), torch.tensor(cw, dtype=dtype)
    if kind == "linear":
        k = sv.view(1, -1, 1, 1) * (z @ z.transpose(1, 2)).unsqueeze(1)
    else:
        d2 = ((z.unsqueeze(2) - z.unsqueeze(1)) ** 2).sum(-1)
        k = sv.view(1, -1, 1, 1) * torch.exp(-0.5 * d2.unsqueeze(1) / ls.view(1, -1, 1, 1) ** 2)
    obj = _obj_from_k(k, yt, cwt, y, dtype)
    obj.sum().backward()
    return dict(obj=obj.detach().double().numpy(), dz=z.grad.double().numpy(), dsv=sv.grad.double().numpy(),
                dls=None if ls.grad is None else ls.grad.double().numpy())


@pytest.mark.parametrize("kind", ["linear", "rbf"])
def test_objective_end_to_end_matches_float64_autograd(kind, cuda):
    rng = np.random.default_rng(3)
    z = np.stack([lm.clustered(rng, 5, 5, 1, 64, 0.3)[0] for _ in range(2)]).astype(np.float32).astype(np.float64)          # [2, 25, 64], unit rows
    sv, ls = np.array([0.5, 2.0, 1.0, 3.0, 0.7]), np.array([0.6, 0.8, 1.0, 1.2, 0.9])
    y, cw = lm.one_vs_rest(5, 5), np.full(5, -1.0 / 125)
    r64, r32 = _chain(z, sv, ls, y, cw, kind, torch.float64), _chain(z, sv, ls, y, cw, kind, torch.float32)
    zt, svt, lst = (torch.tensor(a, dtype=torch.float32, device=cuda, requires_grad=True) for a in (z, sv, ls))
    obj, lml, iters, _ = ops.episode_loss_laplace(zt, _t(y, cuda), svt, _t(cw, cuda), "bncossim" if kind == "linear" else "rbf", lengthscale=lst,
                                                  unit_rows=kind == "linear")
    obj.sum().backward()
    got = dict(obj=obj, dz=zt.grad, dsv=svt.grad, dls=lst.grad)
    assert int(iters.max()) < 100
    for q in ("obj", "dz", "dsv") + (("dls",) if kind == "rbf" else ()):
        e32 = float(np.abs(r32[q] - r64[q]).max())
        err = float(np.abs(got[q].detach().double().cpu().numpy() - r64[q]).max())
        print(kind, q, "err %.3g, float32 CPU chain %.3g (%.2f x)" % (err, e32, err / e32))
        assert err <= 4 * e32, (kind, q, err, e32)


def _bn_chain(x, gamma, beta, sv, y, cw, use_bn, dtype, eps=1e-5):
    """The fused front end in torch on the CPU: [train-mode BatchNorm1d per episode +] F.normalize + linear kernel, then the chain above."""
    x, sv = (torch.tensor(a, dtype=dtype, requires_grad=True) for a in (x, sv))
    gamma, beta = (torch.tensor(a, dtype=dtype, requires_grad=True) for a in (gamma, beta))
    yt, cwt = torch.tensor(y, dtype=dtype), torch.tensor(cw, dtype=dtype)
    h = x
    if use_bn:
        h = (x - x.mean(1, keepdim=True)) / torch.sqrt(x.var(1, unbiased=False, keepdim=True) + eps) * gamma + beta
    z = torch.nn.functional.normalize(h, p=2, dim=2)
    obj = _obj_from_k(sv.view(1, -1, 1, 1) * (z @ z.transpose(1, 2)).unsqueeze(1), yt, cwt, y, dtype)
    obj.sum().backward()
    out = dict(obj=obj.detach().double().numpy(), dx=x.grad.double().numpy(), dsv=sv.grad.double().numpy())
    if use_bn:
        out.update(dgamma=gamma.grad.double().numpy(), dbeta=beta.grad.double().numpy())
    return out


@pytest.mark.parametrize("use_bn, fused_stats", [(True, "1"), (True, "0"), (False, "1")])
def test_fused_front_end_gradients_match_float64_autograd(use_bn, fused_stats, cuda, monkeypatch):
    """ops.episode_loss_laplace_bn (the default training path of bncossim / cossim): dX, dgamma, dbeta, d outputscale through dkt_gram_bn_bwd_f32 fed with
    dE, against float64 autograd; bound 4 x the error of the same chain in float32 on the CPU."""
    monkeypatch.setenv("DKT_FUSED_STATS", fused_stats)
    rng = np.random.default_rng(5)
    centres = rng.standard_normal((5, 64))
    x = np.stack([np.repeat(centres, 5, 0) + 0.7 * rng.standard_normal((25, 64)) for _ in range(2)]).astype(np.float32).astype(np.float64)
    gamma, beta = 1.0 + 0.2 * rng.standard_normal(64), 0.1 * rng.standard_normal(64)
    sv, y, cw = np.array([0.5, 2.0, 1.0, 3.0, 0.7]), lm.one_vs_rest(5, 5), np.full(5, -1.0 / 125)
    gamma, beta = gamma.astype(np.float32).astype(np.float64), beta.astype(np.float32).astype(np.float64)
    r64, r32 = (_bn_chain(x, gamma, beta, sv, y, cw, use_bn, dt) for dt in (torch.float64, torch.float32))
    xt, gt, bt, svt = (torch.tensor(a, dtype=torch.float32, device=cuda, requires_grad=True) for a in (x, gamma, beta, sv))
    out = ops.episode_loss_laplace_bn(xt, gt if use_bn else None, bt if use_bn else None, _t(y, cuda), svt, _t(cw, cuda), use_bn=use_bn)
    out[0].sum().backward()
    got = dict(obj=out[0], dx=xt.grad, dsv=svt.grad, dgamma=gt.grad, dbeta=bt.grad)
    for q in r64:
        e32 = float(np.abs(r32[q] - r64[q]).max())
        err = float(np.abs(got[q].detach().double().cpu().numpy() - r64[q]).max())
        print("bn" if use_bn else "no bn", "fused stats " + fused_stats, q, "err %.3g, float32 CPU chain %.3g (%.2f x)" % (err, e32, err / e32))
        assert err <= 4 * e32, (use_bn, q, err, e32)


def test_laplace_objective_is_the_raw_calls_and_differentiable(cuda, ref):
    d = ref["cases"][("shape", 3, 5, 25)]
    k, y, cw = _t(d["k"], cuda).requires_grad_(True), _t(d["y"], cuda), _t(d["cw"], cuda)
    sc = torch.tensor([0.5, 5.0, 1.0, 2.0, 0.5], device=cuda, requires_grad=True)
    obj, lml, iters = ops.laplace_objective(k, y, cw, scale=sc)
    md = ops.laplace_mode(k.detach().unsqueeze(1) * sc.detach().view(1, -1, 1, 1), y)
    lml2, dk, dscale = ops.laplace_grad(k.detach(), y, md["f"], cw, sc.detach())
    gout = torch.tensor([1.0, -2.0, 0.5], device=cuda)
    (obj * gout).sum().backward()
    assert torch.equal(lml, lml2) and torch.equal(iters, md["iters"]) and torch.equal(obj, ops.objective(lml2, cw))
    assert torch.equal(k.grad, dk * gout.view(-1, 1, 1)) and torch.allclose(sc.grad, (gout.view(-1, 1) * dscale).sum(0), rtol=1e-6, atol=0)


# ---- the DKT surface --------------------------------------------------------------------------------------------------------------------------
def _episode(seed, n_way=5, per_class=5):
    return torch.rand(n_way, per_class, 3, 28, 28, generator=torch.Generator().manual_seed(seed))


def _train(cuda, monkeypatch, graph, loader, **kw):
    monkeypatch.setenv("DKT_TRAIN_GRAPH", graph)
    torch.manual_seed(0)
    m = dkt_amd.DKT(dkt_amd.backbone.Conv4S, n_way=5, n_support=1, likelihood="bernoulli", **kw).to(cuda)
    m.train()
    m.train_loop(0, loader, None, print_freq=1000)
    return m


def test_bernoulli_adam_step_eager_and_graph(cuda, capsys, monkeypatch):
    """5-way 1-shot, 4 queries: N = 25 rows through the fused front end.  A first step under DKT_TRAIN_GRAPH=1 is one of the graph's eager warm-up steps (side
    stream, capturable Adam): its loss has the eager loop's bits.  Four steps (the fourth is a graph replay) agree with the eager loop to 1e-4 only: eager
    runs the fused Adam, graph mode the capturable one.  The replay itself is held to the bit in the next test."""
    one = [(_episode(1), None)]
    e1, g1 = _train(cuda, monkeypatch, "0", one), _train(cuda, monkeypatch, "1", one)
    print("one step: eager %.9g graph %.9g" % (float(e1._last["loss"]), float(g1._last["loss"])))
    assert torch.isfinite(e1._last["loss"]) and torch.equal(e1._last["loss"], g1._last["loss"])
    assert e1.model.raw_outputscale.grad is not None and e1.model.raw_noise.requires_grad is False
    four = [(_episode(s), None) for s in (1, 2, 3, 4)]
    e4, g4 = _train(cuda, monkeypatch, "0", four), _train(cuda, monkeypatch, "1", four)
    le, lg = float(e4._last["loss"]), float(g4._last["loss"])
    print("four steps: eager %.9g graph %.9g" % (le, lg))
    assert abs(le - lg) < 1e-4 * abs(le)
    capsys.readouterr()


def test_bernoulli_graph_replay_is_bit_equal_to_an_eager_forward_on_the_same_state(cuda):
    """The captured step, replayed: three warm-up steps, a snapshot of the whole state, then capture + replay of step four; an eager `_train_forward` of a
    second model loaded with that snapshot gives the same loss bits, and the replay did move the weights."""
    import copy
    from dkt_amd.dkt import _GraphedTrainStep
    torch.manual_seed(0)
    m = dkt_amd.DKT(dkt_amd.backbone.Conv4S, n_way=5, n_support=1, likelihood="bernoulli").to(cuda)
    m.train()
    opt = torch.optim.Adam([{'params': m.model.parameters(), 'lr': 1e-4}, {'params': m.feature_extractor.parameters(), 'lr': 1e-3}], capturable=True)
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
    assert "model.raw_outputscale" in moved and len(moved) > 10
    m2 = dkt_amd.DKT(dkt_amd.backbone.Conv4S, n_way=5, n_support=1, likelihood="bernoulli").to(cuda)
    m2.load_state_dict(snap)
    loss_eager = m2._train_forward(xs[3], y, 1, 25, True)[0].detach()
    print("step 4: graph replay %.9g, eager on the same state %.9g" % (float(loss_graph), float(loss_eager)))
    assert torch.isfinite(loss_eager) and torch.equal(loss_graph, loss_eager)


@pytest.mark.parametrize("kernel_type", ["bncossim", "rbf"])
def test_bernoulli_loss_decreases_and_correct_adapts(cuda, capsys, monkeypatch, kernel_type):
    ep = _episode(7)
    first = _train(cuda, monkeypatch, "0", [(ep, None)], kernel_type=kernel_type)
    loss0 = float(first._last["loss"])
    first.train_loop(1, [(ep, None)] * 19, None, print_freq=1000)
    loss20 = float(first._last["loss"])
    print(kernel_type, "loss step 1: %.6f, step 20: %.6f" % (loss0, loss20))
    assert np.isfinite(loss0) and loss20 < loss0
    first.eval()
    first.n_query = 4
    assert first.laplace == "deep"
    top1, count, avg = first.correct(_episode(8), N=2)
    assert count == 20 and 0.0 <= top1 <= 20.0 and np.isfinite(avg) and avg != 0.0
    top1, count, avg = first.correct(_episode(8))
    assert count == 20 and avg == 0.0
    capsys.readouterr()


def test_bernoulli_takes_up_to_127_rows(cuda):
    m = dkt_amd.DKT(dkt_amd.backbone.Conv4S, n_way=5, n_support=5, likelihood="bernoulli", kernel_type="rbf").to(cuda)
    with pytest.raises(ValueError, match="127"):
        m._episode_loss(torch.randn(130, 64, device=cuda), m._targets(5, 26, cuda))
