"""dkt_rownoise_lowrank_f32 / _bwd_f32 / _predict_f32, ops.episode_loss_dirichlet[_bn] above 127 rows and DKT(likelihood="dirichlet") on 20-way episodes,
on the GPU against the N x N float64 formulas of tests/dirichlet_model.py on E = Z Z^T (tests/dirichlet_lowrank_model.py `reference`).

Tolerances, as in tests/test_dirichlet_gpu.py: e32[q] is the largest absolute error of the float32 run of the feature-space restatement against that
float64 reference over the whole case list, per quantity, computed on the CPU (once per process); the kernels are allowed 4 x e32[q].  The end-to-end
chains do the same with their own case list (float32 torch autograd on the CPU).  Inputs are fp32-representable."""
import numpy as np
import pytest
import torch

import dirichlet_lowrank_model as lm
import dirichlet_model as dm
import dkt_amd

pytestmark = pytest.mark.gpu
ops, L = dkt_amd.ops, dkt_amd._lib
Q = lm.QUANTITIES
_t = lm.as_tensor


@pytest.fixture(scope="module")
def ref():
    f = lm.all_floors()
    print("e32:", {q: "%.3g" % v for q, v in {**f["e32"], **f["p32"]}.items()})
    return f


def _gpu(d, cuda):
    a = [_t(d[k], cuda) for k in ("z", "y", "nr", "sv", "mean", "cw")]
    out = ops.rownoise_lowrank(*a, want_grad=True)
    out["dz"] = ops.rownoise_lowrank_bwd(*a, out["state"], _t(d["gobj"], cuda))
    return out


def _errors(key, got, want, e32, names):
    err = {q: float(np.abs(got[q].double().cpu().numpy() - want[q]).max()) for q in names}
    print(key, {q: "%.3g (%.2f x e32)" % (err[q], err[q] / e32[q]) for q in names})
    for q in names:
        assert err[q] <= 4 * e32[q], (key, q, err[q], e32[q])


def _check(key, ref, cuda):
    got = _gpu(ref["cases"][key], cuda)
    assert int(got["info"].abs().max()) == 0
    _errors(key, got, ref["ref"][key], ref["e32"], Q)
    return got


@pytest.mark.parametrize("shape", lm.SHAPES, ids=str)
def test_calls_match_float64_at_their_edges(shape, ref, cuda):
    _check(("shape",) + shape, ref, cuda)


@pytest.mark.parametrize("key", [("20-way",), ("batched-y",), ("random-noise",)], ids=str)
def test_calls_match_float64_on_the_training_episode_batched_targets_and_random_noise(key, ref, cuda):
    _check(key, ref, cuda)


@pytest.mark.parametrize("key", [("shape", 2, 5, 5, 64), ("shape", 1, 2, 65, 64), ("shape", 1, 3, 127, 60), ("batched-y",)], ids=str)
def test_forced_route_agrees_with_the_resident_kernel_below_128_rows(key, ref, cuda):
    """The same inputs through ops.mll_rownoise + gram_bwd (E = Z Z^T in fp32 on the device): within the sum of both tolerances, 4 x e32 of this route plus
    4 x e32 of the resident kernel's own case list (tests/dirichlet_model.py; its dE floor carried to dZ = 2 g dE Z: an error of at most 2 |g| N max|z| times that of an element of dE)."""
    d = ref["cases"][key]
    mine = _gpu(d, cuda)
    z = _t(d["z"], cuda)
    res = ops.mll_rownoise(ops.gram(z, None, ops.KERNEL_LINEAR), _t(d["y"], cuda), _t(d["nr"], cuda), _t(d["sv"], cuda), _t(d["mean"], cuda), want_grad=True,
                           cls_weight=_t(d["cw"], cuda))
    res["dz"] = ops.gram_bwd(res["de"], z, _t(d["gobj"], cuda), w_symmetric=True)
    _, r32 = dm.floors(dm.cases())
    n = z.shape[1]
    both = dict(logp=r32["logp"], alpha=r32["alpha"], dsv=r32["dsv"], dmean=r32["dmean"],
                dz=2.0 * float(np.abs(d["gobj"]).max()) * r32["de"] * n * float(np.abs(d["z"]).max()))
    for q in Q:
        err = float((mine[q] - res[q]).abs().max())
        tol = 4 * ref["e32"][q] + 4 * both[q]
        print(key, q, "difference %.3g, allowed %.3g" % (err, tol))
        assert err <= tol, (key, q, err, tol)


@pytest.mark.parametrize("key", list(lm.predict_cases()), ids=str)
def test_prediction_matches_float64(key, ref, cuda):
    d = ref["pcases"][key]
    a = [_t(d[k], cuda) for k in ("z", "y", "nr", "sv", "mean")]
    out = ops.rownoise_lowrank(*a)
    mu, var, labels = ops.rownoise_lowrank_predict(_t(d["zq"], cuda), out["state"], a[3], a[4])
    want = ref["pref"][key]
    assert int(out["info"].abs().max()) == 0 and tuple(mu.shape) == want["mu"].shape and labels.dtype == torch.int32
    _errors(key, dict(mu=mu, var=var), want, ref["p32"], lm.PREDICT_QUANTITIES)
    # no query is left out: test_dirichlet_lowrank_host.py asserts that every float64 top-two margin is at least 100 x e32(mu)
    assert (labels.cpu().numpy() == want["mu"].argmax(1)).all()
    sure = want["var"] >= 100 * ref["p32"]["var"]
    assert sure.any() and (var.cpu().numpy()[sure] >= 0).all()
    again = ops.rownoise_lowrank_predict(_t(d["zq"], cuda), out["state"], a[3], a[4])
    assert all(torch.equal(x, y) for x, y in zip((mu, var, labels), again))


def test_first_maximum_wins_and_a_bad_noise_is_reported(cuda):
    z = torch.nn.functional.normalize(torch.randn(1, 130, 64, generator=torch.Generator().manual_seed(0)), dim=2).to(cuda)
    y = torch.zeros(3, 130, device=cuda)
    y[1:, :5] = 1.0                                            # class models 1 and 2 are the same problem: equal means, the first one wins
    nr, sv, mean = torch.ones(3, 130, device=cuda), torch.ones(3, device=cuda), torch.zeros(3, device=cuda)
    out = ops.rownoise_lowrank(z, y, nr, sv, mean)
    mu, var, labels = ops.rownoise_lowrank_predict(z[:, :5].contiguous(), out["state"], sv, mean)
    assert torch.equal(mu[:, 1], mu[:, 2]) and bool((mu[:, 1] > mu[:, 0]).all()) and labels.cpu().tolist() == [[1] * 5]
    nr[1, 7] = float("nan")
    bad = ops.rownoise_lowrank(z, y, nr, sv, mean, want_grad=True)
    info = bad["info"].cpu().numpy()
    assert info[0, 1] >= 1 and info[0, 0] == 0 and info[0, 2] == 0
    assert bool(torch.isnan(bad["logp"][0, 1])) and bool(torch.isnan(bad["alpha"][0, 1]).all()) and bool(torch.isnan(bad["state"][0, 1]).all())
    for q in ("logp", "alpha", "state"):
        assert torch.equal(bad[q][0, 0], out[q][0, 0]) and torch.equal(bad[q][0, 2], out[q][0, 2]), q


@pytest.mark.parametrize("key", [("20-way",), ("shape", 2, 5, 129, 36), ("random-noise",)], ids=str)
def test_two_runs_agree_bitwise(key, ref, cuda):
    first, again = _gpu(ref["cases"][key], cuda), _gpu(ref["cases"][key], cuda)
    for q in Q + ("state", "info"):
        assert torch.equal(first[q], again[q]), q


def test_shape_limits_reach_the_caller(cuda):
    z = torch.zeros(1, 130, 68, device=cuda)
    with pytest.raises(RuntimeError, match="DKT_ERR_SHAPE"):
        ops.rownoise_lowrank(z, torch.zeros(2, 130, device=cuda), torch.ones(2, 130, device=cuda), torch.ones(2, device=cuda), torch.zeros(2, device=cuda))
    with pytest.raises(RuntimeError, match="DKT_ERR_SHAPE"):
        ops.rownoise_lowrank(z[:, :, :64].contiguous(), torch.zeros(33, 130, device=cuda), torch.ones(33, 130, device=cuda), torch.ones(33, device=cuda),
                             torch.zeros(33, device=cuda))


# ---- end to end: features -> objective in feature space, against float64 autograd of the N x N chain ------------------------------------------
B_, C_, N_, D_ = 2, 5, 140, 64


def _chain_inputs():
    rng = np.random.default_rng(17)
    zu = dm._f32(np.stack([dm.unit_rows(rng, C_, N_ // C_, spread=0.6) for _ in range(B_)]))
    zl = dm._f32(zu * rng.uniform(0.5, 2.0, size=(B_, N_, 1)))                                      # "linear": rows that are not unit
    centres = rng.standard_normal((C_, D_))
    x = dm._f32(np.stack([np.repeat(centres, N_ // C_, 0) + 0.7 * rng.standard_normal((N_, D_)) for _ in range(B_)]))
    xh = torch.tensor(np.abs(x) + 0.5, dtype=torch.float32).to(torch.bfloat16).double().numpy()     # a ReLU-like trunk output, exact in bf16
    gamma, beta = dm._f32(1.0 + 0.2 * rng.standard_normal(D_)), dm._f32(0.1 * rng.standard_normal(D_))
    yt, nr = (a.astype(np.float64) for a in dm.dirichlet_targets(np.where(np.repeat(np.eye(C_), N_ // C_, 1) > 0, 1.0, -1.0), dtype=np.float32))
    return dict(zu=zu, zl=zl, x=x, xh=xh, gamma=gamma, beta=beta, yt=yt, nr=nr, sv=np.array([0.5, 2.0, 1.0, 3.0, 0.75]),
                mean=np.array([-2.0, -1.5, -2.5, -1.0, -3.0]), cw=np.full(C_, -1.0 / (C_ * N_)))


@pytest.fixture(scope="module")
def chains():
    """The chains in float64 and float32 torch autograd on the CPU (the N x N formulas: tests/dirichlet_lowrank_model.py `chain`, `bn_chain`), once;
    e32[q] = the largest float32 error of quantity q over the list."""
    i = _chain_inputs()
    rest = (i["sv"], i["mean"], i["yt"], i["nr"], i["cw"])
    run = {"linear": lambda dt: lm.chain(i["zl"], *rest, dt), "unit": lambda dt: lm.chain(i["zu"], *rest, dt),
           "bn": lambda dt: lm.bn_chain(i["x"], i["gamma"], i["beta"], *rest, True, dt), "no bn": lambda dt: lm.bn_chain(i["x"], i["gamma"], i["beta"], *rest, False, dt),
           "bf16": lambda dt: lm.bn_chain(i["xh"], i["gamma"], i["beta"], *rest, True, dt)}
    s = _small_inputs()                                    # the two chains of the forced route below 128 rows: part of the same list, one e32 per quantity
    run["rows100"] = lambda dt: lm.chain(s["z"], *s["rest"], dt)
    run["bn100"] = lambda dt: lm.bn_chain(s["x"], s["gamma"], s["beta"], *s["rest"], True, dt)
    out = lm.chain_floors(run)
    print("end-to-end e32:", {q: "%.3g" % v for q, v in out["e32"].items()})
    return dict(out, inputs=i, small=s)


@pytest.mark.parametrize("kind", ["linear", "unit"])
def test_episode_loss_matches_float64_autograd(kind, chains, cuda, monkeypatch):
    i = chains["inputs"]
    monkeypatch.setattr(ops, "mll_rownoise", lambda *a, **k: pytest.fail("the resident kernel was called above 127 rows"))
    zt, svt, mt = (torch.tensor(a, dtype=torch.float32, device=cuda, requires_grad=True) for a in (i["zl" if kind == "linear" else "zu"], i["sv"], i["mean"]))
    obj, logp, alpha, info, e = ops.episode_loss_dirichlet(zt, _t(i["yt"], cuda), _t(i["nr"], cuda), svt, mt, _t(i["cw"], cuda),
                                                           "linear" if kind == "linear" else "bncossim", unit_rows=kind == "unit")
    obj.sum().backward()
    assert int(info.abs().max()) == 0 and e is None and tuple(alpha.shape) == (B_, C_, N_)
    lm.compare(kind, dict(obj=obj, dz=zt.grad, dsv=svt.grad, dmean=mt.grad), chains)


@pytest.mark.parametrize("use_bn", [True, False])
def test_trunk_front_end_matches_float64_autograd(use_bn, chains, cuda, monkeypatch):
    i = chains["inputs"]
    monkeypatch.setattr(ops, "mll_rownoise", lambda *a, **k: pytest.fail("the resident kernel was called above 127 rows"))
    xt, gt, bt, svt, mt = (torch.tensor(i[k], dtype=torch.float32, device=cuda, requires_grad=True) for k in ("x", "gamma", "beta", "sv", "mean"))
    out = ops.episode_loss_dirichlet_bn(xt, gt if use_bn else None, bt if use_bn else None, _t(i["yt"], cuda), _t(i["nr"], cuda), svt, mt, _t(i["cw"], cuda),
                                        use_bn=use_bn)
    out[0].sum().backward()
    assert out[4] is None and int(out[3].abs().max()) == 0
    lm.compare("bn" if use_bn else "no bn", dict(obj=out[0], dx=xt.grad, dsv=svt.grad, dmean=mt.grad, dgamma=gt.grad, dbeta=bt.grad), chains)


def test_bf16_trunk_front_end_matches_float64_autograd(chains, cuda):
    """16-bit trunk features: everything behind the front end is fp32 (4 x e32); the gradient of x comes back in bfloat16 -- one spacing of bfloat16 at the
    float64 value on top of the fp32 bound, as tests/test_x16_gpu.py allows."""
    i, r64, e32 = chains["inputs"], chains["r64"]["bf16"], chains["e32"]
    xt = torch.tensor(i["xh"], dtype=torch.float32).to(torch.bfloat16).to(cuda).requires_grad_(True)
    gt, bt, svt, mt = (torch.tensor(i[k], dtype=torch.float32, device=cuda, requires_grad=True) for k in ("gamma", "beta", "sv", "mean"))
    out = ops.episode_loss_dirichlet_bn(xt, gt, bt, _t(i["yt"], cuda), _t(i["nr"], cuda), svt, mt, _t(i["cw"], cuda))
    out[0].sum().backward()
    assert xt.grad.dtype == torch.bfloat16 and out[4] is None
    got = dict(obj=out[0], dsv=svt.grad, dmean=mt.grad, dgamma=gt.grad, dbeta=bt.grad)
    for q, v in got.items():
        err = float(np.abs(v.detach().double().cpu().numpy() - r64[q]).max())
        print("bf16", q, "err %.3g, e32 %.3g (%.2f x)" % (err, e32[q], err / e32[q]))
        assert err <= 4 * e32[q], (q, err, e32[q])
    fi = torch.finfo(torch.bfloat16)
    ulp = np.maximum(fi.eps * np.exp2(np.floor(np.log2(np.maximum(np.abs(r64["dx"]), fi.tiny)))), fi.tiny * fi.eps)
    over = np.abs(xt.grad.double().cpu().numpy() - r64["dx"]) / (ulp + 4 * e32["dx"])
    print("bf16 dx: worst error %.3g of its bound" % over.max())
    assert over.max() <= 1.0


def _small_inputs(n=100):
    rng = np.random.default_rng(23)
    z = dm._f32(np.stack([dm.unit_rows(rng, C_, n // C_, spread=0.6) for _ in range(B_)]))
    x = dm._f32(np.stack([np.repeat(rng.standard_normal((C_, D_)), n // C_, 0) + 0.7 * rng.standard_normal((n, D_)) for _ in range(B_)]))
    gamma, beta = dm._f32(1.0 + 0.2 * rng.standard_normal(D_)), dm._f32(0.1 * rng.standard_normal(D_))
    yt, nr = (a.astype(np.float64) for a in dm.dirichlet_targets(np.where(np.repeat(np.eye(C_), n // C_, 1) > 0, 1.0, -1.0), dtype=np.float32))
    return dict(z=z, x=x, gamma=gamma, beta=beta, rest=(np.array([0.5, 2.0, 1.0, 3.0, 0.75]), np.array([-2.0, -1.5, -2.5, -1.0, -3.0]), yt, nr,
                                                         np.full(C_, -1.0 / (C_ * n))))


@pytest.mark.parametrize("front", ["rows", "bn"])
def test_forced_route_below_128_rows_through_the_episode_functions(front, chains, cuda, monkeypatch):
    """DKT_DIRICHLET_LOWRANK=force at N = 100: `episode_loss_dirichlet` (rows handed over by the Gram front end) and `episode_loss_dirichlet_bn` (by the
    trunk front end) run in feature space -- E is None, the resident kernel is not called -- and match float64 autograd of the N x N chain within 4 x e32
    (e32 over the whole end-to-end list, of which these two chains are part); the resident route on the same inputs does too, so the two agree within the
    sum of both tolerances, 8 x e32, which is asserted as well."""
    i = chains["small"]
    z, x, gamma, beta, rest = i["z"], i["x"], i["gamma"], i["beta"], i["rest"]
    yt, nr = rest[2], rest[3]
    tag = front + "100"
    real, calls = ops.mll_rownoise, []
    monkeypatch.setattr(ops, "mll_rownoise", lambda *a, **k: (calls.append(1), real(*a, **k))[1])

    def run():
        svt, mt = (torch.tensor(a, dtype=torch.float32, device=cuda, requires_grad=True) for a in rest[:2])
        if front == "rows":
            zt = torch.tensor(z, dtype=torch.float32, device=cuda, requires_grad=True)
            out = ops.episode_loss_dirichlet(zt, _t(yt, cuda), _t(nr, cuda), svt, mt, _t(rest[4], cuda), "bncossim", unit_rows=True)
            out[0].sum().backward()
            return out[4], dict(obj=out[0], dz=zt.grad, dsv=svt.grad, dmean=mt.grad)
        xt, gt, bt = (torch.tensor(a, dtype=torch.float32, device=cuda, requires_grad=True) for a in (x, gamma, beta))
        out = ops.episode_loss_dirichlet_bn(xt, gt, bt, _t(yt, cuda), _t(nr, cuda), svt, mt, _t(rest[4], cuda))
        out[0].sum().backward()
        return out[4], dict(obj=out[0], dx=xt.grad, dsv=svt.grad, dmean=mt.grad, dgamma=gt.grad, dbeta=bt.grad)

    monkeypatch.setenv("DKT_DIRICHLET_LOWRANK", "force")
    e, forced = run()
    assert e is None and calls == []
    lm.compare(tag, forced, chains)
    monkeypatch.delenv("DKT_DIRICHLET_LOWRANK")
    e, resident = run()
    assert e is not None and calls == [1]
    lm.compare(tag, resident, chains)
    for q, v in forced.items():
        diff = float((v - resident[q]).detach().abs().max())
        print(front, q, "forced - resident %.3g (%.2f x e32)" % (diff, diff / chains["e32"][q]))
        assert diff <= 8 * chains["e32"][q], (q, diff)


# ---- the DKT surface on 20-way episodes ----------------------------------------------------------------------------------------------------------
def _episode(seed, n_way=20, per_class=20):
    return torch.rand(n_way, per_class, 3, 28, 28, generator=torch.Generator().manual_seed(seed))


def _model(cuda, n_way=20, n_support=5, **kw):
    torch.manual_seed(0)
    m = dkt_amd.DKT(dkt_amd.backbone.Conv4S, n_way=n_way, n_support=n_support, likelihood="dirichlet", **kw).to(cuda)
    m.train()
    return m


def _no_resident(monkeypatch):
    monkeypatch.setattr(ops, "mll_rownoise", lambda *a, **k: pytest.fail("the resident kernel was called for a 20-way episode"))
    monkeypatch.setattr(ops, "mll", lambda *a, **k: pytest.fail("the Gaussian marginal likelihood was called"))
    monkeypatch.setenv("DKT_TRAIN_GRAPH", "0")


def test_episode_loss_of_a_400_row_episode_equals_float64_and_fills_the_gradients(cuda, ref, monkeypatch):
    _no_resident(monkeypatch)
    m = _model(cuda)
    n = 400
    y = m._targets(20, 20, cuda)
    z = m._embed(_episode(1).view(n, 3, 28, 28).to(cuda))
    loss, aux = m._episode_loss(z, y)
    assert aux["e"] is None and int(aux["info"].abs().max()) == 0 and tuple(aux["alpha"].shape) == (1, 20, n)
    sv, mean, _ = m._hypers()
    yt, nr = dm.dirichlet_targets(y.cpu().numpy(), dtype=np.float32)
    cw = np.full(20, -1.0 / (20 * n))
    d = dict(z=z.detach().double().cpu().numpy()[None], y=yt.astype(np.float64), nr=nr.astype(np.float64), sv=sv.detach().double().cpu().numpy(),
             mean=mean.detach().double().cpu().numpy().reshape(-1), cw=cw, gobj=np.ones(1))
    want = float((lm.solve(d, np.float64)["logp"] * cw).sum())
    # every logp within 4 x e32(logp); the loss is their mean over the 20 classes, divided by N
    tol = 4 * ref["e32"]["logp"] / n
    print("loss %.9g, float64 %.9g, difference %.3g (allowed %.3g)" % (float(loss.detach()), want, abs(float(loss.detach()) - want), tol))
    assert abs(float(loss.detach()) - want) <= tol
    loss.backward()
    grads = [p.grad for p in m.feature_extractor.parameters()] + [m.model.raw_outputscale.grad, m.model.mean_constant.grad]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads) and float(m.model.raw_outputscale.grad.abs().max()) > 0
    assert any(float(p.grad.abs().max()) > 0 for p in m.feature_extractor.parameters())


@pytest.mark.parametrize("meta_batch", [1, 2])
def test_train_loop_on_20_way_episodes_never_calls_the_resident_kernel(cuda, capsys, monkeypatch, meta_batch):
    _no_resident(monkeypatch)
    m = _model(cuda)
    m.meta_batch = meta_batch
    before = {k: v.clone() for k, v in m.model.state_dict().items()}
    m.train_loop(0, [(_episode(s), None) for s in range(1, 1 + 2 * meta_batch)], None, print_freq=1000)
    assert torch.isfinite(m._last["loss"]) and 0.0 <= float(m._last["acc_query"]) <= 100.0
    assert all(bool(torch.isfinite(v).all()) for v in m.state_dict().values() if v.dtype.is_floating_point)
    after = m.model.state_dict()
    assert not torch.equal(after["raw_outputscale"], before["raw_outputscale"]) and not torch.equal(after["mean_constant"], before["mean_constant"])
    capsys.readouterr()


def test_correct_and_proba_on_an_8_shot_20_way_episode(cuda, monkeypatch):
    _no_resident(monkeypatch)
    m = _model(cuda, n_support=8)
    m.eval()
    m.n_query = 4
    top1, count, avg = m.correct(_episode(8, per_class=12), N=2)
    assert count == 80 and 0.0 <= top1 <= 80.0 and np.isfinite(avg) and avg != 0.0
    top1, count, avg = m.correct(_episode(8, per_class=12))
    assert count == 80 and avg == 0.0
    logits = m.get_logits(_episode(8, per_class=12))
    assert tuple(logits.shape) == (80, 20) and bool(torch.isfinite(logits).all())
    assert m.test_loop([(_episode(8, per_class=12), None)]) >= 0.0
    xs = torch.stack([_episode(8, per_class=12), _episode(9, per_class=12)])
    single = [m.dirichlet_proba(x) for x in xs]
    batched = m.dirichlet_proba(xs, batched=True)
    assert tuple(batched.shape) == (2, 80, 20) and torch.equal(batched[0], single[0]) and torch.equal(batched[1], single[1])
    assert float((batched.sum(-1) - 1).abs().max()) <= 1e-6 and float(batched.min()) >= 0.0


def test_5_way_model_still_takes_the_resident_kernel_and_other_kernels_still_stop_at_127_rows(cuda, capsys, monkeypatch):
    calls = []
    real = ops.mll_rownoise
    monkeypatch.setattr(ops, "mll_rownoise", lambda *a, **k: (calls.append(bool(k.get("want_grad"))), real(*a, **k))[1])
    monkeypatch.setattr(ops, "rownoise_lowrank", lambda *a, **k: pytest.fail("the feature-space route was taken below 128 rows"))
    monkeypatch.setenv("DKT_TRAIN_GRAPH", "0")
    m = _model(cuda, n_way=5, n_support=1)
    m.train_loop(0, [(_episode(s, 5, 5), None) for s in (1, 2)], None, print_freq=1000)
    assert calls.count(True) == 2 and calls.count(False) == 2, calls
    capsys.readouterr()
    big = _model(cuda, kernel_type="rbf")
    with pytest.raises(ValueError, match="127"):
        big._episode_loss(torch.randn(400, 64, device=cuda), big._targets(20, 20, cuda))
    wide = _model(cuda, kernel_type="linear")
    with pytest.raises(ValueError, match="127"):                # D > 64: no feature-space route
        wide._episode_loss(torch.randn(400, 128, device=cuda), wide._targets(20, 20, cuda))
