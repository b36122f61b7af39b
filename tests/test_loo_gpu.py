"""dkt_loo_f32 and everything built on it, on the GPU (docs/LOO.md): ops.loo against the float64 model of tests/loo_model.py at the kernel's tile edges, both
layouts of E, shared and per-episode targets, every class-weight form; the jitter ladder and the poisoned problem; the training episodes ops.episode_loss_loo /
_bn against float64 autograd; DKT(objective="loo"); the guard arena on operands that are not 16-byte aligned; bitwise reproducibility.

Tolerance: the float32 CPU evaluation of the same closed form gives the floor of a case group (the largest error over its cases, per quantity,
max |got - ref| / max |ref|); the bound is 4 x that floor.  Nothing is skipped.  Measured floors and GPU maxima: docs/LOO.md."""
import numpy as np
import pytest
import torch

import dkt_amd
from dkt_amd import backbone, ops

import guard_arena as ga
import loo_model as lm

pytestmark = pytest.mark.gpu


def _dev(x, dev):
    return None if x is None else torch.tensor(np.asarray(x), dtype=torch.float32, device=dev)


def _call(inp, dev, want_grad=True, **kw):
    return ops.loo(_dev(inp["e"], dev), _dev(inp["y"], dev), _dev(inp["sv"], dev), _dev(inp["mean"], dev), _dev(inp["noise"], dev), want_grad=want_grad,
                   cls_weight=_dev(inp["cw"], dev), **kw)


def _np(out):
    return {k: None if v is None else v.detach().cpu().numpy() for k, v in out.items()}


# ---- against the float64 model -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(lm.CASES)), ids=[repr(k) for k in lm.CASES])
def test_loo_matches_float64(index, cuda):
    kase = lm.CASES[index]
    ref, e32 = lm.reference(index)
    floor = lm.floors(kase.group)
    got = _np(_call(kase.inputs(), cuda))
    assert (got["info"] == 0).all() and (got["jitter"] == 0).all()
    assert got["w"].shape == ref["w"].shape and np.array_equal(got["w"], np.swapaxes(got["w"], -1, -2))
    err = lm.errors(got, ref, lm.VALUES + lm.GRADS)
    for q in lm.VALUES + lm.GRADS:
        print("LOO %r %s: gpu %.3e  f32 %.3e  floor(%s) %.3e  ratio %.2f" % (kase, q, err[q], e32[q], kase.group, floor[q], err[q] / floor[q] if floor[q] else 0.0))
    bad = [q for q in lm.VALUES + lm.GRADS if not err[q] <= lm.BOUND * floor[q]]
    assert not bad, {q: (err[q], lm.BOUND * floor[q]) for q in bad}


def test_forward_only_call_equals_the_values_of_the_gradient_call(cuda):
    inp = lm.CASES[7].inputs()
    a, b = _call(inp, cuda, want_grad=False), _call(inp, cuda, want_grad=True)
    assert a["w"] is None and a["dsv"] is None and a["dmean"] is None and a["dnoise"] is None
    for q in lm.VALUES + ("jitter", "info"):
        assert torch.equal(a[q], b[q]), q


@pytest.mark.parametrize("index", [7, 16, 40], ids=lambda i: repr(lm.CASES[i]))
def test_two_runs_give_the_same_bits(index, cuda):
    inp = lm.CASES[index].inputs()
    a, b = _call(inp, cuda), _call(inp, cuda)
    for q in a:
        assert torch.equal(a[q].view(torch.int32), b[q].view(torch.int32)), q


def test_shared_w_is_the_class_sum_of_the_per_class_w(cuda):
    """A shared E's W[b] is the sum over the classes, in index order, of what the per-class layout writes for the same matrices: bit for bit."""
    kase = lm.Case(33, 5, 3, False, True, "mixed", 8, "rbf", 0.1, 1.0)
    inp = kase.inputs()
    shared = _call(inp, cuda)
    inp4 = dict(inp, e=np.ascontiguousarray(np.broadcast_to(inp["e"][:, None], (3, 5, 33, 33))))
    per = _call(inp4, cuda)
    acc = per["w"][:, 0].clone()
    for c in range(1, 5):
        acc = acc + per["w"][:, c]
    assert torch.equal(acc, shared["w"])
    for q in lm.VALUES + ("dsv", "dmean", "dnoise"):
        assert torch.equal(per[q], shared[q]), q


# ---- the jitter ladder ------------------------------------------------------------------------------------------------------------------------------
def test_rank_deficient_matrix_climbs_the_ladder(cuda):
    """A rank-3 E at N = 20 without noise: attempt 0 meets a pivot that is not positive, a rung of the ladder factors (kappa ~ 1e7 there: the values are finite,
    no accuracy is claimed for them)."""
    z = np.random.default_rng(3).standard_normal((2, 20, 3))
    e = (z @ np.swapaxes(z, -1, -2)).astype(np.float32)
    sv, mean, _ = lm.hypers(3, 1.0, 1.0)
    inp = dict(e=e, y=lm.targets(3, 20), sv=sv, mean=mean, noise=np.zeros(3, np.float32), cw=None)
    out = _np(_call(inp, cuda, jitter0=1e-6, max_tries=3))
    print("jitter ladder: jitter_used %s" % sorted(set(out["jitter"].reshape(-1).tolist())))
    assert (out["info"] == 0).all() and (out["jitter"] > 0).all()
    assert set(np.round(np.log10(out["jitter"].reshape(-1).astype(np.float64))).astype(int).tolist()) <= {-6, -5, -4}
    for q in lm.VALUES + lm.GRADS:
        assert np.isfinite(out[q]).all(), q


@pytest.mark.parametrize("per_class", [True, False], ids=["perclass", "shared"])
def test_a_matrix_that_is_not_positive_definite_poisons_itself_only(per_class, cuda):
    kase = lm.Case(20, 4, 3, per_class, True, "mixed", 8, "rbf", 0.1, 1.0)
    inp = kase.inputs()
    clean = _np(_call(inp, cuda))
    e = inp["e"].copy()
    if per_class:
        e[1, 2, 0, 0] = -1.0
        hit = np.zeros((3, 4), bool)
        hit[1, 2] = True
    else:
        e[1, 0, 0] = -1.0
        hit = np.zeros((3, 4), bool)
        hit[1] = True
    out = _np(_call(dict(inp, e=e), cuda))
    assert ((out["info"] != 0) == hit).all() and (out["info"][hit] == 1).all()
    for q in lm.VALUES + ("dsv", "dmean", "dnoise"):
        assert np.isnan(out[q][hit]).all(), q
        assert np.array_equal(out[q][~hit], clean[q][~hit]), q
    whit = hit if per_class else hit.any(1)
    assert np.isnan(out["w"][whit]).all() and np.array_equal(out["w"][~whit], clean["w"][~whit])
    assert np.array_equal(out["jitter"][~hit], clean["jitter"][~hit]) and np.allclose(out["jitter"][hit], 1e-4)      # the last rung was tried


# ---- the training episodes against float64 autograd ----------------------------------------------------------------------------------------------
E2E_SEEDS = (0, 1, 2)            # one group per front end: the floor is the largest float32 error over its three draws


def _e2e_inputs(front, seed, b=2, n=25, d=64, c=5):
    rng = np.random.default_rng(50 + seed)
    sv, mean, noise = lm.hypers(c, 1.0, 0.1)
    y = lm.targets(c, n)
    cw = np.full(c, -1.0 / (c * n), np.float32)
    if front == "bn":
        x = (np.abs(rng.standard_normal((b, n, d))) + 0.5 * rng.random(d)).astype(np.float32)
        ins = [x, (1.0 + 0.2 * rng.standard_normal(d)).astype(np.float32), (0.1 * rng.standard_normal(d)).astype(np.float32)]
    elif front == "rbf":
        ins = [lm.unit_rows(70 + seed, b, n, d).astype(np.float32), np.linspace(0.6, 1.5, c).astype(np.float32)]
    else:
        ins = [lm.unit_rows(70 + seed, b, n, d).astype(np.float32)]
    return ins, y, sv, mean, noise, cw


_E2E_CACHE = {}


def _e2e_reference(front):
    """[(inputs, float64 loss, float64 grads, float32 errors)] per seed, and the floor per gradient: computed once"""
    if front not in _E2E_CACHE:
        rows = []
        for seed in E2E_SEEDS:
            args = _e2e_inputs(front, seed)
            l64, g64 = lm.episode_loss_torch(front, *args, dtype=torch.float64)
            l32, g32 = lm.episode_loss_torch(front, *args, dtype=torch.float32)
            e32 = [float(np.abs(a.astype(np.float64) - r).max() / np.abs(r).max()) for a, r in zip(g32, g64)] + [abs(float(l32) - float(l64)) / abs(float(l64))]
            rows.append((args, l64, g64, e32))
        _E2E_CACHE[front] = rows, [max(r[3][i] for r in rows) for i in range(len(rows[0][3]))]
    return _E2E_CACHE[front]


@pytest.mark.parametrize("seed", E2E_SEEDS)
@pytest.mark.parametrize("front", ["linear", "rbf", "bn"])
def test_training_episode_gradients_match_float64_autograd(front, seed, cuda):
    rows, floor = _e2e_reference(front)
    (ins, y, sv, mean, noise, cw), l64, g64, _ = rows[seed]
    leaves = [_dev(t, cuda).requires_grad_(True) for t in ins + [sv, mean, noise]]
    *tins, svt, mt, nt = leaves
    yt, cwt = _dev(y, cuda), _dev(cw, cuda)
    if front == "bn":
        out = ops.episode_loss_loo_bn(tins[0], tins[1], tins[2], yt, svt, mt, nt, cwt)
    elif front == "rbf":
        out = ops.episode_loss_loo(tins[0], yt, svt, mt, nt, cwt, "rbf", lengthscale=tins[1])
    else:
        out = ops.episode_loss_loo(tins[0], yt, svt, mt, nt, cwt, "linear")
    obj, info = out[0], out[3]
    loss = obj.mean()
    loss.backward()
    assert int(info.abs().max()) == 0
    names = {"linear": ["z"], "rbf": ["z", "lengthscale"], "bn": ["x", "gamma", "beta"]}[front] + ["sv", "mean", "noise", "loss"]
    errs = [float(np.abs(t.grad.cpu().numpy().astype(np.float64) - r).max() / np.abs(r).max()) for t, r in zip(leaves, g64)] + [abs(float(loss.detach()) - float(l64)) / abs(float(l64))]
    for name, e, f in zip(names, errs, floor):
        print("LOO-E2E %s seed %d d/d%s: gpu %.3e  floor %.3e  ratio %.2f" % (front, seed, name, e, f, e / f))
    bad = {name: (e, lm.BOUND * f) for name, e, f in zip(names, errs, floor) if not e <= lm.BOUND * f}
    assert not bad, bad


# ---- the model ------------------------------------------------------------------------------------------------------------------------------------
def _images(seed, *shape):
    return torch.rand(*shape, 1, 28, 28, generator=torch.Generator().manual_seed(seed))


class _Loader:
    def __init__(self, n_ep, n_way, per, seed):
        self.x = list(_images(seed, n_ep, n_way, per))

    def __len__(self):
        return len(self.x)

    def __iter__(self):
        return iter((x, None) for x in self.x)


def _model(dev, kernel="bncossim", n_way=5, n_support=2, **kw):
    torch.manual_seed(0)
    return dkt_amd.DKT(lambda: backbone.Conv4S(), n_way=n_way, n_support=n_support, kernel_type=kernel, objective="loo", **kw).to(dev)


@pytest.mark.parametrize("kernel", ["bncossim", "rbf"])
def test_one_train_loop_step_moves_the_parameters(kernel, cuda):
    m = _model(cuda, kernel)
    before = {k: v.detach().clone() for k, v in m.named_parameters() if v.requires_grad}
    m.train_loop(0, _Loader(1, 5, 5, 4), None)
    loss = float(m._last["loss"])
    assert np.isfinite(loss) and int(m._last["info"].abs().max()) == 0
    moved = [k for k, v in m.named_parameters() if v.requires_grad and not torch.equal(v.detach(), before[k])]
    assert any(k.startswith("model.") for k in moved) and any(k.startswith("feature") for k in moved), moved
    assert all(bool(torch.isfinite(v).all()) for v in m.parameters())


def test_five_adam_steps_lower_the_loss(cuda):
    m = _model(cuda)
    x = _images(6, 5, 5).view(25, 1, 28, 28).to(cuda)
    y = m._targets(5, 5, cuda)
    opt = m._adam()
    losses = []
    for _ in range(6):
        opt.zero_grad()
        loss, aux, _, _ = m._train_forward(x, y, 1, 25, False)
        losses.append(float(loss.detach()))
        loss.backward()
        opt.step()
    print("LOO five Adam steps: %s" % ["%.5f" % v for v in losses])
    assert all(np.isfinite(losses)) and losses[5] < losses[0]


@pytest.mark.parametrize("kernel", ["linear", "rbf"])
def test_loo_accuracy_is_the_argmax_of_mu_loo(kernel, cuda):
    m = _model(cuda, kernel, n_support=5)
    m.eval()
    x = _images(8, 5, 8)
    acc = m.loo_accuracy(x)
    with torch.no_grad():
        zs = m._embed(x[:, :5].reshape(25, 1, 28, 28).to(cuda)).float().unsqueeze(0)
        sv, mean, noise, ls, off = m._hypers_detached()
        e = ops.kernel_matrix(zs, None, kernel) if kernel == "linear" else ops.kernel_matrix_per_class(zs, None, kernel, ls, off)
        mu = ops.loo(e, m._targets(5, 5, cuda), sv, mean, noise)["mu_loo"][0].cpu().numpy()
    want = float((np.argmax(mu, 0) == np.repeat(np.arange(5), 5)).mean() * 100.0)
    assert acc == pytest.approx(want, abs=1e-4) and 0.0 <= acc <= 100.0
    assert torch.equal(m._last["loo"]["mu_loo"][0].cpu(), torch.tensor(mu))


def test_an_episode_of_128_rows_is_refused_before_any_launch(cuda, monkeypatch):
    m = _model(cuda, n_way=8)
    launched = []
    monkeypatch.setattr(ops, "loo", lambda *a, **k: launched.append("loo"))
    x = _images(9, 8, 16).view(128, 1, 28, 28).to(cuda)
    with pytest.raises(ValueError, match="up to 127 rows"):
        m._train_forward(x, m._targets(8, 16, cuda), 1, 128, False)
    m2 = _model(cuda, "rbf", n_way=8)
    with pytest.raises(ValueError, match="up to 127 rows"):
        m2._train_forward(x, m2._targets(8, 16, cuda), 1, 128, False)
    assert not launched
    with pytest.raises(RuntimeError, match="DKT_ERR_SHAPE"):                 # the library's own answer, on the host
        ops._lib.check(ops._lib.load_loo().dkt_loo_f32(*_null_call(128)), "dkt_loo_f32")


def _null_call(n):
    import ctypes
    p = ctypes.c_void_p(4096)
    return [p, n * n, 0, p, 0, p, p, p, None, 1, 2, n, 1e-6, 3, 0, p, p, p, p, None, None, None, None, p, p, None]


# ---- the guard arena --------------------------------------------------------------------------------------------------------------------------------
def _skewed(x):
    """x behind one spare float: placed in the arena at a 512-byte boundary, the operand itself then starts 4 bytes past a 16-byte boundary"""
    return torch.cat([torch.zeros(1), torch.as_tensor(x, dtype=torch.float32).reshape(-1)])


@pytest.mark.parametrize("grad", [False, True], ids=["fwd", "grad"])
@pytest.mark.parametrize("per_class", [False, True], ids=["shared", "perclass"])
@pytest.mark.parametrize("n", [17, 127])
def test_guard_arena_on_operands_off_the_16_byte_grid(n, per_class, grad, cuda, monkeypatch):
    kase = lm.Case(n, 3, 2, per_class, True, "mixed", 64, "rbf", 0.1, 1.0)
    inp = kase.inputs()
    shapes = {k: np.asarray(v).shape for k, v in inp.items()}
    seen = []

    def call(p):
        ops_in = {k: p[k][1:].view(shapes[k]) for k in p}
        seen.append(all(t.data_ptr() % 16 == 4 for t in ops_in.values()))
        return ops.loo(ops_in["e"], ops_in["y"], ops_in["sv"], ops_in["mean"], ops_in["noise"], want_grad=grad, cls_weight=ops_in["cw"])

    report = ga.check(call, {k: _skewed(v) for k, v in inp.items()}, cuda, monkeypatch, [ops])
    assert seen[1:] == [True, True]                      # the two arena runs
    failures = report.failures()
    for name, t in report.results.items():
        if t.dtype.is_floating_point and not bool(torch.isfinite(t).all()):
            failures.append("%s of the ordinary run is not finite" % name)
        if (name.endswith(".info") or name.endswith(".jitter")) and bool((t != 0).any()):
            failures.append("%s of the ordinary run is not zero" % name)
    want = {"out." + q for q in lm.VALUES + ("jitter", "info") + (lm.GRADS if grad else ())}
    assert set(report.results) == want and all(report.inside.values())
    assert not failures, "\n".join(failures)
    assert ops.torch is torch
