"""dkt_loofs_f32 and everything built on it, on the GPU (docs/LOOFS.md): ops.loo_lowrank against the float64 model of tests/loo_lowrank_model.py at the edges of
the kernel's row block, of the resident kernel and of the route, at the 20-way shapes; against the resident kernel below 128 rows; the jitter ladder and the
poisoned problem; bitwise reproducibility; the guard arena; a graph capture; the training episodes ops.episode_loss_loo / _bn in feature space against float64
autograd of the dense model; DKT(objective="loo") on a 420-row episode.

Tolerance: the float32 CPU evaluation of the same closed form gives the floor of a case group (the largest error over its cases, per quantity,
max |got - ref| / max |ref|); the bound is 4 x that floor.  Nothing is skipped.  Measured floors and GPU maxima: docs/LOOFS.md."""
import numpy as np
import pytest
import torch

import dkt_amd
from dkt_amd import backbone, ops

import guard_arena as ga
import loo_lowrank_model as fm

lm = fm.lm
pytestmark = pytest.mark.gpu
QUANTITIES = fm.VALUES + fm.GRADS


def _dev(x, dev):
    return None if x is None else torch.tensor(np.asarray(x), dtype=torch.float32, device=dev)


def _call(inp, dev, want_grad=True, **kw):
    return ops.loo_lowrank(_dev(inp["z"], dev), _dev(inp["y"], dev), _dev(inp["sv"], dev), _dev(inp["mean"], dev), _dev(inp["noise"], dev), want_grad=want_grad,
                           cls_weight=_dev(inp["cw"], dev), **kw)


def _np(out):
    return {k: None if v is None else v.detach().cpu().numpy() for k, v in out.items()}


def _index(n, d=None):
    return next(i for i, k in enumerate(fm.CASES) if k.n == n and (d is None or k.d == d))


# ---- against the float64 model -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(fm.CASES)), ids=[repr(k) for k in fm.CASES])
def test_loo_lowrank_matches_float64(index, cuda):
    kase = fm.CASES[index]
    ref, e32 = fm.reference(index)
    floor = fm.floors(kase.group)
    got = _np(_call(kase.inputs(), cuda))
    assert (got["info"] == 0).all() and (got["jitter"] == 0).all()
    assert got["dz"].shape == ref["dz"].shape
    err = fm.errors(got, ref, QUANTITIES)
    for q in QUANTITIES:
        print("LOOFS %r %s: gpu %.3e  f32 %.3e  floor(%s) %.3e  ratio %.2f" % (kase, q, err[q], e32[q], kase.group, floor[q], err[q] / floor[q] if floor[q] else 0.0))
    bad = [q for q in QUANTITIES if not err[q] <= fm.BOUND * floor[q]]
    assert not bad, {q: (err[q], fm.BOUND * floor[q]) for q in bad}


def test_the_case_list_is_the_models(cuda):
    r = fm.R
    assert {k.n for k in fm.CASES} == {1, 2, r - 1, r, r + 1, 2 * r + 1, 63, 64, 65, 127, 128, 129, 257, 420}
    assert {k.d for k in fm.CASES} == {4, 8, 60, 64} and {k.c for k in fm.CASES} == {1, 5, 20, 32} and {k.b for k in fm.CASES} == {1, 3, 70}


# ---- against the resident kernel -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [25, 105, 127])
def test_against_the_resident_kernel(n, cuda, monkeypatch):
    monkeypatch.setenv("DKT_LOO_LOWRANK", "force")
    assert ops.loo_lowrank_applies(n, 64, 5)
    kase = fm.Case(n, 64, 5, 3, True, "mixed", True, 0.1, 1.0)
    inp = kase.inputs()
    args = (inp["z"], inp["y"], inp["sv"], inp["mean"], inp["noise"], inp["cw"])
    ref = fm.feature_form(*args)
    # each side against float64 within 4 x the float32 floor of ITS closed form: the D x D one here, the N x N one of docs/LOO.md for the resident kernel
    f32 = fm.errors(fm.feature_form(*args, dtype=np.float32), ref, QUANTITIES)
    d32 = fm.errors(fm.dense(*args, dtype=np.float32), ref, QUANTITIES)
    z = _dev(inp["z"], cuda)
    fs = _call(inp, cuda)
    res = ops.loo(ops.gram(z), _dev(inp["y"], cuda), _dev(inp["sv"], cuda), _dev(inp["mean"], cuda), _dev(inp["noise"], cuda), want_grad=True,
                  cls_weight=_dev(inp["cw"], cuda))
    res["dz"] = ops.gram_bwd(res["w"], z, None, w_symmetric=True)
    assert int(fs["info"].abs().max()) == 0 and int(res["info"].abs().max()) == 0
    a, b = fm.errors(_np(fs), ref, QUANTITIES), fm.errors(_np(res), ref, QUANTITIES)
    mutual = fm.errors(_np(fs), {q: _np(res)[q].astype(np.float64) for q in QUANTITIES}, QUANTITIES)
    for q in QUANTITIES:
        print("LOOFS-vs-resident N=%d %s: feature space %.3e (f32 floor %.3e)  resident %.3e (f32 floor %.3e)  mutual %.3e" % (n, q, a[q], f32[q], b[q], d32[q], mutual[q]))
    bad = {q: (a[q], fm.BOUND * f32[q], b[q], fm.BOUND * d32[q]) for q in QUANTITIES if not (a[q] <= fm.BOUND * f32[q] and b[q] <= fm.BOUND * d32[q])}
    assert not bad, bad


# ---- the ladder ------------------------------------------------------------------------------------------------------------------------------------
def _ladder_inputs(bad_noise):
    z = fm.rows(5, 3, 8, 64)
    y = lm.targets(3, 8)
    sv = np.ones(3, np.float32)
    mean = np.zeros(3, np.float32)
    noise = np.array([0.1, 0.1, 0.2], np.float32)
    return dict(z=z, y=y, sv=sv, mean=mean, noise=noise, cw=None), dict(z=z, y=y, sv=sv, mean=mean, noise=np.array([0.1, bad_noise, 0.2], np.float32), cw=None)


def test_the_ladder_climbs_to_the_rung_that_makes_a_positive(cuda):
    """noise -5e-4: rungs 0 and 1e-4 leave noise + jitter < 0 (A has D - N negative eigenvalues), rung 1e-3 gives lam = 5e-4"""
    clean, inp = _ladder_inputs(-5e-4)
    got = _np(_call(inp, cuda, jitter0=1e-4, max_tries=3))
    assert (got["info"] == 0).all()
    assert (got["jitter"][:, 1] == np.float32(1e-4) * np.float32(10.0)).all() and (got["jitter"][:, [0, 2]] == 0).all()
    one = {k: (v[1:2] if k in ("sv", "mean", "noise") else v) for k, v in inp.items()}
    one["y"] = inp["y"][1:2]
    jit = float(np.float32(1e-4) * np.float32(10.0))
    ref = fm.feature_form(one["z"], one["y"], one["sv"], one["mean"], one["noise"], jitter=jit)
    f32 = fm.errors(fm.feature_form(one["z"], one["y"], one["sv"], one["mean"], one["noise"], jitter=jit, dtype=np.float32), ref, fm.VALUES + ("dsv", "dmean", "dnoise"))
    mine = {q: got[q][:, 1:2] for q in fm.VALUES + ("dsv", "dmean", "dnoise")}
    err = fm.errors(mine, ref, fm.VALUES + ("dsv", "dmean", "dnoise"))
    for q, e in err.items():
        print("LOOFS ladder %s: gpu %.3e  f32 %.3e (max h %.4f)" % (q, e, f32[q], ref["h"].max()))
    bad = {q: (e, fm.BOUND * f32[q]) for q, e in err.items() if not e <= fm.BOUND * f32[q]}
    assert not bad, bad
    # the classes beside it are what they are without it (their own dZ cannot be told apart in the sum: the values and the hyper-parameter parts are)
    base = _np(_call(clean, cuda, jitter0=1e-4, max_tries=3))
    for q in fm.VALUES + ("dsv", "dmean", "dnoise"):
        assert np.array_equal(got[q][:, [0, 2]], base[q][:, [0, 2]]), q


def test_a_problem_that_fails_every_rung_is_nan_and_the_other_episodes_keep_their_bits(cuda):
    clean, inp = _ladder_inputs(-1.0)
    # the poisoned class in episode 1 only: per-episode targets are shared, so the noise is -- poison it through a row of NaN instead
    z = clean["z"].copy()
    z[1, 3, 5] = np.nan
    got = _np(_call(dict(clean, z=z), cuda, jitter0=1e-4, max_tries=3))
    base = _np(_call(clean, cuda, jitter0=1e-4, max_tries=3))
    assert (got["info"][1] != 0).all() and (got["info"][[0, 2]] == 0).all()
    for q in QUANTITIES:
        assert np.isnan(got[q][1]).all(), q
        assert np.array_equal(got[q][[0, 2]], base[q][[0, 2]]), q
    # noise -1: every rung leaves A indefinite
    got = _np(_call(inp, cuda, jitter0=1e-4, max_tries=3))
    assert (got["info"][:, 1] != 0).all() and (got["info"][:, [0, 2]] == 0).all()
    assert (got["jitter"][:, 1] == np.float32(1e-4) * np.float32(10.0) * np.float32(10.0)).all()
    for q in fm.VALUES + ("dsv", "dmean", "dnoise"):
        assert np.isnan(got[q][:, 1]).all(), q
        assert np.array_equal(got[q][:, [0, 2]], base[q][:, [0, 2]]), q
    assert np.isnan(got["dz"]).all()                     # every episode holds the failed class


# ---- bits -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 420])
def test_two_runs_give_the_same_bits(n, cuda):
    inp = fm.CASES[_index(n)].inputs()
    a, b = _call(inp, cuda), _call(inp, cuda)
    for q in QUANTITIES + ("jitter", "info"):
        assert torch.equal(a[q], b[q]), q


def test_a_batch_equals_its_episodes_one_by_one(cuda):
    kase = fm.Case(129, 60, 5, 3, True, "mixed", False, 0.1, 1.0)
    inp = kase.inputs()
    whole = _call(inp, cuda)
    for b in range(3):
        one = _call(dict(inp, z=inp["z"][b:b + 1], y=inp["y"][b:b + 1]), cuda)
        for q in QUANTITIES + ("jitter", "info"):
            assert torch.equal(whole[q][b:b + 1], one[q]), (b, q)


def test_forward_only_call_equals_the_values_of_the_gradient_call(cuda):
    inp = fm.CASES[_index(129)].inputs()
    a, b = _call(inp, cuda, want_grad=False), _call(inp, cuda, want_grad=True)
    assert a["dz"] is None and a["dsv"] is None and a["dmean"] is None and a["dnoise"] is None
    for q in fm.VALUES + ("jitter", "info"):
        assert torch.equal(a[q], b[q]), q
    c = _call(dict(inp, cw=None), cuda, want_grad=True)                # no cls_weight: the raw outputs keep their bits
    for q in fm.VALUES + ("dsv", "dmean", "dnoise", "jitter", "info"):
        assert torch.equal(c[q], b[q]), q


# ---- the guard arena --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grad", [False, True], ids=["fwd", "grad"])
@pytest.mark.parametrize("n,d,c", [(420, 64, 20), (1, 4, 1)])
def test_guard_arena(n, d, c, grad, cuda, monkeypatch):
    kase = fm.Case(n, d, c, 2, True, "mixed", True, 0.1, 1.0)
    inp = kase.inputs()

    def call(p):
        return ops.loo_lowrank(p["z"], p["y"], p["sv"], p["mean"], p["noise"], want_grad=grad, cls_weight=p["cw"])

    report = ga.check(call, {k: torch.as_tensor(v) for k, v in inp.items()}, cuda, monkeypatch, [ops])
    failures = report.failures()
    for name, t in report.results.items():
        if t.dtype.is_floating_point and not bool(torch.isfinite(t).all()):
            failures.append("%s of the ordinary run is not finite" % name)
        if (name.endswith(".info") or name.endswith(".jitter")) and bool((t != 0).any()):
            failures.append("%s of the ordinary run is not zero" % name)
    want = {"out." + q for q in fm.VALUES + ("jitter", "info") + (fm.GRADS if grad else ())}
    assert set(report.results) == want and all(report.inside.values())
    assert not failures, "\n".join(failures)
    assert ops.torch is torch


# ---- graph capture ----------------------------------------------------------------------------------------------------------------------------------
def test_a_captured_call_replays_to_the_eager_bits(cuda):
    inp = fm.CASES[_index(257)].inputs()
    args = [_dev(inp[k], cuda) for k in ("z", "y", "sv", "mean", "noise")]
    cw = _dev(inp["cw"], cuda)
    eager = ops.loo_lowrank(*args, want_grad=True, cls_weight=cw)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.loo_lowrank(*args, want_grad=True, cls_weight=cw)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.loo_lowrank(*args, want_grad=True, cls_weight=cw)
    for t in out.values():
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for q in QUANTITIES + ("jitter", "info"):
        assert torch.equal(out[q], eager[q]), q


# ---- the training episodes against float64 autograd of the dense model -------------------------------------------------------------------------------
E2E = dict(b=2, n=130, d=64, c=5)
_E2E_CACHE = {}


def _bf16(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32).to(torch.bfloat16).float().numpy()


def _e2e_reference(front, x16):
    """inputs, float64 loss and gradients (the dense model, torch autograd), and the floors: the same chain in float32 on the CPU -- for a bf16 trunk, on the
    bf16 values of X, with dX rounded to bfloat16 as the chain returns it"""
    key = (front, x16)
    if key not in _E2E_CACHE:
        b, n, d, c = (E2E[k] for k in "bndc")
        rng = np.random.default_rng(31)
        y = lm.targets(c, n, b, 3)
        sv, mean, noise = lm.hypers(c, 0.7, 0.1)
        cw = np.full(c, -1.0 / (c * n), np.float32)
        if front == "linear":
            ins = [fm.rows(17, b, n, d)]
        else:
            x = rng.standard_normal((b, n, d)).astype(np.float32)
            ins = [_bf16(x) if x16 else x, (1.0 + 0.1 * rng.standard_normal(d)).astype(np.float32), (0.1 * rng.standard_normal(d)).astype(np.float32)]
        l64, g64 = lm.episode_loss_torch(front, ins, y, sv, mean, noise, cw, torch.float64)
        l32, g32 = lm.episode_loss_torch(front, ins, y, sv, mean, noise, cw, torch.float32)
        if x16:
            g32[0] = _bf16(g32[0])
        floor = [float(np.abs(a.astype(np.float64) - r).max() / np.abs(r).max()) for a, r in zip(g32, g64)] + [abs(float(l32) - float(l64)) / abs(float(l64))]
        _E2E_CACHE[key] = (ins, y, sv, mean, noise, cw), l64, g64, floor
    return _E2E_CACHE[key]


@pytest.mark.parametrize("front,x16", [("linear", False), ("bn", False), ("bn", True)], ids=["linear", "bn-fp32", "bn-bf16"])
def test_training_episode_gradients_match_float64_autograd(front, x16, cuda, monkeypatch):
    monkeypatch.delenv("DKT_LOO_LOWRANK", raising=False)
    (ins, y, sv, mean, noise, cw), l64, g64, floor = _e2e_reference(front, x16)
    leaves = [_dev(t, cuda).requires_grad_(True) for t in ins + [sv, mean, noise]]
    if x16:
        leaves[0] = leaves[0].detach().to(torch.bfloat16).requires_grad_(True)
    *tins, svt, mt, nt = leaves
    yt, cwt = _dev(y, cuda), _dev(cw, cuda)
    if front == "bn":
        out = ops.episode_loss_loo_bn(tins[0], tins[1], tins[2], yt, svt, mt, nt, cwt)
    else:
        out = ops.episode_loss_loo(tins[0], yt, svt, mt, nt, cwt, "linear", unit_rows=True)
    obj, info, e = out[0], out[3], out[7]
    assert e is None                                     # feature space: no E
    loss = obj.mean()
    loss.backward()
    assert int(info.abs().max()) == 0
    names = {"linear": ["z"], "bn": ["x", "gamma", "beta"]}[front] + ["sv", "mean", "noise", "loss"]
    errs = ([float(np.abs(t.grad.float().cpu().numpy().astype(np.float64) - r).max() / np.abs(r).max()) for t, r in zip(leaves, g64)]
            + [abs(float(loss.detach()) - float(l64)) / abs(float(l64))])
    for name, err, f in zip(names, errs, floor):
        print("LOOFS-E2E %s%s d/d%s: gpu %.3e  floor %.3e  ratio %.2f" % (front, "-bf16" if x16 else "", name, err, f, err / f))
    bad = {name: (err, fm.BOUND * f) for name, err, f in zip(names, errs, floor) if not err <= fm.BOUND * f}
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


def _model(dev, kernel="bncossim", n_way=20, n_support=5, **kw):
    torch.manual_seed(0)
    return dkt_amd.DKT(lambda: backbone.Conv4S(), n_way=n_way, n_support=n_support, kernel_type=kernel, objective="loo", **kw).to(dev)


def test_one_train_loop_step_on_a_420_row_episode(cuda, monkeypatch):
    monkeypatch.delenv("DKT_LOO_LOWRANK", raising=False)
    m = _model(cuda)
    before = {k: v.detach().clone() for k, v in m.named_parameters() if v.requires_grad}
    m.train_loop(0, _Loader(1, 20, 21, 4), None)
    loss = float(m._last["loss"])
    assert np.isfinite(loss) and int(m._last["info"].abs().max()) == 0
    assert m._last.get("e") is None                      # no N x N matrix was formed
    moved = [k for k, v in m.named_parameters() if v.requires_grad and not torch.equal(v.detach(), before[k])]
    assert any(k.startswith("model.") for k in moved) and any(k.startswith("feature") for k in moved), moved
    assert all(bool(torch.isfinite(v).all()) for v in m.parameters())


def test_loo_accuracy_takes_a_200_row_support_set(cuda, monkeypatch):
    monkeypatch.delenv("DKT_LOO_LOWRANK", raising=False)
    m = _model(cuda, n_support=10)
    m.eval()
    acc = m.loo_accuracy(_images(8, 20, 12))
    assert 0.0 <= acc <= 100.0 and tuple(m._last["loo"]["mu_loo"].shape) == (1, 20, 200)


def test_105_rows_stay_on_the_resident_kernel(cuda, monkeypatch):
    monkeypatch.delenv("DKT_LOO_LOWRANK", raising=False)
    m = _model(cuda, n_way=5)
    launched = []
    monkeypatch.setattr(ops, "loo_lowrank", lambda *a, **k: launched.append("loo_lowrank"))
    x = _images(9, 5, 21).view(105, 1, 28, 28).to(cuda)
    loss, aux, _, _ = m._train_forward(x, m._targets(5, 21, cuda), 1, 105, False)
    assert not launched and np.isfinite(float(loss.detach())) and aux["e"] is not None
