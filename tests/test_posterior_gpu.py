"""dkt_posterior_f32 and everything built on it, on the GPU (docs/POSTERIOR.md): ops.posterior against the float64 model of tests/posterior_model.py at the
kernel's tile, row-group and wave edges and at its limits, both layouts of the base matrices, shared and per-episode targets, noisy and latent covariance, with
and without held-out targets and draws; the tie to the shipped mean / variance calls; symmetry, reproducibility, independence of the optional outputs; both
jitter ladders and the poisoned problem; the guard arena; DKTRegression.posterior / sample / joint_log_likelihood; graph capture.

Tolerance: the float32 CPU evaluation of the same closed form gives the floor of a case group (the largest error over its cases, per quantity,
max |got - ref| / max |ref|); the bound is 4 x that floor.  Nothing is skipped.  Measured floors and GPU maxima: docs/POSTERIOR.md."""
import numpy as np
import pytest
import torch

import dkt_amd
from dkt_amd import ops
from oracle import dkt_oracle as O

import guard_arena as ga
import posterior_model as pm

pytestmark = pytest.mark.gpu
OUTPUTS = ("mu", "cov", "chol", "logp", "lpd", "samples", "jitter_s", "jitter_q", "info_s", "info_q")


def _dev(x, dev):
    return None if x is None else torch.tensor(np.asarray(x), dtype=torch.float32, device=dev)


def _call(inp, dev, with_noise, **kw):
    kw = dict(dict(yq=_dev(inp["yq"], dev), eps=_dev(inp["eps"], dev), want_chol=True), **kw)
    return ops.posterior(_dev(inp["e_ss"], dev), _dev(inp["e_qs"], dev), _dev(inp["e_qq"], dev), _dev(inp["y"], dev), _dev(inp["sv"], dev), _dev(inp["mean"], dev),
                         _dev(inp["noise"], dev), with_noise=with_noise, **kw)


def _np(out):
    return {k: None if v is None else v.detach().cpu().numpy() for k, v in out.items()}


def _bits(t):
    return t.view(torch.int32)


def _same_bits(a, b, keys=OUTPUTS):
    return [q for q in keys if (a[q] is None) != (b[q] is None) or (a[q] is not None and not torch.equal(_bits(a[q]), _bits(b[q])))]


# ---- against the float64 model -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(pm.CASES)), ids=[repr(k) for k in pm.CASES])
def test_posterior_matches_float64(index, cuda):
    kase = pm.CASES[index]
    ref, e32 = pm.reference(index)
    floor = pm.floors(kase.group)
    out = _call(kase.inputs(), cuda, kase.with_noise)
    got = _np(out)
    for q in ("info_s", "info_q", "jitter_s", "jitter_q"):
        assert (got[q] == 0).all(), q                         # the conditioning cap: rung 0 is the only one fp32 needs
    assert np.array_equal(got["cov"], np.swapaxes(got["cov"], -1, -2)) and np.array_equal(got["chol"], np.tril(got["chol"]))
    assert {q for q in pm.QUANTITIES if got[q] is not None} == set(kase.quantities())
    err = pm.errors(got, ref, kase.quantities())
    for q in kase.quantities():
        print("POST %r %s: gpu %.3e  f32 %.3e  floor(%s) %.3e  ratio %.2f" % (kase, q, err[q], e32[q], kase.group, floor[q], err[q] / floor[q]))
    bad = [q for q in kase.quantities() if not err[q] <= pm.BOUND * floor[q]]
    assert not bad, {q: (err[q], pm.BOUND * floor[q]) for q in bad}


TIES = [pm.Case(5, 19, 1, 3, False, True, True, 0, False, 64, "rbf", 0.1, 1.0), pm.Case(33, 33, 3, 3, False, False, True, 0, False, 8, "rbf", 1.0, 0.3),
        pm.Case(64, 127, 3, 2, False, True, True, 0, False, 64, "linear", 0.1, 1.0)]


@pytest.mark.parametrize("kase", TIES, ids=repr)
def test_mean_and_diagonal_tie_to_the_shipped_calls(kase, cuda):
    """mu against ops.mll + ops.predict and diag(cov) against ops.predict_var (the exact-fp32 route of the marginal likelihood) on the same inputs: both sides
    are inside the float32 floor of the float64 model."""
    inp = kase.inputs()
    args, kw = pm._model_args(inp, True)
    ref = pm.closed_form(*args, **kw)
    floor = pm.floors(kase.group)
    t = {k: _dev(v, cuda) for k, v in inp.items()}
    new = _call(inp, cuda, True, want_chol=False)
    old = ops.mll(t["e_ss"], t["y"], t["sv"], t["mean"], t["noise"], want_chol=True, force_f32mfma=True)
    assert int(old["info"].abs().max()) == 0 and float(old["jitter"].abs().max()) == 0.0
    mu_old, _ = ops.predict(t["e_qs"], old["alpha"], t["sv"], t["mean"], want_labels=False)
    var_old = ops.predict_var(t["e_qs"], torch.diagonal(t["e_qq"], dim1=-2, dim2=-1).contiguous(), old["chol"], t["sv"], t["noise"])
    var_ref = np.einsum("bcii->bci", ref["cov"])
    scale_mu, scale_cov = np.abs(ref["mu"]).max(), np.abs(ref["cov"]).max()
    errs = {"mu new": np.abs(new["mu"].cpu().numpy() - ref["mu"]).max() / scale_mu, "mu shipped": np.abs(mu_old.cpu().numpy() - ref["mu"]).max() / scale_mu,
            "var new": np.abs(torch.diagonal(new["cov"], dim1=-2, dim2=-1).cpu().numpy() - var_ref).max() / scale_cov,
            "var shipped": np.abs(var_old.cpu().numpy() - var_ref).max() / scale_cov}
    for name, e in errs.items():
        f = floor["mu" if name.startswith("mu") else "cov"]
        print("POST-TIE %r %s: %.3e  floor %.3e  ratio %.2f" % (kase, name, e, f, e / f))
    bad = {name: e for name, e in errs.items() if not e <= pm.BOUND * floor["mu" if name.startswith("mu") else "cov"]}
    assert not bad, bad


@pytest.mark.parametrize("index", [13, 24, 32], ids=lambda i: repr(pm.CASES[i]))
def test_two_runs_give_the_same_bits(index, cuda):
    kase = pm.CASES[index]
    a, b = _call(kase.inputs(), cuda, kase.with_noise), _call(kase.inputs(), cuda, kase.with_noise)
    assert not _same_bits(a, b)


@pytest.mark.parametrize("index", [14, 29], ids=lambda i: repr(pm.CASES[i]))
def test_null_outputs_change_no_other_outputs_bits(index, cuda):
    kase = pm.CASES[index]
    inp = kase.inputs()
    assert kase.has_yq and kase.s > 0
    full = _call(inp, cuda, kase.with_noise)
    always = ("mu", "jitter_s", "jitter_q", "info_s", "info_q")
    bare = _call(inp, cuda, kase.with_noise, yq=None, eps=None, want_cov=False, want_chol=False)           # Sigma lives in the workspace
    assert all(bare[q] is None for q in ("cov", "chol", "logp", "lpd", "samples")) and not _same_bits(full, bare, always)
    no_cov = _call(inp, cuda, kase.with_noise, want_cov=False)
    assert no_cov["cov"] is None and not _same_bits(full, no_cov, always + ("chol", "logp", "lpd", "samples"))
    no_draws = _call(inp, cuda, kase.with_noise, eps=None, want_chol=False)
    assert no_draws["samples"] is None and not _same_bits(full, no_draws, always + ("cov", "logp", "lpd"))
    no_yq = _call(inp, cuda, kase.with_noise, yq=None)
    assert no_yq["logp"] is None and not _same_bits(full, no_yq, always + ("cov", "chol", "samples"))


# ---- the jitter ladders --------------------------------------------------------------------------------------------------------------------------
def _ladder_inputs(repeat_query_row):
    """N = 16, M = 17, C = 2, B = 3, shared base matrices, latent covariance; with repeat_query_row, query rows 1, 2 and 3 of episode 1 ARE its query row 0
    (one copy leaves a pivot of rounding noise, of either sign; the copies behind it are divided by that noise, and no such factor survives rung 0)."""
    b, n, m, c, d = 3, 16, 17, 2, 64
    zs, zq = pm.unit_rows(501, b, n, d), pm.unit_rows(502, b, m, d)
    if repeat_query_row:
        zq[1, 1:4] = zq[1, 0]
    sv, mean, noise = pm.hypers(c, 1.0, 0.1)
    rng = np.random.default_rng(503)
    return dict(e_ss=pm.base_matrix(zs, None, "rbf"), e_qs=pm.base_matrix(zq, zs, "rbf"), e_qq=pm.base_matrix(zq, None, "rbf"), y=pm.targets(504, c, n, b),
                sv=sv, mean=mean, noise=noise, yq=pm.targets(505, c, m, b), eps=rng.standard_normal((b, c, 4, m)).astype(np.float32))


def test_a_singular_query_covariance_climbs_the_ladder_or_says_so(cuda):
    """Two identical query rows make the latent Sigma exactly singular: either a rung of the ladder factors it (info_q = 0, jitter_q > 0, R R^T within the bound
    of the float64 Sigma + jitter_q I) or none does (info_q != 0: chol, logp and samples NaN, mu and cov valid).  Which rung is not asserted.  Every other
    problem of the call is bit for bit what it is without the repeated row."""
    clean_in, inp = _ladder_inputs(False), _ladder_inputs(True)
    clean, out = _call(clean_in, cuda, False), _call(inp, cuda, False)
    got = _np(out)
    args, kw = pm._model_args(inp, False)
    ref = pm.closed_form(*args, **dict(kw, jitter_q=1.0))                 # (mu and cov do not depend on jitter_q; the float64 factor needs some)
    floor = pm.floors("15-17")
    assert (got["info_s"] == 0).all() and (got["jitter_s"] == 0).all()
    for k in range(2):
        info, jit = int(got["info_q"][1, k]), float(got["jitter_q"][1, k])
        print("POST-LADDER class %d: info_q %d jitter_q %g" % (k, info, jit))
        err = pm.errors({q: got[q][1, k] for q in ("mu", "cov")}, {q: ref[q][1, k] for q in ("mu", "cov")}, ("mu", "cov"))
        assert err["mu"] <= pm.BOUND * floor["mu"] and err["cov"] <= pm.BOUND * floor["cov"], err
        if info == 0:
            assert jit > 0
            r = got["chol"][1, k].astype(np.float64)
            want = ref["cov"][1, k] + jit * np.eye(17)
            assert np.abs(r @ r.T - want).max() <= pm.BOUND * floor["cov"] * np.abs(want).max()
            assert np.isfinite(got["logp"][1, k]) and np.isfinite(got["samples"][1, k]).all()
        else:
            assert jit > 0 and np.isnan(got["chol"][1, k]).all() and np.isnan(got["logp"][1, k]) and np.isnan(got["samples"][1, k]).all()
        assert np.isfinite(got["lpd"][1, k])
    for q in OUTPUTS:
        assert torch.equal(_bits(out[q][[0, 2]]), _bits(clean[q][[0, 2]])), q


def test_a_support_matrix_that_is_not_positive_definite_poisons_itself_only(cuda):
    inp = _ladder_inputs(False)
    clean = _call(inp, cuda, True)
    e = inp["e_ss"].copy()
    e[1, 0, 0] = -1.0
    out = _call(dict(inp, e_ss=e), cuda, True)
    got = _np(out)
    assert (got["info_s"][1] == 1).all() and (got["info_s"][[0, 2]] == 0).all() and (got["info_q"][1] != 0).all()
    assert np.allclose(got["jitter_s"][1], 1e-4)                           # the last rung was tried
    for q in pm.QUANTITIES:
        assert np.isnan(got[q][1]).all(), q
    for q in OUTPUTS:
        assert torch.equal(_bits(out[q][[0, 2]]), _bits(clean[q][[0, 2]])), q


# ---- the guard arena --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("want_cov", [True, False], ids=["cov", "workspace"])
@pytest.mark.parametrize("n,m", [(127, 127), (5, 19)])
def test_guard_arena(n, m, want_cov, cuda, monkeypatch):
    kase = pm.Case(n, m, 3, 2, True, True, True, 2, True, 64, "rbf", 0.1, 1.0)
    inp = {k: torch.as_tensor(v) for k, v in kase.inputs().items()}

    def call(p):
        return ops.posterior(p["e_ss"], p["e_qs"], p["e_qq"], p["y"], p["sv"], p["mean"], p["noise"], yq=p["yq"], eps=p["eps"], want_cov=want_cov, want_chol=True)

    report = ga.check(call, inp, cuda, monkeypatch, [ops])
    failures = report.failures()
    for name, t in report.results.items():
        if t.dtype.is_floating_point and not bool(torch.isfinite(t).all()):
            failures.append("%s of the ordinary run is not finite" % name)
        if name.split(".")[-1] in ("info_s", "info_q", "jitter_s", "jitter_q") and bool((t != 0).any()):
            failures.append("%s of the ordinary run is not zero" % name)
    assert set(report.results) == {"out." + q for q in OUTPUTS if want_cov or q != "cov"} and all(report.inside.values())
    matrices = [b for b in report.blocks if b.role == "allocated" and b.nbytes == 4 * 2 * 3 * m * m]
    assert len(matrices) == 2                                             # cov and chol -- or chol and the workspace, of exactly the size the library asks for
    assert not failures, "\n".join(failures)
    assert ops.torch is torch


# ---- the model ------------------------------------------------------------------------------------------------------------------------------------
SEEDS = (0, 1, 2)
N_SUPPORT, N_FRAMES, FEATURES = 5, 19, 8


def _model(kernel, dev):
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Linear(3, 16), torch.nn.Tanh(), torch.nn.Linear(16, FEATURES))
    return dkt_amd.DKTRegression(net, kernel_type=kernel, num_mixtures=2, ard_num_dims=FEATURES).to(dev).eval()


def _tasks(seed, dev, b=3):
    g = torch.Generator().manual_seed(40 + seed)
    x = torch.randn(b, N_FRAMES, 3, generator=g)
    y = torch.sin(x.sum(-1)) + 0.1 * torch.randn(b, N_FRAMES, generator=g)
    return x.to(dev), y.to(dev)


def _model_reference(model, kernel, zs, zq, ys, yq, eps, dtype_e):
    """The float64 model on the same features: the oracle's kernels, then the closed form.  With dtype_e = float32 the whole chain runs in float32 on the CPU,
    the kernel matrices included (squared distances in their Gram form |a|^2 + |b|^2 - 2 a.b, as a matrix-product kernel has them): the floor."""
    m = model.model
    zs, zq = zs.double().cpu().numpy(), zq.double().cpu().numpy()
    if kernel == "spectral":
        mix = [t.detach().double().cpu().numpy() for t in (m.mixture_weights, m.mixture_means, m.mixture_scales)]
        k64 = lambda a, b: np.stack([O.gram_spectral_mixture(a[i], b[i], *mix) for i in range(len(a))])      # noqa: E731
        w, mu, sg = (np.asarray(x, dtype_e).reshape(len(mix[0]), -1) for x in mix)

        def k(a, b):
            tau = a[:, :, None, None, :] - b[:, None, :, None, :]                                             # [B,R,S,1,D]
            two_pi = dtype_e(2.0 * np.pi)
            return ((np.exp(dtype_e(-0.5) * (two_pi * tau * sg) ** 2) * np.cos(two_pi * tau * mu)).prod(-1) * w[:, 0]).sum(-1)
    else:
        ls = float(m.lengthscale.detach().reshape(-1)[0])
        k64 = lambda a, b: np.stack([O.gram_rbf(a[i], b[i], ls) for i in range(len(a))])                      # noqa: E731

        def k(a, b):
            d2 = (a * a).sum(-1)[:, :, None] + (b * b).sum(-1)[:, None, :] - dtype_e(2.0) * (a @ np.swapaxes(b, -1, -2))
            return np.exp(dtype_e(-0.5) * np.maximum(d2, dtype_e(0.0)) / dtype_e(ls) ** 2)
    pairs = ((zs, zs), (zq, zs), (zq, zq))
    if dtype_e == np.float64:
        es = [k64(a, b) for a, b in pairs]
        assert all(np.abs(k(a, b) - e).max() < 1e-12 for (a, b), e in zip(pairs, es))                         # (the float32 chain below is the oracle's formula)
    else:
        es = [k(a.astype(dtype_e), b.astype(dtype_e)) for a, b in pairs]
        assert all(e.dtype == dtype_e for e in es)
    hyp = [t.detach().double().cpu().numpy().reshape(-1) for t in (m.scale_times_variance(), m.mean, m.noise)]
    ys, yq = ys.double().cpu().numpy()[:, None], yq.double().cpu().numpy()[:, None]
    noisy = pm.closed_form(*es, ys, *hyp, yq=yq, dtype=dtype_e)
    latent = pm.closed_form(*es, ys, *hyp, eps=eps.double().cpu().numpy(), with_noise=False, dtype=dtype_e)
    return dict(mu=noisy["mu"][:, 0], cov=noisy["cov"][:, 0], logp=noisy["logp"][:, 0], lpd=noisy["lpd"][:, 0], samples=latent["samples"][:, 0])


_MODEL_CACHE = {}


def _model_case(kernel, seed, dev):
    """(model, features, targets, eps, float64 reference, float32 errors) of one draw of three tasks: computed once"""
    if (kernel, seed) not in _MODEL_CACHE:
        model = _model(kernel, dev)
        x, y = _tasks(seed, dev)
        with torch.no_grad():
            z = model._features(x.reshape(-1, 3)).reshape(3, N_FRAMES, FEATURES)
        zs, ys = z[:, :N_SUPPORT].contiguous(), y[:, :N_SUPPORT].contiguous()
        eps = torch.randn((3, 1, 4, N_FRAMES), device=dev, generator=torch.Generator(device=dev).manual_seed(77))
        ref = _model_reference(model, kernel, zs, z, ys, y, eps, np.float64)
        f32 = _model_reference(model, kernel, zs, z, ys, y, eps, np.float32)
        _MODEL_CACHE[kernel, seed] = model, (zs, ys, z, y), ref, pm.errors(f32, ref, tuple(ref))
    return _MODEL_CACHE[kernel, seed]


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("kernel", ["rbf", "spectral"])
def test_model_methods_match_float64_and_the_batch_is_the_tasks_one_by_one(kernel, seed, cuda):
    model, (zs, ys, zq, yq), ref, _ = _model_case(kernel, seed, cuda)
    floor = {q: max(_model_case(kernel, s, cuda)[3][q] for s in SEEDS) for q in ref}      # one group per kernel: the largest float32 error over its draws
    gen = lambda: torch.Generator(device=cuda).manual_seed(77)                            # noqa: E731
    mu, cov = model.posterior(zs, ys, zq)
    draws = model.sample(zs, ys, zq, 4, generator=gen())
    logp, lpd = model.joint_log_likelihood(zs, ys, zq, yq)
    assert mu.shape == (3, 19) and cov.shape == (3, 19, 19) and draws.shape == (3, 4, 19) and logp.shape == lpd.shape == (3,)
    got = dict(mu=mu, cov=cov, logp=logp, lpd=lpd, samples=draws)
    err = pm.errors({k: v.cpu().numpy() for k, v in got.items()}, ref, tuple(ref))
    for q in ref:
        print("POST-MODEL %s seed %d %s: gpu %.3e  floor %.3e  ratio %.2f" % (kernel, seed, q, err[q], floor[q], err[q] / floor[q]))
    bad = {q: (err[q], pm.BOUND * floor[q]) for q in ref if not err[q] <= pm.BOUND * floor[q]}
    assert not bad, bad
    for i in range(3):                      # one task at a time: the same bits (the draws of task i are rows i of the batch's standard normals)
        mu1, cov1 = model.posterior(zs[i], ys[i], zq[i])
        logp1, lpd1 = model.joint_log_likelihood(zs[i], ys[i], zq[i], yq[i])
        assert mu1.shape == (19,) and cov1.shape == (19, 19) and logp1.dim() == 0
        assert torch.equal(mu1, mu[i]) and torch.equal(cov1, cov[i]) and torch.equal(logp1, logp[i]) and torch.equal(lpd1, lpd[i])
    one = model.sample(zs[0], ys[0], zq[0], 4, generator=gen())
    eps0 = torch.randn((1, 1, 4, 19), device=cuda, generator=gen())
    want = ops.posterior(*_model_matrices(model, kernel, zs[:1], zq[:1]), ys[:1, None], model.model.scale_times_variance(), model.model.mean,
                         model.model.noise, eps=eps0, with_noise=False, want_cov=False)["samples"][0, 0]
    assert one.shape == (4, 19) and torch.equal(one, want)


def _model_matrices(model, kernel, zs, zq):
    m = model.model
    if kernel == "spectral":
        mix = (m.mixture_weights, m.mixture_means, m.mixture_scales)
        return ops.smk(zs, None, *mix)[0], ops.smk(zq, zs, *mix)[0], ops.smk(zq, None, *mix)[0]
    return tuple(ops.gram(a, b, ops.KERNEL_RBF, m.lengthscale) for a, b in ((zs, None), (zq, zs), (zq, None)))


def test_test_loop_is_what_it_was(cuda):
    """test_loop's MSE is the predict path's, bit for bit, with the new methods called in between."""
    model = _model("rbf", cuda)
    x, y = _tasks(5, cuda, b=4)

    def expected():
        np.random.seed(11)
        ind = list(np.random.choice(list(range(N_FRAMES)), replace=False, size=N_SUPPORT))
        n = np.random.randint(0, 3)
        with torch.no_grad():
            mean, _ = model.predict(model._features(x[n, ind]), y[n, ind], model._features(x[n]), with_variance=True)
        return model.mse(mean, y[n]), ind, n

    want, ind, n = expected()
    np.random.seed(11)
    first = model.test_loop(N_SUPPORT, None, x, y)
    with torch.no_grad():
        logp, lpd = model.joint_log_likelihood(model._features(x[n, ind]), y[n, ind], model._features(x[n]), y[n])
    model.sample(model._features(x[n, ind]).detach(), y[n, ind], model._features(x[n]).detach(), 2)
    model.posterior(model._features(x[n, ind]).detach(), y[n, ind], model._features(x[n]).detach())
    np.random.seed(11)
    second = model.test_loop(N_SUPPORT, None, x, y)
    assert torch.equal(first, want) and torch.equal(second, want) and first.dim() == 0
    assert bool(torch.isfinite(logp)) and bool(torch.isfinite(lpd))


def test_eval_regression_prints_test_regressions_lines_and_the_nll(cuda, tmp_path, monkeypatch, capsys):
    """eval_regression.py: without --nll what test_regression.py prints, with it the same MSE lines and the two NLL lines behind them."""
    import eval_regression
    import test_regression
    import train_regression
    from dkt_amd import configs, io_utils
    from dkt_amd.data import SyntheticHeadPoseSampler
    monkeypatch.setattr(configs, "save_dir", str(tmp_path) + "/")
    params = io_utils.parse_args_regression("eval_regression", ["--n_test_epochs", "2"])
    assert params.nll is False
    train_regression.seed_everything(0)
    train_regression.build_model(params, SyntheticHeadPoseSampler(seed=1)).save_checkpoint(train_regression.checkpoint_path(params))
    want = test_regression.main(["--n_test_epochs", "2"])
    plain = capsys.readouterr().out
    assert eval_regression.main(["--n_test_epochs", "2"]) == want and capsys.readouterr().out == plain
    mse, joint, marginal = eval_regression.main(["--n_test_epochs", "2", "--nll"])
    out = capsys.readouterr().out
    assert mse == want and out.startswith(plain) and len(joint) == len(marginal) == 2 and np.isfinite(joint + marginal).all()
    assert "Average joint NLL per point: %s +- %s" % (np.mean(joint), np.std(joint)) in out
    assert "Average marginal NLL per point: %s +- %s" % (np.mean(marginal), np.std(marginal)) in out


# ---- graph capture --------------------------------------------------------------------------------------------------------------------------------
def test_one_capture_and_one_replay_equal_the_eager_call(cuda):
    """One straight-line launch, nothing read back: captured once, replayed once, the same bits as the eager call."""
    kase = pm.CASES[14]
    t = {k: _dev(v, cuda) for k, v in kase.inputs().items()}
    call = lambda: ops.posterior(t["e_ss"], t["e_qs"], t["e_qq"], t["y"], t["sv"], t["mean"], t["noise"], yq=t["yq"], eps=t["eps"],      # noqa: E731
                                 with_noise=kase.with_noise, want_chol=True)
    eager = call()                                                       # (loads the library and sizes the kernel's LDS outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = call()
    graph.replay()
    torch.cuda.synchronize()
    assert not _same_bits(eager, captured)
