"""CPU-side checks of the Dirichlet classification likelihood: the float64 restatement of dkt_mll_rownoise_f32 / dkt_dirichlet_proba_f32
(tests/dirichlet_model.py) against scipy's multivariate normal density, the worked target values and central finite differences; the shared form; the new
symbols of the product ABI (still version 7, still at most 250 kernels, no spill); the float32 floors and label margins the GPU tests rely on; the DKT
surface and the command line without a GPU."""
import json
import os
import re

import numpy as np
import pytest
import torch
from scipy.stats import multivariate_normal

import dirichlet_model as dm
import dkt_amd

L = dkt_amd._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _problem(n, seed, sv=2.0, mean=-1.5):
    rng = np.random.default_rng(seed)
    z = dm.unit_rows(rng, 5, (n + 4) // 5)[:n]
    y, nr = dm.dirichlet_targets(np.where(rng.random(n) < 0.2, 1.0, -1.0))
    return z @ z.T, y, nr, sv, mean


def test_worked_target_values():
    y, nr = dm.dirichlet_targets(np.array([1.0, -1.0]))
    # the formulas, to rounding: a = 1.01 and a = 0.01
    assert abs(nr[0] - np.log(1 / 1.01 + 1)) < 1e-15 and abs(y[0] - (np.log(1.01) - np.log(1 / 1.01 + 1) / 2)) < 1e-15
    assert abs(nr[1] - np.log(101.0)) < 1e-15 and abs(y[1] - (np.log(0.01) - np.log(101.0) / 2)) < 1e-14
    # worked values as commonly quoted (0.688172, -0.334135 on the positive class; 4.615121, -6.912731 elsewhere): the formulas give 0.688184 and -0.334142
    # on the positive class, 1.2e-5 and 7e-6 away -- held to 2e-5; the other two agree to 1e-6
    got = np.array([nr[0], y[0], nr[1], y[1]])
    print("targets:", got)
    assert np.abs(got - np.array([0.688172, -0.334135, 4.615121, -6.912731])).max() < 2e-5
    assert np.abs(got[2:] - np.array([4.615121, -6.912731])).max() < 1e-6
    y32, nr32 = dm.dirichlet_targets(np.array([1.0, -1.0]), dtype=np.float32)
    assert y32.dtype == np.float32 and np.abs(y32 - y).max() < 1e-6
    yt, nt = dkt_amd.ops.dirichlet_targets(torch.tensor([1.0, -1.0]))
    assert np.abs(yt.numpy() - y).max() < 1e-6 and np.abs(nt.numpy() - nr).max() < 1e-6


@pytest.mark.parametrize("n", [1, 5, 25, 100])
def test_logp_is_the_multivariate_normal_density(n):
    e, y, nr, sv, mean = _problem(n, n)
    p = dm.one(e, y, nr, sv, mean)
    want = multivariate_normal.logpdf(y, mean=np.full(n, mean), cov=sv * e + np.diag(nr))
    k = sv * e + np.diag(nr)
    print("n = %d: logp %.12g, scipy %.12g" % (n, p["logp"], want))
    assert abs(p["logp"] - want) < 1e-10 * abs(want)              # (scipy goes through an eigendecomposition: rounding-level agreement)
    assert np.abs(k @ p["alpha"] - (y - mean)).max() < 1e-12 and np.abs(p["chol"] @ p["chol"].T - k).max() < 1e-13 and p["info"] == 0


@pytest.mark.parametrize("n", [5, 12, 25])
def test_gradients_match_central_differences(n):
    e, y, nr, sv, mean = _problem(n, 100 + n)
    p = dm.one(e, y, nr, sv, mean)
    rng = np.random.default_rng(n + 1)
    f = lambda e_, sv_, mean_: float(dm.one(e_, y, nr, sv_, mean_, want_grad=False)["logp"])
    h, worst = 1e-5, 0.0
    for _ in range(3):
        d = rng.standard_normal((n, n))
        d = (d + d.T) / 2
        fd = (f(e + h * d, sv, mean) - f(e - h * d, sv, mean)) / (2 * h)
        worst = max(worst, abs(fd - sv * (p["g"] * d).sum()) / abs(fd))
    fd_sv = (f(e, sv + h, mean) - f(e, sv - h, mean)) / (2 * h)
    fd_mean = (f(e, sv, mean + h) - f(e, sv, mean - h)) / (2 * h)
    worst = max(worst, abs(fd_sv - (p["g"] * e).sum()) / abs(fd_sv), abs(fd_mean - p["alpha"].sum()) / abs(fd_mean))
    print("n = %d: worst relative difference to central differences %.3g" % (n, worst))
    # central differences at h = 1e-5 in float64: truncation ~ h^2 |f'''| / 6 ~ 1e-10 and rounding ~ eps |f| / h ~ 1e-16 * 50 / 1e-5 = 5e-10, relative to
    # derivatives of order 1: 1e-7 leaves two orders of magnitude (measured here: 3.5e-9 at the worst)
    assert worst < 1e-7


def test_shared_form_is_the_sum_of_the_per_class_outputs_and_the_float32_mode_is_float32():
    d = dm.shape_case(2, 5, 25)
    s = dm.solve(d, np.float64)
    p = dm.solve(dict(d, e=np.repeat(d["e"][:, None], 5, 1)), np.float64)
    assert s["de"].shape == (2, 25, 25) and p["de"].shape == (2, 5, 25, 25)
    acc = np.zeros_like(s["de"])
    for ci in range(5):
        acc = acc + p["de"][:, ci]
    assert np.array_equal(s["de"], acc) and all(np.array_equal(s[q], p[q]) for q in ("logp", "alpha", "dsv", "dmean", "chol"))
    one = dm.one(d["e"][1], d["y"][3], d["nr"][3], d["sv"][3], d["mean"][3])
    assert s["logp"][1, 3] == one["logp"] and np.allclose(p["de"][1, 3], d["cw"][3] * d["sv"][3] * one["g"], rtol=1e-12, atol=0)
    assert np.allclose(s["dmean"][1, 3], d["cw"][3] * one["alpha"].sum(), rtol=1e-12) and np.allclose(s["de"], s["de"].transpose(0, 2, 1), rtol=0, atol=1e-18)
    assert dm.solve(d, np.float32)["de"].dtype == np.float32
    bad = dm.one(d["e"][0], d["y"][0], np.where(np.arange(25) == 7, -50.0, d["nr"][0]), 1.0, 0.0)
    assert bad["info"] != 0 and np.isnan(bad["logp"])


def test_proba_restatement():
    d = dm.proba_cases()[("shape", 2, 5, 80, 256)]
    prob, labels = dm.proba(d["mu"], d["var"], d["eps"])
    assert prob.shape == (2, 80, 5) and np.abs(prob.sum(-1) - 1).max() < 1e-14 and (labels == d["mu"].argmax(1)).all()
    p0, _ = dm.proba(d["mu"], np.zeros_like(d["var"]), d["eps"])
    sm = np.exp(d["mu"] - d["mu"].max(1, keepdims=True))
    assert np.abs(p0 - (sm / sm.sum(1, keepdims=True)).transpose(0, 2, 1)).max() < 1e-14
    assert np.array_equal(dm.proba(d["mu"], np.full_like(d["var"], -1e-6), d["eps"])[0], p0)          # a negative variance is clamped at 0
    assert dm.proba(np.array([[[1.0], [3.0], [3.0]]]), np.zeros((1, 3, 1)), np.zeros((1, 3)))[1][0, 0] == 1      # the first maximum


def test_float32_floors_and_label_margins_of_the_gpu_cases():
    """What tests/test_dirichlet_gpu.py scales its bounds from, stated on the CPU: e32 per quantity over the case list (docs/DIRICHLET.md tables them), and the
    float64 top-two margins of the label case against 100 x e32(mu): float64 itself leaves out no query."""
    _, e32 = dm.floors(dm.cases())
    _, p32 = dm.floors(dm.proba_cases(), ("prob",), dm.solve_proba)
    print("e32:", {q: "%.3g" % v for q, v in {**e32, **p32}.items()})
    assert all(0 < v < 1e-4 for v in e32.values()) and 0 < p32["prob"] < 1e-5
    zs, zq = dm.episode_case()
    sv, mean = np.array([0.5, 2.0, 1.0, 3.0, 0.75]), np.array([-2.0, -1.5, -2.5, -1.0, -3.0])
    yt, nr = (a.astype(np.float64) for a in dm.dirichlet_targets(np.where(np.repeat(np.eye(5), 5, 1) > 0, 1.0, -1.0), dtype=np.float32))
    margins, e32_mu = [], 0.0
    for b in range(2):
        e, ex, exx = dm._f32(zs[b] @ zs[b].T), dm._f32(zq[b] @ zs[b].T), dm._f32((zq[b] * zq[b]).sum(-1))
        mu64, var64 = dm.predict(e, ex, exx, yt, nr, sv, mean)
        mu32, _ = dm.predict(e, ex, exx, yt, nr, sv, mean, np.float32)
        e32_mu = max(e32_mu, float(np.abs(mu32 - mu64).max()))
        margins.append(dm.top_two_margin(mu64))
        assert var64.min() > 0
    smallest = float(np.min(margins))
    print("e32(mu) %.3g, smallest float64 top-two margin %.3g (%.0f x e32)" % (e32_mu, smallest, smallest / e32_mu))
    assert smallest >= 100 * e32_mu


def test_new_symbols_are_in_the_header_the_table_and_the_library(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dkt_abi.h")).read(), flags=re.S)
    for name in ("dkt_mll_rownoise_workspace_bytes", "dkt_mll_rownoise_f32", "dkt_dirichlet_proba_f32"):
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1)
        assert name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == proto.count(",") + 1 and hasattr(lib, name)
    assert L.SOURCES[-2:] == ["dkt_mll_rownoise.hip", "dkt_laplace_grad.hip"] and L.LIBS["hip"].sources is L.SOURCES and L.LIBS["hip"].src_dir is None
    assert lib.dkt_abi_version() == 8 and L.abi_version_of_header() == 8
    assert lib.dkt_mll_rownoise_workspace_bytes(2, 20, 100) == 2 * 20 * 100 * 100 * 4 and lib.dkt_mll_rownoise_workspace_bytes(0, 5, 25) == 0
    assert lib.dkt_mll_rownoise_workspace_bytes(1, 1, 1) == 4 and lib.dkt_mll_rownoise_workspace_bytes(3, 5, -1) == 0
    null = [None, 0, 0, None, 0, None, 0] + [None] * 10
    assert lib.dkt_mll_rownoise_f32(*null, 1, 5, 25, 0, None, 0, None) == -1                    # DKT_ERR_BAD_ARG comes before the shape test
    assert lib.dkt_mll_rownoise_f32(*null, 1, 5, 128, 0, None, 0, None) == -1
    assert lib.dkt_dirichlet_proba_f32(None, None, None, None, None, 1, 5, 10, 8, None) == -1
    usage = json.load(open(os.path.join(L.OBJ_DIR, "libdkt_hip.so.resource_usage.json")))
    mine = {k: u for k, u in usage.items() if "rownoise_kernel" in k or "dirichlet_proba_kernel" in k}
    assert len(usage) <= 250 and len(mine) == 2 and len([k for k in usage if "dkt_mll_rownoise" in k]) == 0
    for u in mine.values():
        assert u["vgpr_spill"] == 0 and u["sgpr_spill"] == 0 and u["scratch"] == 0
    assert L.check_resources(usage) == []


def test_dirichlet_needs_the_gpu_and_the_other_likelihoods_are_unchanged(monkeypatch):
    monkeypatch.setattr(dkt_amd.configs, "likelihood", None)
    keys = set(dkt_amd.DKT(dkt_amd.backbone.Conv4S, n_way=5, n_support=5).state_dict())
    m = dkt_amd.DKT(dkt_amd.backbone.Conv4S, n_way=5, n_support=1, likelihood="dirichlet")
    assert set(m.state_dict()) == keys and m.laplace is False and "dirichlet" in dkt_amd.dkt.LIKELIHOODS
    assert dkt_amd.DKT(dkt_amd.backbone.Conv4S, n_way=5, n_support=1, likelihood="bernoulli").laplace == "deep"
    assert not m.model.raw_noise.requires_grad and m.model.raw_outputscale.requires_grad and m.model.mean_constant.requires_grad
    y = m._targets(5, 5, torch.device("cpu"))
    yt, nr = m._dirichlet_targets(y)
    assert tuple(yt.shape) == (5, 25) and m._dirichlet_targets(y)[0] is yt and abs(float(nr.min()) - 0.688184) < 1e-5
    with pytest.raises(RuntimeError, match="HIP-only"):
        m._episode_loss(torch.nn.functional.normalize(torch.randn(25, 64)), y)
    with pytest.raises(RuntimeError, match="HIP-only"):
        dkt_amd.ops.dirichlet_objective(torch.eye(5)[None], torch.zeros(2, 5), torch.ones(2, 5), torch.ones(2), torch.zeros(2), torch.ones(2))
    with pytest.raises(RuntimeError, match="HIP-only"):
        dkt_amd.ops.dirichlet_proba(torch.zeros(1, 2, 3), torch.zeros(1, 2, 3), torch.zeros(4, 2))
    with pytest.raises(ValueError, match="127"):
        m._episode_loss(torch.randn(130, 64), m._targets(5, 26, torch.device("cpu")))
    with pytest.raises(ValueError, match="32"):
        m._episode_loss(torch.randn(66, 64), torch.ones(33, 66))
    with pytest.raises(ValueError):
        dkt_amd.DKT(dkt_amd.backbone.Conv4S, n_way=5, n_support=5, likelihood="probit")
    from dkt_amd.io_utils import checkpoint_dir_for, parse_args
    a, b = parse_args("train", []), parse_args("train", ["--likelihood", "dirichlet"])
    assert a.likelihood == "gaussian" and b.likelihood == "dirichlet" and checkpoint_dir_for(b, "s") == checkpoint_dir_for(a, "s") + "_dirichlet"
    # the evaluation drivers' flag is the default likelihood of the models the process builds (test_uncertainty.py does not pass it on); train.py's is not
    assert dkt_amd.configs.likelihood is None and dkt_amd.DKT(dkt_amd.backbone.Conv4S, 5, 1).likelihood_type == "gaussian"
    assert parse_args("test", ["--likelihood", "dirichlet"]).likelihood == "dirichlet" and dkt_amd.configs.likelihood == "dirichlet"
    assert dkt_amd.DKT(dkt_amd.backbone.Conv4S, 5, 1).likelihood_type == "dirichlet"
    assert dkt_amd.DKT(dkt_amd.backbone.Conv4S, 5, 1, likelihood="gaussian").likelihood_type == "gaussian"
    assert parse_args("test", []).likelihood == "gaussian" and dkt_amd.DKT(dkt_amd.backbone.Conv4S, 5, 1).likelihood_type == "gaussian"
