"""CPU-side checks of Bernoulli-likelihood training: the float64 restatement of dkt_laplace_grad_f32 (tests/laplace_grad_model.py) against central finite
differences of the polished-mode lml and against scikit-learn's `log_marginal_likelihood(eval_gradient=True)`; the shared form; the new symbols of the
product ABI (still version 7, still at most 250 kernels, no spill); the DKT surface without a GPU."""
import json
import os
import re

import numpy as np
import pytest
import torch
from sklearn.gaussian_process import GaussianProcessClassifier
from sklearn.gaussian_process.kernels import RBF, ConstantKernel

import dkt_amd
import laplace_grad_model as gm
import laplace_model as lm

L = dkt_amd._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# scikit-learn differentiates with the temporaries of its LAST Newton iteration (pi, W, L one step before the returned f), this project at f_hat itself: the two
# gradients differ by what that last step still moved.  Measured here (float64, N = 25, C(2.0) * RBF(1.0), both hyper-parameters, the 5 one-vs-rest problems; scikit-learn converges
# further than its 1e-10 test suggests -- Newton is quadratic -- so the gap is at rounding level):
SKLEARN_GAP = 1.04e-15          # relative; measured with scikit-learn 1.7.2 on OpenBLAS-backed numpy / scipy (another BLAS may round a few ulps differently)


def _problem(n, c, ls, spread, seed):
    rng = np.random.default_rng(seed)
    zs, _ = lm.clustered(rng, c, n // c, 1, 64, spread)
    return zs, lm.rbf(zs, zs, ls), lm.one_vs_rest(c, n // c)


@pytest.mark.parametrize("n, c, ls, spread, scale", [(5, 5, 0.1, 0.3, 1.0), (25, 5, 0.1, 0.1, 1.0), (12, 4, 0.1, 0.1, 5.0)], ids=str)
def test_gradient_matches_central_differences_of_the_polished_mode_lml(n, c, ls, spread, scale):
    _, k, y = _problem(n, c, ls, spread, n)
    rng = np.random.default_rng(n + 1)
    worst = 0.0
    for ci in (0, c - 1):
        lml, g = gm.grad_one(scale * k, y[ci], gm.mode_polished(scale * k, y[ci]))
        for _ in range(3):
            d = rng.standard_normal((n, n))
            d, h = (d + d.T) / 2, 1e-5
            fd = (gm.lml_at(scale * (k + h * d), y[ci], gm.mode_polished(scale * (k + h * d), y[ci]))
                  - gm.lml_at(scale * (k - h * d), y[ci], gm.mode_polished(scale * (k - h * d), y[ci]))) / (2 * h)
            worst = max(worst, abs(fd - scale * (g * d).sum()) / abs(fd))
    print("n = %d: worst relative difference to central differences %.3g" % (n, worst))
    assert worst < 1e-7          # the truncation + rounding error of the difference quotient at h = 1e-5 (measured: 5e-10)


def test_gradient_against_sklearn_at_its_last_iterates_temporaries():
    zs, _, y = _problem(25, 5, 1.0, 0.5, 3)
    kern = ConstantKernel(2.0) * RBF(1.0)
    gp = GaussianProcessClassifier(kern, optimizer=None).fit(zs, np.repeat(np.arange(5), 5))
    k, kgrad = kern(zs, eval_gradient=True)                                  # d K / d log(theta)
    gap = 0.0
    for ci, est in enumerate(gp.base_estimator_.estimators_):
        sk_lml, sk_grad = est.log_marginal_likelihood(kern.theta, eval_gradient=True)
        lml, g = gm.grad_one(k, y[ci], gm.mode_polished(k, y[ci]))
        ours = np.array([(g * kgrad[:, :, t]).sum() for t in range(2)])
        # relative to the size of what is compared (lml is about -10, the gradient entries about 1): a rounding-level figure in units of the quantities
        gap = max(gap, float(np.abs(ours - sk_grad).max() / np.abs(sk_grad).max()), abs(lml - sk_lml) / abs(sk_lml))
    print("largest relative difference to scikit-learn (gradient and value): %.3g" % gap)
    assert gap <= 10 * SKLEARN_GAP


def test_shared_form_is_the_sum_of_the_per_class_outputs():
    _, k, y = _problem(25, 5, 0.1, 0.1, 9)
    k = np.stack([k, k * k])
    sc, cw = np.array([0.5, 5.0, 1.0, 2.0, 0.5]), np.linspace(0.5, 1.5, 5) / -25.0
    f = gm.modes(k, y, sc)
    lml_s, dk_s, ds_s = gm.laplace_grad(k, y, f, cw, sc)
    lml_p, dk_p, ds_p = gm.laplace_grad(np.repeat(k[:, None], 5, 1), y, f, cw, sc)
    assert dk_s.shape == (2, 25, 25) and dk_p.shape == (2, 5, 25, 25)
    acc = np.zeros_like(dk_s)
    for ci in range(5):
        acc = acc + dk_p[:, ci]
    assert np.array_equal(dk_s, acc) and np.array_equal(lml_s, lml_p) and np.array_equal(ds_s, ds_p)
    for b in range(2):
        for ci in range(5):
            lml, g = gm.grad_one(sc[ci] * k[b], y[ci], f[b, ci])
            assert np.allclose(ds_s[b, ci], cw[ci] * (g * k[b]).sum(), rtol=1e-12) and np.allclose(dk_p[b, ci], cw[ci] * sc[ci] * g, rtol=1e-12, atol=0)
            assert lml_s[b, ci] == lml and abs(lml - lm.mode_one(sc[ci] * k[b], y[ci])["lml"]) < 1e-8
    assert gm.laplace_grad(k, y, f, cw, sc, dtype=np.float32)[1].dtype == np.float32


def test_new_symbols_are_in_the_header_the_table_and_the_library(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dkt_abi.h")).read(), flags=re.S)
    for name in ("dkt_laplace_grad_workspace_bytes", "dkt_laplace_grad_f32"):
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1)
        assert name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == proto.count(",") + 1 and hasattr(lib, name)
    assert "dkt_laplace_grad.hip" in L.SOURCES and L.SOURCES[-1] == "dkt_laplace_grad.hip"
    assert lib.dkt_abi_version() == 8 and L.abi_version_of_header() == 8
    assert lib.dkt_laplace_grad_workspace_bytes(2, 20, 100) == 2 * 20 * 100 * 100 * 4 and lib.dkt_laplace_grad_workspace_bytes(0, 5, 25) == 0
    assert lib.dkt_laplace_grad_f32(None, 0, 0, None, None, 0, None, None, None, None, None, 1, 5, 25, None, 0, None) == -1
    usage = json.load(open(os.path.join(L.OBJ_DIR, "libdkt_hip.so.resource_usage.json")))
    mine = [u for k, u in usage.items() if "laplace_grad_kernel" in k]
    assert len(usage) <= 250 and len(mine) == 1 and mine[0]["vgpr_spill"] == 0 and mine[0]["scratch"] == 0 and mine[0]["sgpr_spill"] == 0
    assert L.check_resources(usage) == []
    # what paid for it: the 64-row Gram-backward instances beyond 256 rows, which the product's dispatch never reaches (csrc/dkt_gram_big.hip: launch_rows)
    assert not [k for k in usage if re.search(r"gram_bwd_rows_f16x2_kernelILi1[024]ELi4E", k)]


def test_bernoulli_needs_the_gpu_and_gaussian_is_unchanged():
    keys = set(dkt_amd.DKT(dkt_amd.backbone.Conv4S, n_way=5, n_support=5).state_dict())
    assert set(dkt_amd.DKT(dkt_amd.backbone.Conv4S, n_way=5, n_support=5, likelihood="gaussian").state_dict()) == keys
    m = dkt_amd.DKT(dkt_amd.backbone.Conv4S, n_way=5, n_support=1, likelihood="bernoulli")
    assert set(m.state_dict()) == keys and m.laplace == "deep" and dkt_amd.DKT(dkt_amd.backbone.Conv4S, 5, 5).laplace is False
    assert not m.model.raw_noise.requires_grad
    with pytest.raises(RuntimeError, match="HIP-only"):
        m._episode_loss(torch.nn.functional.normalize(torch.randn(25, 64)), m._targets(5, 5, torch.device("cpu")))
    with pytest.raises(RuntimeError, match="HIP-only"):
        dkt_amd.ops.laplace_objective(torch.eye(5)[None], torch.zeros(2, 5), torch.ones(2))
    with pytest.raises(ValueError, match="127"):
        m._episode_loss(torch.randn(130, 64), m._targets(5, 26, torch.device("cpu")))
    with pytest.raises(ValueError):
        dkt_amd.DKT(dkt_amd.backbone.Conv4S, n_way=5, n_support=5, likelihood="probit")
    from dkt_amd.io_utils import checkpoint_dir_for, parse_args
    a, b = parse_args("train", []), parse_args("train", ["--likelihood", "bernoulli"])
    assert a.likelihood == "gaussian" and checkpoint_dir_for(b, "s") == checkpoint_dir_for(a, "s") + "_bernoulli"
