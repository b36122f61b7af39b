"""-m gpu: the test-time path -- cross Gram (gram_nt_kernel<KIND, false>), posterior mean + labels (predict_mean_kernel), predictive variance
(predict_var_kernel) -- against float64 arithmetic on the float32-rounded inputs, at the tiling, block and LDS edges of those kernels.

Every case runs the product library (no variant switch; `_on_product_library()` right before the first kernel call).  The reference is never
another call into the library.  Each test prints the figures it asserts on (`pytest -s` shows them; docs/MEASUREMENTS.md records a run).

Tolerances
  LINEAR cross Gram   2e-6 max|ref| + 1e-6                 (test_gpu_parity.test_gram_linear_cross)
  RBF cross Gram      2e-5 absolute                         (test_gpu_parity.test_gram_rbf)
  SQDIST cross Gram   derived, see test_cross_gram_edges
  posterior mean      derived, see _predict_reference
  variance            measured against a float32 CPU restatement of the same recurrence, see _check_variance
"""
import functools

import numpy as np
import pytest
import torch

import dkt_amd
from dkt_amd import ops
from oracle import dkt_oracle as O

pytestmark = pytest.mark.gpu
U = 2.0 ** -24          # unit roundoff of float32


def dev_t(a, dev):
    return torch.as_tensor(np.asarray(a, dtype=np.float32), device=dev)


def _on_product_library():
    """Right before a kernel call of a test that claims the product library: the call really goes there (a renamed switch cannot quietly move it to the twins)."""
    assert ops._lib_now()._name == dkt_amd._lib.LIB_PATH


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _up(a):
    """The float32-rounded values, as float64."""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


# ----------------------------------------------------------------------------------------------
# (a) cross Gram edges: 64 x 64 output tile, 32-wide K stage, the 16-byte-load switch (D % 4)
# ----------------------------------------------------------------------------------------------
GRAM_SHAPES = [(1, 1, 1), (63, 65, 31), (64, 64, 32), (65, 63, 33), (129, 64, 36), (64, 129, 70), (130, 131, 3), (80, 25, 64), (320, 100, 64)]
KINDS = {"linear": ops.KERNEL_LINEAR, "rbf": ops.KERNEL_RBF, "sqdist": ops.KERNEL_SQDIST}


def _gram_inputs(kind, m, n, d):
    """Two episodes with different data; asymmetric content in the second operand (a transposed store changes the result)."""
    rng = np.random.default_rng(100000 * m + 100 * n + d)
    if kind == "linear":
        a, bm = rng.standard_normal((2, m, d)), rng.standard_normal((2, n, d))
        bm[0, 0, :] = np.arange(d)
        return _f32(a), _f32(bm), None
    a = np.abs(rng.standard_normal((2, m, d))) * 0.5 + 5.0          # ReLU-like, common offset 5
    bm = np.abs(rng.standard_normal((2, n, d))) * 0.5 + 5.0
    bm[0, 0, :] += np.linspace(0.0, 1.0, d)
    return _f32(a), _f32(bm), np.float32(0.45 * np.sqrt(d))          # E|a - b|^2 = 0.18 D: the scaled distances are of order 1


def _sqdist_f32_restatement(a, bm, ls):
    """The kernel's formula in float32 numpy: operands shifted by row 0 of A, d2 = |a'|^2 + |b'|^2 - 2 a'.b' clamped at 0, times 1 / l^2."""
    out = np.empty((a.shape[0], a.shape[1], bm.shape[1]), dtype=np.float32)
    inv_l2 = np.float32(1.0) / (ls * ls)
    for i in range(a.shape[0]):
        ap, bp = a[i] - a[i, :1], bm[i] - a[i, :1]
        d2 = (ap * ap).sum(1, dtype=np.float32)[:, None] + (bp * bp).sum(1, dtype=np.float32)[None, :] - np.float32(2.0) * (ap @ bp.T)
        out[i] = np.maximum(d2, np.float32(0.0)) * inv_l2
    assert out.dtype == np.float32
    return out


def _sqdist_reference(a, bm, ls):
    """float64 squared distances / l^2 and the element-wise bound 4 (D + 4) 2^-24 (|a'|^2 + |b'|^2) / l^2, a' = a - r, b' = b - r, r = row 0 of A."""
    a64, b64, l64 = _up(a), _up(bm), float(ls)
    d = a.shape[2]
    ref = ((a64[:, :, None, :] - b64[:, None, :, :]) ** 2).sum(-1) / l64 ** 2
    ap, bp = a64 - a64[:, :1], b64 - a64[:, :1]
    bound = 4.0 * (d + 4) * U * ((ap * ap).sum(-1)[:, :, None] + (bp * bp).sum(-1)[:, None, :]) / l64 ** 2
    return ref, bound


@pytest.mark.parametrize("m,n,d", GRAM_SHAPES)
@pytest.mark.parametrize("kind", ["linear", "rbf", "sqdist"])
def test_cross_gram_edges(cuda, kind, m, n, d):
    """dkt_gram_f32 with a second operand at M, N around one and two tiles, D around one K stage, D % 4 != 0 with several tiles, D < 32.

    SQDIST tolerance, derived from the kernel's formula d2 = |a'|^2 + |b'|^2 - 2 a'.b' (a' = a - r, b' = b - r, r = row 0 of A, all in fp32):
    the shift rounds every element once (relative 2^-24: 2u on each norm and on the dot product), a D-term fp32 accumulation adds at most D u of
    the sum of the absolute terms, 2 |a'.b'| <= |a'|^2 + |b'|^2, and the three final additions, 1 / l^2 (two roundings) and the product add a
    few u of |a'|^2 + |b'|^2 more: in all <= (2 D + 16) u (|a'|^2 + |b'|^2) / l^2 <= 4 (D + 4) 2^-24 (|a'|^2 + |b'|^2) / l^2 per element.
    The float32 numpy restatement of the same formula is held to the same bound first: if that fails the derivation is wrong, not the kernel."""
    a, bm, ls = _gram_inputs(kind, m, n, d)
    lst = None if ls is None else dev_t([ls], cuda)
    _on_product_library()
    e = ops.gram(dev_t(a, cuda), dev_t(bm, cuda), KINDS[kind], lst).cpu().numpy()
    assert e.shape == (2, m, n) and np.isfinite(e).all()
    if kind == "linear":
        ref = np.einsum("bmd,bnd->bmn", _up(a), _up(bm))
        err, tol = np.abs(e - ref).max(), 2e-6 * np.abs(ref).max() + 1e-6
        print("MEASURED cross_gram linear (%d,%d,%d): err %.3e tol %.3e fraction %.3f" % (m, n, d, err, tol, err / tol))
        assert err <= tol, (err, tol)
    elif kind == "rbf":
        err = max(np.abs(e[i] - O.gram_rbf(_up(a[i]), _up(bm[i]), float(ls))).max() for i in range(2))
        print("MEASURED cross_gram rbf (%d,%d,%d): err %.3e tol 2e-5 fraction %.3f" % (m, n, d, err, err / 2e-5))
        assert err < 2e-5, err
    else:
        ref, bound = _sqdist_reference(a, bm, ls)
        frac_np = (np.abs(_sqdist_f32_restatement(a, bm, ls) - ref) / bound).max() if bound.max() > 0 else 0.0
        nz = bound > 0
        assert (e[~nz] == ref[~nz]).all()                                  # (M = 1 and b = row 0 of A: both shifted rows are zero, the distance is exact)
        frac = (np.abs(e - ref)[nz] / bound[nz]).max() if nz.any() else 0.0
        print("MEASURED cross_gram sqdist (%d,%d,%d): kernel %.3f of the bound, float32 numpy %.3f of the bound" % (m, n, d, frac, frac_np))
        assert frac_np <= 1.0, "the derivation of the bound is wrong: float32 numpy restatement at %.3f of it" % frac_np
        assert frac <= 1.0, frac


# ----------------------------------------------------------------------------------------------
# (b) posterior mean and labels
# ----------------------------------------------------------------------------------------------
def _predict_reference(ex, alpha, sv, mean):
    """float64 mu on the float32 inputs and the derived bound: a sequential fp32 dot product of N terms (N products, N - 1 additions), one
    multiplication by sv and one addition of the mean (fused or not): |mu - ref| <= (N + 3) 2^-24 (|mean_c| + sv_c sum_n |ex_n alpha_n|)."""
    ex64, al64, sv64, mean64 = _up(ex), _up(alpha), _up(sv), _up(mean)
    sub = "bcmn,bcn->bcm" if ex.ndim == 4 else "bmn,bcn->bcm"
    ref = mean64[None, :, None] + sv64[None, :, None] * np.einsum(sub, ex64, al64)
    bound = (ex.shape[-1] + 3) * U * (np.abs(mean64)[None, :, None] + sv64[None, :, None] * np.einsum(sub, np.abs(ex64), np.abs(al64)))
    return ref, bound


def _check_mean_and_labels(tag, mu, labels, ref, bound):
    """mu inside the derived bound; labels = first-maximum arg-max of the kernel's own mu, and = the float64 arg-max wherever the float64
    top-two gap exceeds twice the bound (at most one query of the case may be that close: asserted on the float64 side alone)."""
    assert mu.shape == ref.shape and np.isfinite(mu).all()
    frac = (np.abs(mu - ref) / bound).max()
    print("MEASURED predict %s: max |mu - ref| %.3e, %.3f of the bound" % (tag, np.abs(mu - ref).max(), frac))
    assert frac <= 1.0, frac
    assert labels.dtype == np.int32 and labels.shape == (ref.shape[0], ref.shape[2])
    assert (labels == mu.argmax(1)).all(), "labels must be the first-maximum arg-max of the kernel's own means"
    if ref.shape[1] > 1:
        top = np.sort(ref, axis=1)
        decided = (top[:, -1] - top[:, -2]) > 2.0 * bound.max(1)
        assert (~decided).sum() <= 1, "the float64 reference leaves %d queries undecided: choose another seed" % (~decided).sum()
        assert (labels[decided] == ref.argmax(1)[decided]).all()


def _predict_inputs(b, c, m, n, per_class, seed):
    rng = np.random.default_rng(seed)
    ex = rng.standard_normal((b, c, m, n) if per_class else (b, m, n))
    alpha = rng.standard_normal((b, c, n))
    return _f32(ex), _f32(alpha), _f32(np.linspace(0.5, 2.0, c)), _f32(0.1 * rng.standard_normal(c))


# M at 255 / 256 / 257 (the 256-thread block edge: the threads past M leave after the barrier), C N 4 bytes of LDS up to and above 48 KB and 64 KB
# (the hipFuncSetAttribute branch), C > 20
PREDICT_SHARED = [(1, 1, 1, 1), (2, 5, 255, 25), (2, 5, 256, 105), (2, 5, 257, 105), (1, 20, 513, 100), (1, 20, 80, 420), (1, 32, 70, 420), (1, 40, 70, 420)]
PREDICT_PER_CLASS = [(3, 4, 37, 29), (1, 20, 257, 100), (2, 33, 65, 7)]


@pytest.mark.parametrize("b,c,m,n", PREDICT_SHARED)
def test_predict_shared_cross_kernel(cuda, b, c, m, n):
    ex, alpha, sv, mean = _predict_inputs(b, c, m, n, False, 7 + 1000 * m + n + c)
    ref, bound = _predict_reference(ex, alpha, sv, mean)
    _on_product_library()
    mu, labels = ops.predict(dev_t(ex, cuda), dev_t(alpha, cuda), dev_t(sv, cuda), dev_t(mean, cuda))
    _check_mean_and_labels("shared (%d,%d,%d,%d)" % (b, c, m, n), mu.cpu().numpy(), labels.cpu().numpy(), ref, bound)


@pytest.mark.parametrize("b,c,m,n", PREDICT_PER_CLASS)
def test_predict_per_class_cross_kernel(cuda, b, c, m, n):
    ex, alpha, sv, mean = _predict_inputs(b, c, m, n, True, 11 + 1000 * m + n + c)
    ref, bound = _predict_reference(ex, alpha, sv, mean)
    _on_product_library()
    mu, labels = ops.predict(dev_t(ex, cuda), dev_t(alpha, cuda), dev_t(sv, cuda), dev_t(mean, cuda))
    _check_mean_and_labels("per class (%d,%d,%d,%d)" % (b, c, m, n), mu.cpu().numpy(), labels.cpu().numpy(), ref, bound)


@pytest.mark.parametrize("per_class", [False, True], ids=["shared", "per_class"])
@pytest.mark.parametrize("tied", [(0, 1), (2, 4), (0, 4), (0, 2, 4)], ids=["first_two", "middle_last", "first_last", "three"])
def test_predict_exact_ties_lower_index_wins(cuda, per_class, tied):
    """Bitwise identical rows of alpha, sv and mean (and of a per-class Ex) give bitwise equal means; their mean of 40 puts them above every
    other class at every query (checked in float64), so the label must be the lowest tied index."""
    b, c, m, n = (2, 5, 65, 29) if per_class else (2, 5, 257, 105)
    ex, alpha, sv, mean = _predict_inputs(b, c, m, n, per_class, 23 + len(tied) + sum(tied))
    alpha *= np.float32(1.0 / np.sqrt(n))
    mean[list(tied)] = 40.0
    for k in tied[1:]:
        alpha[:, k], sv[k] = alpha[:, tied[0]], sv[tied[0]]
        if per_class:
            ex[:, k] = ex[:, tied[0]]
    ref, bound = _predict_reference(ex, alpha, sv, mean)
    others = [k for k in range(c) if k not in tied]
    assert (ref[:, tied[0]] - ref[:, others].max(1) > 1.0).all()           # the tied classes lead everywhere, far beyond the rounding bound
    _on_product_library()
    mu, labels = ops.predict(dev_t(ex, cuda), dev_t(alpha, cuda), dev_t(sv, cuda), dev_t(mean, cuda))
    mu, labels = mu.cpu().numpy(), labels.cpu().numpy()
    assert (np.abs(mu - ref) <= bound).all()
    for k in tied[1:]:
        assert (mu[:, k].view(np.int32) == mu[:, tied[0]].view(np.int32)).all(), "identical class rows must give bitwise equal means"
    assert len(np.unique(mu[:, tied[0]])) > 1                                # (the dot products still show below the mean of 40)
    assert (labels == tied[0]).all(), "the lowest tied index must win"


# ----------------------------------------------------------------------------------------------
# (c) predictive variance, isolated from the factorisation
# ----------------------------------------------------------------------------------------------
def _variance_f32_restatement(ex, exx, chol, sv, noise):
    """The kernel's recurrence in float32 numpy, one episode and class: forward substitution of sv ex_q, every right-hand side element updated
    in the order k = 0, 1, ... (as the kernel's inner loop), then sv exx - |v|^2 + noise.  ex [M,N], exx [M], chol [N,N]."""
    n = ex.shape[1]
    r = sv * ex
    acc = np.zeros(ex.shape[0], dtype=np.float32)
    for k in range(n):
        v = r[:, k] / chol[k, k]
        acc += v * v
        if k + 1 < n:
            r[:, k + 1:] -= v[:, None] * chol[None, k + 1:, k]
    out = sv * exx - acc + noise
    assert out.dtype == np.float32
    return out


def _variance_float64(ex, exx, chol, sv, noise):
    """sv exx - sv^2 ex K^-1 ex^T + noise in float64, K = L L^T.  ex [M,N], exx [M], chol [N,N] (float64 values)."""
    import scipy.linalg as sla
    v = sla.solve_triangular(chol, sv * ex.T, lower=True)
    return sv * exx - (v * v).sum(0) + noise


def _check_variance(tag, var, ref, rest, slack):
    """The rule of the variance tests: the kernel's error against float64 is at most 4 times the largest error of the float32 restatement (the
    factor covers the other summation order and FMA contraction) plus 4 * 2^-24 (sv exx + noise), element by element (`slack`)."""
    assert var.shape == ref.shape and np.isfinite(var).all()
    err_k, err_r = np.abs(var - ref), np.abs(rest.astype(np.float64) - ref).max()
    print("MEASURED variance %s: kernel %.3e, float32 restatement %.3e, ratio %.2f" % (tag, err_k.max(), err_r, err_k.max() / max(err_r, 1e-300)))
    assert (err_k <= 4.0 * err_r + slack).all(), (err_k.max(), err_r)


@functools.lru_cache(maxsize=None)
def _variance_case(b, c, m, n):
    """Float64 problem built on the CPU: unit-norm support rows, K_c = sv_c E + noise_c I, L = chol(K_c); every (b, c) its own L, every b its own
    Ex; the query rows have norms in [0.5, 1] so that exx depends on (b, q).  The kernel is given float32(L)."""
    rng = np.random.default_rng(31 + 1000 * m + 10 * n + b + c)
    d = 16
    zs = rng.standard_normal((b, n, d))
    zs /= np.linalg.norm(zs, axis=2, keepdims=True)
    zq = rng.standard_normal((b, m, d))
    zq *= rng.uniform(0.5, 1.0, (b, m, 1)) / np.linalg.norm(zq, axis=2, keepdims=True)
    sv, noise = _f32(rng.uniform(0.5, 2.0, c)), _f32(rng.uniform(0.1, 0.3, c))
    ex, exx = _f32(zq @ zs.transpose(0, 2, 1)), _f32((zq * zq).sum(2))
    e = zs @ zs.transpose(0, 2, 1)
    chol = np.empty((b, c, n, n), dtype=np.float32)
    ref, rest = np.empty((b, c, m)), np.empty((b, c, m), dtype=np.float32)
    for i in range(b):
        for k in range(c):
            chol[i, k] = np.linalg.cholesky(float(sv[k]) * e[i] + float(noise[k]) * np.eye(n))
            ref[i, k] = _variance_float64(_up(ex[i]), _up(exx[i]), _up(chol[i, k]), float(sv[k]), float(noise[k]))
            rest[i, k] = _variance_f32_restatement(ex[i], exx[i], chol[i, k], sv[k], noise[k])
    slack = 4.0 * U * (_up(sv)[None, :, None] * _up(exx)[:, None, :] + _up(noise)[None, :, None])
    return ex, exx, chol, sv, noise, ref, rest, slack


# M around the 64-thread workgroup (second workgroup, M % 64 != 0), C > 1, B > 1 with C > 1, N past 31, N = 192 / 193 (dynamic LDS 48 KB / above:
# the other launch configuration) and N = 600, the largest size the entry point accepts (150 KB of LDS)
VARIANCE_CASES = [(1, 1, 1, 1), (1, 1, 19, 5), (3, 3, 63, 19), (2, 3, 64, 31), (2, 2, 65, 64), (1, 3, 130, 100), (1, 1, 65, 192), (2, 2, 65, 193),
                  (1, 1, 64, 257), (1, 1, 65, 600)]


@pytest.mark.parametrize("b,c,m,n", VARIANCE_CASES)
def test_predict_var_kernel_alone(cuda, b, c, m, n):
    ex, exx, chol, sv, noise, ref, rest, slack = _variance_case(b, c, m, n)
    assert (ref > 0).all()
    _on_product_library()
    var = ops.predict_var(dev_t(ex, cuda), dev_t(exx, cuda), dev_t(chol, cuda), dev_t(sv, cuda), dev_t(noise, cuda)).cpu().numpy()
    _check_variance("alone (%d,%d,%d,%d)" % (b, c, m, n), var, ref, rest, slack)


# ----------------------------------------------------------------------------------------------
# (d) the chain that users run
# ----------------------------------------------------------------------------------------------
def _rbf_f32(a, bm, ls):
    """The RBF kernel as the library forms it, in float32 numpy: exp(-0.5 d2 / l^2) from the shifted-norm squared distances; bm None: symmetric, unit diagonal."""
    u = _sqdist_f32_restatement(a[None], (a if bm is None else bm)[None], ls)[0]
    e = np.exp(np.float32(-0.5) * u)
    if bm is None:
        e = np.float32(0.5) * (e + e.T)
        np.fill_diagonal(e, np.float32(1.0))
    assert e.dtype == np.float32
    return e


@pytest.mark.parametrize("n", [19, 40, 100, 150])
def test_regression_chain_every_cholesky_route(cuda, n):
    """gram -> mll(want_chol) -> cross gram -> predict + predict_var against O.regression_predict, RBF kernel, hyper-parameters of
    test_predict_variance_vs_oracle; the factor comes from the MFMA route (N = 19), the generic route (N = 40, 100) and the blocked route (N = 150).
    Variance: the rule of _check_variance, the float32 restatement being the same chain in float32 numpy (the kernel matrices by the library's
    formula, numpy's float32 Cholesky, the forward substitution of _variance_f32_restatement)."""
    b, m, d = 2, 70, 60
    rng = np.random.default_rng(4 + n)
    zs, zq, y = _f32(np.abs(rng.standard_normal((b, n, d)))), _f32(np.abs(rng.standard_normal((b, m, d)))), _f32(rng.standard_normal((b, n)))
    sv, mean, noise, ls = np.float32(0.8), np.float32(0.1), np.float32(0.3), np.float32(4.0)
    hyp = O.GPHypers(_up([sv]), _up([mean]), _up([noise]), lengthscale=float(ls))
    refs = [O.regression_predict(_up(zs[i]), _up(y[i]), _up(zq[i]), hyp) for i in range(b)]
    rest = np.empty((b, 1, m), dtype=np.float32)
    for i in range(b):
        k32 = sv * _rbf_f32(zs[i], None, ls) + noise * np.eye(n, dtype=np.float32)
        l32 = np.linalg.cholesky(k32)
        assert l32.dtype == np.float32
        rest[i, 0] = _variance_f32_restatement(_rbf_f32(zq[i], zs[i], ls), np.ones(m, dtype=np.float32), l32, sv, noise)
    lst, svt, meant, noiset = dev_t([ls], cuda), dev_t([sv], cuda), dev_t([mean], cuda), dev_t([noise], cuda)
    zst, zqt = dev_t(zs, cuda), dev_t(zq, cuda)
    _on_product_library()
    out = ops.mll(ops.gram(zst, None, ops.KERNEL_RBF, lst), dev_t(y[:, None, :], cuda), svt, meant, noiset, want_chol=True)
    assert int(out["info"].abs().max().item()) == 0 and float(out["jitter"].abs().max().item()) == 0.0
    ex = ops.gram(zqt, zst, ops.KERNEL_RBF, lst)
    mu, _ = ops.predict(ex, out["alpha"], svt, meant, want_labels=False)
    var = ops.predict_var(ex, torch.ones(b, m, device=cuda), out["chol"], svt, noiset)
    mu, var = mu.cpu().numpy(), var.cpu().numpy()
    err_mu = max(np.abs(mu[i, 0] - refs[i]["mean"]).max() for i in range(b))
    print("MEASURED regression chain N=%d: max |mean - ref| %.3e (tolerance 1e-4)" % (n, err_mu))
    assert err_mu < 1e-4, err_mu
    ref_var = np.stack([r["var"] for r in refs])[:, None, :]
    _check_variance("chain N=%d" % n, var, ref_var, rest, np.full(ref_var.shape, 4.0 * U * (float(sv) + float(noise))))


@pytest.mark.parametrize("c,s,q,d", [(5, 5, 16, 64), (5, 21, 3, 64), (20, 5, 16, 64), (20, 21, 2, 32)])
def test_classification_chain_vs_eval_episode(cuda, c, s, q, d):
    """gram -> mll -> cross gram -> predict against O.eval_episode, two episodes; (20, 21, 2, 32) is N = 420: alpha from the tile-array kernels."""
    z = _f32(O.synthetic_features(2, c * (s + q), d, 41 + c + s))
    h = O.perturbed_hypers(c, 43 + c + s)
    hyp = O.GPHypers(_up(h.outputscale), _up(h.mean), _up(h.noise))
    zall = z.reshape(2, c, s + q, d)
    zs, zq = np.ascontiguousarray(zall[:, :, :s]).reshape(2, c * s, d), np.ascontiguousarray(zall[:, :, s:]).reshape(2, c * q, d)
    refs = [O.eval_episode(_up(zs[i]), _up(zq[i]), c, hyp) for i in range(2)]
    for r in refs:
        top = np.sort(r["mu"], axis=0)
        assert ((top[-1] - top[-2]) <= 2e-4).sum() <= 1, "the float64 reference leaves more than one query undecided: choose another seed"
    svt, meant, noiset = dev_t(hyp.outputscale, cuda), dev_t(hyp.mean, cuda), dev_t(hyp.noise, cuda)
    zst, zqt = dev_t(zs, cuda), dev_t(zq, cuda)
    _on_product_library()
    out = ops.mll(ops.gram(zst), dev_t(O.one_vs_rest_targets(c, s), cuda), svt, meant, noiset)
    assert int(out["info"].abs().max().item()) == 0
    mu, labels = ops.predict(ops.gram(zqt, zst), out["alpha"], svt, meant)
    mu, labels = mu.cpu().numpy(), labels.cpu().numpy()
    err = max(np.abs(mu[i] - refs[i]["mu"]).max() for i in range(2))
    print("MEASURED classification chain (%d,%d,%d,%d): max |mu - ref| %.3e (tolerance 1e-4)" % (c, s, q, d, err))
    assert err < 1e-4, err
    for i in range(2):
        top = np.sort(refs[i]["mu"], axis=0)
        decided = (top[-1] - top[-2]) > 2e-4
        assert (labels[i][decided] == refs[i]["labels"][decided]).all()
        assert (labels[i] == mu[i].argmax(0)).all()


# ----------------------------------------------------------------------------------------------
# (e) per-class cross kernel maps
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,c,m,n,d", [(2, 3, 37, 29, 12), (1, 20, 80, 100, 16), (1, 5, 1, 7, 5), (1, 3, 65, 64, 33)])
@pytest.mark.parametrize("kernel", ["rbf", "matern", "poli1", "poli2"])
def test_per_class_cross_kernel_maps_into_predict(cuda, kernel, b, c, m, n, d):
    """ops.kernel_matrix_per_class(zq, zs, ...) with per-class lengthscales / offsets, per class against the oracle's kernel; its result goes
    through the per-class posterior mean, checked with the bound of _predict_reference on the kernel matrices the library produced."""
    rng = np.random.default_rng(53 + 1000 * m + 10 * n + d + c)
    zq, zs = _f32(0.4 * rng.standard_normal((b, m, d))), _f32(0.4 * rng.standard_normal((b, n, d)))
    param = _f32(np.linspace(0.7, 1.8, c))
    alpha, sv, mean = _f32(rng.standard_normal((b, c, n))), _f32(np.linspace(0.5, 2.0, c)), _f32(0.1 * rng.standard_normal(c))
    oracle = {"rbf": lambda x, y_, p: O.gram_rbf(x, y_, p), "matern": lambda x, y_, p: O.gram_matern25(x, y_, p),
              "poli1": lambda x, y_, p: O.gram_poly(x, y_, 1, p), "poli2": lambda x, y_, p: O.gram_poly(x, y_, 2, p)}[kernel]
    _on_product_library()
    ext = ops.kernel_matrix_per_class(dev_t(zq, cuda), dev_t(zs, cuda), kernel, dev_t(param, cuda), dev_t(param, cuda))
    ex = ext.cpu().numpy()
    assert ex.shape == (b, c, m, n) and np.isfinite(ex).all()
    worst = 0.0
    for i in range(b):
        for k in range(c):
            ref = oracle(_up(zq[i]), _up(zs[i]), float(param[k]))
            err, tol = np.abs(ex[i, k] - ref).max(), 2e-5 * max(1.0, np.abs(ref).max())
            worst = max(worst, err / tol)
            assert err <= tol, (i, k, err, tol)
    print("MEASURED per-class cross kernel %s (%d,%d,%d,%d,%d): %.3f of the tolerance" % (kernel, b, c, m, n, d, worst))
    mu, labels = ops.predict(ext, dev_t(alpha, cuda), dev_t(sv, cuda), dev_t(mean, cuda))
    ref, bound = _predict_reference(ex, alpha, sv, mean)
    mu, labels = mu.cpu().numpy(), labels.cpu().numpy()
    frac = (np.abs(mu - ref) / bound).max()
    print("MEASURED per-class cross kernel %s (%d,%d,%d,%d,%d) -> predict: %.3f of the bound" % (kernel, b, c, m, n, d, frac))
    assert frac <= 1.0, frac
    assert (labels == mu.argmax(1)).all()


# ----------------------------------------------------------------------------------------------
# (f) limits that launch nothing, (2) argument checks of ops.predict_var
# ----------------------------------------------------------------------------------------------
def test_predict_lds_limit_is_an_error(cuda):
    """C N = 38 401 floats of mean caches are 4 bytes above the 150 KB the kernel may ask for: DKT_ERR_TOO_LARGE before any launch."""
    n = 38401
    _on_product_library()
    with pytest.raises(RuntimeError, match="DKT_ERR_TOO_LARGE"):
        ops.predict(torch.zeros(1, 1, n, device=cuda), torch.zeros(1, 1, n, device=cuda), torch.ones(1, device=cuda), torch.zeros(1, device=cuda))


def test_predict_var_size_limit_is_an_error(cuda):
    n = 601
    _on_product_library()
    with pytest.raises(RuntimeError, match="DKT_ERR_TOO_LARGE"):
        ops.predict_var(torch.zeros(1, 1, n, device=cuda), torch.ones(1, 1, device=cuda), torch.eye(n, device=cuda).reshape(1, 1, n, n),
                        torch.ones(1, device=cuda), torch.ones(1, device=cuda))


def test_predict_batch_limit_is_an_error(cuda):
    b = 65536
    _on_product_library()
    with pytest.raises(RuntimeError, match="DKT_ERR_TOO_LARGE"):
        ops.predict(torch.zeros(b, 1, 1, device=cuda), torch.zeros(b, 1, 1, device=cuda), torch.ones(1, device=cuda), torch.zeros(1, device=cuda))


@pytest.mark.parametrize("what", ["exx_length", "exx_batch", "chol_n", "chol_batch", "chol_not_square", "sv", "noise", "ex_dims"])
def test_predict_var_rejects_malformed_arguments(cuda, what):
    """ops.predict_var checks what it is given before the kernel reads it: ex [B,M,N], exx [B,M], chol [B,C,N,N], sv and noise of C elements."""
    b, c, m, n = 2, 3, 7, 5
    z = lambda *shape: torch.zeros(*shape, device=cuda)  # noqa: E731
    args = dict(ex=z(b, m, n), exx=z(b, m), chol=torch.eye(n, device=cuda).expand(b, c, n, n).contiguous(), sv=torch.ones(c, device=cuda), noise=torch.ones(c, device=cuda))
    _on_product_library()
    assert ops.predict_var(**args).shape == (b, c, m)                           # the well-formed call goes through
    args.update({"exx_length": dict(exx=z(b, m - 1)), "exx_batch": dict(exx=z(1, m)), "chol_n": dict(chol=z(b, c, n + 1, n + 1)),
                 "chol_batch": dict(chol=z(1, c, n, n)), "chol_not_square": dict(chol=z(b, c, n, n + 1)), "sv": dict(sv=torch.ones(c + 1, device=cuda)),
                 "noise": dict(noise=torch.ones(1, device=cuda)), "ex_dims": dict(ex=z(b, 1, m, n))}[what])
    with pytest.raises(RuntimeError, match="predict_var|must have"):
        ops.predict_var(**args)
