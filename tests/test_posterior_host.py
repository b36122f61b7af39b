"""CPU-side checks of the joint posterior (docs/POSTERIOR.md): the closed form of tests/posterior_model.py IS the definition (the conditional of the joint
Gaussian, scipy's density, the chain rule of the marginal likelihoods); the cases of the GPU comparison cover what they claim and respect the conditioning
cap; its bound (4 x the float32 floor) catches two seeded defects of the model; libdkt_post.so exports exactly include/dkt_abi_post.h (the _lib signature
table too), cross-compiles without spills or scratch, carries its header's version, answers bad arguments on the host, and stands beside both of the
loader's tables; the Python surface refuses what it does not serve."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
from scipy.stats import multivariate_normal

import dkt_amd
import posterior_model as pm
from oracle import dkt_oracle as O

L = dkt_amd._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the model -------------------------------------------------------------------------------------------------------------------------------
def _small(n, m, c, per_class=False, b=2, kernel="rbf"):
    zs, zq = pm.unit_rows(100 * n + m + c, b, n, 8), pm.unit_rows(100 * n + m + c + 7, b, m, 8)
    cc = c if per_class else None
    sv, mean, noise = pm.hypers(c, 0.7, 0.3)
    return (pm.base_matrix(zs, None, kernel, cc), pm.base_matrix(zq, zs, kernel, cc), pm.base_matrix(zq, None, kernel, cc), pm.targets(n, c, n, b), sv, mean,
            noise), pm.targets(m + 1, c, m, b)


@pytest.mark.parametrize("with_noise", [True, False], ids=["noisy", "latent"])
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("n,m", [(1, 1), (5, 19), (19, 19), (40, 33)])
def test_closed_form_is_the_conditional_of_the_joint_gaussian(n, m, c, with_noise):
    args, yq = _small(n, m, c, per_class=c == 3)
    a, d = pm.closed_form(*args, yq=yq, with_noise=with_noise), pm.definition(*args, yq=yq, with_noise=with_noise)
    for key in ("mu", "cov", "logp", "lpd"):
        err = np.abs(a[key] - d[key]).max() / np.abs(d[key]).max()
        print("closed form vs definition N=%d M=%d C=%d %s %s: %.2e" % (n, m, c, "noisy" if with_noise else "latent", key, err))
        assert err < 1e-12, key
    assert np.abs(np.matmul(a["chol"], np.swapaxes(a["chol"], -1, -2)) - a["cov"]).max() < 1e-13 * np.abs(a["cov"]).max()
    assert np.array_equal(a["chol"], np.tril(a["chol"]))


@pytest.mark.parametrize("n,m,c", [(1, 1, 1), (5, 19, 3), (19, 19, 1), (40, 33, 3)])
def test_logp_is_scipys_density_and_the_chain_rule_of_the_marginal_likelihoods(n, m, c):
    """log N(yq | mu, Sigma) by scipy, and log p(y_s, y_q) = log p(y_s) + log p(y_q | y_s) with both marginal likelihoods from the oracle (noise on every row)."""
    args, yq = _small(n, m, c)
    ess, eqs, eqq, y, sv, mean, noise = args
    a = pm.closed_form(*args, yq=yq)
    for b in range(ess.shape[0]):
        joint_e = np.block([[ess[b].astype(np.float64), eqs[b].T.astype(np.float64)], [eqs[b].astype(np.float64), eqq[b].astype(np.float64)]])
        both = O.mll_terms(joint_e, np.concatenate([y[b], yq[b]], -1), sv, mean, noise, jitter0=0.0, max_tries=0).logp
        support = O.mll_terms(ess[b], y[b], sv, mean, noise, jitter0=0.0, max_tries=0).logp
        for k in range(c):
            want = multivariate_normal.logpdf(yq[b, k].astype(np.float64), a["mu"][b, k], a["cov"][b, k])
            assert abs(a["logp"][b, k] - want) < 1e-12 * max(1.0, abs(want))
            assert abs(a["logp"][b, k] - (both[k] - support[k])) < 1e-11 * max(1.0, abs(both[k]), abs(support[k]))
            marg = sum(multivariate_normal.logpdf(float(yq[b, k, i]), a["mu"][b, k, i], a["cov"][b, k, i, i]) for i in range(m))
            assert abs(a["lpd"][b, k] - marg) < 1e-12 * max(1.0, abs(marg))


def test_samples_have_the_posterior_moments():
    """mu + R eps: with eps = the identity the draws are mu + the columns of R, so that their scatter is exactly Sigma."""
    args, _ = _small(5, 19, 1, b=1)
    eps = np.eye(19)[None, None]
    a = pm.closed_form(*args, eps=eps)
    dev = a["samples"][0, 0] - a["mu"][0, 0]
    assert np.abs(dev.T @ dev - a["cov"][0, 0]).max() < 1e-13


def test_the_cases_cover_what_they_claim():
    ks = pm.CASES
    assert 38 <= len(ks) <= 42 and len({(k.n, k.m) for k in ks}) == len(ks)
    assert {k.n for k in ks} == set(pm.NS) | {5, 19} and {k.m for k in ks} == set(pm.MS) | {19}
    assert {(1, 1), (1, 127), (127, 1), (127, 127), (5, 19), (19, 19)} <= {(k.n, k.m) for k in ks}
    assert {k.c for k in ks} == {1, 3, 32} and {k.b for k in ks} == {1, 3, 70}
    assert all(k.b * k.c * (k.n + k.m) ** 2 <= pm.MAX_ELEMENTS for k in ks if k.b == 70)
    assert {k.per_class for k in ks} == {False, True} and {k.y_per_episode for k in ks} == {False, True} and {k.with_noise for k in ks} == {False, True}
    assert {k.s for k in ks} == {0, 1, 7} and {k.has_yq for k in ks} == {False, True}
    assert {k.d for k in ks} == {8, 64} and {k.kernel for k in ks} == {"rbf", "linear"} and {k.noise0 for k in ks} == {0.1, 1.0} and {k.sv0 for k in ks} == {0.3, 1.0}
    assert list(pm.GROUPS) == ["1-2", "15-17", "33", "63-65", "127"]
    for g in pm.GROUPS:          # every group meets both layouts, both covariances, every optional operand and every quantity
        mine = [k for k in ks if k.group == g]
        assert {k.per_class for k in mine} == {False, True} and {k.with_noise for k in mine} == {False, True}, g
        assert {k.has_yq for k in mine} == {False, True} and {k.s > 0 for k in mine} == {False, True} and any(k.b > 1 for k in mine), g
        assert set(pm.floors(g)) == set(pm.QUANTITIES), g
    for k in ks:                 # the query rows are not the support rows
        inp = k.inputs()
        assert inp["e_qs"].shape[-2:] == (k.m, k.n) and float(inp["e_qs"].max()) < 1.0 - 1e-3, k


@pytest.mark.parametrize("index", range(len(pm.CASES)), ids=[repr(k) for k in pm.CASES])
def test_the_cases_respect_the_conditioning_cap(index):
    """In float64 the smallest eigenvalue of Sigma is at least 1e-3 of its largest: rung 0 of the ladder is the only one fp32 should need."""
    ref, _ = pm.reference(index)
    ev = np.linalg.eigvalsh(ref["cov"])
    ratio = float((ev[..., 0] / ev[..., -1]).min())
    print("%r: lambda_min / lambda_max = %.2e" % (pm.CASES[index], ratio))
    assert ratio >= pm.MIN_EIG_RATIO


@pytest.mark.parametrize("group", list(pm.GROUPS))
def test_the_bound_catches_the_seeded_defects(group):
    """V^T V with one operand lacking its sv, and Sigma without its with_noise term (the float64 model otherwise untouched), land outside 4 x the float32 floor
    on cov -- and on logp where the case has it -- at the inputs of the GPU comparison: on every case of the group where the defect can differ (sv != 1 in
    some class; with_noise = 1)."""
    floor = pm.floors(group)
    print("floors %s: %s" % (group, {k: "%.2e" % v for k, v in floor.items()}))
    hits = {"vtv": 0, "noise": 0}
    for i, k in enumerate(pm.CASES):
        if k.group != group:
            continue
        ref, _ = pm.reference(i)
        args, kw = pm._model_args(k.inputs(), k.with_noise)
        for defect, can_differ in (("vtv", bool((pm.hypers(k.c, k.sv0, k.noise0)[0] != 1.0).any())), ("noise", k.with_noise)):
            if not can_differ:
                continue
            bad = pm.closed_form(*args, defect=defect, **kw)
            keys = ("cov",) + (("logp",) if k.has_yq else ())
            err = pm.errors(bad, ref, keys)
            print("  %r %s: %s, bounds %s" % (k, defect, {q: "%.2e" % v for q, v in err.items()}, {q: "%.2e" % (pm.BOUND * floor[q]) for q in keys}))
            for q in keys:                    # (the GPU comparison's own criterion; a defective Sigma that is not positive definite has no logp at all: NaN)
                assert not err[q] <= pm.BOUND * floor[q], (k, defect, q)
            hits[defect] += 1
    assert hits["vtv"] >= 3 and hits["noise"] >= 2


# ---- the library ----------------------------------------------------------------------------------------------------------------------------
def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dkt_\w+)\s*\(", text)))


@pytest.fixture(scope="module")
def post_path():
    if not shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")) and not os.path.exists(L.POST_LIB_PATH):
        pytest.skip("no hipcc and no built libdkt_post.so")
    return L.build_post()


def test_signature_table_is_the_header():
    declared = _declared("dkt_abi_post.h")
    assert declared == ["dkt_post_abi_version", "dkt_posterior_f32", "dkt_posterior_workspace_bytes"]
    assert sorted(L.POST_SIGNATURES) == declared
    text = open(os.path.join(ROOT, "include", "dkt_abi_post.h")).read()
    for macro, value in (("N", L.POST_MAX_N), ("M", L.POST_MAX_M), ("C", L.POST_MAX_C)):
        assert int(re.search(r"#define\s+DKT_POST_MAX_%s\s+(\d+)" % macro, text).group(1)) == value == {"N": 127, "M": 127, "C": 32}[macro]
    flat = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, (_, args) in L.POST_SIGNATURES.items():
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % name, flat).group(1).strip()
        assert len(args) == (0 if proto == "void" else proto.count(",") + 1), name
    assert len(L.POST_SIGNATURES["dkt_posterior_f32"][1]) == 37


def test_post_is_an_extension_library_of_the_table():
    spec = L.LIBS["post"]
    assert all(s.path != L.POST_LIB_PATH and "dkt_posterior.hip" not in s.sources for k, s in L.LIBS.items() if k != "post") and "dkt_posterior.hip" not in L.SOURCES
    assert spec.sources == ["dkt_posterior.hip"] and spec.header == "dkt_abi_post.h" and spec.spill_budget and not spec.twins
    assert spec.src_dir == L.CSRC_EXT and os.path.isfile(os.path.join(spec.src_dir, "dkt_posterior.hip")) and spec.path == L.POST_LIB_PATH
    assert os.path.basename(spec.path) == "libdkt_post.so" and not os.path.exists(os.path.join(L.CSRC, "dkt_posterior.hip"))
    assert L.post_abi_version_of_header() == 1 and L.abi_version_of_header() == 8
    assert not [line for line in open(os.path.join(L.CSRC, "dkt_switches.def")) if "POST" in line]          # no environment switch of its own
    assert "dkt_posterior" not in "".join(L.SIGNATURES)                                                      # nothing added to the product ABI


def test_graft_build_builds_it_after_loo_and_guarded(monkeypatch, capsys):
    import __graft_entry__ as g
    built = []
    monkeypatch.setattr(L, "build", lambda force=False: built.append("build") or L.LIB_PATH)

    def build_lib(key):
        built.append(key)
        if key == "post":
            raise RuntimeError("no compiler today")

    monkeypatch.setattr(L, "build_lib", build_lib)
    monkeypatch.setattr(L, "load", lambda: type("Lib", (), {"dkt_abi_version": staticmethod(L.abi_version_of_header)}))
    g.build()                                                                   # (a failed build of it warns and does not stop the product's)
    assert [k for k in built if k in ("build", "loo", "post", "diag", "twins")] == ["build", "loo", "post", "diag", "twins"]
    assert "libdkt_post.so not built: no compiler today" in capsys.readouterr().err


def test_library_exports_exactly_its_header_and_its_version(post_path):
    out = subprocess.run(["nm", "-D", "--defined-only", post_path], capture_output=True, text=True, check=True).stdout
    exports = sorted({line.split()[-1] for line in out.splitlines() if line.split()[-1].startswith("dkt_")})
    assert exports == _declared("dkt_abi_post.h")
    assert L.device_code_objects(post_path), "no gfx950 code object in the library"
    assert int(L.load_post().dkt_post_abi_version()) == L.post_abi_version_of_header() == 1
    assert not os.path.exists(post_path + ".stamp") or not L._stale(L.LIBS["post"])


def test_library_does_not_spill(post_path):
    usage = json.load(open(os.path.join(L.OBJ_DIR, "libdkt_post.so.resource_usage.json")))
    assert 1 <= len(usage) <= 4 and all("posterior_kernel" in k for k in usage)          # a handful of instances at the most
    assert all(u.get("vgpr_spill", 0) == 0 and u.get("scratch", 0) == 0 for u in usage.values())
    assert L.check_resources(usage) == []


def test_bad_arguments_are_answered_on_the_host(post_path):
    """DKT_ERR_BAD_ARG (-1), DKT_ERR_WORKSPACE (-3) and DKT_ERR_SHAPE (-5) come back before any launch: the pointers below are never dereferenced (this
    machine needs no GPU)."""
    lib = L.load_post()
    p = ctypes.c_void_p(4096)

    def call(Ess=p, ssb=25, ssc=0, Eqs=p, qsb=95, qsc=0, Eqq=p, qqb=361, qqc=0, Y=p, ybs=0, sv=p, mean=p, noise=p, Yq=None, eps=None, B=1, C=2, N=5, M=19, S=0,
             with_noise=1, jitter0=1e-6, tries=3, mu=p, cov=p, chol=None, logp=None, lpd=None, samples=None, jit_s=p, jit_q=p, info_s=p, info_q=p, ws=None,
             ws_bytes=0):
        return lib.dkt_posterior_f32(Ess, ssb, ssc, Eqs, qsb, qsc, Eqq, qqb, qqc, Y, ybs, sv, mean, noise, Yq, eps, B, C, N, M, S, with_noise, jitter0, tries, mu,
                                     cov, chol, logp, lpd, samples, jit_s, jit_q, info_s, info_q, ws, ws_bytes, None)

    for name in ("Ess", "Eqs", "Eqq", "Y", "sv", "mean", "noise", "jit_s", "jit_q", "info_s", "info_q"):
        assert call(**{name: None}) == -1, name
    assert call(B=0) == -1 and call(tries=-1) == -1 and call(with_noise=2) == -1
    assert call(ssb=-1) == -1 and call(qsb=-1) == -1 and call(qqb=-1) == -1 and call(ybs=-1) == -1
    assert call(ssc=7) == -1 and call(qsc=25) == -1 and call(qqc=95) == -1                # neither shared (0) nor the matrix' own size
    assert call(logp=p) == -1 and call(lpd=p) == -1                                       # no held-out targets to score
    assert call(S=3) == -1 and call(S=3, eps=p) == -1 and call(S=3, samples=p) == -1 and call(S=0, eps=p) == -1 and call(S=0, samples=p) == -1
    for kw in (dict(N=0), dict(N=128), dict(M=0), dict(M=128), dict(C=0), dict(C=33), dict(S=-1), dict(N=128, ssc=128 * 128)):
        assert call(**kw) == -5, kw
    assert call(cov=None) == -3 and call(cov=None, ws=p, ws_bytes=4 * 2 * 361 - 1) == -3  # Sigma needs a home
    assert int(lib.dkt_posterior_workspace_bytes(3, 2, 19, 0)) == 4 * 3 * 2 * 361 and int(lib.dkt_posterior_workspace_bytes(3, 2, 19, 1)) == 0
    assert int(lib.dkt_posterior_workspace_bytes(3, 2, 128, 0)) == 0 and int(lib.dkt_posterior_workspace_bytes(3, 33, 19, 0)) == 0


# ---- the Python surface ---------------------------------------------------------------------------------------------------------------------
def _cpu_args(n=4, m=3, c=2, b=1):
    return [torch.eye(n).repeat(b, 1, 1), torch.zeros(b, m, n), torch.eye(m).repeat(b, 1, 1), torch.ones(c, n), torch.ones(c), torch.zeros(c), torch.ones(c)]


def test_ops_posterior_refuses_what_it_does_not_serve_before_any_launch(monkeypatch):
    from dkt_amd import ops
    loaded = []
    monkeypatch.setattr(L, "load_post", lambda: loaded.append("load_post"))
    with pytest.raises(RuntimeError, match="HIP-only"):
        ops.posterior(*_cpu_args())
    for kw in (dict(n=128), dict(m=128), dict(c=33)):
        with pytest.raises(RuntimeError, match="dkt_posterior_f32 serves"):
            ops.posterior(*_cpu_args(**kw))
    for kw in (dict(n=0), dict(m=0)):
        with pytest.raises(RuntimeError, match="dkt_posterior_f32 serves|inconsistent shapes"):
            ops.posterior(*_cpu_args(**kw))
    for pos, bad in ((0, torch.eye(5).unsqueeze(0)), (1, torch.zeros(1, 3, 5)), (2, torch.zeros(1, 3, 4)), (3, torch.ones(2, 5)), (4, torch.ones(3)),
                     (1, torch.zeros(2, 3, 4)), (0, torch.eye(4).repeat(1, 3, 1, 1))):
        args = _cpu_args()
        args[pos] = bad
        with pytest.raises(RuntimeError, match="inconsistent shapes"):
            ops.posterior(*args)
    with pytest.raises(RuntimeError, match="inconsistent shapes"):
        ops.posterior(*_cpu_args(), yq=torch.zeros(1, 2, 4))
    with pytest.raises(RuntimeError, match="inconsistent shapes"):
        ops.posterior(*_cpu_args(), eps=torch.zeros(1, 2, 5, 4))
    assert not loaded
    assert ops.posterior_supported(127, 127, 32) and ops.posterior_supported(1, 1, 1) and ops.posterior_supported(5, 19, 1)
    assert not ops.posterior_supported(128, 5, 1) and not ops.posterior_supported(5, 128, 1) and not ops.posterior_supported(5, 5, 33)
    assert not ops.posterior_supported(0, 5, 1) and not ops.posterior_supported(5, 0, 1) and not ops.posterior_supported(5, 5, 0)


def test_model_methods_fail_loudly_on_cpu_tensors():
    from dkt_amd import backbone, dkt_regression
    model = dkt_regression.DKT(backbone.Conv3(), kernel_type="rbf")
    zs, ys, zq = torch.zeros(5, 8), torch.zeros(5), torch.zeros(19, 8)
    for call in (lambda: model.posterior(zs, ys, zq), lambda: model.sample(zs, ys, zq, 3), lambda: model.joint_log_likelihood(zs, ys, zq, torch.zeros(19))):
        with pytest.raises(RuntimeError, match="HIP-only"):
            call()


def test_cli_nll_is_off_by_default():
    from dkt_amd import io_utils
    """eval_regression.py takes test_regression.py's flags and --nll."""
    plain, ev = io_utils.parse_args_regression("test_regression", []), io_utils.parse_args_regression("eval_regression", [])
    assert ev.nll is False and {k: v for k, v in vars(ev).items() if k != "nll"} == vars(plain)
    assert io_utils.parse_args_regression("eval_regression", ["--nll", "--n_support", "7"]).nll is True
    with pytest.raises(SystemExit):
        io_utils.parse_args_regression("train_regression", ["--nll"])
    text = open(os.path.join(ROOT, "eval_regression.py")).read()
    assert "parse_args_regression('eval_regression'" in text and "joint_log_likelihood" in text
