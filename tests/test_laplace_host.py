"""CPU-side checks of the Laplace GP classifier: the numpy restatement (tests/laplace_model.py) in float64 IS scikit-learn's classifier
(probabilities to 1e-12, labels, the all-classes-tie and the two-class conventions); libdkt_gpc.so exports exactly include/dkt_abi_gpc.h (the _lib
signature table too), cross-compiles without spills and carries its header's version."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from sklearn.gaussian_process import GaussianProcessClassifier
from sklearn.gaussian_process.kernels import RBF

import dkt_amd
import laplace_model as lm

L = dkt_amd._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fit(zs, c, shots, ls):
    return GaussianProcessClassifier(1.0 * RBF(ls), optimizer=None).fit(zs, np.repeat(np.arange(max(c, 2)), shots))


def _model(zs, zq, c, shots, ls):
    md = lm.mode(lm.rbf(zs, zs, ls)[None], lm.one_vs_rest(c, shots))
    return md, lm.predict(lm.rbf(zq, zs, ls)[None], np.ones((1, len(zq))), md)


@pytest.mark.parametrize("case", lm.CASES + [lm.NEAR_IDENTITY_CASE], ids=str)
def test_float64_restatement_is_sklearn(case):
    _, c, n, m, _, _, ls = case
    d = lm.build_case(case)
    zs, zq = d["zs"][0], d["zq"][0]
    gp = _fit(zs, c, n // c, ls)
    md, (mu, var, prob, labels) = _model(zs, zq, c, n // c, ls)
    sk = np.stack([e.predict_proba(zq)[:, 1] for e in gp.base_estimator_.estimators_])
    assert np.abs(sk - prob[0]).max() < 1e-12
    assert np.abs(np.array([e.log_marginal_likelihood_value_ for e in gp.base_estimator_.estimators_]) - md["lml"][0]).max() < 1e-10
    assert (gp.predict(zq) == labels[0]).all()
    assert np.abs(gp.predict_proba(zq) - prob[0].T / prob[0].sum(0)[:, None]).max() < 1e-12
    assert (md["iters"] < 100).all()


def test_far_queries_tie_and_the_last_class_wins():
    d = lm.build_case(lm.CASES[1])
    zs, far = d["zs"][0], np.full((3, 64), 30.0)
    _, (mu, var, prob, labels) = _model(zs, far, 5, 5, 0.1)
    assert (mu == 0).all() and (var == 1).all() and (prob == prob[0, 0, 0]).all()
    assert (labels == 4).all() and (_fit(zs, 5, 5, 0.1).predict(far) == 4).all()
    assert np.allclose(_fit(zs, 5, 5, 0.1).predict_proba(far), 0.2, atol=1e-12)


def test_two_classes_are_one_binary_problem():
    rng = np.random.default_rng(5)
    zs, zq = lm.clustered(rng, 2, 5, 40, 64, 0.1)
    gp = _fit(zs, 2, 5, 0.1)
    md, (mu, var, prob, labels) = _model(zs, zq, 1, 5, 0.1)
    assert md["g"].shape == (1, 1, 10)
    assert np.abs(gp.predict_proba(zq)[:, 1] - prob[0, 0]).max() < 1e-12
    assert (gp.predict(zq) == labels[0]).all() and set(labels[0]) == {0, 1}
    far = np.full((2, 64), 30.0)
    assert (lm.predict(lm.rbf(far, zs, 0.1)[None], np.ones((1, 2)), md)[3] == 0).all() and (gp.predict(far) == 0).all()      # mu == 0 is not > 0


def test_float32_model_keeps_fp32_but_sums_the_mixture_in_double():
    d = lm.build_case(lm.CASES[1])
    md = lm.mode(d["k"], d["y"], dtype=np.float32)
    mu, var, prob, _ = lm.predict(d["ks"], d["kss"], md, dtype=np.float32)
    assert all(md[k].dtype == np.float32 for k in ("f", "g", "w_sr", "chol", "lml")) and mu.dtype == var.dtype == prob.dtype == np.float32
    p64 = lm.predict(d["ks"], d["kss"], lm.mode(d["k"], d["y"]))[2]
    assert np.abs(prob - p64).max() < 1e-6          # (an all-fp32 mixture sum is off by 1e-4)


# ---- the library ----------------------------------------------------------------------------------------------------------------------------
def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dkt_\w+)\s*\(", text)))


@pytest.fixture(scope="module")
def gpc_path():
    if not shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")) and not os.path.exists(L.GPC_LIB_PATH):
        pytest.skip("no hipcc and no built libdkt_gpc.so")
    return L.build_gpc()


def test_signature_table_is_the_header():
    declared = _declared("dkt_abi_gpc.h")
    assert declared == ["dkt_gpc_abi_version", "dkt_gpc_mode_f32", "dkt_gpc_predict_f32"]
    assert sorted(L.GPC_SIGNATURES) == declared
    text = open(os.path.join(ROOT, "include", "dkt_abi_gpc.h")).read()
    assert int(re.search(r"#define\s+DKT_GPC_MAX_N\s+(\d+)", text).group(1)) == L.GPC_MAX_N == 127
    assert int(re.search(r"#define\s+DKT_GPC_MAX_C\s+(\d+)", text).group(1)) == L.GPC_MAX_C == 32
    # the argument counts of the prototypes
    flat = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, (_, args) in L.GPC_SIGNATURES.items():
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % name, flat).group(1).strip()
        assert len(args) == (0 if proto == "void" else proto.count(",") + 1), name


def test_gpc_is_a_product_library_of_the_table():
    spec = L.LIBS["gpc"]
    assert spec.sources == ["dkt_gpc.hip"] and spec.header == "dkt_abi_gpc.h" and spec.spill_budget and not spec.twins
    assert spec.src_dir is None and not spec.best_effort and "dkt_gpc.hip" not in L.SOURCES and L.abi_version_of_header() == 8      # it adds nothing to the product ABI
    assert "libdkt_gpc.so" in L.__doc__


def test_build_brings_gpc_up_to_date(monkeypatch):
    built = []
    monkeypatch.setattr(L, "needs_build", lambda: False)
    monkeypatch.setattr(L, "_build_if_stale", lambda spec, verbose=False: built.append(os.path.basename(spec.path)))
    L.build()
    assert built == ["libdkt_x16.so", "libdkt_data.so", "libdkt_smk.so", "libdkt_gpc.so"]


def test_library_exports_exactly_its_header_and_its_version(gpc_path):
    out = subprocess.run(["nm", "-D", "--defined-only", gpc_path], capture_output=True, text=True, check=True).stdout
    exports = sorted({line.split()[-1] for line in out.splitlines() if line.split()[-1].startswith("dkt_")})
    assert exports == _declared("dkt_abi_gpc.h")
    # the version the library reports, read from its code without loading it: `mov $imm32, %eax; ret` behind the symbol
    dis = subprocess.run(["objdump", "-d", "--no-show-raw-insn", "--disassemble=dkt_gpc_abi_version", gpc_path], capture_output=True, text=True,
                         check=True).stdout
    assert int(re.search(r"mov\s+\$0x([0-9a-f]+),%eax", dis).group(1), 16) == L.gpc_abi_version_of_header() == 1


def test_library_does_not_spill(gpc_path):
    usage = json.load(open(os.path.join(L.OBJ_DIR, "libdkt_gpc.so.resource_usage.json")))
    assert len(usage) == 3 and any("gpc_predict_kernel" in k for k in usage)          # mode at 64 and 256 threads, predict
    assert all(u.get("vgpr_spill", 0) == 0 and u.get("scratch", 0) == 0 for u in usage.values())
    assert L.check_resources(usage) == []
