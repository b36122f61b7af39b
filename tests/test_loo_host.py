"""CPU-side checks of the leave-one-out objective (docs/LOO.md): the closed form of tests/loo_model.py IS the definition (N refits, each leaving one row out),
values and gradients; the bound of the GPU comparison (4 x the float32 floor) catches a seeded defect of the model; libdkt_loo.so exports exactly
include/dkt_abi_loo.h (the _lib signature table too), cross-compiles without spills or scratch, carries its header's version, answers bad arguments on the
host, and stands beside the loader's table of seven, not in it; the Python surface refuses what it does not serve."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import dkt_amd
import loo_model as lm

L = dkt_amd._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the model -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_class", [False, True], ids=["shared", "perclass"])
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("n", [2, 5, 19])
def test_closed_form_is_n_explicit_refits(n, c, per_class):
    z = lm.unit_rows(100 * n + c, 2, n, 8)
    e = lm.base_matrix(z, "rbf", c if per_class else None)
    y = lm.targets(c, n, 2, seed=n)
    sv, mean, noise = lm.hypers(c, 0.7, 0.3)
    cw = lm.class_weights("mixed", c, n)
    a, r = lm.closed_form(e, y, sv, mean, noise, cw), lm.refits(e, y, sv, mean, noise, cw)
    for key in ("loo", "mu_loo", "var_loo", "w", "dsv", "dmean", "dnoise"):
        err = np.abs(a[key] - r[key]).max()
        print("closed form vs refits N=%d C=%d %s: %.2e" % (n, c, key, err))
        assert err < 1e-11 * max(1.0, np.abs(r[key]).max()), key
    assert np.abs(a["w"] - np.swapaxes(a["w"], -1, -2)).max() < 1e-14 * max(1.0, np.abs(a["w"]).max())


def test_the_cases_cover_what_they_claim():
    ks = lm.CASES
    assert {k.n for k in ks} == set(lm.NS) and {k.c for k in ks} == {1, 5, 32} and {k.b for k in ks} == {1, 3, 70}
    assert {k.per_class for k in ks} == {False, True} and {k.y_per_episode for k in ks} == {False, True} and {k.cw for k in ks} == {"none", "mixed", "zeros"}
    assert {k.d for k in ks} == {8, 64} and {k.kernel for k in ks} == {"rbf", "linear"} and {k.noise0 for k in ks} == {0.1, 1.0} and {k.sv0 for k in ks} == {0.3, 1.0}
    assert sorted(n for ns in lm.GROUPS.values() for n in ns) == sorted(lm.NS)
    for g in lm.GROUPS:          # every group meets both layouts and a batch with a ragged tail
        mine = [k for k in ks if k.group == g]
        assert {k.per_class for k in mine} == {False, True} and any(k.b == 70 for k in mine), g


@pytest.mark.parametrize("group", list(lm.GROUPS))
def test_the_bound_catches_a_seeded_defect(group):
    """G without its alpha r^T term (the float64 model otherwise untouched) lands outside 4 x the float32 floor on W, at the inputs of the GPU comparison: on
    every case of the group whose W is not identically zero (a single class of weight 0)."""
    floor = lm.floors(group)
    print("floors %s: %s" % (group, {k: "%.2e" % v for k, v in floor.items()}))
    hit = 0
    for i, k in enumerate(lm.CASES):
        if k.group != group:
            continue
        ref, _ = lm.reference(i)
        if not np.abs(ref["w"]).max() > 0:
            continue
        inp = k.inputs()
        bad = lm.closed_form(inp["e"], inp["y"], inp["sv"], inp["mean"], inp["noise"], inp["cw"], defect=True)
        err = lm.errors(bad, ref, ("w",))["w"]
        print("  %r: defect %.2e, bound %.2e" % (k, err, lm.BOUND * floor["w"]))
        assert err > lm.BOUND * floor["w"], k
        hit += 1
    assert hit >= 3


# ---- the library ----------------------------------------------------------------------------------------------------------------------------
def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dkt_\w+)\s*\(", text)))


@pytest.fixture(scope="module")
def loo_path():
    if not shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")) and not os.path.exists(L.LOO_LIB_PATH):
        pytest.skip("no hipcc and no built libdkt_loo.so")
    return L.build_loo()


def test_signature_table_is_the_header():
    declared = _declared("dkt_abi_loo.h")
    assert declared == ["dkt_loo_abi_version", "dkt_loo_f32"]
    assert sorted(L.LOO_SIGNATURES) == declared
    text = open(os.path.join(ROOT, "include", "dkt_abi_loo.h")).read()
    assert int(re.search(r"#define\s+DKT_LOO_MAX_N\s+(\d+)", text).group(1)) == L.LOO_MAX_N == 127
    assert int(re.search(r"#define\s+DKT_LOO_MAX_C\s+(\d+)", text).group(1)) == L.LOO_MAX_C == 32
    flat = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, (_, args) in L.LOO_SIGNATURES.items():
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % name, flat).group(1).strip()
        assert len(args) == (0 if proto == "void" else proto.count(",") + 1), name
    assert len(L.LOO_SIGNATURES["dkt_loo_f32"][1]) == 26


def test_loo_is_an_extension_library_of_the_table():
    spec = L.LIBS["loo"]
    assert spec.sources == ["dkt_loo.hip"] and spec.header == "dkt_abi_loo.h" and spec.spill_budget and not spec.twins
    assert spec.src_dir == L.CSRC_EXT and os.path.isfile(os.path.join(spec.src_dir, "dkt_loo.hip")) and spec.path == L.LOO_LIB_PATH
    assert not os.path.exists(os.path.join(L.CSRC, "dkt_loo.hip")) and "dkt_loo.hip" not in L.SOURCES and not spec.best_effort
    assert L.loo_abi_version_of_header() == 1 and L.abi_version_of_header() == 8
    assert not [line for line in open(os.path.join(L.CSRC, "dkt_switches.def")) if "LOO" in line]          # no environment switch of its own


def test_graft_build_brings_loo_up_to_date(monkeypatch):
    import __graft_entry__ as g
    built = []
    monkeypatch.setattr(L, "build", lambda force=False: built.append("build") or L.LIB_PATH)

    def build_lib(key):
        built.append(key)
        if key == "loo":
            raise RuntimeError("hipcc failed on dkt_loo.hip")

    monkeypatch.setattr(L, "build_lib", build_lib)
    monkeypatch.setattr(L, "load", lambda: type("Lib", (), {"dkt_abi_version": staticmethod(L.abi_version_of_header)}))
    with pytest.raises(RuntimeError, match="dkt_loo.hip"):      # product code: a failed build of it stops build()
        g.build()
    assert built[0] == "build" and built[-1] == "loo" and not [k for k in built[1:] if L.LIBS[k].best_effort]


def test_library_exports_exactly_its_header_and_its_version(loo_path):
    out = subprocess.run(["nm", "-D", "--defined-only", loo_path], capture_output=True, text=True, check=True).stdout
    exports = sorted({line.split()[-1] for line in out.splitlines() if line.split()[-1].startswith("dkt_")})
    assert exports == _declared("dkt_abi_loo.h")
    assert L.device_code_objects(loo_path), "no gfx950 code object in the library"
    assert int(L.load_loo().dkt_loo_abi_version()) == L.loo_abi_version_of_header() == 1


def test_library_does_not_spill(loo_path):
    usage = json.load(open(os.path.join(L.OBJ_DIR, "libdkt_loo.so.resource_usage.json")))
    assert 1 <= len(usage) <= 4 and all("loo_kernel" in k for k in usage)          # a handful of instances at the most
    assert all(u.get("vgpr_spill", 0) == 0 and u.get("scratch", 0) == 0 for u in usage.values())
    assert L.check_resources(usage) == []


def test_bad_arguments_are_answered_on_the_host(loo_path):
    """DKT_ERR_BAD_ARG (-1) and DKT_ERR_SHAPE (-5) come back before any launch: the pointers below are never dereferenced (this machine needs no GPU)."""
    lib = L.load_loo()
    p = ctypes.c_void_p(4096)

    def call(E=p, ebs=25, ecs=0, Y=p, ybs=0, sv=p, mean=p, noise=p, cw=None, B=1, C=2, N=5, jitter0=1e-6, tries=3, flags=0, loo=p, alpha=p, mu=p, var=p,
             W=None, dsv=None, dmean=None, dnoise=None, jit=p, info=p):
        return lib.dkt_loo_f32(E, ebs, ecs, Y, ybs, sv, mean, noise, cw, B, C, N, jitter0, tries, flags, loo, alpha, mu, var, W, dsv, dmean, dnoise, jit, info, None)

    for name in ("E", "Y", "sv", "mean", "noise", "loo", "alpha", "mu", "var", "jit", "info"):
        assert call(**{name: None}) == -1, name
    assert call(B=0) == -1 and call(tries=-1) == -1 and call(flags=2) == -1 and call(ebs=-1) == -1 and call(ybs=-1) == -1
    assert call(ecs=7) == -1                                                   # neither shared (0) nor per class (N * N)
    for name in ("W", "dsv", "dmean", "dnoise"):                              # the gradient is asked for and one of its outputs is missing
        grads = dict(W=p, dsv=p, dmean=p, dnoise=p)
        grads[name] = None
        assert call(flags=1, **grads) == -1, name
    assert call(N=128, ebs=128 * 128) == -5 and call(N=0) == -5 and call(C=33) == -5 and call(C=0) == -5
    assert call(N=128, ebs=128 * 128, ecs=128 * 128) == -5


# ---- the Python surface ---------------------------------------------------------------------------------------------------------------------
def test_ops_loo_fails_loudly_on_cpu_tensors():
    from dkt_amd import ops
    args = (torch.eye(4).unsqueeze(0), torch.ones(2, 4), torch.ones(2), torch.zeros(2), torch.ones(2))
    with pytest.raises(RuntimeError, match="HIP-only"):
        ops.loo(*args)
    with pytest.raises(RuntimeError, match="HIP-only"):
        ops.loo_objective(*args, torch.ones(2))
    with pytest.raises(RuntimeError, match="HIP-only"):
        ops.episode_loss_loo(torch.zeros(1, 4, 8), torch.ones(2, 4), torch.ones(2), torch.zeros(2), torch.ones(2), torch.ones(2), "linear")
    assert ops.loo_supported(127, 32) and ops.loo_supported(1, 1)
    assert not ops.loo_supported(128, 5) and not ops.loo_supported(5, 33) and not ops.loo_supported(0, 1)
    assert ops._LooCV.resident_only and not ops._LooCV.on_features


def test_objective_loo_is_for_the_gaussian_likelihood():
    from dkt_amd import backbone, dkt, dkt_regression
    make = lambda **kw: dkt.DKT(lambda: backbone.Conv4S(), 5, 1, kernel_type="linear", **kw)      # noqa: E731
    for likelihood in ("dirichlet", "bernoulli"):
        with pytest.raises(ValueError, match="objective='loo'"):
            make(objective="loo", likelihood=likelihood)
    with pytest.raises(ValueError, match="objective must be"):
        make(objective="cv")
    assert make().objective_type == "mll" and make(objective="loo").objective_type == "loo"
    with pytest.raises(ValueError, match="up to 127 rows"):
        dkt.check_loo_rows(128, 5)
    assert dkt_regression.DKT(backbone.Conv3(), kernel_type="rbf").objective_type == "mll"
    assert dkt_regression.DKT(backbone.Conv3(), kernel_type="rbf", objective="loo").objective_type == "loo"


def test_cli_default_is_the_marginal_likelihood(monkeypatch):
    from dkt_amd import configs, io_utils
    monkeypatch.setattr(configs, "objective", None)
    monkeypatch.setattr(configs, "amp", None)
    monkeypatch.setattr(configs, "likelihood", None)
    for script in ("train", "test"):
        assert io_utils.parse_args(script, []).objective == "mll" and configs.objective is None
        assert io_utils.parse_args(script, ["--objective", "loo"]).objective == "loo" and configs.objective == "loo"
        with pytest.raises(SystemExit):
            io_utils.parse_args(script, ["--objective", "cv"])
    args = io_utils.parse_args("train", ["--objective", "loo"])
    assert io_utils.checkpoint_dir_for(args, "s").endswith("_loo")
    assert not io_utils.checkpoint_dir_for(io_utils.parse_args("train", []), "s").endswith("_loo")
