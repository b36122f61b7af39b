"""CPU-side checks of the feature-space leave-one-out objective (docs/LOOFS.md): the feature-space closed form of tests/loo_lowrank_model.py IS the dense
definition of docs/LOO.md on E = Z Z^T; the cases of the GPU comparison cover what they claim and keep max h_i <= 0.95; the bound (4 x the float32 floor)
catches two seeded defects of the model; libdkt_loofs.so exports exactly include/dkt_abi_loofs.h (the _lib signature table too), cross-compiles without spills
or scratch, carries its header's version, answers bad arguments on the host and stands in neither loader table; the Python surface and the model route."""
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
import loo_lowrank_model as fm

L = dkt_amd._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the model -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unit", [True, False], ids=["unit", "raw"])
@pytest.mark.parametrize("n,d", [(1, 4), (7, 4), (80, 64), (130, 64)])
def test_feature_form_is_the_dense_definition(n, d, unit):
    z = fm.rows(100 * n + d, 2, n, d, unit)
    y = fm.lm.targets(3, n, 2, seed=n)
    sv, mean, noise = fm.lm.hypers(3, 0.7, 0.1)
    cw = fm.lm.class_weights("mixed", 3, n)
    a, r = fm.feature_form(z, y, sv, mean, noise, cw, jitter=1e-3), fm.dense(z, y, sv, mean, noise, cw, jitter=1e-3)
    for key, err in fm.errors(a, r, fm.VALUES + fm.GRADS).items():
        print("feature form vs dense N=%d D=%d %s: %.2e" % (n, d, key, err))
        assert err < 1e-12, key


def test_the_cases_cover_what_they_claim():
    ks, r = fm.CASES, fm.R
    assert r == L.LOOFS_ROWS
    assert {k.n for k in ks} == {1, 2, r - 1, r, r + 1, 2 * r + 1, 63, 64, 65, 127, 128, 129, 257, 420} == set(fm.NS)
    assert {k.d for k in ks} == {4, 8, 60, 64} and {k.c for k in ks} == {1, 5, 20, 32} and {k.b for k in ks} == {1, 3, 70}
    assert {k.y_per_episode for k in ks} == {False, True} and {k.cw for k in ks} == {"none", "mixed", "zeros"} and {k.unit for k in ks} == {False, True}
    assert {k.noise0 for k in ks} == {0.1, 1.0} and {k.sv0 for k in ks} == {0.3, 1.0}
    assert sorted(n for ns in fm.GROUPS.values() for n in ns) == sorted(fm.NS)
    assert all(k.b * k.c * k.n * k.n <= fm.MAX_ELEMENTS for k in ks if k.b == 70)          # (above it, 70 episodes become 3)
    assert any((k.n, k.d, k.c) == (420, 64, 20) for k in ks)


@pytest.mark.parametrize("index", range(len(fm.CASES)), ids=[repr(k) for k in fm.CASES])
def test_every_case_keeps_the_conditioning_cap(index):
    ref, _ = fm.reference(index)
    hmax = float(ref["h"].max())
    print("%r: max h %.3f" % (fm.CASES[index], hmax))
    assert hmax <= fm.H_CAP


def test_a_single_row_has_the_closed_form_h():
    z = fm.rows(3, 1, 1, 8)
    h = fm.feature_form(z, np.ones((1, 1), np.float32), [1.0], [0.0], [0.1])["h"]
    assert abs(float(h[0, 0, 0]) - 1.0 / 1.1) < 1e-6


@pytest.mark.parametrize("group", list(fm.GROUPS))
def test_the_bound_catches_the_seeded_defects(group):
    """dZ without its 2 Q z_i term, and k_i without the division by s (the float64 model otherwise untouched), land outside 4 x the float32 floor at the inputs of
    the GPU comparison, on every case of the group where they can differ: dZ is not identically zero (weights that are not all 0); some noise_c + jitter != 1."""
    floor = fm.floors(group)
    print("floors %s: %s" % (group, {k: "%.2e" % v for k, v in floor.items()}))
    hit = {"q": 0, "k": 0}
    for i, k in enumerate(fm.CASES):
        if k.group != group:
            continue
        ref, _ = fm.reference(i)
        inp = k.inputs()
        args = (inp["z"], inp["y"], inp["sv"], inp["mean"], inp["noise"], inp["cw"])
        if np.abs(ref["dz"]).max() > 0:
            err = fm.errors(fm.feature_form(*args, defect="q"), ref, ("dz",))["dz"]
            print("  %r: without 2 Q z: dz %.2e, bound %.2e" % (k, err, fm.BOUND * floor["dz"]))
            assert err > fm.BOUND * floor["dz"], k
            hit["q"] += 1
        if np.any(inp["noise"] != 1.0):
            errs = fm.errors(fm.feature_form(*args, defect="k"), ref, ("loo", "var_loo"))
            print("  %r: k without / s: loo %.2e var_loo %.2e, bounds %.2e %.2e" % (k, errs["loo"], errs["var_loo"], fm.BOUND * floor["loo"], fm.BOUND * floor["var_loo"]))
            assert errs["loo"] > fm.BOUND * floor["loo"] and errs["var_loo"] > fm.BOUND * floor["var_loo"], k
            hit["k"] += 1
    assert hit["q"] >= 3 and hit["k"] >= 3


# ---- the library ----------------------------------------------------------------------------------------------------------------------------
def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dkt_\w+)\s*\(", text)))


@pytest.fixture(scope="module")
def loofs_path():
    if not shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")) and not os.path.exists(L.LOOFS_LIB_PATH):
        pytest.skip("no hipcc and no built libdkt_loofs.so")
    return L.build_loofs()


def test_signature_table_is_the_header():
    declared = _declared("dkt_abi_loofs.h")
    assert declared == ["dkt_loofs_abi_version", "dkt_loofs_f32", "dkt_loofs_workspace_bytes"]
    assert sorted(L.LOOFS_SIGNATURES) == declared
    text = open(os.path.join(ROOT, "include", "dkt_abi_loofs.h")).read()
    for macro, value in (("DKT_LOOFS_MAX_D", L.LOOFS_MAX_D), ("DKT_LOOFS_MAX_C", L.LOOFS_MAX_C), ("DKT_LOOFS_ROWS", L.LOOFS_ROWS)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % macro, text).group(1)) == value, macro
    flat = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, (_, args) in L.LOOFS_SIGNATURES.items():
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % name, flat).group(1).strip()
        assert len(args) == (0 if proto == "void" else proto.count(",") + 1), name
    assert len(L.LOOFS_SIGNATURES["dkt_loofs_f32"][1]) == 27


def test_loofs_is_an_extension_library_of_the_table():
    spec = L.LIBS["loofs"]
    assert "dkt_loo_lowrank.hip" not in L.SOURCES and not os.path.exists(os.path.join(L.CSRC, "dkt_loo_lowrank.hip"))
    assert spec.sources == ["dkt_loo_lowrank.hip"] and spec.header == "dkt_abi_loofs.h" and spec.spill_budget and not spec.twins
    assert spec.src_dir == L.CSRC_EXT and os.path.isfile(os.path.join(spec.src_dir, "dkt_loo_lowrank.hip")) and spec.path == L.LOOFS_LIB_PATH
    assert L.loofs_abi_version_of_header() == 1 and L.abi_version_of_header() == 8 and L.loo_abi_version_of_header() == 1
    assert not [line for line in open(os.path.join(L.CSRC, "dkt_switches.def")) if "LOO" in line]          # no environment switch in the libraries' table


def test_graft_build_brings_loofs_up_to_date_inside_the_guard(monkeypatch, capsys):
    import __graft_entry__ as g
    built = []
    monkeypatch.setattr(L, "build", lambda force=False: built.append("build") or L.LIB_PATH)

    def build_lib(key):
        built.append(key)
        if key == "loofs":
            raise RuntimeError("hipcc failed on dkt_loo_lowrank.hip")

    monkeypatch.setattr(L, "build_lib", build_lib)
    monkeypatch.setattr(L, "load", lambda: type("Lib", (), {"dkt_abi_version": staticmethod(L.abi_version_of_header)}))
    g.build()                                                    # a failed build of the extension warns and does not stop the product build
    assert [k for k in built if k in ("build", "loo", "post", "loofs", "diag", "twins")] == ["build", "loo", "post", "loofs", "diag", "twins"]
    assert sorted(built[1:]) == sorted(k for k in L.LIBS if k != "hip" and k not in L.BUILT_WITH_PRODUCT)          # the rest of the table: build() has done its own
    assert "libdkt_loofs.so not built" in capsys.readouterr().err


def test_library_exports_exactly_its_header_and_its_version(loofs_path):
    out = subprocess.run(["nm", "-D", "--defined-only", loofs_path], capture_output=True, text=True, check=True).stdout
    exports = sorted({line.split()[-1] for line in out.splitlines() if line.split()[-1].startswith("dkt_")})
    assert exports == _declared("dkt_abi_loofs.h")
    assert L.device_code_objects(loofs_path), "no gfx950 code object in the library"
    assert int(L.load_loofs().dkt_loofs_abi_version()) == L.loofs_abi_version_of_header() == 1


def test_library_does_not_spill(loofs_path):
    usage = json.load(open(os.path.join(L.OBJ_DIR, "libdkt_loofs.so.resource_usage.json")))
    assert 1 <= len(usage) <= 4 and all("loofs_kernel" in k for k in usage)
    assert all(u.get("vgpr_spill", 0) == 0 and u.get("scratch", 0) == 0 for u in usage.values())
    assert L.check_resources(usage) == []


def test_bad_arguments_are_answered_on_the_host(loofs_path):
    """DKT_ERR_BAD_ARG (-1), DKT_ERR_WORKSPACE (-3) and DKT_ERR_SHAPE (-5) come back before any launch: the pointers below are never dereferenced."""
    lib = L.load_loofs()
    p = ctypes.c_void_p(4096)

    def call(Z=p, Y=p, ybs=0, sv=p, mean=p, noise=p, cw=None, B=1, C=2, N=5, D=8, jitter0=1e-6, tries=3, flags=0, loo=p, alpha=p, mu=p, var=p,
             dZ=None, dsv=None, dmean=None, dnoise=None, jit=p, info=p, ws=p, ws_bytes=1 << 20):
        return lib.dkt_loofs_f32(Z, Y, ybs, sv, mean, noise, cw, B, C, N, D, jitter0, tries, flags, loo, alpha, mu, var, dZ, dsv, dmean, dnoise, jit, info,
                                 ws, ws_bytes, None)

    for name in ("Z", "Y", "sv", "mean", "noise", "loo", "alpha", "mu", "var", "jit", "info"):
        assert call(**{name: None}) == -1, name
    assert call(B=0) == -1 and call(tries=-1) == -1 and call(flags=2) == -1 and call(ybs=-1) == -1 and call(ybs=9) == -1          # (9 < C N)
    assert call(Z=ctypes.c_void_p(4100)) == -1                                # rows that are not 16-byte aligned
    for name in ("dZ", "dsv", "dmean", "dnoise"):                             # the gradient is asked for and one of its outputs is missing
        grads = dict(dZ=p, dsv=p, dmean=p, dnoise=p)
        grads[name] = None
        assert call(flags=1, **grads) == -1, name
    assert call(N=0) == -5 and call(D=0) == -5 and call(D=68) == -5 and call(D=6) == -5 and call(C=33) == -5 and call(C=0) == -5
    assert call(ws=None) == -3 and call(ws_bytes=64 * 64 * 4 - 1) == -3
    assert int(lib.dkt_loofs_workspace_bytes(3, 20, 420, 64)) == 3 * 64 * 64 * 4 and int(lib.dkt_loofs_workspace_bytes(3, 20, 420, 66)) == 0


# ---- the Python surface ---------------------------------------------------------------------------------------------------------------------
def test_route_query(monkeypatch):
    from dkt_amd import ops
    monkeypatch.delenv("DKT_LOO_LOWRANK", raising=False)
    assert ops.loo_lowrank_supported(1, 4, 1) and ops.loo_lowrank_supported(100000, 64, 32)
    assert not ops.loo_lowrank_supported(0, 64, 5) and not ops.loo_lowrank_supported(420, 128, 5) and not ops.loo_lowrank_supported(420, 62, 5)
    assert not ops.loo_lowrank_supported(420, 64, 33) and not ops.loo_lowrank_supported(420, 0, 5)
    assert ops.loo_lowrank_applies(129, 64, 20) and ops.loo_lowrank_applies(420, 64, 20) and not ops.loo_lowrank_applies(128, 64, 20)
    assert not ops.loo_lowrank_applies(105, 64, 5) and not ops.loo_lowrank_applies(420, 64, 20, on_gpu=False) and not ops.loo_lowrank_applies(420, 128, 20)
    monkeypatch.setenv("DKT_LOO_LOWRANK", "0")
    assert not ops.loo_lowrank_applies(420, 64, 20) and not ops.loo_lowrank_applies(129, 64, 20)
    monkeypatch.setenv("DKT_LOO_LOWRANK", "force")
    assert ops.loo_lowrank_applies(105, 64, 5) and ops.loo_lowrank_applies(128, 64, 5) and ops.loo_lowrank_applies(1, 4, 1)
    assert not ops.loo_lowrank_applies(105, 128, 5) and not ops.loo_lowrank_applies(105, 64, 5, on_gpu=False)
    assert ops._FeatureSpaceLooCV.on_features and not ops._FeatureSpaceLooCV.resident_only and ops._FeatureSpaceLooCV.de is None
    assert issubclass(ops._FeatureSpaceLooCV, ops._LooCV) and ops._LooCV.resident_only and not ops._LooCV.on_features and not ops.loo_supported(128, 5)


def test_ops_loo_lowrank_fails_loudly_on_cpu_tensors(monkeypatch):
    from dkt_amd import ops
    monkeypatch.delenv("DKT_LOO_LOWRANK", raising=False)
    with pytest.raises(RuntimeError, match="HIP-only"):
        ops.loo_lowrank(torch.zeros(1, 130, 8), torch.ones(2, 130), torch.ones(2), torch.zeros(2), torch.ones(2))
    with pytest.raises(RuntimeError, match="HIP-only"):
        ops.episode_loss_loo(torch.zeros(1, 130, 8), torch.ones(2, 130), torch.ones(2), torch.zeros(2), torch.ones(2), torch.ones(2), "linear")
    with pytest.raises(RuntimeError, match="HIP-only"):
        ops.episode_loss_loo_bn(torch.zeros(1, 130, 8), None, None, torch.ones(2, 130), torch.ones(2), torch.zeros(2), torch.ones(2), torch.ones(2), use_bn=False)


class _OnGpu:
    """The shape and the device of rows that do not exist yet, for the route query"""
    is_cuda = True

    def __init__(self, *shape):
        self.shape = shape


def test_the_model_states_the_route_once(monkeypatch):
    from dkt_amd import backbone, dkt
    monkeypatch.delenv("DKT_LOO_LOWRANK", raising=False)
    make = lambda kernel: dkt.DKT(lambda: backbone.Conv4S(), 20, 5, kernel_type=kernel, objective="loo")      # noqa: E731
    m = make("bncossim")
    assert m._loo_in_feature_space(_OnGpu(420, 64), 20) and m._loo_in_feature_space(_OnGpu(1, 400, 64), 20)
    assert m._loo_in_feature_space(_OnGpu(5, 5), 20, shape=(420, 64))
    assert not m._loo_in_feature_space(_OnGpu(105, 64), 5) and not m._loo_in_feature_space(_OnGpu(127, 64), 20)
    for kernel in ("cossim", "linear"):
        assert make(kernel)._loo_in_feature_space(_OnGpu(420, 64), 20)
    with pytest.raises(ValueError, match="up to 127 rows.*feature space.*64 features"):
        make("rbf")._loo_in_feature_space(_OnGpu(420, 64), 20)
    with pytest.raises(ValueError, match="up to 127 rows.*feature space.*64 features"):
        m._loo_in_feature_space(_OnGpu(420, 128), 20)
    with pytest.raises(ValueError, match="up to 127 rows"):                   # the wart: exactly 128 rows has no route (docs/LOOFS.md)
        m._loo_in_feature_space(_OnGpu(128, 64), 8)
    with pytest.raises(ValueError, match="up to 32 classes"):
        m._loo_in_feature_space(_OnGpu(420, 64), 33)
    with pytest.raises(ValueError, match="up to 127 rows"):
        dkt.check_loo_rows(128, 5)
