"""CPU-side checks of the Dirichlet likelihood in feature space (docs/DIRICHLET.md "Above 127 rows"): the float64 restatement of the three
dkt_rownoise_lowrank_* calls (tests/dirichlet_lowrank_model.py) against the N x N float64 formulas of tests/dirichlet_model.py, the float32 floors and the
label margins the GPU tests rely on, the new symbols of the product ABI (still version 7, still at most 250 kernels, no spill), the argument checks that
come before any launch, and the route selection without a GPU."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import dirichlet_lowrank_model as lm
import dirichlet_model as dm
import dkt_amd

L = dkt_amd._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dkt_rownoise_lowrank_state_bytes", "dkt_rownoise_lowrank_f32", "dkt_rownoise_lowrank_bwd_f32", "dkt_rownoise_lowrank_predict_f32")


def test_float64_restatement_equals_the_n_by_n_reference():
    f = lm.all_floors()
    for names, cs, ref, r64 in ((lm.QUANTITIES, f["cases"], f["ref"], f["r64"]), (lm.PREDICT_QUANTITIES, f["pcases"], f["pref"], f["p64"])):
        for key in cs:
            err = {q: float(np.abs(r64[key][q] - ref[key][q]).max()) for q in names}
            print(key, {q: "%.2g" % v for q, v in err.items()})
            assert max(err.values()) < 1e-10, (key, err)
    # Z^T alpha = t: what makes the D x D model a posterior of the N x N one
    d, o = f["cases"][("20-way",)], f["r64"][("20-way",)]
    assert np.abs(np.einsum("bnd,bcn->bcd", d["z"], f["ref"][("20-way",)]["alpha"]) - o["t"]).max() < 1e-11


def test_float32_floors_and_label_margins_of_the_gpu_cases():
    """e32 per quantity over the case lists (docs/DIRICHLET.md tables them) and the float64 top-two margins of mu of the label case against 100 x e32(mu):
    no query is left out of any label comparison."""
    f = lm.all_floors()
    print("e32:", {q: "%.3g" % v for q, v in {**f["e32"], **f["p32"]}.items()})
    assert all(0 < v < np.inf for v in f["e32"].values()) and all(0 < v < np.inf for v in f["p32"].values())
    assert set(f["e32"]) == set(lm.QUANTITIES) and set(f["p32"]) == set(lm.PREDICT_QUANTITIES)
    smallest = min(float(dm.top_two_margin(f["pref"][k]["mu"]).min()) for k in f["pcases"])
    print("e32(mu) %.3g, smallest float64 top-two margin %.3g (%.0f x e32)" % (f["p32"]["mu"], smallest, smallest / f["p32"]["mu"]))
    assert smallest >= 100 * f["p32"]["mu"]
    for k in f["pcases"]:                                      # the labels of the float32 run are those of the reference
        assert (f["p64"][k]["labels"] == f["pref"][k]["mu"].argmax(1)).all()
        assert (lm.solve_predict(f["pcases"][k], np.float32)["labels"] == f["pref"][k]["mu"].argmax(1)).all()
    # the case list is the one the issue sets: the shapes, 420 rows x 20 classes with sv alternating, per-episode targets, random noise on rows that are not unit
    assert f["cases"][("20-way",)]["z"].shape == (2, 420, 64) and f["cases"][("20-way",)]["sv"][:2].tolist() == [0.5, 5.0]
    assert f["cases"][("batched-y",)]["y"].ndim == 3
    rn = f["cases"][("random-noise",)]
    norms = np.linalg.norm(rn["z"], axis=-1)
    assert rn["nr"].min() >= 0.3 and rn["nr"].max() <= 5.0 and len(np.unique(rn["nr"])) > 100 and norms.min() < 0.5 and norms.max() > 2.0


def test_new_symbols_are_in_the_header_the_table_and_the_library(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dkt_abi.h")).read(), flags=re.S)
    for name in NEW:
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1)
        assert name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == proto.count(",") + 1 and hasattr(lib, name)
    assert L.SOURCES[-2:] == ["dkt_mll_rownoise.hip", "dkt_laplace_grad.hip"] and L.LIBS["hip"].sources is L.SOURCES and L.LIBS["hip"].src_dir is None
    assert lib.dkt_abi_version() == 8 and L.abi_version_of_header() == 8
    per = dkt_amd.ops.ROWNOISE_LOWRANK_STATE * 4
    assert lib.dkt_rownoise_lowrank_state_bytes(2, 20) == 2 * 20 * per and lib.dkt_rownoise_lowrank_state_bytes(0, 5) == 0
    assert lib.dkt_rownoise_lowrank_state_bytes(1, 1) == per == 64 * 65 * 4 and lib.dkt_rownoise_lowrank_state_bytes(3, -1) == 0


def test_argument_checks_come_before_any_launch(lib):
    """NULL pointers: DKT_ERR_BAD_ARG, before the shape test; D = 68, D = 6, C = 33: DKT_ERR_SHAPE; a short state: DKT_ERR_WORKSPACE.  Host memory stands in
    for the operands: none of these calls reaches a launch."""
    buf = np.zeros(64 * 65 * 33 + 16, np.float32)
    p = ctypes.c_void_p(buf.ctypes.data + (-buf.ctypes.data) % 16)
    nbytes = lambda c: lib.dkt_rownoise_lowrank_state_bytes(1, c)

    def fwd(c=5, n=130, d=64, null=(), state_bytes=None):
        a = [None if i in null else p for i in range(11)]      # Z Y nr sv mean cw logp alpha info dsv dmean
        return lib.dkt_rownoise_lowrank_f32(a[0], a[1], 0, a[2], 0, a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], None if "state" in null else p,
                                            nbytes(c) if state_bytes is None else state_bytes, 1, c, n, d, None)

    def bwd(c=5, n=130, d=64, null=(), state_bytes=None):
        a = [None if i in null else p for i in range(9)]       # Z Y nr sv mean cw state gobj dZ
        return lib.dkt_rownoise_lowrank_bwd_f32(a[0], a[1], 0, a[2], 0, a[3], a[4], a[5], a[6], nbytes(c) if state_bytes is None else state_bytes, a[7], a[8],
                                                1, c, n, d, None)

    def pred(c=5, m=10, d=64, null=(), state_bytes=None):
        a = [None if i in null else p for i in range(7)]       # Zq state sv mean mu var labels
        return lib.dkt_rownoise_lowrank_predict_f32(a[0], a[1], nbytes(c) if state_bytes is None else state_bytes, a[2], a[3], a[4], a[5], a[6], 1, c, m, d, None)

    for i in (0, 1, 2, 3, 4, 6, 7, 8, "state"):                # (cls_weight, dsv, dmean may be NULL)
        assert fwd(null=(i,)) == -1 and fwd(c=33, d=68, null=(i,)) == -1, i
    for i in (0, 1, 2, 3, 4, 6, 7, 8):
        assert bwd(null=(i,)) == -1 and bwd(c=33, d=68, null=(i,)) == -1, i
    for i in (0, 1, 2, 3, 4, 5):                               # (labels may be NULL)
        assert pred(null=(i,)) == -1 and pred(c=33, d=68, null=(i,)) == -1, i
    for call in (fwd, bwd, pred):
        assert call(d=68) == -5 and call(d=6) == -5 and call(c=33) == -5 and call(d=0) == -1 and call(c=0) == -1
        assert call(state_bytes=nbytes(5) - 4) == -3
    assert fwd(n=0) == -1 and bwd(n=0) == -1 and pred(m=0) == -1
    odd = ctypes.c_void_p(p.value + 4)                         # Z has to be 16-byte aligned (rows are read four features at a time)
    assert lib.dkt_rownoise_lowrank_predict_f32(odd, p, nbytes(5), p, p, p, p, p, 1, 5, 10, 64, None) == -1


def test_kernel_count_and_resources(lib):
    usage = json.load(open(os.path.join(L.OBJ_DIR, "libdkt_hip.so.resource_usage.json")))
    mine = {k: u for k, u in usage.items() if "rownoise_kernel" in k or "dirichlet_proba_kernel" in k}
    assert len(usage) <= 250 and len(mine) == 2 and len([k for k in usage if "dkt_mll_rownoise" in k or "lowrank_forward" in k]) == 0
    for k, u in mine.items():                                  # the new code is passes 1 to 3 of dirichlet_proba_kernel
        print(k, u)
        assert u["vgpr_spill"] == 0 and u["sgpr_spill"] == 0 and u["scratch"] == 0
    assert L.check_resources(usage) == []


def test_route_selection_without_a_gpu(monkeypatch):
    ops = dkt_amd.ops
    monkeypatch.delenv("DKT_DIRICHLET_LOWRANK", raising=False)
    assert ops.rownoise_lowrank_supported(420, 64, 20) and ops.rownoise_lowrank_supported(1, 4, 1) and ops.rownoise_lowrank_supported(10 ** 6, 60, 32)
    assert not ops.rownoise_lowrank_supported(420, 68, 20) and not ops.rownoise_lowrank_supported(420, 6, 20) and not ops.rownoise_lowrank_supported(420, 64, 33)
    assert ops.rownoise_lowrank_applies(128, 64, 5) and not ops.rownoise_lowrank_applies(127, 64, 5) and not ops.rownoise_lowrank_applies(420, 64, 20, on_gpu=False)
    monkeypatch.setenv("DKT_DIRICHLET_LOWRANK", "force")
    assert ops.rownoise_lowrank_applies(25, 64, 5) and not ops.rownoise_lowrank_applies(25, 68, 5) and not ops.rownoise_lowrank_applies(25, 64, 5, on_gpu=False)
    monkeypatch.setenv("DKT_DIRICHLET_LOWRANK", "0")
    assert not ops.rownoise_lowrank_applies(420, 64, 20)
    monkeypatch.delenv("DKT_DIRICHLET_LOWRANK")
    assert ops._FeatureSpaceDirichlet.on_features is True and ops._FeatureSpaceDirichlet.resident_only is False
    assert ops._FeatureSpaceDirichlet.backward is ops._Dirichlet.backward and ops._Dirichlet.on_features is False
    m = dkt_amd.DKT(dkt_amd.backbone.Conv4S, n_way=20, n_support=5, likelihood="dirichlet")
    with pytest.raises(ValueError, match="127"):               # rows on the CPU never take the new route
        m._episode_loss(torch.nn.functional.normalize(torch.randn(400, 64)), m._targets(20, 20, torch.device("cpu")))
    with pytest.raises(RuntimeError, match="HIP-only"):
        ops.rownoise_lowrank(torch.zeros(1, 130, 64), torch.zeros(2, 130), torch.ones(2, 130), torch.ones(2), torch.zeros(2))
    with pytest.raises(RuntimeError, match="HIP-only"):
        ops.rownoise_lowrank_predict(torch.zeros(1, 3, 64), torch.zeros(1, 2, ops.ROWNOISE_LOWRANK_STATE), torch.ones(2), torch.zeros(2))
