"""CPU-side checks of the sine-wave experiment: libdkt_smk.so exports exactly include/dkt_abi_smk.h (the _lib signature table too), does not
spill and rejects out-of-limit shapes before any launch; the task sampler's contract on CPU tensors; the driver's defaults are the reference's
constants; SineFeature has the reference's parameter names and shapes."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import pytest
import torch

import dkt_amd
from dkt_amd import io_utils, sines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000          # a well-aligned non-NULL address: every call below must return before it is dereferenced or a kernel is launched
ERR_BAD_ARG, ERR_SHAPE = -1, -5


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(dkt_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def smk_lib():
    if not shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")) and not os.path.exists(dkt_amd._lib.SMK_LIB_PATH):
        pytest.skip("no hipcc and no built libdkt_smk.so")
    return dkt_amd._lib.load_smk()


def test_signature_table_is_the_header():
    declared = _declared("dkt_abi_smk.h")
    assert declared == ["dkt_smk_abi_version", "dkt_smk_task_bwd_f32", "dkt_smk_task_f32", "dkt_smk_task_workspace_bytes"]
    assert sorted(dkt_amd._lib.SMK_SIGNATURES) == declared
    text = open(os.path.join(ROOT, "include", "dkt_abi_smk.h")).read()
    limits = {k: int(v) for k, v in re.findall(r"#define\s+DKT_SMK_TASK_MAX_([A-Z])\s+(\d+)", text)}
    assert (limits["N"], limits["M"], limits["D"], limits["Q"]) == (dkt_amd._lib.SMK_MAX_N, dkt_amd._lib.SMK_MAX_M, dkt_amd._lib.SMK_MAX_D,
                                                                   dkt_amd._lib.SMK_MAX_Q)
    assert int(re.search(r"#define\s+DKT_ERR_SHAPE\s+\((-\d+)\)", text).group(1)) == ERR_SHAPE
    assert dkt_amd._lib.STATUS[ERR_SHAPE] == "DKT_ERR_SHAPE"


def test_library_exports_exactly_its_header(smk_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", dkt_amd._lib.SMK_LIB_PATH], capture_output=True, text=True, check=True).stdout
    exports = sorted({line.split()[-1] for line in out.splitlines() if line.split()[-1].startswith("dkt_")})
    assert exports == _declared("dkt_abi_smk.h")
    assert smk_lib.dkt_smk_abi_version() == dkt_amd._lib.smk_abi_version_of_header() == 1


def test_library_does_not_spill(smk_lib):
    path = os.path.join(os.path.dirname(dkt_amd._lib.LIB_PATH), "build", "libdkt_smk.so.resource_usage.json")
    usage = json.load(open(path))
    assert len(usage) == 25 and any("smk_task_sum_kernel" in k for k in usage)      # 8 x 2 forward, 8 backward, 1 sum
    assert all(u.get("vgpr_spill", 0) == 0 and u.get("scratch", 0) == 0 for u in usage.values())
    assert dkt_amd._lib.check_resources(usage) == []


def test_workspace_bytes(smk_lib):
    assert smk_lib.dkt_smk_task_workspace_bytes(1024, 10, 40, 4) == 1024 * (4 + 2 * 4 * 40) * 4
    assert smk_lib.dkt_smk_task_workspace_bytes(0, 10, 40, 4) == 0


def test_limits_and_argument_errors_do_not_launch(smk_lib):
    L, p = smk_lib, FAKE

    def fwd(x2=None, B=2, M=10, N=10, D=40, Q=4, x1=p, E=p):
        return L.dkt_smk_task_f32(x1, x2, p, p, p, E, B, M, N, D, Q, None)

    def bwd(B=2, N=10, D=40, Q=4, ws=p, dx=p):
        return L.dkt_smk_task_bwd_f32(p, p, p, p, p, dx, p, p, p, ws, B, N, D, Q, None)

    assert fwd(N=33, M=33) == ERR_SHAPE and fwd(D=65) == ERR_SHAPE and fwd(Q=9) == ERR_SHAPE
    assert fwd(x2=p, M=257, N=5) == ERR_SHAPE and fwd(x2=p, M=200, N=33) == ERR_SHAPE
    assert bwd(N=33) == ERR_SHAPE and bwd(D=65) == ERR_SHAPE and bwd(Q=9) == ERR_SHAPE
    assert fwd(M=9) == ERR_BAD_ARG                                   # symmetric needs M == N
    assert fwd(x1=None) == ERR_BAD_ARG and fwd(E=None) == ERR_BAD_ARG and fwd(B=0) == ERR_BAD_ARG and fwd(Q=0) == ERR_BAD_ARG
    assert bwd(ws=None) == ERR_BAD_ARG and bwd(dx=None) == ERR_BAD_ARG and bwd(ws=p + 2) == ERR_BAD_ARG and bwd(D=0) == ERR_BAD_ARG


def test_supported_predicate():
    from dkt_amd import ops
    assert ops.smk_task_supported(10, 10, 40, 4) and ops.smk_task_supported(32, 32, 64, 8) and ops.smk_task_supported(256, 32, 64, 8, False)
    assert not ops.smk_task_supported(33, 33, 40, 4) and not ops.smk_task_supported(10, 10, 65, 4) and not ops.smk_task_supported(10, 10, 40, 9)
    assert not ops.smk_task_supported(200, 5, 40, 4, True) and ops.smk_task_supported(200, 5, 40, 4, False)
    assert not ops.smk_task_supported(257, 5, 40, 4, False)


# ---- sampler -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", sines.FAMILIES)
def test_train_batch_shapes_and_ranges(family):
    s = sines.SineTaskSampler(sines.TRAIN_RANGE, family, seed=3, device="cpu", noise=0.0)
    x, y = s.train_batch(64, 10)
    assert x.shape == (64, 10, 1) and y.shape == (64, 10) and x.dtype == torch.float32 and x.device.type == "cpu"
    assert float(x.min()) >= -5.0 and float(x.max()) <= 5.0
    assert float(y.abs().max()) <= 5.0 + 1e-5
    assert not bool((x[:, 1:, 0] >= x[:, :-1, 0]).all())            # training points are not sorted


@pytest.mark.parametrize("family", sines.FAMILIES)
def test_targets_follow_the_family(family):
    s = sines.SineTaskSampler((-5.0, 10.0), family, seed=4, device="cpu", noise=0.0)
    t = s.test_batch(32)
    ref = s.true_function(t["amplitude"][:, None], t["phase"][:, None], t["x_all"][..., 0])
    torch.testing.assert_close(t["y_all"], ref, rtol=0, atol=0)
    a, ph = t["amplitude"], t["phase"]
    assert float(a.min()) >= 0.1 and float(a.max()) <= 5.0 and float(ph.min()) >= 0.0 and float(ph.max()) <= 3.1416
    assert float(t["x_all"].min()) >= -5.0 and float(t["x_all"].max()) <= 10.0
    assert float(t["x_all"].max()) > 5.0                            # the out-of-range condition reaches past the training range


def test_noise_level():
    s = sines.SineTaskSampler(seed=5, device="cpu")
    t = s.test_batch(500)
    r = t["y_all"] - s.true_function(t["amplitude"][:, None], t["phase"][:, None], t["x_all"][..., 0])
    assert abs(float(r.std()) - 0.1) < 0.005 and abs(float(r.mean())) < 0.005


def test_test_batch_support_and_query():
    s = sines.SineTaskSampler(seed=6, device="cpu")
    t = s.test_batch(50, 200, 5)
    assert t["x_all"].shape == (50, 200, 1) and t["support"].shape == (50, 5) and t["query"].shape == (50, 195)
    assert bool((t["x_all"][:, 1:, 0] >= t["x_all"][:, :-1, 0]).all())
    for b in range(50):
        sup, qry = t["support"][b].tolist(), t["query"][b].tolist()
        assert sup == sorted(sup) and qry == sorted(qry) and sorted(sup + qry) == list(range(200))
        assert torch.equal(t["x_support"][b, :, 0], t["x_all"][b, sup, 0]) and torch.equal(t["y_query"][b], t["y_all"][b, qry])
    assert len({tuple(r) for r in t["support"].tolist()}) > 40        # the support sets differ between tasks


def test_same_seed_same_tasks():
    a, b, c = (sines.SineTaskSampler(seed=sd, device="cpu") for sd in (7, 7, 8))
    xa, ya = a.train_batch(16)
    xb, yb = b.train_batch(16)
    xc, _ = c.train_batch(16)
    assert torch.equal(xa, xb) and torch.equal(ya, yb) and not torch.equal(xa, xc)
    ta, tb = a.test_batch(8), b.test_batch(8)
    assert all(torch.equal(ta[k], tb[k]) for k in ta)
    with pytest.raises(ValueError):
        sines.SineTaskSampler(family="square", device="cpu")


# ---- driver and model surface --------------------------------------------------------------------------------------------------------------

def test_parser_defaults_are_the_reference_constants():
    a = io_utils.parse_args_sines([])
    assert (a.iterations, a.n_shot_train, a.n_shot_test, a.lr, a.n_test_tasks) == (50000, 10, 5, 1e-3, 500)
    assert (a.test_range, a.family, a.tasks_per_step, a.seed, a.checkpoint, a.test_only) == ("in", "sine", 1, 0, None, False)
    b = io_utils.parse_args_sines(["--test_range", "out", "--family", "cosine", "--tasks_per_step", "64", "--checkpoint", "m.tar", "--test_only"])
    assert (b.test_range, b.family, b.tasks_per_step, b.checkpoint, b.test_only) == ("out", "cosine", 64, "m.tar", True)
    assert sines.TEST_RANGES == {"in": (-5.0, 5.0), "out": (-5.0, 10.0)}
    with pytest.raises(SystemExit):
        io_utils.parse_args_sines(["--test_only"])


def test_sine_feature_parameters():
    f = sines.SineFeature()
    shapes = {k: tuple(v.shape) for k, v in f.state_dict().items()}
    assert shapes == {"layer1.weight": (40, 1), "layer1.bias": (40,), "layer2.weight": (40, 40), "layer2.bias": (40,)}
    z = f(torch.randn(7, 1))
    assert z.shape == (7, 40) and float(z.detach().min()) >= 0.0


def test_sines_dkt_hyper_parameters():
    m = sines.SinesDKT()
    shapes = {k: tuple(v.shape) for k, v in m.model.named_parameters()}
    assert shapes == {"mean_constant": (1,), "raw_mixture_weights": (4,), "raw_mixture_means": (4, 1, 40), "raw_mixture_scales": (4, 1, 40),
                      "raw_noise": (1,)}
    assert m.kernel_type == "spectral" and m.num_mixtures == 4 and m.ard_num_dims == 40
