"""CPU-side checks of libdkt_x16.so, the front-end kernels for 16-bit trunk features (mixed-precision backbones): it cross-compiles for gfx950, exports
exactly the functions of include/dkt_abi_x16.h, does not spill, and rejects bad arguments on the host before any launch; the product library stays free
of them; the drivers' --amp flag."""
import json
import os
import re
import subprocess

import pytest

import dkt_amd
from dkt_amd import configs
from dkt_amd.io_utils import parse_args, parse_args_regression

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJDUMP = os.environ.get("LLVM_OBJDUMP", "/opt/rocm/lib/llvm/bin/llvm-objdump")
FAKE = 0x10000          # a well-aligned non-NULL address: every call below must return before it is dereferenced or a kernel is launched


@pytest.fixture(scope="module")
def x16():
    dkt_amd._lib.build()
    return dkt_amd._lib.load_x16()


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(dkt_[a-z0-9_]+)\s*\(", text)))


def _exports(path):
    """The functions a shared object defines in its dynamic symbol table (llvm-objdump -T: defined ones are in .text)."""
    out = subprocess.run([OBJDUMP, "-T", path], capture_output=True, text=True, check=True).stdout
    return sorted({line.split()[-1] for line in out.splitlines() if " .text" in line and line.split()[-1].startswith("dkt_")})


def test_x16_library_exports_exactly_its_header(x16):
    declared = _declared("dkt_abi_x16.h")
    assert len(declared) == 9
    assert sorted(dkt_amd._lib.X16_SIGNATURES) == declared
    assert _exports(dkt_amd._lib.X16_LIB_PATH) == declared
    assert x16.dkt_x16_abi_version() == dkt_amd._lib.x16_abi_version_of_header() == 2
    # each entry point is its fp32 twin of dkt_abi.h plus `int xdtype` right after X
    for name, (res, args) in dkt_amd._lib.X16_SIGNATURES.items():
        twin = name.replace("_x16", "_f32")
        if twin in dkt_amd._lib.SIGNATURES:
            targs = dkt_amd._lib.SIGNATURES[twin][1]
            assert len(args) == len(targs) + 1 and res == dkt_amd._lib.SIGNATURES[twin][0], name


def test_x16_library_does_not_spill(x16):
    path = os.path.join(os.path.dirname(dkt_amd._lib.LIB_PATH), "build", "libdkt_x16.so.resource_usage.json")
    usage = json.load(open(path))
    assert len(usage) >= 80                          # bf16 + f16 instances of every front-end kernel
    assert all(u.get("vgpr_spill", 0) == 0 and u.get("scratch", 0) == 0 for u in usage.values()), \
        sorted(k for k, u in usage.items() if u.get("vgpr_spill", 0))
    assert dkt_amd._lib.check_resources(usage) == []
    assert any("DF16b" in k for k in usage) and any("DF16_" in k for k in usage)      # both element types are instantiated


def test_x16_argument_errors_do_not_launch(x16):
    L, p = x16, FAKE
    for bad_dtype in (0, 3, -1):
        assert L.dkt_bn_stats_x16(p, bad_dtype, None, None, 1e-5, p, p, p, p, None, 1, 4, 4, None) == -1
        assert L.dkt_gram_bn_x16(p, bad_dtype, p, p, 0, p, p, 1, 4, 4, None) == -1
        assert L.dkt_gram_bn_train_x16(p, bad_dtype, None, None, 1e-5, p, p, p, p, None, p, p, 1, 4, 4, None) == -1
        assert L.dkt_gram_bn_bwd_x16(p, p, p, bad_dtype, p, p, 0, None, None, p, None, p, None, None, 1, 4, 4, None) == -1
        assert L.dkt_affine_normalize_x16(p, bad_dtype, p, p, 0, p, p, 1, 4, 4, None) == -1
        assert L.dkt_normalize_bn_bwd_x16(p, p, p, bad_dtype, p, 0, None, None, p, p, None, None, p, 1, 4, 4, None) == -1
    for dt in (dkt_amd._lib.X_BF16, dkt_amd._lib.X_F16):
        # NULL pointers
        assert L.dkt_bn_stats_x16(None, dt, None, None, 1e-5, p, p, p, p, None, 1, 4, 4, None) == -1
        assert L.dkt_gram_bn_x16(p, dt, None, p, 0, p, p, 1, 4, 4, None) == -1
        assert L.dkt_gram_bn_train_x16(p, dt, None, None, 1e-5, p, p, p, p, None, None, p, 1, 4, 4, None) == -1
        assert L.dkt_gram_bn_bwd_x16(p, p, p, dt, p, p, 0, None, None, p, None, None, None, None, 1, 4, 4, None) == -1
        assert L.dkt_affine_normalize_x16(None, dt, p, p, 0, p, p, 1, 4, 4, None) == -1
        assert L.dkt_normalize_bn_bwd_x16(p, p, p, dt, p, 0, None, None, p, None, None, None, p, 1, 4, 4, None) == -1
        # D % 4 != 0
        assert L.dkt_bn_stats_x16(p, dt, None, None, 1e-5, p, p, p, p, None, 1, 4, 6, None) == -1
        assert L.dkt_gram_bn_x16(p, dt, p, p, 0, p, p, 1, 4, 6, None) == -1
        assert L.dkt_gram_bn_train_x16(p, dt, None, None, 1e-5, p, p, p, p, None, p, p, 1, 4, 6, None) == -1
        assert L.dkt_gram_bn_bwd_x16(p, p, p, dt, p, p, 0, None, None, p, None, p, None, None, 1, 4, 6, None) == -1
        assert L.dkt_affine_normalize_x16(p, dt, p, p, 0, p, p, 1, 4, 6, None) == -1
        assert L.dkt_normalize_bn_bwd_x16(p, p, p, dt, p, 0, None, None, p, p, None, None, p, 1, 4, 6, None) == -1
        # X / dX not 8-byte aligned
        assert L.dkt_gram_bn_train_x16(p + 4, dt, None, None, 1e-5, p, p, p, p, None, p, p, 1, 4, 4, None) == -1
        assert L.dkt_gram_bn_bwd_x16(p, p, p, dt, p, p, 0, None, None, p, None, p + 2, None, None, 1, 4, 4, None) == -1
        # train-mode backward without its statistics' partial sums
        assert L.dkt_gram_bn_bwd_x16(p, p, p, dt, p, p, 0, p, p, p, None, p, None, None, 1, 4, 4, None) == -1
        assert L.dkt_normalize_bn_bwd_x16(p, p, p, dt, p, 0, p, p, p, p, None, None, p, 1, 4, 4, None) == -1
        # too many rows for the episode-resident kernels
        assert L.dkt_gram_bn_train_x16(p, dt, None, None, 1e-5, p, p, p, p, None, p, p, 1, 129, 4, None) == -2


def test_product_library_has_no_x16_symbol(lib):
    assert not any(name.endswith("_x16") or "x16" in name for name in _exports(dkt_amd._lib.LIB_PATH))
    for name in dkt_amd._lib.X16_SIGNATURES:
        assert not hasattr(lib, name), name
    assert not set(dkt_amd._lib.X16_SIGNATURES) & set(dkt_amd._lib.SIGNATURES)


def test_amp_flag_of_the_drivers(monkeypatch):
    monkeypatch.setattr(configs, "amp", None)            # (parse_args sets it: restored after the test)
    assert parse_args("train", ["--amp", "bf16"]).amp == "bf16"
    assert parse_args("train", []).amp == "none"
    assert parse_args("test", ["--amp", "bf16"]).amp == "bf16" and parse_args("test", []).amp == "none"
    assert parse_args_regression("train_regression", ["--amp", "bf16"]).amp == "bf16"
    assert parse_args_regression("test_regression", []).amp == "none"
    with pytest.raises(SystemExit):
        parse_args("train", ["--amp", "fp16"])
    # the flag is the default of every model the process builds (test_uncertainty.py constructs its DKT without passing it on)
    parse_args("test", ["--amp", "bf16"])
    assert configs.amp == "bf16"
    assert dkt_amd.DKT(dkt_amd.backbone.Conv4S, n_way=5, n_support=5).amp == "bf16"
    assert dkt_amd.DKTRegression(dkt_amd.backbone.Conv3(), "rbf").amp == "bf16"
    assert dkt_amd.DKT(dkt_amd.backbone.Conv4S, n_way=5, n_support=5, amp="none").amp is None
    parse_args("test", [])
    assert configs.amp is None and dkt_amd.DKT(dkt_amd.backbone.Conv4S, n_way=5, n_support=5).amp is None


def test_amp_mode_of_the_models(monkeypatch):
    monkeypatch.setattr(configs, "amp", None)
    m = dkt_amd.DKT(dkt_amd.backbone.Conv4S, n_way=5, n_support=5, amp="bf16")
    assert m.amp == "bf16"
    m.amp = "none"                                       # an attribute too, validated like the argument
    assert m.amp is None
    with pytest.raises(ValueError):
        m.amp = "f16"
    assert dkt_amd.DKT(dkt_amd.backbone.Conv4S, n_way=5, n_support=5).amp is None
    assert dkt_amd.DKT(dkt_amd.backbone.Conv4S, n_way=5, n_support=5, amp="none").amp is None
    with pytest.raises(ValueError):
        dkt_amd.DKT(dkt_amd.backbone.Conv4S, n_way=5, n_support=5, amp="fp16")
    r = dkt_amd.DKTRegression(dkt_amd.backbone.Conv3(), "rbf", amp="bf16")
    assert r.amp == "bf16"
    with pytest.raises(ValueError):
        dkt_amd.DKTRegression(dkt_amd.backbone.Conv3(), "rbf", amp="fp8")
