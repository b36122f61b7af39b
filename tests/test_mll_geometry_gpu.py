"""mll_h2_kernel, mll_h2e_kernel and mll_mfma_kernel over their launch geometry -- every wave count, ragged last round, odd tail of a two-episode workgroup, tile
count edge and forward-only instantiation that tests/mll_geometry_model.py lists -- against float64, and against themselves: the split kernel (not the fix-up
kernel behind it) wrote the answer, a batch is bit for bit its episodes one by one, the surplus waves of the last workgroup write nothing, and the forward-only
call agrees with the gradient call.  One pytest parameter is one (route, N) and loops over C, B, the targets' layout and the class weights; every case prints a
MEASURED line: the fraction of each bound the kernel uses, next to the float32 restatement's (tests/test_mll_geometry_host.py holds that one to the same bounds
and shows that they catch the seeded mistakes).  The bounds are those of tests/test_gpu_parity.py, restated in mll_geometry_model.BOUNDS."""
import numpy as np
import pytest
import torch

import dkt_amd
import mll_geometry_model as gm

pytestmark = pytest.mark.gpu
ops, L = dkt_amd.ops, dkt_amd._lib
SENTINEL = -7.0          # (as tests/test_mll_dispatch.py pre-fills its outputs)
FLOAT_KEYS = ("logp", "alpha", "chol", "w", "dsv", "dmean", "dnoise", "jitter")


def _library(case):
    """The library the case claims, asserted right before the calls that go there."""
    lib = ops._lib_now(want_twin=case.twins)
    assert lib._name == (L.TWINS_LIB_PATH if case.twins else L.LIB_PATH)
    return lib


def _device(x, cuda):
    return {k: None if v is None else torch.tensor(np.ascontiguousarray(v), dtype=torch.float32, device=cuda) for k, v in x.items()}


def _mll(case, d, want_grad, **kw):
    return ops.mll(d["e"], d["y"], d["sv"], d["mean"], d["noise"], want_grad=want_grad, want_chol=case.want_chol, cls_weight=d["cw"], force_f32mfma=case.twins, **kw)


def _same_bits(a, b, where, sel=slice(None)):
    for key in FLOAT_KEYS + ("info",):
        if a[key] is None:
            assert b[key] is None
            continue
        assert torch.equal(a[key][sel], b[key]), (where, key)


def _at_the_abi_with_a_spare_episode(case, lib, d, want_grad):
    """The same call at the C ABI on outputs allocated for B + 1 episodes and pre-filled with the sentinel: (outputs of the B episodes, those of the spare one)."""
    b, c, n = case.b, case.c, case.n
    shapes = dict(logp=(c,), alpha=(c, n), jitter=(c,))
    if case.want_chol:
        shapes["chol"] = (c, n, n)
    if want_grad:
        shapes.update(w=(c, n, n) if case.per_class else (n, n), dsv=(c,), dmean=(c,), dnoise=(c,))
    out = {k: torch.full((b + 1,) + s, SENTINEL, device=d["e"].device) for k, s in shapes.items()}
    out["info"] = torch.full((b + 1, c), int(SENTINEL), device=d["e"].device, dtype=torch.int32)
    flags = (ops.MLL_WANT_GRAD * want_grad | ops.MLL_WANT_CHOL * case.want_chol | ops.MLL_E_PER_CLASS * case.per_class | ops.MLL_FORCE_F32MFMA * case.twins)
    assert lib.dkt_mll_workspace_bytes_for(b, c, n, flags) == 0
    p = lambda k: out[k].data_ptr() if k in out else None          # noqa: E731
    q = lambda t: None if t is None else t.data_ptr()               # noqa: E731
    rc = lib.dkt_mll_f32(q(d["e"]), q(d["y"]), c * n if d["y"].dim() == 3 else 0, q(d["sv"]), q(d["mean"]), q(d["noise"]), b, c, n, 1e-6, 3, flags, q(d["cw"]),
                         p("logp"), p("alpha"), p("chol"), p("w"), p("dsv"), p("dmean"), p("dnoise"), p("jitter"), p("info"), None, 0,
                         torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return {k: out.get(k)[:b] if k in out else None for k in FLOAT_KEYS + ("info",)}, {k: v[b] for k, v in out.items()}


def _check_mode(case, d, want_grad, split_guard):
    """One want_grad setting of a case: the batch call against float64, then against the unguarded call, its single episodes and the sentinel.  -> (outputs, fractions)"""
    lib = _library(case)
    out = _mll(case, d, want_grad)
    torch.cuda.synchronize()
    host = {k: out[k].cpu().numpy() for k in gm.OUTPUTS if out[k] is not None}
    fr = gm.fractions(case, host, want_grad=want_grad)
    where = "%s %s" % (case.name, "grad" if want_grad else "fwd")
    assert int(out["info"].abs().max().item()) == 0 and float(out["jitter"].abs().max().item()) == 0.0, where
    assert max(fr.values()) <= 1.0, (where, fr)
    if want_grad:
        assert torch.equal(out["w"], out["w"].transpose(-1, -2)), where
    if split_guard:
        # the condition guard flagged nothing: the generic fix-up kernel left at once and the split kernel's bits stand
        _same_bits(out, _mll(case, d, want_grad, no_kappa_guard=True), where + " no_kappa_guard")
    if case.b >= 2:
        for i in range(case.b):
            _same_bits(out, _mll(case, gm.episode(d, i), want_grad), "%s episode %d alone" % (where, i), slice(i, i + 1))
    first, spare = _at_the_abi_with_a_spare_episode(case, lib, d, want_grad)
    _same_bits(out, first, where + " at the C ABI")
    for k, v in spare.items():
        assert bool((v == SENTINEL).all()), (where, "episode B of `%s` was written" % k)
    return out, fr


@pytest.mark.parametrize("route,n", gm.PARAMS, ids=lambda v: str(v))
def test_kernels_over_their_launch_geometry(route, n, cuda, monkeypatch):
    for name in ops._VARIANT_SWITCHES + ("DKT_MLL_F32MFMA",):
        monkeypatch.delenv(name, raising=False)
    for case in gm.cases_for(route, n):
        monkeypatch.setenv("DKT_MLL_H2E_MINB", str(case.h2e_min_batch))          # (a product switch)
        d = _device(gm.inputs(case), cuda)
        f32 = gm.fractions(case, gm.reference32(case), want_grad=True)
        geo = case.geometry(True)
        assert geo.family == {"default": "h2", "h2e": "h2e", "chol": "mfma"}.get(route, "h2e" if n <= 111 else "h2")
        grad, fr = _check_mode(case, d, True, split_guard=route != "chol")
        line = gm.measured_line(case, True, fr, f32)
        if False in case.grads:
            fwd, fr_fwd = _check_mode(case, d, False, split_guard=route != "chol")
            line += "; forward only: kernel %s" % " ".join("%s %.2g" % kv for kv in fr_fwd.items())
            if case.geometry(False).family == geo.family and geo.family in ("h2", "mfma"):
                for key in ("logp", "alpha", "info", "jitter"):
                    assert torch.equal(fwd[key], grad[key]), (case.name, "forward-only call", key)
        print(line)
