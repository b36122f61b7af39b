"""The front door of the per-class GP calls of dkt_amd.ops, on the host: `_problem` (what a problem looks like), `_class_strides` (what the C ABI gets for an
operand that is shared by the class models or has a class axis) and `_workspace`.  `_req` refuses CPU tensors, so a stand-in that checks dtype and number of
dimensions and makes the tensor contiguous takes its place; the expected strides are the expressions every wrapper spelled out before these helpers existed."""
import itertools

import pytest
import torch

from dkt_amd import ops

B, C, N, D = 2, 3, 4, 8


@pytest.fixture(autouse=True)
def _req_on_the_host(monkeypatch):
    def req(t, name, ndim=None):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or (ndim is not None and t.dim() != ndim):
            raise RuntimeError("dkt_amd.ops: `%s` must be a float32 tensor%s" % (name, "" if ndim is None else " and must have %d dims" % ndim))
        return t.contiguous()
    monkeypatch.setattr(ops, "_req", req)


def _operands(base, y_dim, nr_dim, weighted):
    kw = dict(sv=torch.rand(C), mean=torch.rand(C), noise=torch.rand(C), cls_weight=torch.rand(C) if weighted else None)
    if base == "rows":
        kw["rows"] = torch.rand(B, N, D)
    else:
        kw["base"] = torch.rand(B, N, N) if base == "shared" else torch.rand(B, C, N, N)
    if nr_dim:
        kw["noise_rows"] = torch.rand(C, N) if nr_dim == 2 else torch.rand(B, C, N)
    return (torch.rand(C, N) if y_dim == 2 else torch.rand(B, C, N)), kw


@pytest.mark.parametrize("base,y_dim,nr_dim,weighted", list(itertools.product(("shared", "per_class", "rows"), (2, 3), (0, 2, 3), (False, True))))
def test_the_record_holds_the_sizes_and_strides_the_wrappers_spelled_out(base, y_dim, nr_dim, weighted):
    y, kw = _operands(base, y_dim, nr_dim, weighted)
    pr = ops._problem("mll", y, **kw)
    b_, c_, n = B, C, N
    per_class = base == "per_class"
    assert (pr.b, pr.c, pr.n, pr.d, pr.per_class) == (B, C, N, D if base == "rows" else None, per_class)
    if base == "rows":
        assert pr.base is None and pr.base_strides is None and pr.rows is not None and torch.equal(pr.rows, kw["rows"])
    else:
        assert pr.rows is None and torch.equal(pr.base, kw["base"])
        assert pr.base_strides == ((c_ if per_class else 1) * n * n, n * n if per_class else 0)
        assert ops._class_strides(kw["base"], c_) == pr.base_strides
    assert pr.y_bstride == (c_ * n if y.dim() == 3 else 0)
    noise_rows = kw.get("noise_rows")
    assert pr.nr_bstride == (0 if noise_rows is None else c_ * n if noise_rows.dim() == 3 else 0)
    assert (pr.noise_rows is None) == (noise_rows is None) and (noise_rows is None or torch.equal(pr.noise_rows, noise_rows))
    assert torch.equal(pr.y, y) and pr.dev == y.device
    sv, mean, noise, cw = pr.hypers                                              # in the order they were named
    assert torch.equal(sv, kw["sv"]) and torch.equal(mean, kw["mean"]) and torch.equal(noise, kw["noise"])
    assert (cw is None) if not weighted else torch.equal(cw, kw["cls_weight"])
    with pytest.raises(AttributeError):
        pr.b = 1                                                                 # immutable


def test_strides_of_the_other_operands_with_an_optional_class_axis():
    """e_qs / Ks [B,(C,)M,N], e_qq [B,(C,)M,M] (posterior, laplace_predict) and kss [B,(C,)M] (laplace_predict), against what those calls wrote inline."""
    b_, c_, m, n = B, C, 5, N
    for per_class in (False, True):
        lead = (b_, c_) if per_class else (b_,)
        assert ops._class_strides(torch.zeros(*lead, m, n), c_) == ((c_ if per_class else 1) * m * n, m * n if per_class else 0)
        assert ops._class_strides(torch.zeros(*lead, m, m), c_) == ((c_ if per_class else 1) * m * m, m * m if per_class else 0)
        assert ops._class_strides(torch.zeros(*lead, m), c_, 1) == ((c_ if per_class else 1) * m, m if per_class else 0)


@pytest.mark.parametrize("shape", [(C,), (C, 1), (1, C)])
def test_hypers_come_back_flat_and_contiguous(shape):
    y, kw = _operands("shared", 2, 0, True)
    given = {k: torch.rand(2 * C).reshape(C, 2)[:, 0].reshape(shape) for k in ("sv", "mean", "noise", "cls_weight")}        # (strided: not contiguous)
    pr = ops._problem("loo", y, base=kw["base"], **given)
    for got, name in zip(pr.hypers, ("sv", "mean", "noise", "cls_weight")):
        assert tuple(got.shape) == (C,) and got.is_contiguous() and torch.equal(got, given[name].reshape(-1))


def test_optional_hypers_may_be_none_and_required_ones_may_not():
    y, kw = _operands("shared", 2, 0, False)
    assert ops._problem("laplace_grad", y, base=kw["base"], cls_weight=None, scale=None).hypers == (None, None)
    with pytest.raises(RuntimeError, match="sv"):
        ops._problem("loo", y, base=kw["base"], sv=None)


def test_a_non_contiguous_y_comes_back_contiguous():
    _, kw = _operands("shared", 3, 0, False)
    y = torch.rand(B, N, C).transpose(1, 2)
    assert not y.is_contiguous()
    pr = ops._problem("mll", y, **kw)
    assert pr.y.is_contiguous() and torch.equal(pr.y, y) and pr.y_bstride == C * N


MALFORMED = {
    "non-square base": dict(base=torch.rand(B, N, N + 1)),
    "y last dim": dict(y=torch.rand(C, N + 1)),
    "y batch": dict(y=torch.rand(B + 1, C, N)),
    "class axis": dict(base=torch.rand(B, C + 1, N, N)),
    "noise_rows shape": dict(noise_rows=torch.rand(C, N + 1)),
    "noise_rows classes": dict(noise_rows=torch.rand(C + 1, N)),
    "noise_rows batch": dict(noise_rows=torch.rand(B + 1, C, N)),
    "hyper too long": dict(mean=torch.rand(C + 1)),
    "cls_weight too short": dict(cls_weight=torch.rand(C - 1)),
    "base dims": dict(base=torch.rand(N, N)),
    "y dims": dict(y=torch.rand(N)),
}


@pytest.mark.parametrize("fn", ["mll", "rownoise_lowrank_bwd"])
@pytest.mark.parametrize("what", sorted(MALFORMED))
def test_malformed_operands_raise_and_name_the_caller(what, fn):
    bad = dict(MALFORMED[what])
    y, kw = _operands("per_class" if what == "class axis" else "shared", 3 if what == "y batch" else 2, 2, True)
    y = bad.pop("y", y)
    kw.update(bad)
    with pytest.raises(RuntimeError, match="^%s: " % fn):
        ops._problem(fn, y, **kw)


def test_rows_reject_the_same_y():
    y, kw = _operands("rows", 2, 0, False)
    for bad in (torch.rand(C, N + 1), torch.rand(B + 1, C, N), torch.rand(N)):
        with pytest.raises(RuntimeError, match="^loo_lowrank: "):
            ops._problem("loo_lowrank", bad, **kw)
    with pytest.raises(RuntimeError, match="must have 3 dims"):
        ops._problem("loo_lowrank", y, rows=torch.rand(N, D))


def test_workspace():
    assert ops._workspace(0) is None and ops._workspace(0, torch.device("cpu")) is None
    for k in (1, 2, 7, 361, 4096, 3 * 64 * 64):
        ws = ops._workspace(4 * k)
        assert ws.dtype == torch.float32 and tuple(ws.shape) == (k,) and ws.numel() * ws.element_size() == 4 * k
        # the four sizes the wrappers used to spell out are this one for a positive multiple of 4 (what every *_workspace_bytes* query returns)
        nbytes = 4 * k
        assert k == (nbytes + 3) // 4 == (max(nbytes, 4) + 3) // 4 == nbytes // 4 == max(nbytes, 4) // 4


def test_allocators_make_what_the_wrappers_spelled_out():
    dev = torch.device("cpu")
    a, i = ops._f32(dev, B, C, N), ops._i32(dev, B, C)
    assert a.dtype == torch.float32 and tuple(a.shape) == (B, C, N) and a.device == dev
    assert i.dtype == torch.int32 and tuple(i.shape) == (B, C) and i.device == dev
