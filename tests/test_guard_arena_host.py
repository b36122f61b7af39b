"""The checks of tests/guard_arena.py can fail: a CPU arena, a small fake module of plain torch code with one seeded defect at a time, and the verdict that has
to report each.  Nothing here touches a GPU: the defects are ordinary indexed writes into a CPU tensor that the arena owns (in the ordinary run, where the
storage behind an output ends with the output, they have nowhere to land and are skipped)."""
import types

import pytest
import torch

import guard_arena as ga

fake = types.ModuleType("fake_ops")          # the module whose `torch` the arena replaces, as it replaces dkt_amd.ops.torch
fake.torch = torch
N, WS_FLOATS = 100, 24


def _poke(t, element, value=None):
    """Write (or read: value None) the element `element` places from the start of t's memory, where t's storage reaches that far."""
    at = t.storage_offset() + element
    if at < 0 or (at + 1) * t.element_size() > t.untyped_storage().nbytes():
        return None
    cell = torch.empty(0, dtype=t.dtype).set_(t.untyped_storage(), at, (1,))
    if value is None:
        return cell.clone()
    cell.fill_(value)
    return None


def scale_and_sum(x, defect=None):
    """out = 2 x, total = sum(x) -- through a workspace the size of `WS_FLOATS` floats, as a library call would."""
    t = fake.torch
    out = t.empty(x.shape, dtype=torch.float32, device=x.device)
    big = t.empty((20000,), dtype=torch.float32, device=x.device)            # a second output, 80 KB: what lies 70 KiB behind `out`
    ws = t.empty((WS_FLOATS,), dtype=torch.float32, device=x.device)
    total = t.zeros((1,), dtype=torch.float32, device=x.device)
    fake.queries.append(("fake_workspace_bytes", WS_FLOATS * 4))
    big.copy_(torch.arange(20000, dtype=torch.float32))
    ws.copy_(x[:WS_FLOATS])
    if defect == "accumulate":
        out += 2 * x
    elif defect == "skip":
        out[:N - 1] = 2 * x[:N - 1]
    else:
        out.copy_(2 * x)
    total += x.sum()
    if defect == "past":
        _poke(out, N, 7.0)
    if defect == "before":
        _poke(out, -1, 7.0)
    if defect == "far":
        _poke(out, N + 70 * 1024 // 4, 7.0)
    if defect == "read-past":
        beyond = _poke(x, N)
        if beyond is not None:
            total += 0.0 * beyond                       # (NaN * 0 = NaN, 1.3e7 * 0 = 0: what a tile row that is used and not masked does)
    if defect == "modify-input":
        x[3] = 0.5
    if defect == "workspace":
        _poke(ws, WS_FLOATS, 1.0)
    if defect == "torch-made":
        return 2 * x, total
    return out, big, total


def _check(monkeypatch, defect):
    fake.queries = []
    x = torch.linspace(1.0, 100.0, N)           # (2 x >= 2: an accumulation into the finite fill, 1.3e7 with an ulp of 1, changes it)

    def extra(standin, report):
        fake.queries = report.queries
        return ga.contextlib.nullcontext()

    return ga.check(lambda inp: scale_and_sum(inp["x"], defect), dict(x=x), "cpu", monkeypatch, [fake], extra=extra)


def test_a_correct_call_passes_all_four(monkeypatch):
    r = _check(monkeypatch, None)
    assert r.failures() == []
    assert r.inside == {"out[0]": True, "out[1]": True, "out[2]": True}
    assert [b.role for b in r.blocks] == ["input", "allocated", "allocated", "allocated", "allocated"]
    assert all(b.address % ga.ALIGN == 0 for b in r.blocks)
    assert fake.torch is torch                           # restored


@pytest.mark.parametrize("defect, verdict", [("past", "footprint"), ("before", "footprint"), ("far", "independence"), ("skip", "coverage"),
                                             ("accumulate", "independence"), ("read-past", "independence"), ("modify-input", "footprint"),
                                             ("workspace", "footprint"), ("torch-made", "placement")])
def test_each_seeded_defect_is_reported_by_its_verdict(monkeypatch, defect, verdict):
    r = _check(monkeypatch, defect)
    got = r.failures()
    print(defect, got)
    assert got and all(f.startswith(verdict + ":") for f in got), got
    if defect == "torch-made":
        assert r.failures(outside=["out[0]"]) == []      # a case that says so passes


def test_a_workspace_smaller_than_the_query_fails_placement(monkeypatch):
    fake.queries = []

    def extra(standin, report):
        report.queries.append(("fake_workspace_bytes", WS_FLOATS * 4 + 4))
        return ga.contextlib.nullcontext()

    r = ga.check(lambda inp: scale_and_sum(inp["x"]), dict(x=torch.ones(N)), "cpu", monkeypatch, [fake], extra=extra)
    assert [f.split(":")[0] for f in r.failures()] == ["placement", "placement"]


def test_blocks_are_plain_tensors_and_work_through_autograd(monkeypatch):
    """Blocks are no views: they serve as outputs of an autograd Function with mark_non_differentiable, and as empty_like results in its backward."""
    class F(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            o = fake.torch.empty((x.shape[0],), dtype=torch.float32, device=x.device).copy_(x.sum(1))
            e = fake.torch.empty_like(x).copy_(2 * x)
            ctx.save_for_backward(e)
            ctx.mark_non_differentiable(e)
            return o, e

        @staticmethod
        def backward(ctx, g, *_):
            e, = ctx.saved_tensors
            return fake.torch.empty_like(e).copy_(g[:, None].expand_as(e))

    def call(inp):
        o, e = F.apply(inp["x"])
        assert not o._is_view() and not e._is_view() and not e.requires_grad
        (o * torch.tensor([1.0, 2.0, 3.0])).sum().backward()
        return o, e, inp["x"].grad

    r = ga.check(call, dict(x=torch.randn(3, 5, generator=torch.Generator().manual_seed(0)).requires_grad_()), "cpu", monkeypatch, [fake])
    assert r.failures() == []
    assert all(r.inside.values())


def test_fill_words_and_other_dtypes():
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        assert torch.isnan(torch.tensor([ga.FILL_NAN], dtype=torch.int32).view(dtype)).all()
        assert torch.isfinite(torch.tensor([ga.FILL_FINITE], dtype=torch.int32).view(dtype)).all()
    assert ga.FILL_NAN != 0x7FC00000
    arena = ga.Arena("cpu", ga.Arena.bytes_for([7, 6, 16]), ga.FILL_NAN)
    a, b, c = arena.take((7,), torch.uint8), arena.take((3,), torch.bfloat16), arena.take((2,), torch.int64)
    for t in (a, b, c):
        assert ga._fill_mask(t, ga.FILL_NAN).all()
    assert arena.footprint() == []
    a.zero_()
    assert arena.footprint() == [] and not ga._fill_mask(a, ga.FILL_NAN).any()
    ga.torch.empty(0, dtype=torch.uint8).set_(arena.buf.untyped_storage(), arena.blocks[0].offset + 7, (1,)).fill_(1)     # the byte behind a 7-byte block
    assert len(arena.footprint()) == 1


def test_the_stand_in_refuses_what_it_would_serve_differently_from_torch():
    """A creation keyword it does not implement, or *_like of a non-contiguous tensor (torch keeps the strides), raises in the measuring run and in the arena:
    a change in the code under test cannot quietly get another tensor here than in production."""
    arena = ga.Arena("cpu", ga.Arena.bytes_for([64] * 4), ga.FILL_FINITE)
    x = torch.ones(4, 6)
    for standin in (ga.StandIn("cpu"), ga.StandIn("cpu", arena)):
        assert standin.empty_like(x).shape == x.shape
        with pytest.raises(TypeError, match="memory_format"):
            standin.empty((4, 6), dtype=torch.float32, device="cpu", memory_format=torch.contiguous_format)
        with pytest.raises(TypeError, match="requires_grad"):
            standin.zeros(3, device="cpu", requires_grad=True)
        with pytest.raises(TypeError, match="non-contiguous"):
            standin.empty_like(x.t())
        with pytest.raises(TypeError, match="non-contiguous"):
            standin.zeros_like(x[:, ::2])
        assert standin.empty(3, pin_memory=False).shape == (3,)          # (no device: torch's own)
