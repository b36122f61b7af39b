"""What DKT's losses and predictions state once (host side, no GPU): the first-maximum arg-max, the table of objectives behind the public episode calls of
dkt_amd.ops (its output names against what the classes return and what the public calls document), and the refusals of the loss ladder, word for word."""
import collections
import inspect
import re

import numpy as np
import pytest
import torch

import dkt_amd
from dkt_amd import dkt, ops


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("dim", [0, 1, -1])
def test_first_argmax_is_np_argmax_on_ties(dim, dtype):
    mu = torch.tensor([[1.0, 3.0, 3.0, 0.0, 2.0], [3.0, 3.0, 1.0, 0.0, 2.0], [3.0, 0.0, 3.0, 0.0, 2.0], [-1.0, -1.0, -1.0, -1.0, -1.0]])
    got = dkt.first_argmax(mu, dim, dtype)
    assert got.dtype == dtype and got.tolist() == np.argmax(mu.numpy(), axis=dim).tolist()
    cube = torch.stack([mu, mu.flip(1)], 0)                              # [2, 4, 5]: a dim in the middle, as _posterior uses it
    assert dkt.first_argmax(cube, 1, dtype).tolist() == np.argmax(cube.numpy(), axis=1).tolist()
    assert dkt.first_argmax(mu, 0).dtype == torch.int64


def _stub_forward(monkeypatch, cls):
    """cls.forward on stub tensors, every library call behind it replaced by one that returns stubs."""
    t = torch.zeros(2)
    anything = collections.defaultdict(lambda: t)
    for name in ("mll", "loo", "loo_lowrank", "_lowrank_forward", "mll_rownoise", "rownoise_lowrank"):
        monkeypatch.setattr(ops, name, lambda *a, **k: anything)
    monkeypatch.setattr(ops, "objective", lambda *a, **k: t)
    monkeypatch.setattr(ops, "_laplace_forward", lambda *a, **k: (t, t, t, t, t))
    nargs = len(inspect.signature(cls.forward).parameters)
    return cls.forward((t, True) if cls.on_features else t, *([t] * (nargs - 1)))


def test_every_objective_names_the_outputs_its_classes_return(monkeypatch):
    assert set(ops.OBJECTIVES) == {"gaussian", "loo", "laplace", "dirichlet"} and set(ops.OBJECTIVE_OUTPUTS) == set(ops.OBJECTIVES)
    for name, row in ops.OBJECTIVES.items():
        assert ops.OBJECTIVE_OUTPUTS[name] == row.outputs and row.outputs[0] == "logp" and len(set(row.outputs)) == len(row.outputs)
        assert (row.on_rows is None) == (row.applies is None)
        for cls in (row.on_e, row.on_rows):
            if cls is None:
                continue
            obj, aux, saved, static = _stub_forward(monkeypatch, cls)
            assert len(aux) == len(row.outputs), (name, cls)
        assert not row.on_e.on_features and callable(row.on_e.de)
        if row.on_rows is not None:
            assert row.on_rows.on_features is True and row.on_rows.de is None and issubclass(row.on_rows, row.on_e)
    assert ops.OBJECTIVES["gaussian"].applies is ops.lowrank_applies and ops.OBJECTIVES["loo"].applies is ops.loo_lowrank_applies
    assert ops.OBJECTIVES["dirichlet"].applies is ops.rownoise_lowrank_applies


WRAPPERS = {
    "mll_objective": ("gaussian", ops.GIVEN_E_OUTPUTS), "laplace_objective": ("laplace", ops.GIVEN_E_OUTPUTS),
    "dirichlet_objective": ("dirichlet", ops.GIVEN_E_OUTPUTS), "loo_objective": ("loo", ops.GIVEN_E_OUTPUTS),
    "episode_loss_linear": ("gaussian", ops.ROWS_OUTPUTS), "episode_loss_class_kernel": ("gaussian", ops.ROWS_OUTPUTS),
    "episode_loss_laplace": ("laplace", ops.ROWS_OUTPUTS), "episode_loss_dirichlet": ("dirichlet", ops.ROWS_OUTPUTS),
    "episode_loss_loo": ("loo", ops.ROWS_OUTPUTS), "episode_loss_bn": ("gaussian", ops.BN_TRUNK_OUTPUTS[:3]),          # (a, s, rnorm only with full=True)
    "episode_loss_laplace_bn": ("laplace", ops.BN_TRUNK_OUTPUTS), "episode_loss_dirichlet_bn": ("dirichlet", ops.BN_TRUNK_OUTPUTS),
    "episode_loss_loo_bn": ("loo", ops.BN_TRUNK_OUTPUTS),
}


@pytest.mark.parametrize("wrapper", sorted(WRAPPERS))
def test_every_public_call_documents_the_table_s_order(wrapper):
    name, front = WRAPPERS[wrapper]
    documented = re.search(r"Returns \(((?:\w+, )+\w+)\)", getattr(ops, wrapper).__doc__).group(1).split(", ")
    assert tuple(documented) == ("obj",) + ops.OBJECTIVE_OUTPUTS[name] + front
    assert ops.ROWS_OUTPUTS == ("e",) and ops.BN_TRUNK_OUTPUTS == ("e", "batch_mean", "batch_var_unbiased", "a", "s", "rnorm")


ROWS = "n_way * (n_support + n_query)"
HINT_DIRICHLET = "; larger ones run in feature space: linear / cossim / bncossim with up to 64 features (a multiple of 4), on the GPU"
HINT_LOO = "; larger ones run in feature space: linear / cossim / bncossim with up to 64 features (a multiple of 4), more than 128 rows, on the GPU"
REFUSALS = [       # (model arguments, rows, classes, the message as the parent commit words it)
    (dict(likelihood="bernoulli"), 130, 5, "likelihood='bernoulli' takes episodes of up to 127 rows (%s), this one has 130" % ROWS),
    (dict(likelihood="bernoulli"), 66, 33, "likelihood='bernoulli' takes up to 32 classes, the episode has 33"),
    (dict(likelihood="dirichlet"), 130, 5, "likelihood='dirichlet' takes episodes of up to 127 rows (%s), this one has 130%s" % (ROWS, HINT_DIRICHLET)),
    (dict(likelihood="dirichlet"), 66, 33, "likelihood='dirichlet' takes up to 32 classes, the episode has 33"),
    (dict(objective="loo"), 128, 4, "objective='loo' takes episodes of up to 127 rows (%s), this one has 128%s" % (ROWS, HINT_LOO)),
    (dict(objective="loo"), 66, 33, "objective='loo' takes up to 32 classes, the episode has 33"),
]


@pytest.mark.parametrize("kw,n,c,message", REFUSALS, ids=lambda v: v if isinstance(v, int) else None)
@pytest.mark.parametrize("kernel", ["bncossim", "rbf"])
def test_both_losses_refuse_in_the_parent_s_words_before_any_launch(kernel, kw, n, c, message, monkeypatch):
    monkeypatch.setattr(dkt_amd.configs, "likelihood", None)
    monkeypatch.setattr(dkt_amd.configs, "objective", None)
    for switch in ("DKT_DIRICHLET_LOWRANK", "DKT_LOO_LOWRANK"):
        monkeypatch.delenv(switch, raising=False)
    monkeypatch.setattr(ops, "_episode", lambda *a, **k: pytest.fail("an episode call was made"))
    m = dkt_amd.DKT(dkt_amd.backbone.Conv4S, n_way=5, n_support=1, kernel_type=kernel, **kw)
    rows, y = torch.randn(n, 64), torch.ones(c, n)
    for loss in (m._episode_loss, m._episode_loss_from_trunk):
        with pytest.raises(ValueError) as exc:
            loss(rows, y)
        assert str(exc.value) == message
