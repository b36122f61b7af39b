"""Every model-level route (tests/model_routes.py: DKT's training step, its test episodes, its two loops, the regression losses) makes exactly the library
launches it is known to make: the kernels in order of first launch, each with its count, read from ops.kernel_timing.  A route that grows a launch, loses one
or reorders two fails here; so does one whose outputs, gradients or printed lines go missing."""
import pytest
import torch

import model_routes as mr

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("route", mr.ROUTES, ids=lambda r: r.name)
def test_route_launches_exactly_these_kernels_this_often_in_this_order(route, cuda):
    got = mr.run(route, cuda, launches=True)
    print(route.name, got["launches"], sorted(got["outs"]), repr(got["stdout"]))
    assert got["launches"] == route.launches
    assert got["outs"] and got["state"] and all(torch.isfinite(t.float()).all() for t in list(got["outs"].values()) + list(got["grads"].values()))
    if route.name.startswith(("train-", "regression-", "correct-adapt", "correct-bernoulli-adapt", "loops/train")):
        assert got["grads"]
    if "info" in got["outs"]:
        assert int(got["outs"]["info"].abs().max().item()) == 0
    if route.name.startswith("logits/"):          # the arg-max of get_logits' posterior means is the label _correct_device counts
        y_q = torch.arange(5, device=cuda).repeat_interleave(3)
        assert float((got["outs"]["logits"].argmax(1) == y_q).sum().item()) == float(got["outs"]["stats"][0].item())
        assert float(got["outs"]["stats"][1].item()) == 0.0
    if route.name.startswith("loops/"):
        lines = got["stdout"].splitlines()
        assert ([ln.split(" | ")[0] for ln in lines] == ["Epoch [0] [0/4]", "Epoch [0] [2/4]"] if "train" in route.name
                else lines[0].startswith("Test | Batch 0/3 | Loss 0.000000 | Acc ") and lines[1].startswith("3 Test Acc = "))
