"""CPU-side checks of the front-end backward's restatement (tests/frontend_bwd_model.py): it is the true gradient (float64 torch.autograd), the float32
floors of every case group (the GPU tests allow the kernels 4 x these), the proof that 4 x the floor still tells a subtly wrong kernel from a right one,
and the condition on the inputs under which neither the F.normalize clamp nor the forward's fix-up flag is in play."""
import numpy as np
import pytest
import torch

import frontend_bwd_model as fm

MARGIN = 4.0


@pytest.fixture(scope="module")
def ref():
    return fm.build_reference()


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("mode, scaled, n, d", [("train", False, 25, 64), ("train", True, 33, 36), ("eval-shared", True, 17, 20), ("eval-episode", False, 48, 68),
                                                ("train", False, 2, 8)], ids=str)
def test_the_restatement_is_the_gradient_float64_autograd_gives(mode, scaled, n, d):
    c = fm.make_case(n=n, d=d, b=3, mode=mode, scaled=scaled, seed=n + d, rounded=False)
    got = fm.run(c)
    x = torch.tensor(c["x"], requires_grad=True)
    gamma, beta = torch.tensor(c["gamma"], requires_grad=True), torch.tensor(c["beta"], requires_grad=True)
    total = 0.0
    for b in range(3):
        if mode == "train":
            y = torch.nn.functional.batch_norm(x[b], None, None, gamma, beta, True, 0.1, fm.EPS)
        else:
            a, s = (torch.tensor(v if v.ndim == 1 else v[b]) for v in (c["a"], c["s"]))
            y = a * x[b] + s
        zn = torch.nn.functional.normalize(y, p=2, dim=1)
        total = total + (1.0 if c["g"] is None else float(c["g"][b])) * (torch.tensor(c["w"][b]) * (zn @ zn.T)).sum()
    total.backward()
    dx = np.stack([o["dx"] for o in got])
    # (two rows: xh = +-(1 - eps / var), dX is what a cancellation by ~ 1e-5 leaves of dY, and so is its float64 rounding error)
    assert _rel(dx, x.grad.numpy()) < (1e-10 if n > 2 else 1e-10 * 1e5)
    if mode == "train":
        assert _rel(sum(o["dbeta"] for o in got), beta.grad.numpy()) < 1e-10 and _rel(sum(o["dgamma"] for o in got), gamma.grad.numpy()) < 1e-10
    else:
        assert all(o["dgamma"] is None and o["dbeta"] is None for o in got)


@pytest.mark.parametrize("mode, n, d", [("train", 40, 36), ("eval-shared", 33, 12), ("eval-episode", 161, 8)], ids=str)
def test_the_streaming_restatement_is_the_gradient_float64_autograd_gives(mode, n, d):
    c = fm.make_case(call="stream", n=n, d=d, b=2, mode=mode, seed=n, rounded=False)
    got = fm.run(c)
    x = torch.tensor(c["x"], requires_grad=True)
    gamma, beta = torch.tensor(c["gamma"], requires_grad=True), torch.tensor(c["beta"], requires_grad=True)
    total = 0.0
    for b in range(2):
        if mode == "train":
            y = torch.nn.functional.batch_norm(x[b], None, None, gamma, beta, True, 0.1, fm.EPS)
        else:
            a, s = (torch.tensor(v if v.ndim == 1 else v[b]) for v in (c["a"], c["s"]))
            y = a * x[b] + s
        total = total + (torch.tensor(c["dzn"][b]) * torch.nn.functional.normalize(y, p=2, dim=1)).sum()
    total.backward()
    assert _rel(np.stack([o["dx"] for o in got]), x.grad.numpy()) < 1e-10
    if mode == "train":
        assert _rel(sum(o["dbeta"] for o in got), beta.grad.numpy()) < 1e-10 and _rel(sum(o["dgamma"] for o in got), gamma.grad.numpy()) < 1e-10


def test_float32_floors_per_group(ref):
    """The floors docs/FRONTEND_BWD.md quotes: finite, above the fp32 unit roundoff wherever the reference is not identically zero, and -- outside the
    tiny-batch groups, whose dX is a cancellation remainder -- small enough that 4 x the floor is still a tight bound."""
    for group, fl in sorted(ref["e32"].items()):
        print("%-18s %3d cases  " % (group, sum(c["group"] == group for c in ref["cases"].values())) + "  ".join("e32[%s] = %.3g" % (q, v) for q, v in fl.items()))
        for q, v in fl.items():
            assert np.isfinite(v), (group, q, v)
            if "tiny" not in group:                        # (one row in train mode: dX and dgamma are identically zero, and so is their floor)
                assert 2.0 ** -26 < v < 1e-4, (group, q, v)


# which group each seeded defect is aimed at (frontend_bwd_model.backward / streaming_backward, `defect`)
DEFECTS = [("a", "tile-edges", "A = g W instead of g (W + W^T)"),
           ("a", "w-structure", "A = g W instead of g (W + W^T), triangular W"),
           ("b", "tile-edges", "the last row of a full tile dropped from the column sums"),
           ("c", "slab-edges", "the features of a partial 64-feature slab left at zero"),
           ("d", "tile-edges", "dgamma / dbeta of features 4k+1 and 4k+2 swapped"),
           ("d", "slab-edges", "dgamma / dbeta of features 4k+1 and 4k+2 swapped"),
           ("e", "tile-edges", "inv_n = 1 / NP instead of 1 / N"),
           ("e", "x16", "inv_n = 1 / NP instead of 1 / N"),
           ("f", "modes", "ep_scale ignored"),
           ("f", "w-structure", "ep_scale ignored"),
           ("g", "tile-edges", "pad columns [N, KP) contributing a nonzero Zn"),
           ("g", "slab-edges", "pad columns [N, KP) contributing a nonzero Zn"),
           ("b", "stream-rows", "streaming: the last row of a full 32-row trip dropped from the column sums"),
           ("c", "stream-slabs", "streaming: the features of a partial 32-feature slab left at zero"),
           ("e", "stream-rows", "streaming: inv_n = 1 / (rows rounded up to 32) instead of 1 / N"),
           ("d", "stream-x16", "streaming: dgamma / dbeta of features 4k+1 and 4k+2 swapped")]


@pytest.mark.parametrize("defect, group, what", DEFECTS, ids=lambda v: v if len(v) < 20 else "")
def test_the_tolerance_discriminates(ref, defect, group, what):
    """Each defect, injected into the float64 model, lands outside 4 x e32 of the group aimed at it on at least one of its cases: a kernel with that
    defect cannot pass the GPU test."""
    caught, worst = [], 0.0
    for k, c in ref["cases"].items():
        if c["group"] != group:
            continue
        err = fm.errors(fm.run(c, np.float64, defect), ref["r64"][k], group)
        ratio = max(err[q] / ref["e32"][group][q] for q in err)
        worst = max(worst, ratio)
        if ratio > MARGIN:
            caught.append(k)
    print("defect (%s) %s: caught on %d cases of %s, worst %.3g x e32" % (defect, what, len(caught), group, worst))
    assert caught, (defect, group, worst)


def test_the_16_bit_store_does_not_hide_a_defect(ref):
    """The x16 group's bound adds one unit in the last place of dX: the defects aimed at dX still land outside it."""
    for defect in ("a", "e", "g"):
        hit = False
        for k, c in ref["cases"].items():
            if c["group"] != "x16":
                continue
            for got, r in zip(fm.run(c, np.float64, defect), ref["r64"][k]):
                fi = torch.finfo(fm.XDTYPES[c["xdtype"]])
                ulp = np.maximum(fi.eps * np.exp2(np.floor(np.log2(np.maximum(np.abs(r["dx"]), fi.tiny)))), fi.tiny * fi.eps)
                hit = hit or bool((np.abs(got["dx"] - r["dx"]) > MARGIN * ref["e32"]["x16"]["dx"] * np.abs(r["dx"]).max() + ulp).any())
        assert hit, defect


def test_the_input_condition_holds_for_every_case(ref):
    """Every row has |y_i| >= 0.05 median |y_i| and no fp32 rnorm is near the 1e-12 clamp of F.normalize (rnorm = 1e12)."""
    worst = (np.inf, None)
    for k, c in ref["cases"].items():
        ratio, rmax = fm.input_condition(c)
        worst = min(worst, (ratio, k))
        assert ratio >= 0.05 and rmax < 1e6, (k, ratio, rmax)
    print("smallest |y_i| / median |y_i| over the case list: %.3g (%s)" % worst)


def test_the_case_list_reaches_every_fp32_instantiation_and_the_listed_16_bit_ones(ref):
    specs = ref["specs"]
    reached = {fm.instantiation(s) for s in specs.values() if s.get("call", "fused") == "fused"}
    for nt in range(1, 9):
        for train in (True, False):
            assert (nt, train, "f32") in reached, (nt, train)
    for xd in ("bf16", "f16"):
        for nt in (2, 3, 6, 7, 8):
            for train in (True, False):
                assert (nt, train, xd) in reached, (nt, train, xd)
    assert all(c["b"] in (2, 3) for c in ref["cases"].values())
