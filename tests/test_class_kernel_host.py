"""CPU-side checks of the class-kernel restatement (tests/class_kernel_model.py): the closed forms are the gradient float64 autograd gives, the float32
restatement of the three backward kernels and of the forward stays inside the derived bounds on every case of the GPU lists (so the inputs leave the
reference alone inside its bound), the route table restates the library's dispatch, and each of the mistakes the bounds are meant to catch lands outside them."""
import numpy as np
import pytest
import torch

import class_kernel_model as cm

BWD = cm.bwd_cases()
_ids = lambda v: "%s" % (v,)          # noqa: E731


def _gpytorch_maps(base, kind, param):
    """The semantics of `_class_kernel_ref` of tests/test_gpu_parity.py (gpytorch RBFKernel / MaternKernel(nu = 2.5) / PolynomialKernel), with the clamp."""
    p = param.reshape(-1, 1, 1)
    if cm.is_poly(kind):
        return (base.unsqueeze(0) + p) ** cm.power_of(kind)
    u = base.unsqueeze(0) / p ** 2
    if kind == "rbf":
        return torch.exp(-0.5 * u)
    r = torch.sqrt(5.0 * u.clamp_min(1e-30))
    return (1.0 + r + r * r / 3.0) * torch.exp(-r)


AUTOGRAD_SHAPES = [s for s in cm.BWD_SHAPES if s[0] * s[1] * s[2] * s[2] <= 700000] + [(127, 2, 65)]


@pytest.mark.parametrize("shape", AUTOGRAD_SHAPES, ids=_ids)
@pytest.mark.parametrize("kind", cm.KINDS)
def test_closed_forms_are_the_gradient_float64_autograd_gives(kind, shape):
    """obj_b = sum_c <W_c, f(base_b; p_c)> with every entry of base an independent variable: G = d obj / d base, and A = G + G^T = 2 G for the symmetric
    W and base of the cases (d obj / d z_i = sum_j A_ij 2 (z_i - z_j) = 2 (Wp z)_i); poly: Wp = G.  Where base is exactly 0 the Matern clamp hands
    autograd a zero gradient while the closed form (and the kernel) take f'(0) = -5 / 6: such an entry multiplies z_i - z_j = 0, and on the diagonal it
    drops out of Wp, so there the closed form's own A is put in before the invariant combination diag(A 1) - A is compared."""
    c = cm.bwd_case(kind, *shape)
    ref = cm.reference(kind, c["w"], c["base"], c["p"])
    b, nc, n, _ = c["w"].shape
    idx = np.arange(n)
    for e in range(b):
        base = torch.tensor(c["base"][e].astype(np.float64), requires_grad=True)
        p = torch.tensor(c["p"].astype(np.float64), requires_grad=True)
        (torch.tensor(c["w"][e].astype(np.float64)) * _gpytorch_maps(base, kind, p)).sum().backward()
        g, dp = base.grad.numpy(), p.grad.numpy()
        assert np.isfinite(g).all() and np.isfinite(dp).all()
        if cm.is_poly(kind):
            wp = g
        else:
            a = 2.0 * g
            if kind == "matern":
                zero = c["base"][e] == 0
                assert (g[zero] == 0).all()
                a_closed = -ref["wp"][e]
                a = np.where(zero & ~np.eye(n, dtype=bool), a_closed, a)
            wp = -a
            wp[idx, idx] = a.sum(1) - a[idx, idx]
        scale = ref["off"][e] / cm.U32          # (the sum of the absolute terms, times a count)
        if not cm.is_poly(kind):
            scale[idx, idx] = ref["diag"][e] / cm.U32
        err = np.abs(ref["wp"][e] - wp)
        assert (err <= 1e-12 * scale).all(), (kind, shape, float((err / scale).max()))
        assert (np.abs(ref["dparam"][e] - dp) <= 1e-12 * ref["dparam_b"][e] / cm.U32).all(), (kind, shape)
    assert np.array_equal(ref["wp"], ref["wp"].transpose(0, 2, 1))
    assert np.abs(ref["parts"].sum(1) - ref["dparam"]).max() <= 1e-12 * np.abs(ref["parts"]).sum(1).max() + 1e-300


@pytest.mark.parametrize("kind, shape", BWD, ids=_ids)
def test_float32_restatement_of_the_backward_stays_inside_the_bounds(kind, shape):
    r = cm.bwd_reference(kind, shape)
    fr = r["f32"]
    name, ns, rp = cm.route(*shape)
    print("MEASURED class_kernel float32 numpy bwd %s %s [%s ns %d]: off %.3f diag %.3f dparam %.3f of the bound" % (kind, shape, name, ns, fr["off"], fr["diag"], fr["dparam"]))
    assert fr["finite"] and max(fr["off"], fr["diag"], fr["dparam"]) <= 1.0, fr
    wp = r["f32_out"][0]
    assert np.array_equal(wp, wp.transpose(0, 2, 1))


@pytest.mark.parametrize("shape", cm.FWD_SHAPES, ids=_ids)
@pytest.mark.parametrize("kind", cm.KINDS)
def test_float32_restatement_of_the_forward_stays_inside_the_bounds(kind, shape):
    for c in cm.FWD_C:
        case = cm.fwd_case(kind, shape, c)
        e64, bound = cm.forward_ref(kind, case["base"], case["p"])
        e32 = cm.forward_f32(kind, case["base"], case["p"])
        frac = float((np.abs(e32 - e64) / bound).max())
        print("MEASURED class_kernel float32 numpy fwd %s %s C %d: %.3f of the bound" % (kind, shape, c, frac))
        assert np.isfinite(e32).all() and frac <= 1.0
        if not cm.is_poly(kind):
            zero = np.broadcast_to((case["base"] == 0)[:, None], e32.shape)
            assert zero.any() and (e32[zero] == 1.0).all() and (e64[zero] == 1.0).all()
            if kind == "rbf" and c > 1 and case["base"].size > 1:          # l = 0.05: d2 / l^2 > 400, exp(-200) underflows: exact zeros, no NaN
                far = case["base"] > 1.0
                assert far.any() and (e32[:, 1][far] == 0).all()


def test_the_route_table_restates_the_dispatch(lib):
    names, splits = set(), set()
    for _, (b, c, n) in BWD:
        name, ns, rp = cm.route(b, c, n)
        names.add(name)
        splits.add(ns)
        assert ns == lib.dkt_class_kernel_bwd_nsplit(b, n), (b, n)
        assert rp * ns >= n and rp == -(-n // ns)
    for shape, ns in cm.SPLIT_SHAPES.items():
        assert cm.route(*shape)[1] == ns
    assert names == {"dword", "n128", "v4"} and splits == {1, 2, 4, 8, 16}
    assert all(cm.route(*s)[0] == "dword" for s in cm.BWD_DWORD) and all(cm.route(*s)[0] == "n128" for s in cm.BWD_N128)
    assert all(cm.route(*s)[0] == "v4" for s in cm.BWD_V4)
    assert cm.has_empty_split(1, 1, 129) and cm.has_empty_split(1, 5, 131) and not cm.has_empty_split(1, 4, 256)
    assert [n for n in range(1, 145) if cm.has_empty_split(1, 1, n)] == list(range(129, 136))          # (the first N with an empty sixteenth split)
    assert (cm.route(1, 3, 15)[1], cm.route(1, 3, 16)[1]) == (1, 2)
    for b in range(1, 300):
        for n in (1, 15, 16, 31, 32, 65, 127, 128, 129, 255, 256, 257, 513):
            assert cm.nsplit(b, n) == lib.dkt_class_kernel_bwd_nsplit(b, n)
    # every thread's chain of additions is far below N^2
    assert cm.chain_length(1, 2, 513) == 5 * 9 + 6 + 3 + 16 and cm.chain_length(256, 2, 65) == 9 * 8 + 6 + 3 + 1


def test_the_case_inputs_hold_their_edges():
    c = cm.bwd_case("rbf", 1, 5, 131)
    base, w, p = c["base"][0], c["w"][0], c["p"]
    off = ~np.eye(131, dtype=bool)
    assert (np.diag(base) == 0).all() and (base[off] == 0).sum() >= 4 and 0.1 < np.median(base[off]) < 2.0
    assert len(set(p.tolist())) == 5 and p.min() == np.float32(0.05) and p.max() == np.float32(30.0)
    assert (base[off] / p.min() ** 2).max() > 300.0                         # exp(-u / 2) underflows
    inner = np.abs(w[0][:60, :60][~np.eye(60, dtype=bool)]).mean()
    assert 10 * inner < np.abs(w[0][:60, 128:]).mean() and 10 * inner < np.abs(np.diag(w[0])).mean() and 10 * inner < np.abs(w[4][:60, :60]).mean()
    assert 10 * inner < np.abs(w[0][:60, 63:66]).mean()
    first, end = cm.last_split_rows(1, 5, 131)
    assert 10 * inner < np.abs(w[0][first:end, :60]).mean()
    g = cm.bwd_case("poli2", 1, 5, 131)
    t = g["base"][0][None] + g["p"].reshape(-1, 1, 1)
    assert (g["p"] < 0).any() and ((t[1] < 0).any() and (t[1] > 0).any())


# ---- the mistakes the bounds must catch -------------------------------------------------------------------------------------------------------------
def _can_show(defect, kind, shape):
    """The cases of the list a mistake can change at all (its route, its kinds); of those, the ones up to 1.2 M elements of W -- the larger cases of a
    route show nothing its smaller ones do not."""
    b, c, n = shape
    name, ns, _ = cm.route(b, c, n)
    if b * c * n * n > 1200000:
        return False
    if defect in ("v4-tail-not-masked", "last-class-group-dropped", "second-column-group-dropped"):
        return name == "v4"
    if defect == "no-diagonal-from-row-64":
        return name == "n128" and not cm.is_poly(kind)
    if defect in ("last-split-rows-lost", "dparam-parts-transposed"):
        return ns > 1
    if defect == "diagonal-keeps-a_ii":
        return not cm.is_poly(kind)
    return dict([("-2u/p^2", not cm.is_poly(kind)), ("poli2-f'=t", kind == "poli2"), ("no-matern-clamp", kind == "matern")]).get(defect, True)


@pytest.mark.parametrize("defect", cm.DEFECTS)
def test_the_bounds_discriminate(defect):
    """Each mistake, injected into the float64 closed form, leaves a bound by a factor of at least 10 on at least one case of the GPU list; the missing
    Matern clamp (f' through the square root at u = 0: 0 . inf) is caught by the finiteness verdict."""
    worst, where, not_finite = 0.0, None, 0
    for kind, shape in BWD:
        if not _can_show(defect, kind, shape):
            continue
        r = cm.bwd_reference(kind, shape)
        c = r["case"]
        m = cm.reference(kind, c["w"], c["base"], c["p"], defect)
        fr = cm.fractions(kind, m["wp"], m["dparam"], r["ref"])
        not_finite += not fr["finite"]
        ratio = max(fr["off"], fr["diag"], fr["dparam"])
        if np.isfinite(ratio) and ratio > worst:
            worst, where = ratio, (kind, shape)
    if defect == "no-matern-clamp":
        print("defect %s: not finite on %d cases" % (defect, not_finite))
        assert not_finite > 0
    else:
        print("defect %s: worst %.3g x the bound at %s" % (defect, worst, where))
        assert worst >= 10.0 and not_finite == 0, (defect, worst)
