"""The per-class kernel maps and their chain rule on the GPU -- dkt_class_kernel_f32 and the three backward kernels of dkt_class_kernel_bwd_f32 at every route,
route boundary and split threshold -- against the float64 closed forms of tests/class_kernel_model.py, element by element inside the bounds derived there
(tests/test_class_kernel_host.py checks the closed forms against float64 autograd, holds the float32 restatement to the same bounds and shows that the
bounds tell the seeded mistakes from a correct kernel).  Every case prints a MEASURED line: the fraction of each bound the kernel uses, next to the float32
restatement's, the route and the number of row splits."""
import numpy as np
import pytest
import torch

import dkt_amd
import class_kernel_model as cm

pytestmark = pytest.mark.gpu
ops, L = dkt_amd.ops, dkt_amd._lib
MAPS = dict(rbf=(ops.CLASSMAP_RBF, 0), matern=(ops.CLASSMAP_MATERN25, 0), poli1=(ops.CLASSMAP_POLY, 1), poli2=(ops.CLASSMAP_POLY, 2))
_ids = lambda v: "%s" % (v,)          # noqa: E731


def _on_product_library():
    assert ops._lib_now()._name == L.LIB_PATH


def _t(a, cuda):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=cuda)


# ---- the backward ---------------------------------------------------------------------------------------------------------------------------------------
def _check_backward(kind, shape, cuda):
    b, c, n = shape
    r = cm.bwd_reference(kind, shape)
    case, ref, f32 = r["case"], r["ref"], r["f32"]
    name, ns, rp = cm.route(b, c, n)
    w, base, p = _t(case["w"], cuda), _t(case["base"], cuda), _t(case["p"], cuda)
    _on_product_library()
    assert ns == int(ops._lib_now().dkt_class_kernel_bwd_nsplit(b, n))
    wp, dp = ops.class_kernel_bwd(w, base, *MAPS[kind], p)
    _on_product_library()
    wp2, dp2 = ops.class_kernel_bwd(w, base, *MAPS[kind], p)
    assert wp.shape == (b, n, n) and dp.shape == (b, c)
    again = torch.equal(wp, wp2) and torch.equal(dp, dp2)
    wp, dp = wp.cpu().numpy(), dp.cpu().numpy()
    fr = cm.fractions(kind, wp, dp, ref)
    print("MEASURED class_kernel bwd %s B %d C %d N %d [%s ns %d x %d rows%s]: kernel off %.3f diag %.3f dparam %.3f of the bound; float32 numpy off %.3f diag %.3f dparam %.3f" % (
        kind, b, c, n, name, ns, rp, ", last split empty" if cm.has_empty_split(b, c, n) else "", fr["off"], fr["diag"], fr["dparam"], f32["off"], f32["diag"], f32["dparam"]))
    assert fr["finite"], (kind, shape)
    assert fr["off"] <= 1.0 and fr["diag"] <= 1.0 and fr["dparam"] <= 1.0, (kind, shape, fr)
    assert np.array_equal(wp, wp.transpose(0, 2, 1)), (kind, shape)          # (both triangles run the same operations on bitwise equal inputs)
    assert again, (kind, shape)
    return ns


@pytest.mark.parametrize("shape", cm.BWD_SHAPES, ids=_ids)
@pytest.mark.parametrize("kind", cm.KINDS)
def test_backward_matches_float64_at_every_route(kind, shape, cuda):
    """Wp off the diagonal, Wp on the diagonal and dparam[b, c] element by element inside the derived bounds; every value finite (the smallest lengthscale
    underflows exp: a zero term, not a NaN); Wp bitwise symmetric; a second call bitwise the same.  The shapes are the routes' first, last and odd sizes:
    dword up to N = 64, at C = 9 up to N = 128 and at N = 513; n128 at N = 65 (one live column in the second half), 127, 128 and C = 1, 8; v4 at
    N % 4 in {1, 2, 3, 0}, C % 4 in {1, 2, 3, 0}, one and two column groups (257: one live column in the second), an empty last split (129, 131) and the
    largest episode of the product (447)."""
    _check_backward(kind, shape, cuda)


@pytest.mark.parametrize("shape", list(cm.SPLIT_SHAPES), ids=_ids)
@pytest.mark.parametrize("kind", cm.SPLIT_KINDS)
def test_backward_at_the_thresholds_of_the_row_split(kind, shape, cuda):
    """B in {127, 128, 255, 256} at C = 2, N = 65: 4, 2, 2 and 1 splits of the rows (B ns < 256)."""
    assert _check_backward(kind, shape, cuda) == cm.SPLIT_SHAPES[shape]


# ---- the forward ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", cm.FWD_SHAPES, ids=_ids)
@pytest.mark.parametrize("kind", cm.KINDS)
def test_forward_matches_float64_element_by_element(kind, shape, cuda):
    """E[b, c] = f(base[b]; p_c) at NN in {1, 255, 256, 257} (the edges of the 256-thread blocks), a [2, 7, 33] cross base and a [1, 513, 513] one, C in
    {1, 5, 32} with a different parameter per class (a wrong class stride puts another class's values where the bound does not reach); RBF and Matern are
    exactly 1 where base is exactly 0."""
    for c in cm.FWD_C:
        case = cm.fwd_case(kind, shape, c)
        e64, bound = cm.forward_ref(kind, case["base"], case["p"])
        e32 = cm.forward_f32(kind, case["base"], case["p"])
        _on_product_library()
        e = ops.class_kernel(_t(case["base"], cuda), *MAPS[kind], _t(case["p"], cuda))
        assert e.shape == (shape[0], c) + tuple(shape[1:])
        e = e.cpu().numpy()
        frac, f32 = float((np.abs(e - e64) / bound).max()), float((np.abs(e32 - e64) / bound).max())
        print("MEASURED class_kernel fwd %s base %s C %d: kernel %.3f of the bound; float32 numpy %.3f" % (kind, shape, c, frac, f32))
        assert np.isfinite(e).all() and frac <= 1.0, (kind, shape, c, frac)
        if c > 1 and case["base"].size > 1:          # the classes differ by far more than the bound: the stride is visible
            assert (np.abs(e64[:, 0] - e64[:, 1]) > 100.0 * (bound[:, 0] + bound[:, 1])).any()
        if not cm.is_poly(kind):
            zero = np.broadcast_to((case["base"] == 0)[:, None], e.shape)
            assert zero.any() and (e[zero] == 1.0).all()


# ---- argument checks --------------------------------------------------------------------------------------------------------------------------------------
def _status_and_outputs(call, outs):
    """(status of a direct library call, whether every output still holds its fill)."""
    for o in outs:
        o.fill_(-7.0)
    _on_product_library()
    st = call(ops._lib_now())
    torch.cuda.synchronize()
    return st, all(bool((o == -7.0).all()) for o in outs)


def test_sizes_beyond_the_limits_are_refused_without_a_launch(cuda):
    """C = 33 in the backward and B = 65536 in the forward: DKT_ERR_TOO_LARGE; power = 3: DKT_ERR_BAD_ARG; no output changes; ops raises with the status."""
    too_large, bad_arg = -2, -1
    assert L.STATUS[too_large] == "DKT_ERR_TOO_LARGE" and L.STATUS[bad_arg] == "DKT_ERR_BAD_ARG"
    ok = lambda *s: torch.ones(s, device=cuda)                     # noqa: E731
    p, st = ops._p, ops._stream
    w, base, par, wp, dpar = ok(1, 33, 7, 7), ok(1, 7, 7), ok(33), ok(1, 7, 7), ok(1, 33)
    assert _status_and_outputs(lambda lib: lib.dkt_class_kernel_bwd_f32(p(w), p(base), ops.CLASSMAP_RBF, p(par), 0, p(wp), p(dpar), 1, 33, 7, st()), (wp, dpar)) == (too_large, True)
    with pytest.raises(RuntimeError, match="DKT_ERR_TOO_LARGE"):
        ops.class_kernel_bwd(w, base, ops.CLASSMAP_RBF, 0, par)
    w3, par3, dpar3, e3 = ok(1, 3, 7, 7), ok(3), ok(1, 3), ok(1, 3, 7, 7)
    assert _status_and_outputs(lambda lib: lib.dkt_class_kernel_bwd_f32(p(w3), p(base), ops.CLASSMAP_POLY, p(par3), 3, p(wp), p(dpar3), 1, 3, 7, st()), (wp, dpar3)) == (bad_arg, True)
    assert _status_and_outputs(lambda lib: lib.dkt_class_kernel_f32(p(base), ops.CLASSMAP_POLY, p(par3), 3, p(e3), 1, 3, 49, st()), (e3,)) == (bad_arg, True)
    with pytest.raises(RuntimeError, match="DKT_ERR_BAD_ARG"):
        ops.class_kernel_bwd(w3, base, ops.CLASSMAP_POLY, 3, par3)
    with pytest.raises(RuntimeError, match="DKT_ERR_BAD_ARG"):
        ops.class_kernel(base, ops.CLASSMAP_POLY, 3, par3)
    big, ebig = ok(65536, 1), ok(65536, 3, 1)
    assert _status_and_outputs(lambda lib: lib.dkt_class_kernel_f32(p(big), ops.CLASSMAP_RBF, p(par3), 0, p(ebig), 65536, 3, 1, st()), (ebig,)) == (too_large, True)
    with pytest.raises(RuntimeError, match="DKT_ERR_TOO_LARGE"):
        ops.class_kernel(big, ops.CLASSMAP_RBF, 0, par3)
    e = ops.class_kernel(big[:65535], ops.CLASSMAP_RBF, 0, par3)          # the largest batch the grid takes
    e64, bound = cm.forward_ref("rbf", np.ones((1, 1), np.float32), np.ones(3, np.float32))
    assert e.shape == (65535, 3, 1) and (np.abs(e.cpu().numpy() - e64) <= bound).all()


def test_shape_checks_raise_before_any_launch(cuda, monkeypatch):
    """A base or a param that does not match w, or a w that is not square, never reaches the library (the kernels would read past the smaller operand)."""
    def no_library(*a, **k):
        raise AssertionError("the call reached the library")

    monkeypatch.setattr(ops, "_lib_now", no_library)
    ok = lambda *s: torch.ones(s, device=cuda)                     # noqa: E731
    for w, base, par in ((ok(2, 3, 7, 7), ok(2, 6, 6), ok(3)),          # a smaller base
                         (ok(2, 3, 7, 7), ok(2, 8, 8), ok(3)),
                         (ok(2, 3, 7, 7), ok(1, 7, 7), ok(3)),          # fewer episodes in base
                         (ok(2, 3, 7, 7), ok(2, 7, 5), ok(3)),          # not square
                         (ok(2, 3, 7, 5), ok(2, 7, 7), ok(3)),
                         (ok(2, 3, 7, 7), ok(2, 7, 7), ok(2)),          # fewer parameters than classes
                         (ok(2, 3, 7, 7), ok(2, 7, 7), ok(4)),
                         (ok(2, 3, 7, 7), ok(2, 7, 7), ok(1)),
                         (ok(3, 7, 7), ok(3, 7, 7), ok(3))):             # no class axis
        with pytest.raises(RuntimeError):
            ops.class_kernel_bwd(w, base, ops.CLASSMAP_RBF, 0, par)
    monkeypatch.undo()
    wp, dpar = ops.class_kernel_bwd(ok(2, 3, 7, 7), ok(2, 7, 7), ops.CLASSMAP_RBF, 0, ok(3, 1))          # [C, 1] is C parameters
    assert wp.shape == (2, 7, 7) and dpar.shape == (2, 3)
