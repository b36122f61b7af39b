"""The distance-kernel backward on the GPU -- dkt_rbf_bwd_f32 / dkt_sqdist_bwd_f32 alone, and the chain gram(RBF | SQDIST) -> ... -> rbf_bwd | sqdist_bwd ->
gram_bwd(Wp, z) under autograd at every pair of forward and backward route -- against the float64 restatement of tests/distance_bwd_model.py
(tests/test_distance_bwd_host.py checks that one against float64 autograd, holds its float32 restatement to the same bounds and shows that the bounds
tell the seeded mistakes from a correct kernel).  Every case prints a MEASURED line: the fraction of its bound the kernel uses, next to the float32
restatement's."""
import numpy as np
import pytest
import torch

import dkt_amd
import distance_bwd_model as dm

pytestmark = pytest.mark.gpu
ops, L = dkt_amd.ops, dkt_amd._lib


def _on_product_library():
    assert ops._lib_now()._name == L.LIB_PATH


def _t(a, cuda):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=cuda)


# ---- (a) the two kernels alone ------------------------------------------------------------------------------------------------------------------------
def _run_kernel(c, cuda):
    fn = ops.rbf_bwd if c["kind"] == "rbf" else ops.sqdist_bwd
    wp, dl = fn(_t(c["w"], cuda), _t(c["m"], cuda), _t([c["l"]], cuda))
    return wp.cpu().numpy(), dl.cpu().numpy()


def _check_kernel(name, c, cuda):
    wp, dl = _run_kernel(c, cuda)
    fr = dm.fractions(c["kind"], wp, dl, c["w"], c["m"], c["l"])
    f32 = dm.fractions(c["kind"], *dm._bwd_f32(c["kind"], c["w"], c["m"], c["l"]), c["w"], c["m"], c["l"])
    print("MEASURED distance_bwd %s: kernel off %.3f diag %.3f rowsum %.3f dl %.3f of the bound; float32 numpy off %.3f diag %.3f rowsum %.3f dl %.3f" % (
        name, fr["off"], fr["diag"], fr["rowsum"], fr["dl"], f32["off"], f32["diag"], f32["rowsum"], f32["dl"]))
    assert wp.shape == c["w"].shape and dl.shape == (c["w"].shape[0],)
    assert fr["finite"], name
    assert fr["off"] <= 1.0 and fr["diag"] <= 1.0 and fr["rowsum"] <= 1.0 and fr["dl"] <= 1.0, (name, fr)
    assert np.array_equal(wp, wp.transpose(0, 2, 1)), name          # (both triangles round the same commutative operations)


@pytest.mark.parametrize("n", dm.KERNEL_N)
@pytest.mark.parametrize("kind", ["rbf", "sqdist"])
def test_kernel_alone_matches_float64(kind, n, cuda):
    """Wp element-wise (off-diagonal and diagonal separately), |Wp 1| and dl[b] per episode inside the derived bounds, B in {1, 3}, l in {0.05, 1.1, 30}:
    one row per thread up to N = 256, two or three from 257 on; a few non-zero partials in block_sum_256 (N < 64) and all of them."""
    _on_product_library()
    for b in dm.KERNEL_B:
        for l in dm.KERNEL_L:
            _check_kernel("%s-n%d-b%d-l%g" % (kind, n, b, l), dm.kernel_case(kind, n, b, l), cuda)


@pytest.mark.parametrize("n", dm.EDGE_N)
def test_rbf_kernel_on_zero_denormal_unit_and_near_unit_entries(n, cuda):
    """E with off-diagonal entries exactly 0 (0 ln 0 := 0: the `e > 0` guard), one subnormal entry, off-diagonal entries exactly 1 (duplicate rows), and a
    whole episode in [1 - 1e-4, 1]: finite, and inside the same bounds -- which are relative to the GIVEN fp32 E (what rounding E itself costs
    dlengthscale is measured by test_small_distance_regime_of_dlengthscale)."""
    _on_product_library()
    for l in dm.KERNEL_L:
        _check_kernel("rbf-edge-n%d-l%g" % (n, l), dm.edge_case(n, l), cuda)


# ---- (b) the chain through autograd -----------------------------------------------------------------------------------------------------------------------
def _chain_gpu(inp, kernel, per_class, cuda, need_z=True, need_l=True):
    z = _t(inp["z"], cuda).requires_grad_(need_z)
    l = _t(inp["l"], cuda).requires_grad_(need_l)
    e = ops.base_matrix_per_class(z, kernel, l) if per_class else ops.base_matrix(z, kernel, l)
    assert e.shape == tuple(inp["g"].shape)
    (_t(inp["g"], cuda) * e).sum().backward()
    return z.grad, l.grad


@pytest.mark.parametrize("kernel, per_class", dm.CHAIN_VARIANTS, ids=lambda v: {True: "per-class", False: "shared"}.get(v, v))
@pytest.mark.parametrize("shape", list(dm.CHAIN_SHAPES), ids=str)
def test_chain_matches_float64_autograd(shape, kernel, per_class, cuda):
    """dz and dlengthscale of sum G o K(z, l), G random and not symmetric, against float64 autograd through the oracle's base_matrix; the route each shape
    takes is stated in distance_bwd_model.CHAIN_SHAPES.  GRAD_RTOL is the hard ceiling; 4 x the error of the float32 CPU autograd of the same formula
    (floor 1e-6) allows another summation order, not another formula.  Then the two identities on the kernels' own output."""
    _on_product_library()
    r = dm.chain_reference(shape, kernel, per_class)
    inp = r["inp"]
    dz, dl = _chain_gpu(inp, kernel, per_class, cuda)
    assert dz.shape == tuple(inp["z"].shape) and dl.shape == tuple(inp["l"].shape)
    dz, dl = dz.double().cpu().numpy(), dl.double().cpu().numpy()
    assert np.isfinite(dz).all() and np.isfinite(dl).all()
    ez, el = dm.rel_l2(dz, r["dz64"]), dm.rel_l2(dl, r["dl64"])
    i1, i1_dz, i2 = dm.identity_residuals(inp["z"], inp["l"], dz, dl, r["terms"])
    f1, f1_dz, f2 = dm.identity_residuals(inp["z"], inp["l"], r["dz32"], r["dl32"], r["terms"])
    print("MEASURED distance_chain %s %s%s [%s | %s]: dz %.3g (float32 cpu %.3g) dl %.3g (float32 cpu %.3g) identities %.3f %.3f of the bound (float32 cpu %.3f %.3f); "
          "sum_i dz_i over N u sum |dz| %.3f (float32 cpu %.3f)" % (
              shape, kernel, "/class" if per_class else "", *dm.CHAIN_SHAPES[shape], ez, r["e32_dz"], el, r["e32_dl"], i1, i2, f1, f2, i1_dz, f1_dz))
    assert ez < dm.GRAD_RTOL and el < dm.GRAD_RTOL, (ez, el)
    assert ez <= dm.FLOOR_MARGIN * max(r["e32_dz"], dm.FLOOR_MIN), (ez, r["e32_dz"])
    assert el <= dm.FLOOR_MARGIN * max(r["e32_dl"], dm.FLOOR_MIN), (el, r["e32_dl"])
    assert i1 <= 1.0 and i2 <= 1.0, (i1, i2)


@pytest.mark.parametrize("kernel, per_class", dm.CHAIN_VARIANTS, ids=lambda v: {True: "per-class", False: "shared"}.get(v, v))
@pytest.mark.parametrize("shape", [(3, 19, 2916), (2, 33, 64), (64, 65, 64), (1, 257, 30)], ids=str)
def test_needs_input_grad_is_honoured(shape, kernel, per_class, cuda):
    """Only z, or only l, requiring a gradient: the other one is None and the one returned is bitwise what the call with both returns."""
    inp = dm.chain_reference(shape, kernel, per_class)["inp"]
    dz, dl = _chain_gpu(inp, kernel, per_class, cuda)
    dz_only, none_l = _chain_gpu(inp, kernel, per_class, cuda, need_l=False)
    none_z, dl_only = _chain_gpu(inp, kernel, per_class, cuda, need_z=False)
    assert none_l is None and none_z is None
    assert torch.equal(dz, dz_only) and torch.equal(dl, dl_only)


# ---- (c) the small-distance regime of dlengthscale ---------------------------------------------------------------------------------------------------------
def _dl_errors(inp, cuda):
    """(kernel, float32 restatement of its formula on the E the kernel was given, float32 dl = -<z - r, dz> / l): relative errors against float64; max d2 / l^2."""
    e = ops.gram(_t(inp["z"], cuda), None, ops.KERNEL_RBF, _t(inp["l"], cuda))          # the forward base_matrix runs: the E rbf_bwd_kernel is handed
    d = dm.dl_three_ways(inp, e.cpu().numpy())
    _, dl = _chain_gpu(inp, "rbf", False, cuda)
    rel = lambda v: abs(float(v) - d["ref"]) / abs(d["ref"])          # noqa: E731
    return rel(dl.double().item()), rel(d["formula32"]), rel(d["homog32"]), d["umax"]


@pytest.mark.parametrize("target", dm.SMALL_TARGETS)
@pytest.mark.parametrize("shape", dm.SMALL_SHAPES, ids=str)
def test_small_distance_regime_of_dlengthscale(shape, target, cuda):
    """rbf_bwd_kernel rebuilds d2 / l^2 as -2 logf(E) from the ROUNDED E: at 1 - u / 2 the fp32 steps of E are 6e-8, so the smaller every u is, the fewer of
    its bits survive.  Measured (docs/MEASUREMENTS.md R15): relative error of dlengthscale 1e-7 .. 1e-6 at max d2 / l^2 = 1, 3e-6 .. 5e-5 at 1e-2,
    1e-3 .. 4e-3 at 1e-4 and 4e-3 .. 0.14 at 1e-6, while dl = -<z - r, dz> / l keeps 1e-7 .. 1e-6 throughout.  Asserted: the kernel is no worse than 4 x
    the float32 restatement of its own formula on the E it was handed (the two agree to three digits: the loss is the formula's)."""
    _on_product_library()
    ek, ef, eh, umax = _dl_errors(dm.small_distance_case(shape, target), cuda)
    print("MEASURED small_distance %s max d2/l2 %.0e (fp32 forward: %.3g): kernel %.3e formula float32 %.3e homogeneity float32 %.3e" % (shape, target, umax, ek, ef, eh))
    assert ek <= dm.FLOOR_MARGIN * ef, (ek, ef)


def test_dlengthscale_at_the_scale_of_the_qmul_fixture(cuda):
    """Features of make_golden.cfg0_features with the fixture's lengthscale (largest d2 / l^2 ~ 2.3): the formula is nowhere near its small-distance regime."""
    _on_product_library()
    ek, ef, eh, umax = _dl_errors(dm.qmul_case(), cuda)
    print("MEASURED small_distance qmul fixture (max d2/l2 %.3g): kernel %.3e formula float32 %.3e homogeneity float32 %.3e" % (umax, ek, ef, eh))
    assert ek < dm.GRAD_RTOL, ek


# ---- (d) argument checks: nothing reaches the library ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn", ["rbf_bwd", "sqdist_bwd"])
def test_argument_checks_raise_before_any_launch(fn, cuda, monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("the call reached the library")

    monkeypatch.setattr(ops, "_lib_now", no_library)
    f = getattr(ops, fn)
    ok = lambda *s: torch.ones(s, device=cuda)                     # noqa: E731
    one = ok(1)
    for w, m, l in ((ok(2, 6, 6), ok(2, 7, 7), one),                # a smaller w: the kernel would read past its end
                    (ok(1, 7, 7), ok(2, 7, 7), one),                # fewer episodes in w
                    (ok(2, 8, 8), ok(2, 7, 7), one),
                    (ok(2, 7, 5), ok(2, 7, 5), one),                # not square
                    (ok(2, 5, 7), ok(2, 5, 7), one),
                    (ok(2, 7, 7), ok(2, 7, 7), ok(3)),              # a [C] lengthscale would silently mean class 0
                    (ok(2, 7, 7), ok(2, 7, 7), ok(2, 1)),
                    (ok(2, 7, 7), ok(2, 7, 7), ok(0))):
        with pytest.raises(RuntimeError):
            f(w, m, l)
    monkeypatch.undo()
    wp, dl = f(ok(2, 7, 7), ok(2, 7, 7), ok(1, 1))                   # one element of any shape is one lengthscale
    assert wp.shape == (2, 7, 7) and dl.shape == (2,)
