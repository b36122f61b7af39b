"""CPU-side checks of the distance-kernel backward's restatement (tests/distance_bwd_model.py): the closed forms are the gradient float64 autograd gives,
the float32 restatements stay inside the derived bounds on every case input (so the inputs leave the reference alone inside its bound), the two
identities the GPU test evaluates on the kernels' output hold in float64, the route table matches the launch conditions, and each of the mistakes the
bounds are meant to catch lands outside them."""
import numpy as np
import pytest
import torch

import distance_bwd_model as dm

CASES = dm.kernel_cases()


def _autograd(kind, w, m, l):
    """float64 autograd of sum W o exp(-d2 / 2 l^2) (rbf) or sum W o d2 / l^2 (sqdist) in d2 and l, d2 recovered from the case's E / U.
    -> (A = G + G^T with G = d obj / d d2: the kernels' A, dl [B])."""
    w, m, l = torch.tensor(np.asarray(w, np.float64)), np.asarray(m, np.float64), float(l)
    if kind == "rbf":         # (an entry that underflowed to 0: any d2 with exp(-d2 / 2 l^2) = 0 in float64)
        d2 = np.where(m > 0, -2.0 * l * l * np.log(np.where(m > 0, m, 1.0)), 4000.0 * l * l)
    else:
        d2 = m * l * l
    d2 = torch.tensor(d2, requires_grad=True)
    dls = []
    for b in range(w.shape[0]):
        lt = torch.tensor(l, dtype=torch.float64, requires_grad=True)
        k = torch.exp(-0.5 * d2[b] / lt ** 2) if kind == "rbf" else d2[b] / lt ** 2
        (w[b] * k).sum().backward()
        dls.append(float(lt.grad))
    g = d2.grad.numpy()          # G = d obj / d d2;  d obj / d z_i = sum_j (G_ij + G_ji) 2 (z_i - z_j) = 2 (Wp z)_i with Wp = diag(A 1) - A, A = G + G^T
    return g + g.transpose(0, 2, 1), np.array(dls)


@pytest.mark.parametrize("name", list(CASES))
def test_closed_forms_are_the_gradient_float64_autograd_gives(name):
    c = CASES[name]
    kind, w, m, l = c["kind"], c["w"], c["m"], c["l"]
    wp, dl = (dm.rbf_bwd_ref if kind == "rbf" else dm.sqdist_bwd_ref)(w, m, l)
    a, dl_ag = _autograd(kind, w, m, l)
    n = w.shape[-1]
    idx = np.arange(n)
    wp_ag = -a
    wp_ag[:, idx, idx] = a.sum(-1) - a[:, idx, idx]
    assert np.abs(wp - wp_ag).max() <= 1e-12 * max(np.abs(wp_ag).max(), 1e-300)
    ws = 0.5 * (w.astype(np.float64) + w.astype(np.float64).transpose(0, 2, 1))
    t = np.abs(ws * m * dm._neg2_log(m.astype(np.float64))) if kind == "rbf" else 2.0 * np.abs(ws * m)
    assert (np.abs(dl - dl_ag) <= 1e-12 * t.sum((1, 2)) / float(l)).all()
    assert np.array_equal(wp, wp.transpose(0, 2, 1))


def test_wp_is_the_matrix_gram_bwd_turns_into_dz():
    """dz = (Wp + Wp^T) z with the closed-form Wp, and dl, against float64 autograd of sum G o exp(-|z_i - z_j|^2 / 2 l^2) and sum G o |z_i - z_j|^2 / l^2 in z."""
    inp = dm.chain_inputs(3, 19, 30)
    z, l, g = inp["z"], float(inp["l"][0]), inp["g"]
    d2 = ((z[:, :, None, :] - z[:, None, :, :]) ** 2).sum(-1)
    for kind in ("rbf", "sqdist"):
        zt, lt = torch.tensor(z, requires_grad=True), torch.tensor(l, dtype=torch.float64, requires_grad=True)
        dt = ((zt[:, :, None, :] - zt[:, None, :, :]) ** 2).sum(-1)
        k = torch.exp(-0.5 * dt / lt ** 2) if kind == "rbf" else dt / lt ** 2
        (torch.tensor(g) * k).sum().backward()
        m = np.exp(-0.5 * d2 / l ** 2) if kind == "rbf" else d2 / l ** 2
        wp, dl = (dm.rbf_bwd_ref if kind == "rbf" else dm.sqdist_bwd_ref)(g, m, l)
        dz = (wp + wp.transpose(0, 2, 1)) @ z
        assert dm.rel_l2(dz, zt.grad.numpy()) < 1e-12 and abs(dl.sum() - float(lt.grad)) < 1e-12 * np.abs(dl).sum()


@pytest.mark.parametrize("name", list(CASES))
def test_float32_restatement_stays_inside_the_bounds(name):
    c = CASES[name]
    wp, dl = dm._bwd_f32(c["kind"], c["w"], c["m"], c["l"])
    fr = dm.fractions(c["kind"], wp, dl, c["w"], c["m"], c["l"])
    print("MEASURED distance_bwd float32 numpy %s: off %.3f diag %.3f rowsum %.3f dl %.3f of the bound" % (name, fr["off"], fr["diag"], fr["rowsum"], fr["dl"]))
    assert fr["finite"] and max(fr["off"], fr["diag"], fr["rowsum"], fr["dl"]) <= 1.0, fr


# ---- the mistakes the bounds must catch -------------------------------------------------------------------------------------------------------------
def _mutated(kind, w, m, l, defect):
    """The float64 closed form with one mistake: what a kernel with that mistake would return (up to its own rounding)."""
    w, m, l = np.asarray(w, np.float64), np.asarray(m, np.float64), float(l)
    b, n, _ = w.shape
    ws = w if defect == "no-symmetrisation" else 0.5 * (w + w.transpose(0, 2, 1))
    a = -ws * m / l ** 2 if kind == "rbf" else 2.0 * ws / l ** 2 + 0.0 * m
    idx = np.arange(n)
    wp = -a
    wp[:, idx, idx] = a.sum(-1) if defect == "diagonal-keeps-a_ii" else a.sum(-1) - a[:, idx, idx]
    if kind == "rbf":
        t = ws * m * (2.0 * (1.0 - m) if defect == "2(1-e)-for-the-logarithm" else dm._neg2_log(m))
    else:
        t = -2.0 * ws * m
    rows = t.sum(2)
    if defect == "stride-128":          # 256 threads striding by 128: every row from 128 on is visited by two threads
        rows[:, 128:] *= 2.0
    dl = rows.sum(1) / l
    if defect == "dl[0]-for-every-episode":          # every block writes dl[0] (say the last one wins); dl[1:] is never written (say it held zeros)
        dl = np.where(np.arange(b) == 0, dl[-1], 0.0)
    return wp, dl


DEFECTS = [("no-symmetrisation", "both"), ("dl[0]-for-every-episode", "both"), ("stride-128", "both"), ("diagonal-keeps-a_ii", "both"),
           ("2(1-e)-for-the-logarithm", "rbf")]


@pytest.mark.parametrize("defect, kinds", DEFECTS, ids=lambda v: v if "-" in v else "")
def test_the_bounds_discriminate(defect, kinds):
    """Each mistake, injected into the float64 closed form, leaves a bound by a factor of at least 10 on at least one case of the list (per kind)."""
    for kind in (("rbf", "sqdist") if kinds == "both" else (kinds,)):
        worst, caught = 0.0, []
        for name, c in CASES.items():
            if c["kind"] != kind or (defect == "dl[0]-for-every-episode" and c["w"].shape[0] == 1):
                continue
            wp, dl = _mutated(kind, c["w"], c["m"], c["l"], defect)
            fr = dm.fractions(kind, wp, dl, c["w"], c["m"], c["l"])
            ratio = max(fr["off"], fr["diag"], fr["dl"])
            worst = max(worst, ratio)
            if ratio > 10.0:
                caught.append(name)
        print("defect %s (%s): outside the bounds on %d cases, worst %.3g x the bound" % (defect, kind, len(caught), worst))
        assert caught, (defect, kind, worst)


# ---- the chain ------------------------------------------------------------------------------------------------------------------------------------
def test_the_route_table_matches_the_launch_conditions():
    want_fwd, want_bwd = set(), set()
    for shape, (fwd, bwd) in dm.CHAIN_SHAPES.items():
        f, b = dm.routes(*shape)
        assert fwd.startswith(f) and (bwd.startswith(b.split(" ")[0])) and (("bf16" in b) == ("bf16" in bwd)), (shape, f, b, fwd, bwd)
        want_fwd.add(f)
        want_bwd.add(b)
    pairs = {dm.routes(*s) for s in dm.CHAIN_SHAPES}
    assert want_fwd == {"small", "dist-ep", "generic"}
    assert {"small", "generic", "ep<5> exact", "ep<6> exact", "ep<7> exact", "ep<8> exact", "ep<7> bf16"} <= want_bwd
    for pair in (("small", "small"), ("generic", "generic"), ("dist-ep", "generic"), ("generic", "ep<7> exact"), ("dist-ep", "ep<5> exact"), ("dist-ep", "ep<7> bf16")):
        assert pair in pairs, pair
    assert any(n > 256 for _, n, _ in dm.CHAIN_SHAPES)


HOST_CHAIN = [s for s in dm.CHAIN_SHAPES if s[0] * s[1] * s[2] <= 200000]


@pytest.mark.parametrize("kernel, per_class", dm.CHAIN_VARIANTS, ids=str)
@pytest.mark.parametrize("shape", HOST_CHAIN, ids=str)
def test_the_two_identities_hold_in_float64(shape, kernel, per_class):
    """sum_i dz_i = 0 and sum_c l_c dl_c + <z - r, dz> = 0 on the float64 reference: residuals at the float64 rounding level, 2^-29 of the fp32 bound."""
    r = dm.chain_reference(shape, kernel, per_class)
    r1, r1_dz, r2 = dm.identity_residuals(r["inp"]["z"], r["inp"]["l"], r["dz64"], r["dl64"], r["terms"])
    assert r1 < 1e-6 and r1_dz < 1e-6 and r2 < 1e-6, (r1, r1_dz, r2)
    f1, f1_dz, f2 = dm.identity_residuals(r["inp"]["z"], r["inp"]["l"], r["dz32"], r["dl32"], r["terms"])
    assert f1 <= 1.0 and f2 <= 1.0, (f1, f1_dz, f2)              # the fp32 restatement of the chain stays inside both bounds
    assert (np.abs(r["dz64"]).sum(1) <= r["terms"] * (1.0 + 1e-9)).all()
    assert np.isfinite(r["dz64"]).all() and np.isfinite(r["dl64"]).all()
    # the fp32 restatement of the chain is a usable floor: far below the project's gradient tolerance
    print("FLOOR chain float32 %s %s%s: dz %.3g dl %.3g" % (shape, kernel, "/class" if per_class else "", r["e32_dz"], r["e32_dl"]))
    assert r["e32_dz"] < dm.GRAD_RTOL / dm.FLOOR_MARGIN and r["e32_dl"] < dm.GRAD_RTOL / dm.FLOOR_MARGIN


def test_the_chain_inputs_hold_a_duplicate_pair_and_an_outlier():
    inp = dm.chain_inputs(3, 19, 30)
    z, l = inp["z"], float(inp["l"][0])
    for b in range(3):
        u = ((z[b][:, None] - z[b][None]) ** 2).sum(-1) / l ** 2
        off = u[~np.eye(19, dtype=bool)]
        assert (off == 0).sum() == 2 and u.max() > 25.0 and 0.05 < np.median(off) < 5.0


def test_small_distance_regime_of_the_formula_on_the_cpu():
    """What the kernel's formula (the logarithm of the rounded E) keeps of dlengthscale as d2 / l^2 shrinks, next to dl = -<z - r, dz> / l, both in fp32:
    printed for docs/MEASUREMENTS.md; at the scale of the QMUL fixture the formula must be far inside the gradient tolerance."""
    for shape in dm.SMALL_SHAPES:
        for target in dm.SMALL_TARGETS:
            d = dm.dl_three_ways(dm.small_distance_case(shape, target))
            print("MEASURED small_distance float32 numpy %s max d2/l2 %.0e: formula %.3e homogeneity %.3e" % (
                shape, target, abs(d["formula32"] - d["ref"]) / abs(d["ref"]), abs(d["homog32"] - d["ref"]) / abs(d["ref"])))
    d = dm.dl_three_ways(dm.qmul_case())
    ef, eh = abs(d["formula32"] - d["ref"]) / abs(d["ref"]), abs(d["homog32"] - d["ref"]) / abs(d["ref"])
    print("MEASURED small_distance float32 numpy qmul fixture (max d2/l2 %.3g): formula %.3e homogeneity %.3e" % (d["umax"], ef, eh))
    assert ef < dm.GRAD_RTOL / 10.0, ef
