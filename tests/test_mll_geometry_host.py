"""tests/mll_geometry_model.py against the built libraries and against itself, without a GPU: its geometry() reaches exactly the mll_h2_kernel / mll_h2e_kernel /
mll_mfma_kernel instantiations the product library contains (and, for the chol route from N = 32 on, instantiations the twins library contains); the case list
walks every wave count, ragged round, odd tail and tile count the launchers can produce; the references agree with the oracle; the bounds of the GPU test hold
for a float32 restatement and tell three seeded mistakes from it."""
import json
import os
import re

import numpy as np
import pytest

import dkt_amd
import mll_geometry_model as gm
from oracle import dkt_oracle as O

L = dkt_amd._lib
THREE = ("h2", "h2e", "mfma")


def _instantiations(key):
    """{(kernel, NT, template booleans ...)} of the three kernels in a built library, from the mangled names of its resource-usage table."""
    with open(os.path.join(L.OBJ_DIR, os.path.basename(L.LIBS[key].path) + ".resource_usage.json")) as fh:
        usage = json.load(fh)
    out = set()
    for name in usage:
        m = re.search(r"\d+(mll_h2_kernel|mll_h2e_kernel|mll_mfma_kernel)I((?:L[ib]\d+E)+)E", name)
        if m:
            args = re.findall(r"L([ib])(\d+)E", m.group(2))
            assert args[0][0] == "i" and all(t == "b" for t, _ in args[1:]), name
            out.add((m.group(1), int(args[0][1])) + tuple(v == "1" for _, v in args[1:]))
    return out


def _launches(twins=None):
    """(case, want_grad, geometry) of every launch of the case list (the batch, as the GPU test launches it)."""
    return [(case, g, case.geometry(g)) for case in gm.ALL_CASES for g in case.grads if twins is None or case.twins == twins]


def test_the_case_list_reaches_exactly_the_instantiations_the_product_library_contains(lib):
    built = _instantiations("hip")
    assert len(built) == 24 + 7 + 6, sorted(built)          # h2: NT 1..8 x {fwd, grad, grad + 5 waves}; h2e: NT 1..7; mfma with the Cholesky output: NT 1..2 x 3
    assert all(geo.family in THREE for _, _, geo in _launches()), "a case leaves the three kernels"
    reached = {geo.instantiation for _, _, geo in _launches(twins=False)}
    assert built - reached == set(), "instantiations no case reaches"
    assert reached - built == set(), "geometry() names instantiations the product library lacks"


def test_the_chol_cases_beyond_the_product_library_name_instantiations_of_the_twins_library(lib):
    L.build_twins()
    built = _instantiations("twins")
    reached = {geo.instantiation for _, _, geo in _launches(twins=True)}
    assert reached and reached <= built, sorted(reached - built)
    assert {i[1] for i in reached} == set(range(3, 9)) and all(i[0] == "mll_mfma_kernel" and i[3] for i in reached)          # NT 3..8, CHOL
    assert all(case.route == "chol" and case.n >= 32 for case, _, _ in _launches(twins=True))
    # the product library's own answer to those calls is the generic kernel: geometry() says so
    assert gm.geometry(32, 5, 3, False, True, True, gm.H2E_MINB_NEVER).family == "generic"
    assert gm.geometry(31, 5, 3, False, True, True, gm.H2E_MINB_NEVER).family == "mfma"


def test_the_case_list_holds_every_case_the_axes_call_for():
    assert gm.N_AXIS == (1, 15, 16, 31, 32, 47, 48, 63, 64, 79, 80, 95, 96, 111, 112, 127) and gm.C_AXIS == (1, 2, 3, 4, 5, 6, 9, 11, 32) and gm.B_AXIS == (1, 2, 3)
    assert len(set(gm.ALL_CASES)) == len(gm.ALL_CASES)
    have = set(gm.ALL_CASES)
    for route in gm.ROUTES:
        ns = gm.route_ns(route)
        assert ns == (gm.N_AXIS[:-2] if route == "h2e" else gm.N_AXIS)
        for n in ns:
            assert (route, n) in gm.PARAMS
            at = lambda c, b, yb: [k for k in have if (k.route, k.n, k.c, k.b, k.y_per_episode) == (route, n, c, b, yb)]          # noqa: E731
            for c in gm.C_AXIS:
                assert at(c, 3, False), (route, n, c)
            for c in (5, 9):
                assert at(c, 1, False) and at(c, 2, False), (route, n, c)
            for c in (1, 5, 11):
                assert at(c, 3, True), (route, n, c)
            mine = [k for k in have if (k.route, k.n) == (route, n)]
            assert {k.weighted for k in mine} == {True, False}
            assert (False in mine[0].grads) == (route != "h2e") and all(True in k.grads for k in mine)          # forward-only at every N, on every route that has it
    for c in (3, 4, 5, 32):
        cw = gm.class_weights(c, 16)
        assert (cw > 0).any() and (cw < 0).any() and (cw == 0).sum() == 1 and cw[-1] != 0


@pytest.mark.parametrize("family", ["h2", "mfma"])
def test_the_case_list_walks_the_whole_geometry_of_the_wave_per_matrix_kernels(family):
    shared = [(g, geo) for case, g, geo in _launches() if geo.family == family and not case.per_class]
    assert all(geo.grid == gm.ceil_div(geo.units, geo.epw) and geo.block == 64 * geo.wpg * geo.epw and geo.epw == (2 if geo.nt <= 7 else 1) for _, geo in shared)
    assert {geo.wpg for _, geo in shared} == {1, 2, 3, 4, 5}
    assert {geo.wpg for _, geo in shared if geo.partial_round} >= {4, 5}
    assert max(geo.rounds for _, geo in shared) >= 3 and any(geo.rounds >= 3 and geo.partial_round for _, geo in shared)
    assert {geo.nt for _, geo in shared if geo.surplus_episode} == set(range(1, 8))
    assert not any(geo.surplus_episode for _, geo in shared if geo.nt == 8)
    for grad in (True, False):
        assert {geo.nt for g, geo in shared if g == grad} == set(range(1, 9)), grad
    # per N: the ragged round next to the odd tail, at every tile-count edge
    for n in gm.N_AXIS:
        assert any(geo.partial_round and (geo.surplus_episode or geo.nt == 8) for (case, _, geo) in _launches() if geo.family == family and case.n == n), n


def test_the_case_list_walks_both_grids_of_the_wave_per_episode_kernel():
    geos = [(case, geo) for case, _, geo in _launches() if geo.family == "h2e"]
    assert {geo.nt for case, geo in geos if case.per_class} == set(range(1, 8)) == {geo.nt for case, geo in geos if not case.per_class}
    assert all(geo.grid == (case.b * case.c if case.per_class else case.b) and geo.block == 64 for case, geo in geos)
    # NT = 8 with per-class matrices: the wave-per-matrix kernel, one wave per workgroup
    nt8 = [geo for case, _, geo in _launches() if case.per_class and case.n >= 112]
    assert nt8 and all(geo.family == "h2" and (geo.wpg, geo.epw, geo.rounds, geo.block) == (1, 1, 1, 64) and geo.grid == geo.units for geo in nt8)


def test_geometry_against_numbers_worked_out_by_hand():
    never = gm.H2E_MINB_NEVER
    # N = 47 (48 with the augmented row: 3 tiles), 9 classes: 2 rounds of 5 waves, the last with 4; 3 episodes in 2 workgroups of 2 x 5 waves
    g = gm.geometry(47, 9, 3, False, True, False, never)
    assert (g.family, g.nt, g.rounds, g.wpg, g.epw, g.grid, g.block, g.partial_round, g.surplus_episode) == ("h2", 3, 2, 5, 2, 2, 640, True, True)
    assert g.instantiation == ("mll_h2_kernel", 3, True, True)
    # N = 48: 4 tiles; 11 classes: 3 rounds of 4 waves (4 + 4 + 3); forward only
    g = gm.geometry(48, 11, 2, False, False, False, never)
    assert (g.family, g.nt, g.rounds, g.wpg, g.epw, g.grid, g.block, g.partial_round, g.surplus_episode) == ("h2", 4, 3, 4, 2, 1, 512, True, False)
    assert g.instantiation == ("mll_h2_kernel", 4, False, False)
    # N = 127: 8 tiles, one episode per workgroup; 32 classes: 7 rounds of 5 waves, 2 in the last
    g = gm.geometry(127, 32, 3, False, True, False, never)
    assert (g.family, g.nt, g.rounds, g.wpg, g.epw, g.grid, g.block, g.partial_round, g.surplus_episode) == ("h2", 8, 7, 5, 1, 3, 320, True, False)
    # the wave-per-episode kernel from DKT_MLL_H2E_MINB episodes on: one wave per episode
    g = gm.geometry(111, 6, 3, False, True, False, 1)
    assert (g.family, g.nt, g.rounds, g.wpg, g.epw, g.grid, g.block, g.instantiation) == ("h2e", 7, 6, 1, 1, 3, 64, ("mll_h2e_kernel", 7))
    assert gm.geometry(111, 6, 3, False, False, False, 1).family == "h2" and gm.geometry(112, 6, 3, False, True, False, 1).family == "h2"
    # per-class base matrices: B * C single waves (NT <= 7), B * C one-wave workgroups of the wave-per-matrix kernel (NT = 8)
    g = gm.geometry(15, 11, 3, True, True, False, never)
    assert (g.family, g.nt, g.grid, g.block, g.units) == ("h2e", 1, 33, 64, 33)
    g = gm.geometry(112, 11, 3, True, False, False, never)
    assert (g.family, g.nt, g.rounds, g.wpg, g.epw, g.grid, g.block, g.instantiation) == ("h2", 8, 1, 1, 1, 33, 64, ("mll_h2_kernel", 8, False, False))
    # the Cholesky output: 6 classes in 2 rounds of 3 waves; one episode in a workgroup built for two
    g = gm.geometry(16, 6, 1, False, True, True, never)
    assert (g.family, g.nt, g.rounds, g.wpg, g.epw, g.grid, g.block, g.partial_round, g.surplus_episode) == ("mfma", 2, 2, 3, 2, 1, 384, False, True)
    assert g.instantiation == ("mll_mfma_kernel", 2, True, True, False)
    # the host's round count and the kernel's (ceil(C / wpg)) agree for every class count a call can bring
    for c in range(1, 65):
        rounds = gm.ceil_div(c, gm.MAX_WPG)
        assert gm.ceil_div(c, gm.ceil_div(c, rounds)) == rounds and gm.geometry(16, c, 2, False, True, False, never).rounds == rounds


def test_the_condition_bound_keeps_every_case_away_from_the_fix_up_kernel():
    worst = max(float(gm.condition_bounds(case).max()) for case in gm.ALL_CASES if case.route in ("default", "per_class"))
    assert worst < 1.5e3 < gm.MLL_H2_KAPPA_MAX, worst
    for c in gm.C_AXIS:
        sv, mean, noise = gm.hypers(c)
        assert 0.7 <= sv.min() and sv.max() <= 1.1 + 1e-6 and np.abs(mean).max() <= 0.1 + 1e-6 and 0.1 <= noise.min() and noise.max() <= 0.3 + 1e-6
        assert len(set(sv)) == len(set(mean)) == len(set(noise)) == c


def _cases_at(n, routes=("default", "per_class")):
    return [case for case in gm.ALL_CASES if case.n == n and case.route in routes]


@pytest.mark.parametrize("n", gm.N_AXIS)
def test_reference_is_the_oracle_on_shared_targets_and_a_shared_base_matrix(n):
    for case in _cases_at(n, ("default",)):
        if case.y_per_episode:
            continue
        x, ref = gm.inputs(case), gm.reference(case)
        cw = np.ones(case.c) if x["cw"] is None else x["cw"].astype(np.float64)
        for i in range(case.b):
            e = x["e"][i].astype(np.float64)
            res = O.mll_terms(e, x["y"], x["sv"], x["mean"], x["noise"])
            w, _, _, _ = O.mll_grads(e, res, x["sv"], x["noise"], cw)
            _, dsv, dmean, dnoise = O.mll_grads(e, res, x["sv"], x["noise"], np.ones(case.c))
            for key, want in (("logp", res.logp), ("alpha", res.alpha), ("chol", res.chol), ("w", w), ("dsv", dsv), ("dmean", dmean), ("dnoise", dnoise)):
                assert np.abs(ref[key][i] - want).max() <= 1e-12 * np.abs(want).max(), (case.name, key)


def test_reference_layouts_of_per_episode_targets_and_per_class_matrices():
    """One (episode, class) of each extension against the oracle called on that matrix and that target row alone."""
    for case in (gm.Case("default", 31, 11, 3, True, True), gm.Case("per_class", 31, 5, 3, True, False), gm.Case("per_class", 16, 9, 2, False, True)):
        assert case in gm.ALL_CASES
        x, ref = gm.inputs(case), gm.reference(case)
        i, k = case.b - 1, case.c - 2
        e = (x["e"][i, k] if case.per_class else x["e"][i]).astype(np.float64)
        y = x["y"][i, k] if case.y_per_episode else x["y"][k]
        res = O.mll_terms(e, y[None, :], x["sv"][k:k + 1], x["mean"][k:k + 1], x["noise"][k:k + 1])
        assert np.allclose(ref["logp"][i, k], res.logp[0], rtol=1e-12) and np.allclose(ref["alpha"][i, k], res.alpha[0], rtol=1e-12, atol=1e-14)
        if case.y_per_episode:
            assert sorted(x["y"][i, k].tolist()) == sorted(x["y"][0, k].tolist()) and not np.array_equal(x["y"][i], x["y"][0])
        if case.per_class:
            w, _, _, _ = O.mll_grads(e, res, x["sv"][k:k + 1], x["noise"][k:k + 1], [1.0 if x["cw"] is None else x["cw"][k]])
            assert ref["w"].shape == (case.b, case.c, case.n, case.n) and np.abs(ref["w"][i, k] - w).max() <= 1e-12 * np.abs(w).max()


@pytest.mark.parametrize("n", gm.N_AXIS)
def test_float32_restatement_passes_every_bound_and_the_bounds_catch_the_seeded_mistakes(n):
    for case in _cases_at(n):
        f32 = gm.reference32(case)
        fr = gm.fractions(case, f32, want_grad=True, want_chol=True)
        print("float32 numpy %s: %s" % (case.name, " ".join("%s %.3f" % kv for kv in fr.items())))
        assert set(fr) == set(gm.BOUNDS) and max(fr.values()) <= 1.0, (case.name, fr)
        geo = case.geometry()
        if not case.per_class and geo.partial_round:
            # (a) the ragged round's last class counted twice in W
            assert gm.fractions(case, gm.seed_last_class_w_twice(case, f32))["w"] > 1.0, case.name
        if not case.per_class and geo.rounds >= 2:
            # (c) round 2 leaves alpha at round 1's values
            assert gm.fractions(case, gm.seed_round2_alpha_from_round1(case, f32))["alpha"] > 1.0, case.name
        if case.b >= 2 and n > 1:
            # (b) the last episode's outputs land on the one before it (N = 1: every base matrix is [[1]], the episodes of a shared-target case are one and the same)
            bad = gm.fractions(case, gm.seed_last_episode_over_previous(case, f32))
            assert bad["alpha"] > 1.0 and bad["w"] > 1.0 and bad["logp"] > 1.0, (case.name, bad)
