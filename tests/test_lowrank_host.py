"""CPU-side checks of the float64 model of the feature-space Gaussian episode (tests/lowrank_model.py): it IS the oracle's N x N problem on E = Z Z^T
(mll_terms, mll_grads, gram_linear_bwd); the device's feature order is a consistent relabelling; zero padding D -> 64 changes no output; the case lists of
tests/test_lowrank_gpu.py cover what they claim; the aligned-row inputs have the condition numbers the GPU test records."""
import numpy as np
import pytest

import lowrank_model as lm
from oracle import dkt_oracle as O

RTOL = 1e-10


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("c,n,d,per_ep", [(1, 3, 4, False), (5, 3, 64, True), (5, 37, 64, False), (9, 35, 12, True), (17, 80, 20, False), (21, 84, 52, True)])
def test_model_is_the_oracle_on_the_nxn_problem(c, n, d, per_ep):
    inp = lm.inputs(c, n, d, b=2, y_per_episode=per_ep)
    m = lm.episode(**inp)
    z, y, sv, mean, noise, cw, g = (inp[k].astype(np.float64) for k in ("z", "y", "sv", "mean", "noise", "cw", "g"))
    for i in range(2):
        e = z[i] @ z[i].T
        yi = y[i] if per_ep else y
        res = O.mll_terms(e, yi, sv, mean, noise)
        assert not res.jitter.any()
        w_e, dsv, dmean, dnoise = O.mll_grads(e, res, sv, noise, cw)
        errs = dict(logp=rel(m["logp"][i], res.logp), alpha=rel(m["alpha"][i], res.alpha), dsv=rel(cw * m["dsv"][i], dsv), dmean=rel(cw * m["dmean"][i], dmean),
                    dnoise=rel(cw * m["dnoise"][i], dnoise), dz=rel(m["dz"][i], g[i] * O.gram_linear_bwd(w_e, z[i])),
                    obj=abs(m["obj"][i] - float((cw * res.logp).sum())) / np.abs(cw * res.logp).sum())
        print("C=%d N=%d D=%d episode %d: %s" % (c, n, d, i, {k: "%.1e" % v for k, v in errs.items()}))
        assert max(errs.values()) < RTOL, errs


def test_the_feature_order_is_a_consistent_relabelling():
    assert sorted(lm.PERM) == list(range(64)) and (lm.PERM[lm.INV] == np.arange(64)).all() and (lm.INV[lm.PERM] == np.arange(64)).all()
    # d' = 16 q + m <-> column 4 m + q: a lane's 16-byte load (columns 4 m .. 4 m + 3) feeds register q of operand tile q
    assert all(lm.PERM[16 * q + m] == 4 * m + q for q in range(4) for m in range(16))
    x = np.random.default_rng(0).standard_normal((2, 64, 64))
    assert (lm.to_natural(lm.to_device(x, (-1, -2)), (-1, -2)) == x).all() and (lm.to_device(x)[..., 5] == x[..., lm.PERM[5]]).all()
    assert list(lm.padded_device_indices(64)) == [] and list(lm.padded_device_indices(4)) == [i for i in range(64) if i % 16 != 0]
    assert set(lm.padded_device_indices(12)) == {16 * q + m for q in range(4) for m in range(3, 16)}
    # the same problem in the device's order: the relabelled operands give the relabelled results, and the scalars do not move
    inp = lm.inputs(5, 37, 20)
    m = lm.episode(**inp)
    dev = lm.inner(m["A_dev"], m["P_dev"], inp["sv"], inp["noise"], inp["cw"])
    assert rel(dev["t"], m["t_dev"]) < 1e-12 and rel(dev["wd"], m["wd_dev"]) < 1e-12 and rel(lm.to_natural(dev["t"]), m["t"]) < 1e-12
    assert rel(dev["logp_d"], m["logp_d"]) < 1e-13 and rel(dev["dnoise_d"], m["dnoise_d"]) < 1e-12
    pads = lm.padded_device_indices(20)
    assert not m["A_dev"][:, pads].any() and not m["A_dev"][:, :, pads].any() and not m["P_dev"][..., pads].any() and not m["t_dev"][..., pads].any()
    assert m["A_dev"][:, np.setdiff1d(np.arange(64), pads)].any()


@pytest.mark.parametrize("d", [4, 20, 52])
def test_zero_padding_changes_no_output(d):
    inp = lm.inputs(9, 35, d)
    m = lm.episode(**inp)
    wide = dict(inp, z=np.concatenate([inp["z"], np.zeros((2, 35, 64 - d), np.float32)], axis=2))
    w = lm.episode(**wide)
    for k in ("logp", "alpha", "v", "dsv", "dmean", "dnoise", "obj", "A", "P", "t", "wd"):
        assert rel(w[k], m[k]) < 1e-13, k
    assert rel(w["dz"][..., :d], m["dz"]) < 1e-12
    # and against a D x D statement without any padding: log det and trace absorb the 64 - D eigenvalues noise_c
    z, y, sv, mean, noise = (inp[k].astype(np.float64) for k in ("z", "y", "sv", "mean", "noise"))
    for c in range(9):
        kd = sv[c] * z[0].T @ z[0] + noise[c] * np.eye(d)
        r = y[c] - mean[c]
        p = z[0].T @ r
        t = np.linalg.solve(kd, p)
        logp = -0.5 * (r @ r - sv[c] * p @ t) / noise[c] - 0.5 * ((35 - d) * np.log(noise[c]) + np.linalg.slogdet(kd)[1]) - 0.5 * 35 * lm.LOG_2PI
        assert abs(logp - m["logp"][0, c]) < 1e-11 * abs(logp) and rel(m["t"][0, c, :d], t) < 1e-11


def test_the_bounds_scale_with_the_unit_roundoff_and_are_not_vacuous():
    """Every bound is far below the value it guards (a dropped or doubled 4-column group moves a value by its own size), and positive wherever the value can round."""
    inp = lm.inputs(9, 35, 52)
    gr = lm.gram(inp["z"], inp["y"], inp["mean"])
    m = lm.episode(**inp)
    fin = lm.finish(inp["z"], inp["y"], inp["sv"], inp["mean"], inp["noise"], inp["cw"], m["t"], m["logp_d"], m["dnoise_d"])
    bw = lm.backward(inp["z"], m["v"], m["t"], m["wd"], inp["g"])
    assert gr["A_bound"].max() < 1e-5 * np.abs(gr["A"]).max() and gr["P_bound"].max() < 1e-5 * np.abs(gr["P"]).max()
    for k in ("alpha", "v", "logp", "dsv", "dmean", "dnoise", "obj"):
        assert (fin[k + "_bound"] > 0).all() and fin[k + "_bound"].max() < 1e-3 * np.abs(fin[k]).max(), k
    assert bw["dz_bound"].max() < 1e-4 * np.abs(bw["dz"]).max()
    # one 4-column group of Z left out of S = Zp T^T (the predicate 16 j + 4 kk < D one group short) lands far outside the bound of alpha
    short = lm.finish(np.concatenate([inp["z"][..., :48], np.zeros((2, 35, 4), np.float32)], 2), inp["y"], inp["sv"], inp["mean"], inp["noise"], inp["cw"],
                      m["t"], m["logp_d"], m["dnoise_d"])
    assert (np.abs(short["alpha"] - fin["alpha"]) > 100 * fin["alpha_bound"]).mean() > 0.9


def test_the_cases_cover_what_they_claim():
    assert len(lm.CASES) == len(set(lm.CASES)) == 2 * len(lm.CLASS_COUNTS) + 2 * len(lm.N_EDGES) + len(lm.D_EDGES)
    assert {c for c, n, d in lm.CLASS_CASES} == {1, 4, 5, 8, 9, 12, 16, 17, 20, 21, 32} and {(n, d) for c, n, d in lm.CLASS_CASES} == {(37, 64), (80, 20)}
    assert {n for c, n, d in lm.N_CASES} == {1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 35, 63, 64, 65, 127, 128, 129} and {(c, d) for c, n, d in lm.N_CASES} == {(5, 64), (17, 12)}
    assert {d for c, n, d in lm.D_CASES} == {4, 12, 16, 20, 36, 48, 52, 60, 64} and {(c, n) for c, n, d in lm.D_CASES} == {(9, 35)}
    # every instantiation by at least two class counts, at the first and the last class count it serves
    for nkc, (lo, hi) in {2: (1, 8), 4: (9, 16), 5: (17, 20), 8: (21, 32)}.items():
        cs = {c for c, n, d in lm.CASES if lm.nkc_of(c) == nkc}
        assert len(cs) >= 2 and lo in cs and hi in cs and all(lo <= c <= hi for c in cs), nkc
        assert lm.nkc_of(lo) == lm.nkc_of(hi) == nkc and (hi == 32 or lm.nkc_of(hi + 1) != nkc)
    for nct, (lo, hi) in {1: (1, 16), 2: (17, 32)}.items():
        cs = {c for c, n, d in lm.CASES if lm.nct_of(c) == nct}
        assert len(cs) >= 2 and lo in cs and hi in cs, nct
    assert {lm.case_flags(i)[0] for i in range(len(lm.CASES))} == {2, 3} and {lm.case_flags(i)[1] for i in range(len(lm.CASES))} == {False, True}
    assert all(n >= 80 for c, n, d in lm.END_TO_END) and {c for c, n, d in lm.END_TO_END_EXTRA} == {9, 12, 16, 21} and {n for c, n, d in lm.END_TO_END_EXTRA} == {84, 96}
    assert {k for k in lm.CASES if k[1] >= 80} <= set(lm.END_TO_END)
    assert lm.GUARD_CASES == [(9, 35, 12), (16, 33, 52), (21, 17, 4), (32, 129, 64)]
    inp = lm.inputs(9, 35, 12, b=3, y_per_episode=True)
    assert inp["y"].shape == (3, 9, 35) and (inp["y"][0] != inp["y"][1]).any() and (inp["cw"] > 0).any() and (inp["cw"] < 0).any() and len(set(inp["g"])) == 3
    assert np.allclose(np.linalg.norm(inp["z"].astype(np.float64), axis=-1), 1.0, atol=1e-6)


def test_the_aligned_rows_have_the_recorded_condition_numbers():
    """Seed 5 (re-checked here): non-negative unit rows at noise 0.1 -- lambda_max(Z^T Z) = 147 / 269 / 347 of N = 420 at shift 0 / 1 / 2, so cond(K_c) runs from
    1.5e3 (sv 1, shift 0) to 1.04e4 (sv 3, shift 2), across MLL_H2_KAPPA_MAX = 5e3 of csrc/dkt_mll.hip; the 105-row episodes from 4e2 to 2.6e3."""
    conds = {}
    for c, per, d in lm.ALIGNED_SHAPES:
        for shift in lm.ALIGNED_SHIFTS:
            z = lm.aligned_rows(lm.ALIGNED_SEED, c, per, d, shift).astype(np.float32)
            assert (z >= 0).all() and np.allclose(np.linalg.norm(z.astype(np.float64), axis=1), 1.0, atol=1e-6)
            for sv in lm.ALIGNED_SV:
                conds[(c * per, shift, sv)] = lm.cond_k(z, sv, lm.ALIGNED_NOISE)
    print({k: "%.3g" % v for k, v in conds.items()})
    assert [round((conds[(420, s, 3.0)] - 1) / 30) for s in (0, 1, 2)] == [147, 269, 347]
    big, small = [v for k, v in conds.items() if k[0] == 420], [v for k, v in conds.items() if k[0] == 105]
    assert 1.4e3 < min(big) < 1.6e3 and 1.0e4 < max(big) < 1.08e4 and 3.5e2 < min(small) < 4.5e2 and 2.4e3 < max(small) < 2.8e3
