"""-m gpu: the three kernels of the feature-space Gaussian episode (csrc/dkt_lowrank.hip) one by one against the float64 model of tests/lowrank_model.py, each
within the rounding bound written next to its formula there, each fed with the DEVICE outputs of the kernels before it (so the conditioning of the 64 x 64
solve blurs nobody's error); then the whole episode at the same edges, the wave-per-episode inner solve, and the unguarded inner solve on aligned features.

Which case launches which instantiation (lowrank_model.nkc_of / nct_of restate the dispatch; ops.kernel_timing counts the calls):
  lowrank_bwd_kernel<2>   C = 1, 4, 5, 8      lowrank_bwd_kernel<4>   C = 9, 12, 16      lowrank_bwd_kernel<5>   C = 17, 20      lowrank_bwd_kernel<8>   C = 21, 32
  lowrank_gram_kernel<1>, lowrank_finish_kernel<1>   C = 1 .. 16 (a full class tile at 16)      <2>   C = 17, 20, 21, 32
each at (N, D) = (37, 64) and (80, 20); the N edges run <2> / NCT 1 (C = 5, D = 64) and <5> / NCT 2 (C = 17, D = 12); the D edges run <4> / NCT 1 (C = 9, N = 35)."""
import os
import re

import numpy as np
import pytest
import torch

from dkt_amd import _lib, ops
from oracle import dkt_oracle as O

import lowrank_model as lm
from test_gpu_parity import GRAD_RTOL, MLL_RTOL, dev_t, rel_l2

pytestmark = pytest.mark.gpu
ALPHA_RTOL = 5e-4                                # the standing tolerance of the mean cache (test_episode_in_feature_space_vs_oracle_and_nxn_twin)
_runs = {}


def _np(t):
    return t.detach().double().cpu().numpy()


def device_run(index, cuda):
    """CASES[index] through ops._lowrank_forward / _lowrank_backward, once per session: the inputs, what the forward returns, dZ of two backward calls and the
    operands and results of the inner dkt_mll_f32 call (A, P in the device's feature order; t = its alpha, logp_d, dnoise_d, jitter)."""
    if index not in _runs:
        c, n, d = lm.CASES[index]
        b, per_ep = lm.case_flags(index)
        inp = lm.inputs(c, n, d, b=b, y_per_episode=per_ep)
        t = {k: torch.as_tensor(v, device=cuda) for k, v in inp.items()}
        seen, real = {}, ops.mll

        def spy(e, y, *args, **kw):
            out = real(e, y, *args, **kw)
            seen.update(A=e, P=y, inner=out, no_kappa_guard=kw.get("no_kappa_guard"))
            return out

        ops.mll = spy
        try:
            ops.kernel_timing(True)
            fwd = ops._lowrank_forward(t["z"], t["y"], t["sv"], t["mean"], t["noise"], t["cw"], 1e-6, 3, True)
            dz = ops._lowrank_backward(t["z"], fwd["v"], fwd["t"], fwd["wd"], t["g"])
            dz2 = ops._lowrank_backward(t["z"], fwd["v"], fwd["t"], fwd["wd"], t["g"])
            torch.cuda.synchronize()
            launches = {k: v[0] for k, v in ops.kernel_timing_results().items()}
        finally:
            ops.mll = real
            ops.kernel_timing(False)
        assert launches == dict(dkt_lowrank_gram_f32=1, dkt_mll_f32=1, dkt_lowrank_finish_f32=1, dkt_lowrank_bwd_f32=2), launches
        assert seen["no_kappa_guard"] is True and tuple(seen["A"].shape) == (b, 64, 64) and tuple(seen["P"].shape) == (b, c, 64)
        assert int(fwd["info"].abs().max()) == 0 and float(fwd["jitter"].abs().max()) == 0.0 and float(seen["inner"]["jitter"].abs().max()) == 0.0
        _runs[index] = dict(inp=inp, fwd=fwd, dz=dz, dz2=dz2, A=seen["A"], P=seen["P"], inner=seen["inner"])
    return _runs[index]


def within(tag, got, ref, bound):
    """|got - ref| <= bound elementwise; prints the worst ratio before it asserts"""
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    assert got.shape == ref.shape == bound.shape, (tag, got.shape, ref.shape, bound.shape)
    err = np.abs(got - ref)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print("%s: max err %.3g, worst err / bound %.3f (max |ref| %.3g)" % (tag, float(err.max()), worst, float(np.abs(ref).max())))
    assert np.isfinite(got).all() and worst <= 1.0, tag


IDS = ["C%d-N%d-D%d" % k for k in lm.CASES]


@pytest.mark.parametrize("index", range(len(lm.CASES)), ids=IDS)
def test_gram_kernel(cuda, index):
    """A = Zp^T Zp and P = Zp^T (y - m) within gamma(N) (|Z|^T |Z|) resp. gamma(N) |Z|^T |r|, gamma(N) = 2 (N + 4) 2^-24; A bitwise symmetric; the rows and
    columns of the padded features exactly zero, in the permuted positions the model predicts, and nothing else on the diagonal."""
    c, n, d = lm.CASES[index]
    run = device_run(index, cuda)
    inp = run["inp"]
    ref = lm.gram(inp["z"], inp["y"], inp["mean"])
    a_dev, p_dev = _np(run["A"]), _np(run["P"])
    assert torch.equal(run["A"], run["A"].transpose(1, 2))
    pads = lm.padded_device_indices(d)
    live = np.setdiff1d(np.arange(64), pads)
    assert len(pads) == 64 - d and (a_dev[:, pads, :] == 0).all() and (a_dev[:, :, pads] == 0).all() and (p_dev[:, :, pads] == 0).all()
    assert (a_dev[:, live, live] > 0).all()
    within("A %s" % IDS[index], lm.to_natural(a_dev, (-1, -2)), ref["A"], ref["A_bound"])
    within("P %s" % IDS[index], lm.to_natural(p_dev), ref["P"], ref["P_bound"])


@pytest.mark.parametrize("index", range(len(lm.CASES)), ids=IDS)
def test_finish_kernel(cuda, index):
    """alpha, V, logp, dsv, dmean, dnoise and obj against the model evaluated in float64 from the device's t, logp_d, dnoise_d and jitter (lowrank_model.finish:
    accumulation length 64 for S, N for the row sums, the cancelling terms |r| + sv |S| as the magnitude)."""
    run = device_run(index, cuda)
    inp, fwd, inner = run["inp"], run["fwd"], run["inner"]
    nz = inp["noise"].astype(np.float64)[None] + _np(inner["jitter"])
    ref = lm.finish(inp["z"], inp["y"], inp["sv"], inp["mean"], nz, inp["cw"], lm.to_natural(_np(inner["alpha"])), _np(inner["logp"]), _np(inner["dnoise"]))
    assert fwd["t"] is inner["alpha"] and fwd["wd"] is inner["w"]
    for key in ("alpha", "v", "logp", "dsv", "dmean", "dnoise", "obj"):
        within("%s %s" % (key, IDS[index]), _np(fwd[key]), ref[key], ref[key + "_bound"])


@pytest.mark.parametrize("index", range(len(lm.CASES)), ids=IDS)
def test_backward_kernel(cuda, index):
    """dZ = g_b (V^T T + 2 Z W') from the device's V, t and W', within 2 (C + 64 + 2) 2^-24 |g| (|V|^T |T| + 2 |Z| |W'|) elementwise, bitwise repeatable.
    (Rows >= N and columns >= D are not written: the guard arena, tests/test_guard_bands_gpu.py "lowrank-kernels-*".)"""
    run = device_run(index, cuda)
    inp, fwd = run["inp"], run["fwd"]
    ref = lm.backward(inp["z"], _np(fwd["v"]), lm.to_natural(_np(fwd["t"])), lm.to_natural(_np(fwd["wd"]), (-1, -2)), inp["g"])
    assert torch.equal(run["dz"], run["dz2"])
    within("dZ %s" % IDS[index], _np(run["dz"]), ref["dz"], ref["dz_bound"])


# ---- the whole episode at the same edges ------------------------------------------------------------------------------------------------------------
def _episode(inp, cuda, unit_rows=True):
    z = dev_t(inp["z"], cuda).requires_grad_(True)
    sv, mean, noise = (dev_t(inp[k], cuda).requires_grad_(True) for k in ("sv", "mean", "noise"))
    out = ops.episode_loss_linear(z, dev_t(inp["y"], cuda), sv, mean, noise, dev_t(inp["cw"], cuda), unit_rows=unit_rows)
    (out[0] * dev_t(inp["g"], cuda)).sum().backward()
    return out, z.grad, sv.grad, mean.grad, noise.grad


def _oracle(inp):
    """per episode: MLLResult, dZ; summed over the episodes (upstream gradient and class weights applied): d sv, d mean, d noise"""
    z, y, sv, mean, noise, cw, g = (np.asarray(inp[k], np.float32).astype(np.float64) for k in ("z", "y", "sv", "mean", "noise", "cw", "g"))
    res, dz, gs = [], [], np.zeros((3, len(sv)))
    for i in range(z.shape[0]):
        e = z[i] @ z[i].T
        r = O.mll_terms(e, y[i] if y.ndim == 3 else y, sv, mean, noise)
        w, dsv, dmean, dnoise = O.mll_grads(e, r, sv, noise, cw)
        res.append(r)
        dz.append(g[i] * O.gram_linear_bwd(w, z[i]))
        gs += g[i] * np.stack([dsv, dmean, dnoise])
    return res, dz, gs


def _against_oracle(tag, got, ref, inp, every=1):
    """The standing tolerances of the suite: logp MLL_RTOL per class, alpha 5e-4 and dZ GRAD_RTOL in relative L2 per episode, the hyper-parameter gradients
    GRAD_RTOL.  Prints every figure before it asserts; returns the worst of each."""
    (obj, logp, alpha, info, jit, _), dz, gsv, gmean, gnoise = got
    res, rdz, gs = ref
    cw = np.asarray(inp["cw"], np.float64)
    assert int(info.abs().max().item()) == 0 and float(jit.abs().max()) == 0.0
    worst = dict(logp=0.0, alpha=0.0, dz=0.0, obj=0.0)
    for k, i in enumerate(range(0, logp.shape[0], every)):
        worst["logp"] = max(worst["logp"], float(np.abs((_np(logp[i]) - res[k].logp) / res[k].logp).max()))
        worst["alpha"] = max(worst["alpha"], rel_l2(_np(alpha[i]), res[k].alpha))
        worst["dz"] = max(worst["dz"], rel_l2(_np(dz[i]), rdz[k]))
        worst["obj"] = max(worst["obj"], abs(obj[i].item() - float((cw * res[k].logp).sum())) / np.abs(cw * res[k].logp).sum())
    if every == 1:
        worst.update(dsv=rel_l2(_np(gsv), gs[0]), dnoise=rel_l2(_np(gnoise), gs[2]), dmean=float(np.abs(_np(gmean) - gs[1]).max() / (np.abs(gs[1]).max() + 1e-5 / GRAD_RTOL)))
    print("%s: %s" % (tag, " ".join("%s %.2e" % kv for kv in worst.items())))
    assert worst["logp"] < MLL_RTOL and worst["obj"] < MLL_RTOL and worst["alpha"] < ALPHA_RTOL and worst["dz"] < GRAD_RTOL, (tag, worst)
    assert all(worst.get(k, 0.0) < GRAD_RTOL for k in ("dsv", "dnoise", "dmean")), (tag, worst)
    return worst


@pytest.mark.parametrize("c,n,d", lm.END_TO_END, ids=["C%d-N%d-D%d" % k for k in lm.END_TO_END])
def test_episode_at_the_edges_vs_oracle(cuda, c, n, d, monkeypatch):
    """ops.episode_loss_linear in feature space (DKT_LOWRANK=force) at every edge case the ops-level gate lets through (N >= 80) and at C = 9, 12, 16, 21
    (lowrank_bwd_kernel<4> and the first class count of <8>, a full single class tile) against the float64 oracle on the N x N problem."""
    monkeypatch.setenv("DKT_LOWRANK", "force")
    inp = lm.inputs(c, n, d, b=2, y_per_episode=(c + n) % 2 == 1)
    assert ops.lowrank_applies(n, d, c, 2)
    got = _episode(inp, cuda)
    assert got[0][5] is None
    _against_oracle("C%d-N%d-D%d" % (c, n, d), got, _oracle(inp), inp)


def _h2e_min_batch():
    """the default of DKT_MLL_H2E_MINB, as the library states it"""
    text = open(os.path.join(_lib.CSRC, "dkt_mll_h2.hip")).read()
    return int(re.search(r"dkt_env_int\(DKT_SW_MLL_H2E_MINB,\s*(\d+)\)", text).group(1))


def test_inner_solve_in_the_wave_per_episode_kernel(cuda, monkeypatch):
    """From DKT_MLL_H2E_MINB episodes per call (its default, read from the source) the 64 x 64 models go to the wave-per-episode split kernel, on a base matrix
    A = Z^T Z whose diagonal is not 1 (trace N = 85).  Eight episodes against float64; every episode against the same inputs three at a time (the
    wave-per-matrix kernel), at the standing tolerances."""
    monkeypatch.setenv("DKT_LOWRANK", "force")
    monkeypatch.delenv("DKT_MLL_H2E_MINB", raising=False)
    b, c, n, d = _h2e_min_batch(), 5, 85, 64
    assert b >= 64
    inp = lm.inputs(c, n, d, b=b)
    a = lm.gram(inp["z"][:2], inp["y"], inp["mean"])["A"]
    assert np.abs(np.einsum("bdd->bd", a) - 1.0).max() > 0.5 and np.allclose(np.einsum("bdd->b", a), n, atol=1e-4)          # (A_dd ~ N / D = 1.3 on average)
    got = _episode(inp, cuda)
    (obj, logp, alpha, info, jit, e), dz = got[0], got[1]
    assert e is None
    every = b // 8
    sub = {k: (v[::every] if k in ("z", "g") else v) for k, v in inp.items()}
    _against_oracle("wave-per-episode B%d" % b, got, _oracle(sub), inp, every=every)
    t = {k: torch.as_tensor(v, device=cuda) for k, v in inp.items()}
    small = dict(logp=torch.empty_like(logp), alpha=torch.empty_like(alpha), dz=torch.empty_like(dz))
    for i0 in range(0, b, 3):
        i0 = min(i0, b - 3)
        z3 = t["z"][i0:i0 + 3].contiguous()
        f = ops._lowrank_forward(z3, t["y"], t["sv"], t["mean"], t["noise"], t["cw"], 1e-6, 3, True)
        small["logp"][i0:i0 + 3], small["alpha"][i0:i0 + 3] = f["logp"], f["alpha"]
        small["dz"][i0:i0 + 3] = ops._lowrank_backward(z3, f["v"], f["t"], f["wd"], t["g"][i0:i0 + 3].contiguous())

    def rel(x, y):
        return float(((x - y).double().flatten(1).norm(dim=1) / y.double().flatten(1).norm(dim=1)).max())

    errs = dict(logp=float(((logp - small["logp"]) / small["logp"]).abs().max()), alpha=rel(alpha, small["alpha"]), dz=rel(dz, small["dz"]))
    print("B = %d vs 3 at a time: %s" % (b, errs))
    assert errs["logp"] < MLL_RTOL and errs["alpha"] < ALPHA_RTOL and errs["dz"] < GRAD_RTOL


# ---- aligned (non-negative) unit rows: the 64 x 64 solve without its condition guard -----------------------------------------------------------------
ALIGNED = [(shape, shift, sv) for shape in lm.ALIGNED_SHAPES for shift in lm.ALIGNED_SHIFTS for sv in lm.ALIGNED_SV]
_aligned_oracle = {}


@pytest.mark.parametrize("shape,shift,sv", ALIGNED, ids=["N%d-shift%d-sv%g" % (s[0] * s[1], sh, v) for s, sh, v in ALIGNED])
def test_aligned_unit_rows_in_feature_space_and_nxn_twin(cuda, shape, shift, sv, monkeypatch):
    """The plain cossim kernel on a ReLU trunk: non-negative rows are strongly aligned, lambda_max(Z^T Z) is a large fraction of N and cond(K_c) = 1 + sv
    lambda_max / noise reaches 1.04e4 at N = 420 (sv 3, shift 2), 2.6e3 at N = 105 -- past MLL_H2_KAPPA_MAX = 5e3, the condition from which dkt_mll_f32 re-solves
    a matrix of the f16-split kernels in exact fp32, while the unit-row feature-space path calls those kernels without that guard (DKT_MLL_NO_KAPPA_GUARD).
    Measured on the MI355X (the table of DESIGN.md 4.6): feature space worst logp 2.7e-5, alpha 3.3e-5, dZ 4.1e-5, d sv 1.1e-5, d noise 2.2e-6 over the twelve
    inputs; the N x N twin (DKT_LOWRANK=0) logp 7.4e-6, alpha 3.9e-5, dZ 4.7e-5.  Inputs: lowrank_model.aligned_rows at seed 5 (re-checked on the CPU,
    tests/test_lowrank_host.py), noise 0.1, mean 0.05.  logp, alpha, dZ, d sv, d noise of both paths against the float64 oracle at the standing tolerances."""
    c, per, d = shape
    n = c * per
    z = lm.aligned_rows(lm.ALIGNED_SEED, c, per, d, shift)
    inp = dict(z=lm.f32(z[None]), y=lm.f32(O.one_vs_rest_targets(c, per)), sv=lm.f32(np.full(c, sv)), mean=lm.f32(np.full(c, lm.ALIGNED_MEAN)),
               noise=lm.f32(np.full(c, lm.ALIGNED_NOISE)), cw=lm.f32(np.full(c, -1.0 / (c * n))), g=lm.f32([1.0]))
    cond = lm.cond_k(inp["z"][0], float(inp["sv"][0]), float(inp["noise"][0]))
    key = (shape, shift, sv)
    if key not in _aligned_oracle:
        _aligned_oracle[key] = _oracle(inp)
    print("N=%d shift=%d sv=%g: cond(K_c) = %.3g" % (n, shift, sv, cond))
    assert (3.5e2 < cond < 2.8e3) if n == 105 else (1.4e3 < cond < 1.08e4)          # (the ranges tests/test_lowrank_host.py pins at this seed)
    worst = {}
    for mode in ("force", "0"):
        monkeypatch.setenv("DKT_LOWRANK", mode)
        got = _episode(inp, cuda)
        assert (got[0][5] is None) == (mode == "force")
        try:
            worst[mode] = _against_oracle("N=%d shift=%d sv=%g cond %.3g %s" % (n, shift, sv, cond, "feature space" if mode == "force" else "N x N twin"), got,
                                          _aligned_oracle[key], inp)
        except AssertionError as err:
            worst[mode] = err
    for mode, w in worst.items():
        if isinstance(w, AssertionError):
            raise w
