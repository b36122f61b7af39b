"""The front door of the per-class GP calls of dkt_amd.ops, on the GPU: a stride that came out wrong for ONE layout.  Each of mll, mll_rownoise, loo, loo_lowrank,
rownoise_lowrank and posterior is called on every layout it takes -- base matrix [B,N,N] or [B,C,N,N] (or rows), targets [C,N] or [B,C,N] -- at the smallest
shape that has more than one episode, more than one class and an odd row count, and compared with the same problems in the explicitly expanded layout
(base broadcast to [B,C,N,N], targets to [B,C,N], both contiguous):

  mll_rownoise, loo      bit for bit; a shared base's gradient is the in-order class sum of the per-class one (docs/DIRICHLET.md, docs/LOO.md;
                         test_two_runs_and_both_forms_agree_bitwise, test_shared_w_is_the_class_sum_of_the_per_class_w)
  loo_lowrank,           bit for bit: only the targets' layout varies, a batch stride of 0 or C N on the same values, and both kernels reduce in a fixed order
  rownoise_lowrank       (docs/LOOFS.md, docs/DIRICHLET.md: two runs agree bit for bit)
  mll                    a shared and a per-class base take different kernels of dkt_mll_f32: every layout against the float64 closed form of
                         test_gpu_parity._mll_vs_float64, at its tolerances (logp 1e-4 relative, alpha 5e-4 and the gradients 1e-3 in relative l2)
  posterior              every layout against posterior_model.closed_form in float64 within BOUND x the float32 floor of the case group that holds (17, 5)

and a malformed operand is refused with a RuntimeError before the library is called."""
import numpy as np
import pytest
import torch

from dkt_amd import _lib, ops

import posterior_model as pm

pytestmark = pytest.mark.gpu
B, C, N, D, M = 2, 3, 17, 8, 5
MLL_RTOL, GRAD_RTOL, ALPHA_RTOL = 1e-4, 1e-3, 5e-4           # tests/test_gpu_parity.py
LAYOUTS = [(per_class, y_batched) for per_class in (False, True) for y_batched in (False, True)]
IDS = ["%s-%s" % ("perclass" if p else "shared", "yB" if y else "y") for p, y in LAYOUTS]


def _dev(x, dev):
    return None if x is None else torch.tensor(np.ascontiguousarray(x), dtype=torch.float32, device=dev)


@pytest.fixture(scope="module")
def data():
    """The operands once, as float32 numpy arrays, never modified: unit rows, their RBF base matrices (shared and per class), targets, row noises, hypers."""
    zs, zq = pm.unit_rows(11, B, N, D), pm.unit_rows(12, B, M, D)
    rng = np.random.default_rng(5)
    sv, mean, noise = pm.hypers(C, 1.0, 0.1)
    d = dict(z=zs.astype(np.float32), sv=sv, mean=mean, noise=noise, cw=np.linspace(0.5, 1.5, C).astype(np.float32))
    for per_class in (False, True):
        cc = C if per_class else None
        d["e", per_class] = pm.base_matrix(zs, None, "rbf", cc)
        d["e_qs", per_class], d["e_qq", per_class] = pm.base_matrix(zq, zs, "rbf", cc), pm.base_matrix(zq, None, "rbf", cc)
    for y_batched in (False, True):
        d["y", y_batched] = pm.targets(3, C, N, B if y_batched else None)
        d["nr", y_batched] = rng.uniform(0.2, 2.0, (B, C, N) if y_batched else (C, N)).astype(np.float32)
    d["yq"], d["eps"] = pm.targets(4, C, M, B), rng.standard_normal((B, C, 3, M)).astype(np.float32)
    return d


def _bc(a, item_ndim):
    """[..item] | [B,..item] -> [B,C,..item] for the base matrices (class axis), [C,N] -> [B,C,N] for the targets (batch axis): contiguous copies"""
    if a.ndim == item_ndim + 2:
        return a
    return np.ascontiguousarray(np.broadcast_to(a[:, None] if item_ndim == 2 else a[None], ((B, C) + a.shape[-item_ndim:])))


def _same_bits(got, want, keys):
    return [k for k in keys if (got[k] is None) != (want[k] is None) or (got[k] is not None and not torch.equal(got[k], want[k]))]


def _class_sum(t):
    acc = t[:, 0].clone()
    for c in range(1, t.shape[1]):                            # the classes in index order
        acc = acc + t[:, c]
    return acc


# ---- the N x N calls that are bitwise the expanded layout ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_class,y_batched", LAYOUTS, ids=IDS)
def test_mll_rownoise_is_the_expanded_layout_bit_for_bit(per_class, y_batched, data, cuda):
    hyp = [_dev(data[k], cuda) for k in ("sv", "mean")]
    call = lambda e, y, nr: ops.mll_rownoise(_dev(e, cuda), _dev(y, cuda), _dev(nr, cuda), *hyp, want_grad=True, want_chol=True, cls_weight=_dev(data["cw"], cuda))  # noqa: E731
    got = call(data["e", per_class], data["y", y_batched], data["nr", y_batched])
    want = call(_bc(data["e", per_class], 2), _bc(data["y", y_batched], 1), _bc(data["nr", y_batched], 1))
    assert int(want["info"].abs().max()) == 0 and bool(torch.isfinite(want["logp"]).all())
    assert not _same_bits(got, want, ("logp", "alpha", "info", "chol", "dsv", "dmean"))
    assert tuple(got["de"].shape) == ((B, C, N, N) if per_class else (B, N, N))
    assert torch.equal(got["de"], want["de"] if per_class else _class_sum(want["de"]))


@pytest.mark.parametrize("per_class,y_batched", LAYOUTS, ids=IDS)
def test_loo_is_the_expanded_layout_bit_for_bit(per_class, y_batched, data, cuda):
    hyp = [_dev(data[k], cuda) for k in ("sv", "mean", "noise")]
    call = lambda e, y: ops.loo(_dev(e, cuda), _dev(y, cuda), *hyp, want_grad=True, cls_weight=_dev(data["cw"], cuda))  # noqa: E731
    got = call(data["e", per_class], data["y", y_batched])
    want = call(_bc(data["e", per_class], 2), _bc(data["y", y_batched], 1))
    assert int(want["info"].abs().max()) == 0 and bool(torch.isfinite(want["loo"]).all())
    assert not _same_bits(got, want, ("loo", "alpha", "mu_loo", "var_loo", "dsv", "dmean", "dnoise", "jitter", "info"))
    assert tuple(got["w"].shape) == ((B, C, N, N) if per_class else (B, N, N))
    assert torch.equal(got["w"], want["w"] if per_class else _class_sum(want["w"]))


# ---- the calls on the rows: only the targets have two layouts ----------------------------------------------------------------------------------
def test_loo_lowrank_is_the_expanded_layout_bit_for_bit(data, cuda):
    hyp = [_dev(data[k], cuda) for k in ("sv", "mean", "noise")]
    call = lambda y: ops.loo_lowrank(_dev(data["z"], cuda), _dev(y, cuda), *hyp, want_grad=True, cls_weight=_dev(data["cw"], cuda))  # noqa: E731
    got, want = call(data["y", False]), call(_bc(data["y", False], 1))
    assert int(want["info"].abs().max()) == 0 and bool(torch.isfinite(want["loo"]).all()) and tuple(got["dz"].shape) == (B, N, D)
    assert not _same_bits(got, want, tuple(want))
    again = call(data["y", True])                              # per-episode targets: every episode its own
    for b in range(B):
        one = ops.loo_lowrank(_dev(data["z"][b:b + 1], cuda), _dev(data["y", True][b], cuda), *hyp, want_grad=True, cls_weight=_dev(data["cw"], cuda))
        assert not [k for k in one if not torch.equal(one[k][0], again[k][b])], b


def test_rownoise_lowrank_is_the_expanded_layout_bit_for_bit(data, cuda):
    z, g = _dev(data["z"], cuda), _dev(np.linspace(0.5, 1.0, B), cuda)
    hyp = [_dev(data[k], cuda) for k in ("sv", "mean", "cw")]

    def call(y, nr):
        y, nr = _dev(y, cuda), _dev(nr, cuda)
        out = ops.rownoise_lowrank(z, y, nr, *hyp, want_grad=True)
        return dict(out, dz=ops.rownoise_lowrank_bwd(z, y, nr, *hyp, out["state"], g))

    want = call(_bc(data["y", False], 1), _bc(data["nr", False], 1))
    assert int(want["info"].abs().max()) == 0 and bool(torch.isfinite(want["logp"]).all()) and tuple(want["dz"].shape) == (B, N, D)
    assert not _same_bits(call(data["y", False], data["nr", False]), want, tuple(want))
    assert not _same_bits(call(data["y", False], _bc(data["nr", False], 1)), want, tuple(want))          # (the two batch strides are independent)
    assert not _same_bits(call(_bc(data["y", False], 1), data["nr", False]), want, tuple(want))
    # per-episode targets and row noises, every episode its own: a workgroup never reads another episode's rows and reduces in a fixed order
    # (docs/DIRICHLET.md "feature space"), so the batch is its episodes one by one
    per_episode = call(data["y", True], data["nr", True])
    for b in range(B):
        y1, nr1 = _dev(data["y", True][b], cuda), _dev(data["nr", True][b], cuda)
        one = ops.rownoise_lowrank(z[b:b + 1].contiguous(), y1, nr1, *hyp, want_grad=True)
        one["dz"] = ops.rownoise_lowrank_bwd(z[b:b + 1].contiguous(), y1, nr1, *hyp, one["state"], g[b:b + 1].contiguous())
        assert not [k for k in one if not torch.equal(one[k][0], per_episode[k][b])], b


# ---- against float64 ---------------------------------------------------------------------------------------------------------------------------
def _rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.mark.parametrize("per_class,y_batched", LAYOUTS, ids=IDS)
def test_mll_matches_float64_on_every_layout(per_class, y_batched, data, cuda):
    e, y, sv, mean, noise, cw = data["e", per_class], data["y", y_batched], data["sv"], data["mean"], data["noise"], data["cw"]
    out = ops.mll(_dev(e, cuda), _dev(y, cuda), _dev(sv, cuda), _dev(mean, cuda), _dev(noise, cuda), want_grad=True, cls_weight=_dev(cw, cuda))
    got = {k: v.cpu().numpy() for k, v in out.items() if v is not None}
    assert (got["info"] == 0).all() and (got["jitter"] == 0).all()
    assert got["w"].shape == ((B, C, N, N) if per_class else (B, N, N)) and (got["w"] == np.swapaxes(got["w"], -1, -2)).all()
    e4, y3 = _bc(e, 2).astype(np.float64), _bc(y, 1).astype(np.float64)
    for b in range(B):
        w_ref, hyper = np.zeros((C, N, N)), ([], [], [])
        for c in range(C):
            kk = sv[c] * e4[b, c] + noise[c] * np.eye(N)
            r = y3[b, c] - mean[c]
            kinv = np.linalg.inv(kk)
            alpha = kinv @ r
            logp = -0.5 * r @ alpha - 0.5 * np.linalg.slogdet(kk)[1] - 0.5 * N * np.log(2 * np.pi)
            assert abs(got["logp"][b, c] - logp) < MLL_RTOL * abs(logp), (b, c, got["logp"][b, c], logp)
            assert _rel_l2(got["alpha"][b, c], alpha) < ALPHA_RTOL, (b, c)
            m = 0.5 * (np.outer(alpha, alpha) - kinv)
            w_ref[c] = cw[c] * sv[c] * m
            hyper[0].append((m * e4[b, c]).sum()); hyper[1].append(np.trace(m)); hyper[2].append(alpha.sum())
        assert _rel_l2(got["w"][b], w_ref if per_class else w_ref.sum(0)) < GRAD_RTOL, b
        for key, ref in zip(("dsv", "dnoise", "dmean"), hyper):
            assert _rel_l2(got[key][b], np.array(ref)) < GRAD_RTOL, (b, key)


@pytest.mark.parametrize("per_class,y_batched", LAYOUTS, ids=IDS)
def test_posterior_matches_float64_on_every_layout(per_class, y_batched, data, cuda):
    floor = pm.floors(next(g for g, top in pm.GROUPS.items() if max(N, M) <= top))
    args = [data["e", per_class], data["e_qs", per_class], data["e_qq", per_class], data["y", y_batched], data["sv"], data["mean"], data["noise"]]
    ref = pm.closed_form(*args, yq=data["yq"], eps=data["eps"], with_noise=True)
    out = ops.posterior(*[_dev(a, cuda) for a in args], yq=_dev(data["yq"], cuda), eps=_dev(data["eps"], cuda), with_noise=True, want_chol=True)
    got = {k: None if v is None else v.cpu().numpy() for k, v in out.items()}
    for q in ("info_s", "info_q", "jitter_s", "jitter_q"):
        assert (got[q] == 0).all(), q
    err = pm.errors(got, ref, pm.QUANTITIES)
    print("FRONT DOOR posterior", {q: "%.3e (bound %.3e)" % (err[q], pm.BOUND * floor[q]) for q in pm.QUANTITIES})
    bad = [q for q in pm.QUANTITIES if not err[q] <= pm.BOUND * floor[q]]
    assert not bad, {q: (err[q], pm.BOUND * floor[q]) for q in bad}


@pytest.mark.parametrize("mixed", ["e_qs", "e_ss", "e_qq"])
def test_posterior_takes_each_base_matrix_in_a_layout_of_its_own(mixed, data, cuda):
    """One of the three shared base matrices handed over with a class axis (the same matrix for every class, so the model is the shared one): each operand has
    its own stride pair.  Against the float64 closed form, as above."""
    floor = pm.floors(next(g for g, top in pm.GROUPS.items() if max(N, M) <= top))
    mats = {"e_ss": data["e", False], "e_qs": data["e_qs", False], "e_qq": data["e_qq", False]}
    rest = [data["y", False], data["sv"], data["mean"], data["noise"]]
    ref = pm.closed_form(mats["e_ss"], mats["e_qs"], mats["e_qq"], *rest, yq=data["yq"], eps=data["eps"], with_noise=True)
    mats[mixed] = _bc(mats[mixed], 2)
    assert mats[mixed].ndim == 4
    out = ops.posterior(*[_dev(a, cuda) for a in [mats["e_ss"], mats["e_qs"], mats["e_qq"]] + rest], yq=_dev(data["yq"], cuda), eps=_dev(data["eps"], cuda),
                        with_noise=True, want_chol=True)
    got = {k: None if v is None else v.cpu().numpy() for k, v in out.items()}
    assert (got["info_s"] == 0).all() and (got["info_q"] == 0).all()
    err = pm.errors(got, ref, pm.QUANTITIES)
    bad = [q for q in pm.QUANTITIES if not err[q] <= pm.BOUND * floor[q]]
    assert not bad, {q: (err[q], pm.BOUND * floor[q]) for q in bad}


# ---- a malformed operand is refused before the library is called -------------------------------------------------------------------------------
def _good(name, data, cuda):
    t = lambda k: _dev(data[k], cuda)  # noqa: E731
    e, z, y, nr = t(("e", False)), t("z"), t(("y", False)), t(("nr", False))
    return {"mll": lambda **kw: ops.mll(**dict(dict(e=e, y=y, sv=t("sv"), mean=t("mean"), noise=t("noise")), **kw)),
            "mll_rownoise": lambda **kw: ops.mll_rownoise(**dict(dict(e=e, y=y, noise_rows=nr, sv=t("sv"), mean=t("mean")), **kw)),
            "loo": lambda **kw: ops.loo(**dict(dict(e=e, y=y, sv=t("sv"), mean=t("mean"), noise=t("noise")), **kw)),
            "loo_lowrank": lambda **kw: ops.loo_lowrank(**dict(dict(z=z, y=y, sv=t("sv"), mean=t("mean"), noise=t("noise")), **kw)),
            "rownoise_lowrank": lambda **kw: ops.rownoise_lowrank(**dict(dict(z=z, y=y, noise_rows=nr, sv=t("sv"), mean=t("mean")), **kw)),
            "posterior": lambda **kw: ops.posterior(**dict(dict(e_ss=e, e_qs=t(("e_qs", False)), e_qq=t(("e_qq", False)), y=y, sv=t("sv"), mean=t("mean"),
                                                                noise=t("noise")), **kw))}[name]


MALFORMED = [("mll", "load", "dkt_mll_f32", "y", (C, N + 1)), ("mll", "load", "dkt_mll_f32", "cls_weight", (C - 1,)),
             ("mll_rownoise", "load", "dkt_mll_rownoise_f32", "noise_rows", (B, C + 1, N)), ("loo", "load_loo", "dkt_loo_f32", "e", (B, C + 1, N, N)),
             ("loo_lowrank", "load_loofs", "dkt_loofs_f32", "sv", (C + 1,)), ("rownoise_lowrank", "load", "dkt_rownoise_lowrank_f32", "y", (B + 1, C, N)),
             ("posterior", "load_post", "dkt_posterior_f32", "mean", (C + 1,))]


@pytest.mark.parametrize("name,loader,entry,operand,shape", MALFORMED, ids=["%s-%s" % (m[0], m[3]) for m in MALFORMED])
def test_a_malformed_operand_is_refused_before_any_library_call(name, loader, entry, operand, shape, data, cuda, monkeypatch):
    monkeypatch.delenv("DKT_TWINS", raising=False)              # (the product library serves the call)
    lib, calls = getattr(_lib, loader)(), []
    real = getattr(lib, entry)
    monkeypatch.setattr(lib, entry, lambda *a: (calls.append(entry), real(*a))[1])
    call = _good(name, data, cuda)
    call()
    assert calls == [entry]                                     # the counter sees the well-formed call
    with pytest.raises(RuntimeError, match="^(%s|dkt_amd.ops): " % name):
        call(**{operand: torch.ones(shape, device=cuda)})
    assert calls == [entry]
