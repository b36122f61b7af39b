"""The front-end backward on the GPU -- dkt_gram_bn_bwd_f32 / _x16 (gram_bn_bwd_ep_kernel, all 8 tile counts, train and eval statistics) and its streaming
twin dkt_normalize_bn_bwd_f32 / _x16 -- against the float64 restatement (tests/frontend_bwd_model.py; test_frontend_bwd_host.py checks that one against
float64 autograd, states the float32 floors and proves that the bound used here tells seeded defects from a correct kernel).

Bound: per episode and quantity, max |got - ref| / max |ref| <= 4 x e32 of the case's group (docs/FRONTEND_BWD.md); a 16-bit dX gets one unit in the last
place of its type on top, element by element (the rounding of the store).  Every test prints its ratio err / e32."""
import ctypes

import numpy as np
import pytest
import torch

import dkt_amd
import frontend_bwd_model as fm

pytestmark = pytest.mark.gpu
ops, L = dkt_amd.ops, dkt_amd._lib
MARGIN = 4.0
SPECS = fm.case_specs()


@pytest.fixture(scope="module")
def ref():
    return fm.build_reference()


def _t(a, cuda, dtype=torch.float32):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=torch.float64).to(dtype).to(cuda)


def _call(c, cuda, **over):
    """The case's call on the GPU: (dX, dgamma_part, dbeta_part) as the op returns them."""
    c = dict(c, **over)
    x = _t(c["x"], cuda, fm.XDTYPES[c["xdtype"]])
    if c["call"] == "fused":
        return ops.gram_bn_bwd(_t(c["w"], cuda), _t(c["e"], cuda), x, _t(c["a"], cuda), _t(c["s"], cuda), _t(c["rnorm"], cuda), _t(c["mean"], cuda),
                               _t(c["rstd"], cuda), _t(c["g"], cuda))
    return ops.normalize_bn_bwd(_t(c["dzn"], cuda), _t(c["zn"], cuda), x, _t(c["a"], cuda), _t(c["rnorm"], cuda), _t(c["mean"], cuda), _t(c["rstd"], cuda))


def _episodes(out):
    dx, dg, db = (None if o is None else o.double().cpu().numpy() for o in out)
    return [dict(dx=dx[b], dgamma=None if dg is None else dg[b], dbeta=None if db is None else db[b]) for b in range(dx.shape[0])]


def _ulp(v, dtype):
    """Spacing of `dtype` at |v| (subnormals: the smallest subnormal), as in tests/test_x16_gpu.py."""
    fi = torch.finfo(dtype)
    return np.maximum(fi.eps * np.exp2(np.floor(np.log2(np.maximum(np.abs(v), fi.tiny)))), fi.tiny * fi.eps)


def test_every_instantiation_is_reached_by_a_parity_case():
    reached = {fm.instantiation(s) for s in SPECS.values() if s.get("call", "fused") == "fused"}
    missing = [(nt, train) for nt in range(1, 9) for train in (True, False) if (nt, train, "f32") not in reached]
    missing += [(nt, train, xd) for xd in ("bf16", "f16") for nt in (2, 3, 6, 7, 8) for train in (True, False) if (nt, train, xd) not in reached]
    assert not missing, missing


@pytest.mark.parametrize("name", list(SPECS))
def test_backward_matches_float64(name, ref, cuda):
    """Every non-chained case of the list.  [tile-n2] (two rows, train mode) is the case that found the rounding of mean rstd in the fused kernel's xh
    (docs/FRONTEND_BWD.md "Found"): 5.7 x (dX) and 6.0 x (dgamma) the floor before the per-feature correction xc of that rounding, 0.03 x / 0.16 x with it."""
    c, r64 = ref["cases"][name], ref["r64"][name]
    e32 = ref["e32"][c["group"]]
    got = _episodes(_call(c, cuda))
    if c["xdtype"] != "f32":                               # the 16-bit store of dX: one unit in the last place at |ref|, element by element
        for gb, rb in zip(got, r64):
            slack = _ulp(rb["dx"], fm.XDTYPES[c["xdtype"]])
            excess = np.maximum(np.abs(gb["dx"] - rb["dx"]) - slack, 0.0)
            gb["dx"] = rb["dx"] + excess
    err = fm.errors(got, r64, c["group"])
    print("RATIO %s %s " % (c["group"], name) + " ".join("%s %.3g (%.2f x e32)" % (q, v, v / e32[q] if e32[q] else (0.0 if v == 0 else np.inf)) for q, v in err.items()))
    for gb, rb in zip(got, r64):
        assert (gb["dgamma"] is None) == (rb["dgamma"] is None) and (gb["dbeta"] is None) == (rb["dbeta"] is None)
    for q, v in err.items():
        assert v <= MARGIN * e32[q], (name, q, v, e32[q])


# ---- chained: the forward taken from the GPU -----------------------------------------------------------------------------------------------------
def _autograd(x, gamma, beta, w, g, dtype):
    x = torch.tensor(x, dtype=dtype, requires_grad=True)
    out = []
    for b in range(x.shape[0]):
        gm, bt = (torch.tensor(v, dtype=dtype, requires_grad=True) for v in (gamma, beta))
        zn = torch.nn.functional.normalize(torch.nn.functional.batch_norm(x[b], None, None, gm, bt, True, 0.1, fm.EPS), p=2, dim=1)
        (float(g[b]) * (torch.tensor(w[b], dtype=dtype) * (zn @ zn.T)).sum()).backward()
        out.append(dict(dgamma=gm.grad.double().numpy(), dbeta=bt.grad.double().numpy()))
    for b, o in enumerate(out):
        o["dx"] = x.grad[b].double().numpy()
    return out


@pytest.fixture(scope="module")
def chained():
    cases = {n: fm.make_case(n=n, d=68, b=2, scaled=True, seed=500 + n) for n in fm.PER_NT_N}
    r64 = {n: _autograd(c["x"], c["gamma"], c["beta"], c["w"], c["g"], torch.float64) for n, c in cases.items()}
    r32 = {n: _autograd(c["x"], c["gamma"], c["beta"], c["w"], c["g"], torch.float32) for n, c in cases.items()}
    e32 = {q: max(fm.errors(r32[n], r64[n])[q] for n in cases) for q in fm.QUANTITIES}
    print("chained e32:", {q: "%.3g" % v for q, v in e32.items()})
    return dict(cases=cases, r64=r64, e32=e32)


@pytest.mark.parametrize("n", fm.PER_NT_N)
def test_fused_and_unfused_chain_from_the_gpu_forward(n, chained, cuda):
    """dkt_gram_bn_train -> dkt_gram_bn_bwd against dkt_bn_stats -> dkt_affine_normalize -> dkt_gram_bwd -> dkt_normalize_bn_bwd on the same X and W: two
    independent implementations (episode-resident MFMA, streaming VALU), both against float64 autograd of the whole expression."""
    c, r64, e32 = chained["cases"][n], chained["r64"][n], chained["e32"]
    x, w, g, gamma, beta = (_t(c[k], cuda) for k in ("x", "w", "g", "gamma", "beta"))
    e, rn, st = ops.gram_bn_train(x, gamma, beta, fm.EPS)
    fused = _episodes(ops.gram_bn_bwd(w, e, x, st["a"], st["s"], rn, st["mean"], st["rstd"], g))
    st2 = ops.bn_stats(x, gamma, beta, fm.EPS)
    zn, rn2 = ops.affine_normalize(x, st2["a"], st2["s"])
    chain = _episodes(ops.normalize_bn_bwd(ops.gram_bwd(w, zn, g, unit_rows=True), zn, x, st2["a"], rn2, st2["mean"], st2["rstd"]))
    ef, ec = fm.errors(fused, r64), fm.errors(chain, r64)
    print("RATIO chained n%d " % n + " ".join("%s fused %.3g (%.2f x e32) chain %.3g (%.2f x e32)" % (q, ef[q], ef[q] / e32[q], ec[q], ec[q] / e32[q]) for q in ef))
    for q in ef:
        assert ef[q] <= 3.0 * ec[q] + MARGIN * e32[q], (n, q, ef[q], ec[q], e32[q])


# ---- exact properties ----------------------------------------------------------------------------------------------------------------------------
def _is_zero(t):
    return t is None or bool((t == 0).all())


@pytest.mark.parametrize("n, mode", [(33, "train"), (33, "eval-shared"), (113, "train"), (113, "eval-episode"), (1, "train")], ids=str)
def test_zero_scale_and_zero_w_give_zero(n, mode, cuda):
    c = fm.make_case(n=n, d=132, b=3, mode=mode, scaled=True, seed=n)
    c["g"] = np.array([-2.0, 0.0, 1.0])
    c["w"] = c["w"].copy()
    c["w"][2] = 0.0
    out = _call(c, cuda)
    for b in (1, 2):
        assert all(_is_zero(None if o is None else o[b]) for o in out), b
    assert float(out[0][0].abs().max()) > 0.0 or n == 1


@pytest.mark.parametrize("n, d", [(45, 68), (105, 132)])
def test_zero_row_and_column_of_w_gives_a_zero_row_of_dx_in_eval_mode(n, d, cuda):
    """Eval mode, W[i, :] = W[:, i] = 0: A_i = 0, so dZn_i = 0 and t_i = 0, dY_i = 0 and dX_i = a dY_i = 0 (from the formula; rmax = 0 is the row scale's clamp)."""
    for mode in ("eval-shared", "eval-episode"):
        c = fm.make_case(n=n, d=d, b=2, mode=mode, scaled=True, wkind="zero-row", seed=n)
        dx = _call(c, cuda)[0]
        assert _is_zero(dx[:, n // 3, :]) and float(dx.abs().max()) > 0.0, mode


@pytest.mark.parametrize("n", fm.PER_NT_N)
def test_an_episode_does_not_depend_on_its_neighbours_and_two_runs_agree(n, cuda):
    c = fm.make_case(n=n, d=68, b=3, scaled=True, seed=700 + n)
    whole, again = _call(c, cuda), _call(c, cuda)
    alone = _call(dict(c, **{k: c[k][1:2] for k in ("x", "w", "e", "a", "s", "mean", "rstd", "rnorm", "g")}), cuda)
    for q in range(3):
        assert torch.equal(whole[q], again[q]) and torch.equal(whole[q][1:2], alone[q]), q


@pytest.mark.parametrize("name", ["stream-n161", "stream-n1024", "stream-d68-eval-shared", "mode-n96-eval-shared-scaled", "x16-bf16-n105-d68-train"])
def test_two_runs_of_the_same_call_are_equal(name, ref, cuda):
    a, b = _call(ref["cases"][name], cuda), _call(ref["cases"][name], cuda)
    assert all(p is None and q is None or torch.equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("name", ["tile-n17", "tile-n97", "tile-n128", "mode-n112-eval-shared-scaled", "stream-n321", "stream-d68-eval-episode"])
def test_product_and_twins_libraries_agree_bitwise(name, ref, cuda, monkeypatch):
    """The conftest default (DKT_TWINS=1, no variant switch: the product library), DKT_TWINS=0 and the twins build of the same sources (DKT_TWINS=force)."""
    c = ref["cases"][name]
    base = _call(c, cuda)
    for v in ("0", "force"):
        monkeypatch.setenv("DKT_TWINS", v)
        out = _call(c, cuda)
        assert all(p is None and q is None or torch.equal(p, q) for p, q in zip(base, out)), v


@pytest.mark.parametrize("n", [45, 105])
def test_w_enters_only_through_w_plus_w_transposed(n, ref, cuda):
    """W0 with entries on a 2^-16 grid and its exact half-sum (W0 + W0^T) / 2; a strictly upper-triangular W and its transpose: bit-equal results."""
    sym = ref["cases"]["w-symmetric-n%d" % n]
    assert not np.array_equal(sym["w_pre"], sym["w"]) and np.array_equal(sym["w"], sym["w"].transpose(0, 2, 1))
    a, b = _call(sym, cuda), _call(sym, cuda, w=sym["w_pre"])
    tri = ref["cases"]["w-triangular-n%d" % n]
    c, d = _call(tri, cuda), _call(tri, cuda, w=tri["w"].transpose(0, 2, 1))
    for q in range(3):
        assert torch.equal(a[q], b[q]) and torch.equal(c[q], d[q]), q


# ---- limits: status only, nothing launched ---------------------------------------------------------------------------------------------------------
def test_shape_limits_and_null_pointers_do_not_launch(cuda):
    lib, x16 = L.load(), L.load_x16()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())       # noqa: E731
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731

    def run(call, xdtype, n, d, d_arg=None, null=()):
        """Buffers of the full size (n, d) whatever is refused; outputs pre-filled with -7.  Returns (status, outputs untouched)."""
        dt = fm.XDTYPES[xdtype]
        f = lambda *s: torch.ones(s, device=cuda)                          # noqa: E731
        a = dict(W=f(1, n, n), E=f(1, n, n), X=torch.ones(1, n, d, device=cuda, dtype=dt), a=f(d), s=f(d), mean=f(1, d), rstd=f(1, d), rnorm=f(1, n),
                 dZn=f(1, n, d), Zn=f(1, n, d), ws=f(1, n))
        outs = dict(dX=torch.full((1, n, d), -7.0, device=cuda, dtype=dt), dg=torch.full((1, d), -7.0, device=cuda), db=torch.full((1, d), -7.0, device=cuda))
        a.update(outs)
        v = {k: (None if k in null else p(t)) for k, t in a.items()}
        xd = [] if xdtype == "f32" else [L.X_BF16 if xdtype == "bf16" else L.X_F16]
        dd = d if d_arg is None else d_arg
        if call == "fused":
            fn = lib.dkt_gram_bn_bwd_f32 if xdtype == "f32" else x16.dkt_gram_bn_bwd_x16
            st = fn(v["W"], v["E"], v["X"], *xd, v["a"], v["s"], 0, v["mean"], v["rstd"], v["rnorm"], None, v["dX"], v["dg"], v["db"], 1, n, dd, stream())
        else:
            fn = lib.dkt_normalize_bn_bwd_f32 if xdtype == "f32" else x16.dkt_normalize_bn_bwd_x16
            st = fn(v["dZn"], v["Zn"], v["X"], *xd, v["a"], 0, v["mean"], v["rstd"], v["rnorm"], v["dX"], v["dg"], v["db"], v["ws"], 1, n, dd, stream())
        torch.cuda.synchronize()
        return st, all(bool((o == -7).all()) for o in outs.values())

    for xd in ("f32", "bf16", "f16"):
        assert run("fused", xd, 129, 8) == (-2, True), xd                   # DKT_ERR_TOO_LARGE
        assert run("stream", xd, 1025, 8) == (-2, True), xd
        for call in ("fused", "stream"):
            assert run(call, xd, 16, 8, d_arg=6) == (-1, True), (call, xd)   # DKT_ERR_BAD_ARG
            for null in ("rstd", "dg", "db"):                              # train mode (mean given) without rstd or a part pointer
                assert run(call, xd, 16, 8, null=(null,)) == (-1, True), (call, xd, null)
    assert run("fused", "f32", 128, 8) == (0, False) and run("stream", "f32", 1024, 8) == (0, False)      # the limits themselves run
