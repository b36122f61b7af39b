"""libdkt_gpc.so on the GPU against the float64 restatement of scikit-learn's Laplace GP classifier (tests/laplace_model.py; test_laplace_host.py shows
that restatement equal to sklearn to 1e-12), and the DKT surface on top of it.

Tolerances are not constants: for each compared quantity, e32 is the largest absolute error of the float32 restatement (numpy / LAPACK, everything
fp32 except the five-term mixture) against float64 over the whole case list below -- the fp32 floor of the reference itself -- and the kernel is
allowed 4 x e32 (its sums run in another order than LAPACK's).  docs/LAPLACE.md records e32 and the kernel's measured errors."""
import ctypes
import sys

import numpy as np
import pytest
import torch

import dkt_amd
import laplace_model as lm

pytestmark = pytest.mark.gpu
ops, L = dkt_amd.ops, dkt_amd._lib
QUANTITIES = ("f", "g", "lml", "mu", "var", "prob")
# tile edges: (N, M) with targets given directly (two binary problems over three clusters), B = 2
EDGES = [(1, 1), (15, 63), (16, 65), (17, 1), (33, 63), (127, 65)]


def _edge_case(n, m):
    rng = np.random.default_rng(100 * n + m)
    shots = (n + 2) // 3
    rows = np.sort(rng.permutation(3 * shots)[:n])                       # N of the 3 * shots rows; their clusters are the targets' classes
    cls = rows // shots
    eps = []
    for _ in range(2):
        zs, zq = lm.clustered(rng, 3, shots, m, 64, 0.1)
        eps.append((zs[rows], zq))
    k = np.stack([lm.rbf(zs, zs, 0.1) for zs, _ in eps]).astype(np.float32).astype(np.float64)
    ks = np.stack([lm.rbf(zq, zs, 0.1) for zs, zq in eps]).astype(np.float32).astype(np.float64)
    return dict(k=k, ks=ks, kss=np.ones((2, m)), y=np.stack([cls == 0, cls == 1]).astype(np.float64))


def _deep_case():
    """The model's own kernel: K_c = sv_c E with E the cosine similarity of unit features, sv alternating 0.5 / 5 over the classes; per-class K."""
    rng = np.random.default_rng(77)
    sv = np.array([0.5, 5.0, 0.5, 5.0, 0.5])
    zs, zq = zip(*(lm.clustered(rng, 5, 5, 80, 64, 0.3) for _ in range(2)))
    e = np.stack([z @ z.T for z in zs]).astype(np.float32).astype(np.float64)
    ex = np.stack([q @ z.T for z, q in zip(zs, zq)]).astype(np.float32).astype(np.float64)
    return dict(k=sv[None, :, None, None] * e[:, None], ks=sv[None, :, None, None] * ex[:, None], kss=np.tile(sv[None, :, None], (2, 1, 80)),
                y=lm.one_vs_rest(5, 5))


def _solve(d, dtype):
    md = lm.mode(d["k"], d["y"], dtype=dtype)
    mu, var, prob, labels = lm.predict(d["ks"], d["kss"], md, dtype=dtype)
    return dict(f=md["f"], g=md["g"], lml=md["lml"], iters=md["iters"], mu=mu, var=var, prob=prob, labels=labels)


@pytest.fixture(scope="module")
def ref():
    """Every case once: inputs, the float64 and float32 restatements, and e32 per quantity over the whole list.  Read-only."""
    cases = {("table",) + c: lm.build_case(c) for c in lm.CASES}
    cases.update({("edge", n, m): _edge_case(n, m) for n, m in EDGES})
    cases[("deep",)] = _deep_case()
    cases[("near-identity",)] = lm.build_case(lm.NEAR_IDENTITY_CASE)
    r64 = {k: _solve(d, np.float64) for k, d in cases.items()}
    r32 = {k: _solve(d, np.float32) for k, d in cases.items()}
    e32 = {q: max(float(np.abs(r32[k][q].astype(np.float64) - r64[k][q]).max()) for k in cases) for q in QUANTITIES}
    print("e32:", {q: "%.3g" % v for q, v in e32.items()})
    return dict(cases=cases, r64=r64, e32=e32)


def _t(a, cuda):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(cuda)


def _gpu(d, cuda):
    md = ops.laplace_mode(_t(d["k"], cuda), _t(d["y"], cuda))
    mu, var, prob, labels = ops.laplace_predict(_t(d["ks"], cuda), _t(d["kss"], cuda), md)
    return dict(f=md["f"], g=md["g"], lml=md["lml"], iters=md["iters"], w_sr=md["w_sr"], chol=md["chol"], mu=mu, var=var, prob=prob, labels=labels)


def _errors(got, want):
    return {q: float(np.abs(got[q].double().cpu().numpy() - want[q]).max()) for q in QUANTITIES}


def _check(key, ref, cuda, quantities=QUANTITIES):
    got = _gpu(ref["cases"][key], cuda)
    err = _errors(got, ref["r64"][key])
    iters = got["iters"].cpu().numpy()
    print(key, "iters gpu", int(iters.min()), int(iters.max()), "float64", int(ref["r64"][key]["iters"].max()),
          {q: "%.3g (%.2f x e32)" % (err[q], err[q] / ref["e32"][q]) for q in quantities})
    assert (iters < 100).all() and (iters >= 1).all()
    for q in quantities:
        assert err[q] <= 4 * ref["e32"][q], (key, q, err[q], ref["e32"][q])
    return got


@pytest.mark.parametrize("case", lm.CASES, ids=str)
def test_mode_and_predict_match_float64_and_sklearn_labels(case, ref, cuda):
    from sklearn.gaussian_process import GaussianProcessClassifier
    from sklearn.gaussian_process.kernels import RBF
    key = ("table",) + case
    got = _check(key, ref, cuda)
    b_, c, n, m, _, _, ls = case
    d, labels = ref["cases"][key], got["labels"].cpu().numpy()
    srt = np.sort(ref["r64"][key]["prob"], axis=1)
    decided = (srt[:, -1] - srt[:, -2]) > 100 * ref["e32"]["prob"]                           # [B, M]
    print(key, "smallest float64 top-two margin %.3g, excluded %d of %d" % ((srt[:, -1] - srt[:, -2]).min(), (~decided).sum(), decided.size))
    assert (~decided).mean() <= 0.02
    for b in range(b_):
        sk = GaussianProcessClassifier(1.0 * RBF(ls), optimizer=None).fit(d["zs"][b], np.repeat(np.arange(c), n // c)).predict(d["zq"][b])
        assert (labels[b] == sk)[decided[b]].all()


@pytest.mark.parametrize("n, m", EDGES)
def test_tile_edges(n, m, ref, cuda):
    _check(("edge", n, m), ref, cuda)


def test_the_models_own_kernel_per_class(ref, cuda):
    got = _check(("deep",), ref, cuda)
    r64 = ref["r64"][("deep",)]
    srt = np.sort(r64["prob"], axis=1)
    decided = (srt[:, -1] - srt[:, -2]) > 100 * ref["e32"]["prob"]
    assert (~decided).mean() <= 0.02 and (got["labels"].cpu().numpy() == r64["labels"])[decided].all()


def test_near_identity_kernel_probabilities_only(ref, cuda):
    """spread 0.3 at lengthscale 0.1: K is the identity to 1e-5, the top-two margins (4e-7 .. 5e-5) are below fp32: no label claim."""
    _check(("near-identity",), ref, cuda, quantities=("prob",))


@pytest.mark.parametrize("key", [("table",) + lm.CASES[1], ("table",) + lm.CASES[3], ("edge", 17, 1)], ids=str)
def test_shared_and_per_class_forms_are_bitwise_equal_and_reproducible(key, ref, cuda):
    d = ref["cases"][key]
    c = d["y"].shape[0]
    shared = _gpu(d, cuda)
    again = _gpu(d, cuda)
    b_, m = d["kss"].shape
    per_class = _gpu(dict(k=np.repeat(d["k"][:, None], c, 1), ks=np.repeat(d["ks"][:, None], c, 1), kss=np.repeat(d["kss"][:, None], c, 1),
                          y=np.repeat(d["y"][None], b_, 0)), cuda)
    for q in shared:
        assert torch.equal(shared[q], again[q]), q
        assert torch.equal(shared[q], per_class[q]), q


@pytest.mark.parametrize("c", [1, 2, 5])
def test_far_queries(c, ref, cuda):
    """30 * 1 is far from every support point: Ks underflows to 0, every class gives the same probability and the LAST one wins; the two-class
    problem (C = 1) follows the binary rule mu > 0, so 0."""
    d = ref["cases"][("table",) + lm.CASES[1]]
    zs, far = d["zs"][0], np.full((3, 64), 30.0)
    ks = lm.rbf(far, zs, 0.1)[None]
    assert (ks == 0).all()
    got = _gpu(dict(k=d["k"][:1], ks=ks, kss=np.ones((1, 3)), y=d["y"][:c]), cuda)
    assert (got["labels"].cpu().numpy() == (c - 1 if c > 1 else 0)).all()
    assert (got["mu"] == 0).all() and (got["var"] == 1).all() and (got["prob"] == got["prob"][0, 0, 0]).all()
    assert abs(float(got["prob"][0, 0, 0]) - 0.5) < 1e-6


def test_shape_limits_fail_before_any_launch(cuda):
    lib = L.load_gpc()
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def run(c, n):
        k, y = torch.eye(n, device=cuda).repeat(1, 1, 1).contiguous(), torch.zeros(c, n, device=cuda)
        outs = [torch.full(s, -7.0, device=cuda) for s in ((1, c, n), (1, c, n), (1, c, n), (1, c, n, n), (1, c))] + [
            torch.full((1, c), -7, device=cuda, dtype=torch.int32)]
        st = lib.dkt_gpc_mode_f32(p(k), n * n, 0, p(y), 0, *[p(o) for o in outs], 1, c, n, 100, None)
        pouts = [torch.full((1, c, 4), -7.0, device=cuda) for _ in range(3)] + [torch.full((1, 4), -7, device=cuda, dtype=torch.int32)]
        ks, kss = torch.zeros(1, 4, n, device=cuda), torch.ones(1, 4, device=cuda)
        st2 = lib.dkt_gpc_predict_f32(p(ks), 4 * n, 0, p(kss), 4, 0, p(outs[1]), p(outs[2]), p(outs[3]), *[p(o) for o in pouts], 1, c, 4, n, None)
        torch.cuda.synchronize()
        return st, st2, all(bool((o == -7).all()) for o in outs + pouts)

    assert run(5, 128) == (-5, -5, True) and run(33, 10) == (-5, -5, True)
    st, st2, untouched = run(32, 127)
    assert (st, st2, untouched) == (0, 0, False)
    assert not ops.laplace_supported(128, 5) and not ops.laplace_supported(10, 33) and ops.laplace_supported(127, 32)
    with pytest.raises(RuntimeError, match="DKT_ERR_SHAPE"):
        ops.laplace_mode(torch.eye(128, device=cuda)[None], torch.zeros(2, 128, device=cuda))


# ---- the DKT surface --------------------------------------------------------------------------------------------------------------------------
def _model(cuda, n_way=5, n_support=5, **kw):
    torch.manual_seed(0)
    m = dkt_amd.DKT(dkt_amd.backbone.Conv4S, n_way=n_way, n_support=n_support, **kw).to(cuda)
    m.eval()
    m.n_query = 16
    return m


def _episode(n_way=5, per_class=21, seed=2):
    return torch.rand(n_way, per_class, 3, 28, 28, generator=torch.Generator().manual_seed(seed))


def _count(monkeypatch, name):
    calls, fn = [], getattr(ops, name)
    monkeypatch.setattr(ops, name, lambda *a, **k: (calls.append(1), fn(*a, **k))[1])
    return calls


def test_correct_laplace_runs_on_the_device_without_sklearn(cuda, monkeypatch):
    m, x = _model(cuda), _episode()
    monkeypatch.setitem(sys.modules, "sklearn.gaussian_process", None)          # `from sklearn.gaussian_process import ...` raises ImportError
    calls, read_back, cpu = _count(monkeypatch, "laplace_mode"), [], torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **k: (read_back.append(tuple(t.shape)), cpu(t, *a, **k))[1])
    top1, count, avg_loss = m.correct(x, laplace=True)
    assert isinstance(top1, float) and 0.0 <= top1 <= 80.0 and (count, avg_loss) == (80, 0.0)
    assert len(calls) == 1 and read_back == [(2,)]                              # one mode launch; only the stats tensor comes back, no features
    md = m._last["laplace_mode"]
    assert md["f"].shape == (1, 5, 25) and int(md["iters"].max()) < 100


def test_correct_laplace_beyond_127_rows_takes_the_sklearn_route(cuda, monkeypatch):
    m, x = _model(cuda, n_support=26), _episode(per_class=28)
    m.n_query = 2
    calls = _count(monkeypatch, "laplace_mode")
    top1, count, avg_loss = m.correct(x, laplace=True)
    assert isinstance(top1, float) and 0.0 <= top1 <= 10.0 and (count, avg_loss) == (10, 0.0) and not calls
    with pytest.raises(RuntimeError, match="up to 127 support rows"):
        m.correct(x, laplace="deep")


def test_two_way_episode_is_one_binary_problem(cuda):
    m = _model(cuda, n_way=2)
    x = _episode(n_way=2)
    top1, count, _ = m.correct(x, laplace=True)
    assert m._last["laplace_mode"]["f"].shape == (1, 1, 10) and count == 32 and 0.0 <= top1 <= 32.0
    proba = m.laplace_proba(x)
    assert proba.shape == (32, 2) and float((proba.sum(1) - 1).abs().max()) <= 1e-6


@pytest.mark.parametrize("kernel_type", ["bncossim", "rbf"])
def test_deep_kernel_and_proba(cuda, kernel_type):
    m = _model(cuda, kernel_type=kernel_type)
    xs = torch.stack([_episode(seed=s) for s in (2, 3, 4)])
    top1, count, avg_loss = m.correct(xs[0], laplace="deep")
    assert isinstance(top1, float) and 0.0 <= top1 <= 80.0 and (count, avg_loss) == (80, 0.0)
    for kernel in ("rbf0.1", "deep"):
        batched = m.laplace_proba(xs, kernel, batched=True)
        assert batched.shape == (3, 80, 5) and float((batched.sum(2) - 1).abs().max()) <= 1e-6
        assert bool(((batched > 0) & (batched < 1)).all())
        for b in range(3):
            assert torch.equal(m.laplace_proba(xs[b], kernel), batched[b]), (kernel, b)
    with pytest.raises(ValueError):
        m.laplace_proba(xs[0], "rbf")


def test_test_loop_honours_the_laplace_attribute(cuda, monkeypatch, capsys):
    m = _model(cuda)
    loader = [(_episode(seed=s), None) for s in (5, 6)]
    calls = _count(monkeypatch, "laplace_mode")
    assert m.laplace is False
    m.test_loop(loader)
    assert not calls
    m.laplace = True
    acc = m.test_loop(loader)
    assert len(calls) == 2 and 0.0 <= acc <= 100.0
