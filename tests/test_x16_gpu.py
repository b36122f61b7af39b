"""16-bit trunk features (mixed-precision backbones) through the front end on the GPU: the *_x16 kernels of libdkt_x16.so against the float64 oracle on the
upcast input and against the product's fp32 kernels on x.float(); the training episode and its gradients; the native route (no fp32 copy of X); and the
model layer with amp="bf16" / a caller's own torch.autocast."""
import numpy as np
import pytest
import torch

import dkt_amd
from dkt_amd import ops
from oracle import dkt_oracle as O
from oracle import dkt_oracle_torch as T

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
FE_SHAPES = [(2, 5, 12), (3, 25, 64), (2, 85, 512), (2, 105, 1600), (1, 128, 100), (2, 19, 2916), (5, 1, 36), (2, 33, 8), (2, 150, 512), (1, 420, 512)]
FE_NAMES = ("bn_stats", "gram_bn", "gram_bn_train", "gram_bn_bwd", "affine_normalize", "normalize_bn_bwd")


def rel_l2(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _x16(rng, b, n, d, dtype, dev):
    """ReLU-like trunk outputs with a large common offset per feature, rounded to `dtype`; returns (x16 on the device, its exact float64 value)."""
    x = np.abs(rng.standard_normal((b, n, d))) * rng.uniform(0.2, 3.0, (1, 1, d)) + rng.uniform(0.0, 5.0, (1, 1, d))
    xh = torch.tensor(x, dtype=torch.float32).to(dtype).to(dev)
    return xh, xh.double().cpu().numpy()


def _ulp(v, dtype):
    """Spacing of `dtype` at |v| (subnormals: the smallest subnormal)."""
    fi = torch.finfo(dtype)
    e = np.floor(np.log2(np.maximum(np.abs(v), fi.tiny)))
    return np.maximum(fi.eps * np.exp2(e), fi.tiny * fi.eps)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("b,n,d", FE_SHAPES)
def test_x16_forward_ops_match_float64_and_the_fp32_kernels(cuda, dtype, b, n, d):
    rng = np.random.default_rng(n * 41 + d)
    xh, x64 = _x16(rng, b, n, d, dtype, cuda)
    gamma = torch.tensor(rng.uniform(0.5, 1.5, d), dtype=torch.float32, device=cuda)
    beta = torch.tensor(rng.normal(0.0, 0.2, d), dtype=torch.float32, device=cuda)
    g64, b64 = gamma.double().cpu().numpy(), beta.double().cpu().numpy()
    xf = xh.float()
    st = ops.bn_stats(xh, gamma, beta, 1e-5)
    st_ref = ops.bn_stats(xf, gamma, beta, 1e-5)
    same = all(torch.equal(st[k], st_ref[k]) for k in st)
    for i in range(b):
        y, mu, var_u = O.batchnorm1d_train(x64[i], g64, b64)
        assert np.abs(st["mean"][i].cpu().numpy() - mu).max() < 1e-5 * (1.0 + np.abs(mu).max())
        if n > 1:
            assert rel_l2(st["var_unbiased"][i].cpu().numpy(), var_u) < 2e-5
        assert rel_l2(st["a"][i].cpu().numpy(), g64 / np.sqrt(x64[i].var(0) + 1e-5)) < 2e-5
    for k in st:
        assert rel_l2(st[k].cpu().numpy(), st_ref[k].cpu().numpy()) < 2e-5, k
    # Zn of the streaming front end (any N) and, for N <= 128, the fused Gram kernels
    zn, rn = ops.affine_normalize(xh, st["a"], st["s"])
    zn_ref, rn_ref = ops.affine_normalize(xf, st["a"], st["s"])
    assert zn.dtype == torch.float32
    assert (zn - zn_ref).abs().max().item() < 2e-5 and rel_l2(rn.cpu().numpy(), rn_ref.cpu().numpy()) < 2e-5
    same = same and torch.equal(zn, zn_ref) and torch.equal(rn, rn_ref)
    if n > 1:
        for i in range(b):
            y, _, _ = O.batchnorm1d_train(x64[i], g64, b64)
            assert np.abs(zn[i].cpu().numpy() - O.l2_normalize(y)).max() < 2e-5
    if n <= 128:
        e, rnorm, st1 = ops.gram_bn_train(xh, gamma, beta, 1e-5)
        e_ref, rnorm_ref, st1_ref = ops.gram_bn_train(xf, gamma, beta, 1e-5)
        e2, rnorm2 = ops.gram_bn(xh, st["a"], st["s"])
        e2_ref, _ = ops.gram_bn(xf, st["a"], st["s"])
        for k in st1:
            assert rel_l2(st1[k].cpu().numpy(), st1_ref[k].cpu().numpy()) < 2e-5, k
        assert torch.equal(e, e.transpose(1, 2)) and torch.equal(e2, e2.transpose(1, 2))
        if n > 1:
            for i in range(b):
                y, _, _ = O.batchnorm1d_train(x64[i], g64, b64)
                zn64 = O.l2_normalize(y)
                ref = zn64 @ zn64.T
                assert np.abs(e[i].cpu().numpy() - ref).max() < 2e-5
                assert np.abs(e2[i].cpu().numpy() - ref).max() < 2e-5
                assert rel_l2(rnorm[i].cpu().numpy(), 1.0 / np.linalg.norm(y, axis=1)) < 2e-5
            assert (e - e_ref).abs().max().item() < 2e-5 and (e2 - e2_ref).abs().max().item() < 2e-5
        same = same and torch.equal(e, e_ref) and torch.equal(rnorm, rnorm_ref) and torch.equal(e2, e2_ref)
        same = same and all(torch.equal(st1[k], st1_ref[k]) for k in st1)
    print("x16 forward vs fp32 kernels on x.float(): %s" % ("bitwise equal" if same else "NOT bitwise equal"))


EP_SHAPES = [(2, 5, 5, 64), (2, 5, 21, 1600), (3, 5, 17, 512), (2, 3, 6, 40), (1, 2, 64, 128), (2, 5, 30, 64), (2, 20, 21, 128), (1, 3, 67, 36),
             (2, 5, 21, 64), (1, 20, 21, 64)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("b,c,per,d", EP_SHAPES)
def test_x16_training_episode_matches_float64_autograd(cuda, dtype, b, c, per, d):
    n = c * per
    rng = np.random.default_rng(b * 100 + n + d)
    xh, x64n = _x16(rng, b, n, d, dtype, cuda)
    gamma = rng.uniform(0.5, 1.5, d).astype(np.float32)
    beta = rng.normal(0.0, 0.2, d).astype(np.float32)
    raw_s = rng.normal(0.0, 0.5, c).astype(np.float32)
    mean = rng.normal(0.0, 0.1, c).astype(np.float32)
    xt = xh.clone().requires_grad_(True)
    t = lambda a: torch.tensor(a, dtype=torch.float32, device=cuda).requires_grad_(True)  # noqa: E731
    gt, bt, rst, mt = t(gamma), t(beta), t(raw_s), t(mean)
    noise = torch.full((c,), 0.1, device=cuda)
    cls = torch.arange(c, device=cuda).repeat_interleave(per)
    y = torch.where(cls.unsqueeze(0) == torch.arange(c, device=cuda).unsqueeze(1), 1.0, -1.0).contiguous()
    cw = torch.full((c,), -1.0 / (c * n), device=cuda)
    obj, logp, alpha, info, jit, e, bmean, bvar = ops.episode_loss_bn(xt, gt, bt, y, torch.nn.functional.softplus(rst), mt, noise, cw)
    assert int(info.abs().max().item()) == 0 and obj.dtype == torch.float32
    w_ep = torch.linspace(0.5, 1.5, b, device=cuda)
    (obj * w_ep).sum().backward()
    x64 = torch.tensor(x64n, dtype=torch.float64, requires_grad=True)
    g64, b64 = torch.tensor(gamma, dtype=torch.float64, requires_grad=True), torch.tensor(beta, dtype=torch.float64, requires_grad=True)
    rs64, m64 = torch.tensor(raw_s, dtype=torch.float64, requires_grad=True), torch.tensor(mean, dtype=torch.float64, requires_grad=True)
    total = 0.0
    for i in range(b):
        zi = torch.nn.functional.batch_norm(x64[i], None, None, g64, b64, True, 0.1, 1e-5)
        loss_i, _, _ = T.classification_loss(zi, c, torch.nn.functional.softplus(rs64), m64, torch.full((c,), 0.1, dtype=torch.float64), normalize=True)
        assert abs(obj[i].item() - loss_i.item()) < 1e-4 * abs(loss_i.item())
        total = total + float(w_ep[i].item()) * loss_i
    total.backward()
    assert xt.grad.dtype == dtype
    for got, ref in ((gt, g64), (bt, b64), (rst, rs64), (mt, m64)):
        assert rel_l2(got.grad.cpu().numpy(), ref.grad.numpy()) < 1e-3
    dx = xt.grad.double().cpu().numpy()
    dx64 = x64.grad.numpy()
    tol = _ulp(dx64, dtype) + 1e-5 * np.abs(dx64).max()
    assert (np.abs(dx - dx64) <= tol).all(), float((np.abs(dx - dx64) / tol).max())
    assert rel_l2(bmean.cpu().numpy(), x64n.mean(1)) < 1e-5


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("b,c,per,d", [(64, 5, 21, 1600), (8, 20, 21, 512)])
def test_x16_training_step_is_native(cuda, dtype, b, c, per, d):
    """16-bit X runs the *_x16 kernels and none of the fp32 front-end kernels, and no fp32 copy of X is made: at N <= 128 (nothing of size N x D is
    allocated on the way) the step's peak allocation stays below one; beyond 128 rows (Zn is written in fp32 by design, the marginal likelihood takes a
    workspace) it stays below the peak of the same step on X.float() by at least one such copy."""
    n = c * per
    rng = np.random.default_rng(7)
    xh, _ = _x16(rng, b, n, d, dtype, cuda)
    xt = xh.requires_grad_(True)
    gamma = torch.ones(d, device=cuda, requires_grad=True)
    beta = torch.zeros(d, device=cuda, requires_grad=True)
    cls = torch.arange(c, device=cuda).repeat_interleave(per)
    y = torch.where(cls.unsqueeze(0) == torch.arange(c, device=cuda).unsqueeze(1), 1.0, -1.0).contiguous()
    sv, mean, noise = torch.ones(c, device=cuda), torch.zeros(c, device=cuda), torch.full((c,), 0.1, device=cuda)
    cw = torch.full((c,), -1.0 / (c * n), device=cuda)

    def step_peak(cast):
        xt.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        obj = ops.episode_loss_bn(xt.float() if cast else xt, gamma, beta, y, sv, mean, noise, cw)[0]
        obj.mean().backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    copy = xt.numel() * 4
    if n <= 128:
        assert step_peak(False) < copy, (step_peak(False), copy)
    else:
        step_peak(True)                                   # (warm: the first call of a shape sizes the cached workspaces)
        native, cast = step_peak(False), step_peak(True)
        assert native + copy <= cast, (native, cast, copy)
    xt.grad = None
    ops.kernel_timing(True)
    try:
        obj = ops.episode_loss_bn(xt, gamma, beta, y, sv, mean, noise, cw)[0]
        obj.mean().backward()
        torch.cuda.synchronize()
        names = set(ops.kernel_timing_results())
    finally:
        ops.kernel_timing(False)
    assert xt.grad.dtype == dtype and torch.isfinite(xt.grad.float()).all()
    want = {"dkt_gram_bn_train_x16", "dkt_gram_bn_bwd_x16"} if n <= 128 else {"dkt_bn_stats_x16", "dkt_affine_normalize_x16", "dkt_normalize_bn_bwd_x16"}
    assert want <= names, names
    assert not any("dkt_%s_f32" % k in names for k in FE_NAMES), names


class _Loader:
    def __init__(self, n_ep, n_way, per, hw, seed):
        g = torch.Generator().manual_seed(seed)
        self.x = [torch.rand(n_way, per, 3, hw, hw, generator=g) for _ in range(n_ep)]

    def __len__(self):
        return len(self.x)

    def __iter__(self):
        return iter((x, None) for x in self.x)


@pytest.mark.parametrize("way", [5, 20])
def test_dkt_amp_bf16_train_loop(cuda, capsys, way):
    torch.manual_seed(0)
    m = dkt_amd.DKT(dkt_amd.backbone.Conv4S, n_way=way, n_support=5, amp="bf16").to(cuda)
    bn = m.feature_extractor.trunk.bn_out
    before = [p.detach().clone() for p in m.parameters()]
    rm = bn.running_mean.clone()
    m.train()
    ops.kernel_timing(True)
    try:
        m.train_loop(0, _Loader(3, way, 21, 28, 0), None)
        torch.cuda.synchronize()
        names = set(ops.kernel_timing_results())
    finally:
        ops.kernel_timing(False)
    assert "Epoch [0] [0/3]" in capsys.readouterr().out
    assert torch.isfinite(m._last["loss"]) and float(m._bad_steps.item()) == 0.0
    assert all(p.dtype == torch.float32 for p in m.parameters())
    assert sum(not torch.equal(a, p.detach()) for a, p in zip(before, m.parameters())) >= len(before) // 2
    assert not torch.equal(rm, bn.running_mean) and int(bn.num_batches_tracked) == 3
    want = "dkt_gram_bn_train_x16" if way == 5 else "dkt_affine_normalize_x16"
    assert want in names and not any("dkt_%s_f32" % k in names for k in FE_NAMES), names


@pytest.mark.parametrize("way", [5, 20])
def test_dkt_amp_bf16_train_loop_in_a_hip_graph(cuda, capsys, monkeypatch, way):
    losses = {}
    for graph in ("0", "1"):
        monkeypatch.setenv("DKT_TRAIN_GRAPH", graph)
        torch.manual_seed(0)
        m = dkt_amd.DKT(dkt_amd.backbone.Conv4S, n_way=way, n_support=5, amp="bf16").to(cuda)
        m.train()
        g = torch.Generator().manual_seed(1)
        loader = [(torch.rand(way, 21, 3, 28, 28, generator=g), None) for _ in range(4)]
        m.train_loop(0, loader, None, print_freq=2)
        losses[graph] = float(m._last["loss"])
        assert np.isfinite(losses[graph])
    capsys.readouterr()
    assert abs(losses["1"] - losses["0"]) < 1e-2 * abs(losses["0"])


def test_plain_dkt_trains_inside_a_callers_f16_autocast(cuda, capsys):
    torch.manual_seed(0)
    m = dkt_amd.DKT(dkt_amd.backbone.Conv4S, n_way=5, n_support=5).to(cuda)
    before = m.model.raw_outputscale.detach().clone()
    m.train()
    with torch.autocast("cuda", dtype=torch.float16):
        m.train_loop(0, _Loader(3, 5, 21, 28, 0), None)
    capsys.readouterr()
    assert torch.isfinite(m._last["loss"]) and not torch.equal(before, m.model.raw_outputscale.detach())
    assert all(torch.isfinite(p).all() for p in m.parameters())


def test_dkt_amp_bf16_test_loop_correct_and_logits(cuda, capsys):
    torch.manual_seed(0)
    m = dkt_amd.DKT(dkt_amd.backbone.Conv4S, n_way=5, n_support=5, amp="bf16").to(cuda)
    m.train()
    m.train_loop(0, _Loader(2, 5, 21, 28, 0), None)
    m.eval()
    acc, std = m.test_loop(_Loader(4, 5, 20, 28, 1), return_std=True)
    assert 0.0 <= acc <= 100.0 and std >= 0.0
    x = _Loader(1, 5, 20, 28, 2).x[0]
    m.n_query = 15
    top1, count, avg_loss = m.correct(x)
    logits = m.get_logits(x)
    assert count == 75 and logits.shape == (75, 5) and logits.dtype == torch.float32
    with torch.no_grad():
        xs, xq = m._split(x)
        assert m._embed(xs).dtype == torch.float32
        # the model's own features: the bf16 trunk output of the one backbone pass the fused test episode takes over [support; query], upcast to
        # float64, then bn_out (eval mode) and F.normalize in float64 (bf16 convolutions round differently per batch: features of other passes differ at
        # bf16 resolution)
        f = m._trunk_features(torch.cat([xs, xq], 0))
        assert f.dtype == torch.bfloat16
        f = f.double().cpu().numpy()
    bn = m.feature_extractor.trunk.bn_out
    g64 = lambda t: t.detach().double().cpu().numpy()  # noqa: E731
    y64 = (f - g64(bn.running_mean)) / np.sqrt(g64(bn.running_var) + bn.eps) * g64(bn.weight) + g64(bn.bias)
    zn = O.l2_normalize(y64)
    zs, zq = zn[:25], zn[25:]
    hyp = O.GPHypers(m.model.outputscale.detach().cpu().numpy().astype(np.float64),
                     m.model.mean.detach().cpu().numpy().astype(np.float64), np.full(5, 0.1))
    ref = O.eval_episode(zs, zq, 5, hyp)
    assert np.abs(logits.cpu().numpy() - ref["logits"]).max() < 1e-3
    top1b, countb, avg = m.correct(x, N=2)
    assert countb == 75 and np.isfinite(avg)
    capsys.readouterr()


@pytest.mark.parametrize("kernel", ["rbf", "spectral"])
def test_dkt_regression_amp_bf16_trains(cuda, capsys, kernel):
    torch.manual_seed(0)
    m = dkt_amd.DKTRegression(dkt_amd.backbone.Conv3(), kernel, amp="bf16").to(cuda)
    g = torch.Generator().manual_seed(3)
    inputs = torch.rand(2, 19, 3, 100, 100, generator=g)
    labels = torch.rand(2, 19, generator=g) * 2.0 - 1.0
    before = [p.detach().clone() for p in m.parameters()]
    opt = torch.optim.Adam([{"params": m.model.parameters(), "lr": 1e-3}, {"params": m.feature_extractor.parameters(), "lr": 1e-3}])
    m.train()
    m.train_loop(0, opt, inputs, labels)
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, m.feature_extractor.parameters()))
    assert all(torch.isfinite(p).all() for p in m.parameters())
    mse = m.test_loop(5, None, inputs, labels)
    assert torch.isfinite(mse)
    capsys.readouterr()


def test_drivers_honour_amp_flag(cuda, capsys, monkeypatch, tmp_path):
    """`--amp bf16` on the command line reaches the model of train.py and of test_uncertainty.py (which builds its DKT without passing the flag on:
    io_utils.parse_args sets configs.amp): the 16-bit front-end kernels run, none of the fp32 ones."""
    import train
    import test_uncertainty
    from dkt_amd import configs
    monkeypatch.setattr(configs, "amp", None)
    monkeypatch.setattr(configs, "kernel_type", configs.kernel_type)
    monkeypatch.chdir(tmp_path)                                   # (checkpoints go to ./save/)
    for run in (lambda: train.main(["--model", "Conv4S", "--n_episode", "2", "--stop_epoch", "1", "--amp", "bf16"]),
                lambda: test_uncertainty.main(["--model", "Conv4S", "--n_episode", "2", "--repeat", "1", "--amp", "bf16"])):
        ops.kernel_timing(True)
        try:
            run()
            torch.cuda.synchronize()
            names = set(ops.kernel_timing_results())
        finally:
            ops.kernel_timing(False)
        assert any(k.endswith("_x16") for k in names), names
        assert not any("dkt_%s_f32" % k in names for k in FE_NAMES), names
    assert configs.amp == "bf16"
    capsys.readouterr()
