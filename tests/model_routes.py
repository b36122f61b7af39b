"""The model-level routes of dkt_amd.DKT, dkt_regression.DKT and SinesDKT, each defined once: a name, the environment it needs, a callable that builds a seeded
model and seeded inputs on the device and returns (model, call), and the library launches the call makes, in order of first launch, with their counts, as
ops.kernel_timing records them.  `run` executes one: every output tensor, every parameter gradient, every parameter and buffer after the call (the training routes
take one Adam step) and what the call printed.  tests/test_model_routes_gpu.py pins the launch lists; the same routes serve bit-for-bit comparisons between two
commits.  The backbone is Flatten + Linear over 1x4x4 images, so that no convolution algorithm choice enters a comparison."""
import contextlib
import io

import torch
import torch.nn as nn

import dkt_amd
from dkt_amd import ops
from dkt_amd.dkt_regression import DKT as RegressionDKT
from dkt_amd.sines import SinesDKT
from episode_routes import _environment


class Tiny(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.trunk = nn.Sequential(nn.Flatten(), nn.Linear(16, d))
        self.final_feat_dim = d

    def forward(self, x):
        return self.trunk(x)


class Loader:
    def __init__(self, n_ep, n_way, per, seed):
        self.x = list(_images(seed, n_ep, n_way, per))

    def __len__(self):
        return len(self.x)

    def __iter__(self):
        return iter((x, None) for x in self.x)


def _images(seed, *shape):
    return torch.rand(*shape, 1, 4, 4, generator=torch.Generator().manual_seed(seed))


def _model(dev, kernel, n_way=5, n_support=2, d=64, momentum=0.1, **kw):
    """A seeded DKT over the tiny backbone: distinct hyper-parameters per class, bn_out with running statistics that are not the initial ones."""
    torch.manual_seed(0)
    m = dkt_amd.DKT(lambda: Tiny(d), n_way=n_way, n_support=n_support, kernel_type=kernel, **kw)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        m.model.raw_outputscale.copy_(torch.rand(n_way, generator=g) - 0.4)
        m.model.mean_constant.copy_(0.2 * torch.rand(n_way, generator=g) - 0.1)
        if m.model.raw_lengthscale is not None:
            m.model.raw_lengthscale.copy_(torch.rand(n_way, generator=g) - 0.5)
        bn = getattr(m.feature_extractor.trunk, "bn_out", None)
        if bn is not None:
            bn.momentum = momentum
            bn.running_mean.copy_(0.1 * torch.randn(d, generator=g))
            bn.running_var.copy_(0.5 + torch.rand(d, generator=g))
            bn.weight.copy_(1.0 + 0.2 * torch.randn(d, generator=g))
            bn.bias.copy_(0.1 * torch.randn(d, generator=g))
            bn.num_batches_tracked.fill_(2)
    return m.to(dev)


def train(dev, kernel, nb=1, n_way=5, per=5, n_support=2, d=64, logits=False, **kw):
    """_train_forward + backward + one Adam step on nb episodes; logits=True: then get_logits of the first episode."""
    m = _model(dev, kernel, n_way, n_support, d, **kw)
    x = _images(2, nb, n_way, per)
    n_ep = n_way * per

    def call():
        m.train()
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        loss, aux, z_train, fused = m._train_forward(x.view(nb * n_ep, 1, 4, 4).to(dev), m._targets(n_way, per, dev), nb, n_ep, True)
        loss.backward()
        opt.step()
        outs = dict(aux, loss=loss.detach(), z_train=z_train.detach(), fused=torch.tensor(float(fused)))
        if logits:
            m.eval()
            m.n_query = per - n_support
            outs["logits"] = m.get_logits(x[0])
        return outs
    return m, call


def correct(dev, kernel, N=0, laplace=False, n_way=5, proba=None, logits=False, n_support=2, n_query=3, episode=True, dirichlet_proba=None, loo_accuracy=False,
            **kw):
    """_correct_device (correct when N > 0) on one eval-mode test episode, n_support 2 and n_query 3 unless given; proba: also laplace_proba; logits: also
    get_logits; dirichlet_proba: also dirichlet_proba with that many samples; loo_accuracy: also loo_accuracy and what it left in _last["loo"]; episode=False:
    only those, no _correct_device."""
    m = _model(dev, kernel, n_way, n_support, **kw)
    x = _images(3, n_way, n_support + n_query)

    def call():
        m.eval()
        m.n_query = n_query
        outs = {}
        if logits:
            outs["logits"] = m.get_logits(x)
        if dirichlet_proba is not None:
            outs["dirichlet_proba"] = m.dirichlet_proba(x, samples=dirichlet_proba)
        if loo_accuracy:
            outs["loo_accuracy"] = torch.tensor(m.loo_accuracy(x), dtype=torch.float64)
            outs.update({"loo_" + k: v for k, v in m._last["loo"].items()})
        if not episode:
            return outs
        if N > 0:
            top1, count, avg_loss = m.correct(x, N=N, laplace=laplace)
            outs.update(top1=torch.tensor(top1), avg_loss=torch.tensor(avg_loss, dtype=torch.float64))
        else:
            outs["stats"], count, _ = m._correct_device(x, 0, laplace)
        outs["count"] = torch.tensor(count)
        if proba is not None:
            outs["proba"] = m.laplace_proba(x, proba)
        return outs
    return m, call


def loops(dev, test=False):
    """train_loop over 4 episodes with print_freq=2 (5-way, 2 + 3 per class), or test_loop over 3 episodes: the printed lines, _last, the returned accuracy."""
    m = _model(dev, "bncossim")

    def call():
        if test:
            m.eval()
            return dict(acc=torch.tensor(m.test_loop(Loader(3, 5, 5, 5)), dtype=torch.float64))
        m.train()
        m.train_loop(0, Loader(4, 5, 5, 4), None, print_freq=2)
        return {k: v for k, v in m._last.items() if v is not None}
    return m, call


def regression(dev, kernel=None):
    """_loss + backward of B = 2 tasks of N = 10 points: dkt_regression.DKT (rbf / spectral over the tiny backbone, D = 8) or SinesDKT (kernel None)."""
    torch.manual_seed(0)
    m = (SinesDKT() if kernel is None else RegressionDKT(Tiny(8), kernel, ard_num_dims=8)).to(dev)
    g = torch.Generator().manual_seed(6)
    x = (4.0 * torch.rand(2, 10, 1, generator=g) - 2.0) if kernel is None else _images(6, 20)
    y = torch.randn(2, 10, generator=g).to(dev)

    def call():
        z = m._features(x.to(dev))
        loss, aux = m._loss(z.view(2, 10, -1), y)
        loss.backward()
        return dict(aux, loss=loss.detach())
    return m, call


class Route:
    def __init__(self, name, build, launches, env=None):
        """launches: "kernel[*count] ..." without the dkt_ prefix, in order of first launch; None: not recorded (no event can be recorded inside a graph capture)."""
        self.name, self.build, self.env = name, build, env or {}
        self.launches = launches if launches is None else [("dkt_" + k.split("*")[0], int((k.split("*") + ["1"])[1])) for k in launches.split()]


_UNFUSED = dict(DKT_FUSED_FRONTEND="0")
_GRAPH = dict(DKT_TRAIN_GRAPH="1")
_DIR = dict(likelihood="dirichlet")
_LOO = dict(objective="loo")
ROUTES = [
    Route("train-fused-bn/momentum0.1-mb1", lambda dev: train(dev, "bncossim"), "gram_bn_train_f32 mll_f32 objective_f32 gram_bn_bwd_f32 hyper_grads_f32"),
    Route("train-fused-bn/cumulative-mb3", lambda dev: train(dev, "bncossim", nb=3, momentum=None), "gram_bn_train_f32 mll_f32 objective_f32 gram_bn_bwd_f32 bn_param_grads_f32 hyper_grads_f32"),
    Route("train-fused-bn/momentum0.1-mb3", lambda dev: train(dev, "bncossim", nb=3), "gram_bn_train_f32 mll_f32 objective_f32 gram_bn_bwd_f32 bn_param_grads_f32 hyper_grads_f32"),
    Route("train-unfused/mb1", lambda dev: train(dev, "bncossim"), "gram_f32 mll_f32 objective_f32 gram_bwd_f32 hyper_grads_f32", env=_UNFUSED),
    Route("train-unfused/mb3", lambda dev: train(dev, "bncossim", nb=3), "gram_f32 mll_f32 objective_f32 gram_bwd_f32 hyper_grads_f32", env=_UNFUSED),
    Route("train-rbf", lambda dev: train(dev, "rbf"), "gram_f32 class_kernel_f32 mll_f32 objective_f32 class_kernel_bwd_f32 gram_bwd_f32 hyper_grads_f32"),
    Route("train-rbf-40way", lambda dev: train(dev, "rbf", n_way=40, per=3, logits=True), "gram_f32*6 class_kernel_f32*6 mll_f32*4 objective_f32*2 class_kernel_bwd_f32*2 gram_bwd_f32*2 hyper_grads_f32*2"),
    Route("train-rbf-n450", lambda dev: train(dev, "rbf", n_way=2, per=225, n_support=224, d=16, logits=True), "gram_f32*6 mll_f32*4 objective_f32*2 hyper_grads_f32*2 rbf_bwd_f32*2 gram_bwd_f32*2"),
    Route("train-bernoulli/bncossim", lambda dev: train(dev, "bncossim", likelihood="bernoulli"), "gram_bn_train_f32 gpc_mode_f32 laplace_grad_f32 objective_f32 gram_bn_bwd_f32"),
    Route("train-bernoulli/rbf", lambda dev: train(dev, "rbf", likelihood="bernoulli"), "gram_f32 class_kernel_f32 gpc_mode_f32 laplace_grad_f32 objective_f32 class_kernel_bwd_f32 gram_bwd_f32"),
    Route("correct-fused", lambda dev: correct(dev, "bncossim"), "gram_bn_f32 mll_f32"),
    Route("correct-adapt/bncossim", lambda dev: correct(dev, "bncossim", N=3), "gram_f32*5 mll_f32*4 objective_f32*3 hyper_grads_f32*3"),
    Route("correct-adapt/rbf", lambda dev: correct(dev, "rbf", N=3), "gram_f32*5 class_kernel_f32*5 mll_f32*4 objective_f32*3 class_kernel_bwd_f32*3 hyper_grads_f32*3"),
    Route("correct-bernoulli-adapt", lambda dev: correct(dev, "bncossim", N=2, likelihood="bernoulli"), "gram_f32*4 gpc_mode_f32*3 laplace_grad_f32*2 objective_f32*2 gpc_predict_f32"),
    Route("correct-laplace/rbf0.1", lambda dev: correct(dev, "bncossim", laplace=True, proba="rbf0.1"), "gram_f32*4 gpc_mode_f32*2 gpc_predict_f32*2"),
    Route("correct-laplace/deep-bncossim", lambda dev: correct(dev, "bncossim", laplace="deep", proba="deep"), "gram_f32*4 gpc_mode_f32*2 gpc_predict_f32*2"),
    Route("correct-laplace/deep-rbf", lambda dev: correct(dev, "rbf", laplace="deep", proba="deep"), "gram_f32*6 class_kernel_f32*6 gpc_mode_f32*2 gpc_predict_f32*2"),
    Route("correct-laplace/deep-rbf-2way", lambda dev: correct(dev, "rbf", laplace="deep", proba="deep", n_way=2), "gram_f32*6 class_kernel_f32*6 gpc_mode_f32*2 gpc_predict_f32*2"),
    Route("logits/cossim", lambda dev: correct(dev, "cossim", logits=True), "gram_bn_f32*2 mll_f32*2"),
    Route("logits/rbf", lambda dev: correct(dev, "rbf", logits=True), "gram_f32*4 class_kernel_f32*4 mll_f32*2"),
    Route("logits/bncossim", lambda dev: correct(dev, "bncossim", logits=True), "gram_bn_f32*2 mll_f32*2"),
    Route("loops/train", lambda dev: loops(dev), "gram_bn_train_f32*4 mll_f32*7 objective_f32*4 gram_bn_bwd_f32*4 hyper_grads_f32*4 gram_f32*3"),
    Route("loops/train-graph", lambda dev: loops(dev), None, env=_GRAPH),
    Route("loops/test", lambda dev: loops(dev, test=True), "gram_bn_f32*3 mll_f32*3"),
    Route("regression-loss/rbf", lambda dev: regression(dev, "rbf"), "gram_f32 mll_f32 objective_f32 hyper_grads_f32 rbf_bwd_f32 gram_bwd_f32"),
    Route("regression-loss/spectral", lambda dev: regression(dev, "spectral"), "smk_f32 mll_f32 objective_f32 hyper_grads_f32 smk_bwd_f32"),
    Route("regression-loss/sines", lambda dev: regression(dev), "smk_task_f32 mll_f32 objective_f32 hyper_grads_f32 smk_task_bwd_f32"),
    # the Dirichlet likelihood, the leave-one-out objective and the feature-space forms (26 rows per class: N = 130 > 128, D = 64)
    Route("train-dirichlet/bncossim", lambda dev: train(dev, "bncossim", **_DIR), "gram_bn_train_f32 mll_rownoise_f32 objective_f32 gram_bn_bwd_f32"),
    Route("train-dirichlet/bncossim-unfused", lambda dev: train(dev, "bncossim", **_DIR), "gram_f32 mll_rownoise_f32 objective_f32 gram_bwd_f32", env=_UNFUSED),
    Route("train-dirichlet/rbf", lambda dev: train(dev, "rbf", **_DIR), "gram_f32 class_kernel_f32 mll_rownoise_f32 objective_f32 class_kernel_bwd_f32 gram_bwd_f32"),
    Route("train-dirichlet/mb3", lambda dev: train(dev, "bncossim", nb=3, **_DIR), "gram_bn_train_f32 mll_rownoise_f32 objective_f32 gram_bn_bwd_f32 bn_param_grads_f32"),
    Route("train-dirichlet-feature-space/fused", lambda dev: train(dev, "bncossim", per=26, **_DIR), "bn_stats_f32 affine_normalize_f32 rownoise_lowrank_f32 objective_f32 rownoise_lowrank_bwd_f32 normalize_bn_bwd_f32"),
    Route("train-dirichlet-feature-space/unfused", lambda dev: train(dev, "bncossim", per=26, **_DIR), "rownoise_lowrank_f32 objective_f32 rownoise_lowrank_bwd_f32", env=_UNFUSED),
    Route("train-loo/bncossim", lambda dev: train(dev, "bncossim", **_LOO), "gram_bn_train_f32 loo_f32 objective_f32 gram_bn_bwd_f32 hyper_grads_f32"),
    Route("train-loo/bncossim-unfused", lambda dev: train(dev, "bncossim", **_LOO), "gram_f32 loo_f32 objective_f32 gram_bwd_f32 hyper_grads_f32", env=_UNFUSED),
    Route("train-loo/rbf", lambda dev: train(dev, "rbf", **_LOO), "gram_f32 class_kernel_f32 loo_f32 objective_f32 class_kernel_bwd_f32 gram_bwd_f32 hyper_grads_f32"),
    Route("train-loo/mb3", lambda dev: train(dev, "bncossim", nb=3, **_LOO), "gram_bn_train_f32 loo_f32 objective_f32 gram_bn_bwd_f32 bn_param_grads_f32 hyper_grads_f32"),
    Route("train-loo-feature-space/fused", lambda dev: train(dev, "bncossim", per=26, **_LOO), "bn_stats_f32 affine_normalize_f32 loofs_f32 objective_f32 normalize_bn_bwd_f32 hyper_grads_f32"),
    Route("train-loo-feature-space/unfused", lambda dev: train(dev, "bncossim", per=26, **_LOO), "loofs_f32 objective_f32 hyper_grads_f32", env=_UNFUSED),
    Route("train-gaussian-feature-space/fused", lambda dev: train(dev, "bncossim", per=26), "bn_stats_f32 affine_normalize_f32 lowrank_gram_f32 mll_f32 lowrank_finish_f32 lowrank_bwd_f32 normalize_bn_bwd_f32 hyper_grads_f32"),
    Route("train-gaussian-feature-space/unfused", lambda dev: train(dev, "bncossim", per=26), "lowrank_gram_f32 mll_f32 lowrank_finish_f32 lowrank_bwd_f32 hyper_grads_f32", env=_UNFUSED),
    Route("correct-dirichlet/fused", lambda dev: correct(dev, "bncossim", **_DIR), "gram_bn_f32 mll_rownoise_f32"),
    Route("correct-dirichlet/unfused", lambda dev: correct(dev, "bncossim", **_DIR), "gram_f32*2 mll_rownoise_f32", env=_UNFUSED),
    Route("correct-dirichlet/rbf", lambda dev: correct(dev, "rbf", **_DIR), "gram_f32*2 class_kernel_f32*2 mll_rownoise_f32"),
    Route("correct-dirichlet/feature-space", lambda dev: correct(dev, "bncossim", n_support=26, n_query=2, **_DIR), "rownoise_lowrank_f32 rownoise_lowrank_predict_f32"),
    Route("dirichlet-proba/bncossim", lambda dev: correct(dev, "bncossim", episode=False, dirichlet_proba=8, **_DIR), "gram_f32*2 mll_rownoise_f32 dirichlet_proba_f32"),
    Route("dirichlet-proba/rbf", lambda dev: correct(dev, "rbf", episode=False, dirichlet_proba=8, **_DIR), "gram_f32*3 class_kernel_f32*3 mll_rownoise_f32 dirichlet_proba_f32"),
    Route("dirichlet-proba/feature-space", lambda dev: correct(dev, "bncossim", episode=False, dirichlet_proba=8, n_support=26, n_query=2, **_DIR), "rownoise_lowrank_f32 rownoise_lowrank_predict_f32 dirichlet_proba_f32"),
    Route("loo-accuracy/bncossim", lambda dev: correct(dev, "bncossim", episode=False, loo_accuracy=True, **_LOO), "gram_f32 loo_f32"),
    Route("loo-accuracy/rbf", lambda dev: correct(dev, "rbf", episode=False, loo_accuracy=True, **_LOO), "gram_f32 class_kernel_f32 loo_f32"),
    Route("loo-accuracy/feature-space", lambda dev: correct(dev, "bncossim", episode=False, loo_accuracy=True, n_support=26, n_query=2, **_LOO), "loofs_f32"),
    Route("correct-adapt/dirichlet", lambda dev: correct(dev, "bncossim", N=2, **_DIR), "gram_f32*4 mll_rownoise_f32*3 objective_f32*2"),
    Route("correct-adapt/loo", lambda dev: correct(dev, "bncossim", N=2, **_LOO), "gram_f32*4 loo_f32*2 objective_f32*2 hyper_grads_f32*2 mll_f32"),
]


def run(route, dev, launches=False):
    """dict(outs = every tensor the call returned, grads = the gradient of every parameter that has one, state = every parameter and buffer after the call,
    stdout = what it printed, launches = [(kernel name, launches)] in order of first launch, or None)."""
    record = launches and route.launches is not None
    with _environment(route.env):
        m, call = route.build(dev)
        printed = io.StringIO()
        ops.kernel_timing(record)
        try:
            with contextlib.redirect_stdout(printed):
                outs = call()
            torch.cuda.synchronize()
            got = [(name, count) for name, (count, _) in ops.kernel_timing_results().items()] if record else None
        finally:
            ops.kernel_timing(False)
    return dict(outs={k: v for k, v in outs.items() if isinstance(v, torch.Tensor)}, stdout=printed.getvalue(), launches=got,
                grads={k: p.grad for k, p in m.named_parameters() if p.grad is not None}, state=dict(m.state_dict()))
