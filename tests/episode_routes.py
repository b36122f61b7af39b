"""The training-episode routes of dkt_amd.ops, each defined once: how E is made (given, linear Gram, contraction + class kernel, the BN trunk front end in its
resident and big forms) times what is solved on it (Gaussian marginal likelihood, its feature-space form, Laplace, Dirichlet and its feature-space form).  A route is a name, the environment it
needs, a callable that builds seeded inputs and returns (leaves, call), and the library launches its forward and backward make, in order.  `run` executes one:
forward, backward with a seeded upstream gradient, every output and every leaf gradient returned -- and, with `launches=True`, the launches of each half as
ops.kernel_timing records them.  tests/test_episode_routes_gpu.py pins the launch lists; the same routes serve bit-for-bit comparisons between two commits."""
import contextlib
import os

import torch

from dkt_amd import ops

B, C = 2, 5          # two episodes: one episode's BatchNorm parts ARE the sums (no dkt_bn_param_grads_f32 launch)


def _randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _leaf(t, dev, dtype=torch.float32, grad=True):
    return t.to(dev, dtype).requires_grad_(grad)


def _targets(n, dev, zero_one=False):
    cls = torch.arange(C).repeat_interleave(n // C)
    return torch.where(cls.unsqueeze(0) == torch.arange(C).unsqueeze(1), 1.0, 0.0 if zero_one else -1.0).contiguous().to(dev)


def _hypers(dev, n, grad=True):
    sv = _leaf(torch.tensor([0.5, 2.0, 1.0, 3.0, 0.7]), dev, grad=grad)
    mean = _leaf(torch.tensor([0.1, -0.2, 0.0, 0.3, -0.1]), dev, grad=grad)
    noise = _leaf(torch.tensor([0.1, 0.2, 0.15, 0.1, 0.3]), dev, grad=grad)
    return sv, mean, noise, torch.linspace(0.5, 1.5, C).mul(-1.0 / (C * n)).to(dev)


def _features(n, d, dev, seed=1, grad=True):
    return _leaf(torch.nn.functional.normalize(_randn(seed, B, n, d), dim=2), dev, grad=grad)


def _trunk(n, d, dev, dtype=torch.float32):
    x = _leaf(_randn(2, B, n, d).abs() + 0.5, dev, dtype)
    return x, _leaf(1.0 + 0.2 * _randn(3, d), dev), _leaf(0.1 * _randn(4, d), dev)


def _given_e(dev):
    z = torch.nn.functional.normalize(_randn(1, B, 25, 64), dim=2)
    return _leaf(z @ z.transpose(1, 2), dev)


def mll_objective(dev):
    e = _given_e(dev)
    sv, mean, noise, cw = _hypers(dev, 25)
    return dict(e=e, sv=sv, mean=mean, noise=noise), lambda: ops.mll_objective(e, _targets(25, dev), sv, mean, noise, cw)


def laplace_objective(dev):
    e = _given_e(dev)
    sv, _, _, cw = _hypers(dev, 25)
    return dict(e=e, scale=sv), lambda: ops.laplace_objective(e, _targets(25, dev, True), cw, scale=sv)


def linear(dev, n=25, z_grad=True, only_sv=False):
    z = _features(n, 64, dev, grad=z_grad)
    sv, mean, noise, cw = _hypers(dev, n)
    if only_sv:
        mean, noise = mean.detach(), noise.detach()
    return dict(z=z, sv=sv, mean=mean, noise=noise), lambda: ops.episode_loss_linear(z, _targets(n, dev), sv, mean, noise, cw, unit_rows=True)


def class_kernel(dev, kernel, grads=True):
    z = _features(25, 64, dev, grad=grads)
    sv, mean, noise, cw = _hypers(dev, 25)
    par = _leaf(torch.tensor([0.6, 0.8, 1.0, 1.2, 0.9]), dev, grad=grads)
    kw = dict(offset=par) if kernel in ops.POLY_KINDS else dict(lengthscale=par)
    return (dict(z=z, sv=sv, mean=mean, noise=noise, param=par),
            lambda: ops.episode_loss_class_kernel(z, _targets(25, dev), sv, mean, noise, cw, kernel, **kw))


def bn(dev, n=25, d=64, use_bn=True, dtype=torch.float32):
    x, gamma, beta = _trunk(n, d, dev, dtype)
    sv, mean, noise, cw = _hypers(dev, n)
    leaves = dict(x=x, sv=sv, mean=mean, noise=noise, **(dict(gamma=gamma, beta=beta) if use_bn else {}))
    return leaves, lambda: ops.episode_loss_bn(x, gamma if use_bn else None, beta if use_bn else None, _targets(n, dev), sv, mean, noise, cw, use_bn=use_bn,
                                               full=True)


def laplace(dev, kernel):
    z = _features(25, 64, dev)
    sv, _, _, cw = _hypers(dev, 25)
    ls = _leaf(torch.tensor([0.6, 0.8, 1.0, 1.2, 0.9]), dev)
    leaves = dict(z=z, sv=sv, **(dict(lengthscale=ls) if kernel == "rbf" else {}))
    return leaves, lambda: ops.episode_loss_laplace(z, _targets(25, dev, True), sv, cw, kernel, lengthscale=ls, unit_rows=kernel != "rbf")


def laplace_bn(dev):
    x, gamma, beta = _trunk(25, 64, dev)
    sv, _, _, cw = _hypers(dev, 25)
    return dict(x=x, gamma=gamma, beta=beta, sv=sv), lambda: ops.episode_loss_laplace_bn(x, gamma, beta, _targets(25, dev, True), sv, cw)


def _dirichlet_targets(n, dev):
    return ops.dirichlet_targets(_targets(n, dev))


def dirichlet_objective(dev):
    e = _given_e(dev)
    sv, mean, _, cw = _hypers(dev, 25)
    return dict(e=e, sv=sv, mean=mean), lambda: ops.dirichlet_objective(e, *_dirichlet_targets(25, dev), sv, mean, cw)


def dirichlet(dev, kernel, n=25):
    z = _features(n, 64, dev)
    sv, mean, _, cw = _hypers(dev, n)
    ls = _leaf(torch.tensor([0.6, 0.8, 1.0, 1.2, 0.9]), dev)
    leaves = dict(z=z, sv=sv, mean=mean, **(dict(lengthscale=ls) if kernel == "rbf" else {}))
    return leaves, lambda: ops.episode_loss_dirichlet(z, *_dirichlet_targets(n, dev), sv, mean, cw, kernel, lengthscale=ls, unit_rows=kernel != "rbf")


def dirichlet_bn(dev, n=25, d=64, use_bn=True, dtype=torch.float32):
    x, gamma, beta = _trunk(n, d, dev, dtype)
    sv, mean, _, cw = _hypers(dev, n)
    leaves = dict(x=x, sv=sv, mean=mean, **(dict(gamma=gamma, beta=beta) if use_bn else {}))
    return leaves, lambda: ops.episode_loss_dirichlet_bn(x, gamma if use_bn else None, beta if use_bn else None, *_dirichlet_targets(n, dev), sv, mean, cw,
                                                         use_bn=use_bn)


class Route:
    def __init__(self, name, build, forward, backward, env=None, e_is_none=False, e_index=5):
        self.name, self.build, self.env, self.e_is_none, self.e_index = name, build, env or {}, e_is_none, e_index      # e_index: where E is among the outputs
        self.forward, self.backward = ["dkt_%s" % k for k in forward.split()], ["dkt_%s" % k for k in backward.split()]


_MLL = "mll_f32 objective_f32"
_LAPLACE = "gpc_mode_f32 laplace_grad_f32 objective_f32"
_LOWRANK = "lowrank_gram_f32 mll_f32 lowrank_finish_f32"
_DIRICHLET = "mll_rownoise_f32 objective_f32"
_DIRICHLET_LOWRANK = "rownoise_lowrank_f32 objective_f32"
_BN_BWD = "gram_bn_bwd_f32 bn_param_grads_f32"
ROUTES = [
    Route("mll_objective", mll_objective, _MLL, "hyper_grads_f32"),
    Route("laplace_objective", laplace_objective, _LAPLACE, ""),
    Route("linear", linear, "gram_f32 " + _MLL, "gram_bwd_f32 hyper_grads_f32"),
    Route("linear-feature-space", lambda dev: linear(dev, n=80), _LOWRANK, "lowrank_bwd_f32 hyper_grads_f32", env=dict(DKT_LOWRANK="force"), e_is_none=True),
    Route("class-kernel-rbf", lambda dev: class_kernel(dev, "rbf"), "gram_f32 class_kernel_f32 " + _MLL, "class_kernel_bwd_f32 gram_bwd_f32 hyper_grads_f32"),
    Route("class-kernel-poli2", lambda dev: class_kernel(dev, "poli2"), "gram_f32 class_kernel_f32 " + _MLL, "class_kernel_bwd_f32 gram_bwd_f32 hyper_grads_f32"),
    Route("bn-resident", bn, "gram_bn_train_f32 " + _MLL, _BN_BWD + " hyper_grads_f32"),
    Route("bn-resident-unfused-stats", bn, "bn_stats_f32 gram_bn_f32 " + _MLL, _BN_BWD + " hyper_grads_f32", env=dict(DKT_FUSED_STATS="0")),
    Route("bn-resident-no-bn", lambda dev: bn(dev, use_bn=False), "gram_bn_f32 " + _MLL, "gram_bn_bwd_f32 hyper_grads_f32"),
    Route("bn-resident-bf16", lambda dev: bn(dev, dtype=torch.bfloat16), "gram_bn_train_x16 " + _MLL, "gram_bn_bwd_x16 bn_param_grads_f32 hyper_grads_f32"),
    Route("bn-big", lambda dev: bn(dev, n=130, d=68), "bn_stats_f32 affine_normalize_f32 gram_f32 " + _MLL,
          "gram_bwd_f32 normalize_bn_bwd_f32 bn_param_grads_f32 hyper_grads_f32"),
    Route("bn-big-feature-space", lambda dev: bn(dev, n=130, d=64), "bn_stats_f32 affine_normalize_f32 " + _LOWRANK,
          "lowrank_bwd_f32 normalize_bn_bwd_f32 bn_param_grads_f32 hyper_grads_f32", e_is_none=True),
    Route("laplace-linear", lambda dev: laplace(dev, "bncossim"), "gram_f32 " + _LAPLACE, "gram_bwd_f32"),
    Route("laplace-rbf", lambda dev: laplace(dev, "rbf"), "gram_f32 class_kernel_f32 " + _LAPLACE, "class_kernel_bwd_f32 gram_bwd_f32"),
    Route("laplace-bn", laplace_bn, "gram_bn_train_f32 " + _LAPLACE, _BN_BWD),
    Route("dirichlet-objective", dirichlet_objective, _DIRICHLET, "", e_index=None),
    Route("dirichlet-linear", lambda dev: dirichlet(dev, "bncossim"), "gram_f32 " + _DIRICHLET, "gram_bwd_f32", e_index=4),
    Route("dirichlet-class-kernel-rbf", lambda dev: dirichlet(dev, "rbf"), "gram_f32 class_kernel_f32 " + _DIRICHLET, "class_kernel_bwd_f32 gram_bwd_f32", e_index=4),
    Route("dirichlet-bn-resident", dirichlet_bn, "gram_bn_train_f32 " + _DIRICHLET, _BN_BWD, e_index=4),
    Route("dirichlet-bn-resident-no-bn", lambda dev: dirichlet_bn(dev, use_bn=False), "gram_bn_f32 " + _DIRICHLET, "gram_bn_bwd_f32", e_index=4),
    Route("dirichlet-bn-resident-bf16", lambda dev: dirichlet_bn(dev, dtype=torch.bfloat16), "gram_bn_train_x16 " + _DIRICHLET,
          "gram_bn_bwd_x16 bn_param_grads_f32", e_index=4),
    Route("dirichlet-linear-feature-space", lambda dev: dirichlet(dev, "bncossim", n=130), _DIRICHLET_LOWRANK, "rownoise_lowrank_bwd_f32", e_is_none=True, e_index=4),
    Route("dirichlet-bn-feature-space", lambda dev: dirichlet_bn(dev, n=130, d=64), "bn_stats_f32 affine_normalize_f32 " + _DIRICHLET_LOWRANK,
          "rownoise_lowrank_bwd_f32 normalize_bn_bwd_f32 bn_param_grads_f32", e_is_none=True, e_index=4),
    # gradients nobody asked for skip their launches
    Route("linear-only-sv", lambda dev: linear(dev, z_grad=False, only_sv=True), "gram_f32 " + _MLL, "hyper_grads_f32"),
    Route("class-kernel-hypers-only", lambda dev: class_kernel(dev, "rbf", grads=False), "gram_f32 class_kernel_f32 " + _MLL, "hyper_grads_f32"),
]


@contextlib.contextmanager
def _environment(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _launches():
    torch.cuda.synchronize()
    got = [(name, count) for name, (count, _) in ops.kernel_timing_results().items()]
    ops.kernel_timing(True)          # a fresh record for the next half
    return got


def run(route, dev, launches=False):
    """dict(outs=every output of the public call, grads={name: gradient of every leaf that asked for one}, forward / backward = [(kernel name, launches)] in order of first launch)."""
    with _environment(route.env):
        leaves, call = route.build(dev)
        upstream = torch.tensor([1.0, -2.0], device=dev)
        ops.kernel_timing(launches)
        try:
            outs = call()
            fwd = _launches() if launches else None
            (outs[0] * upstream).sum().backward()
            bwd = _launches() if launches else None
        finally:
            ops.kernel_timing(False)
    torch.cuda.synchronize()
    return dict(outs=outs, grads={k: t.grad for k, t in leaves.items() if t.requires_grad}, forward=fwd, backward=bwd)
