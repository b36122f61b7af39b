"""Classification DKT on the HIP hot path -- keeps the method surface of the reference's
`methods/DKT.py` (class DKT :32-335) so it drops into train.py / test.py / test_uncertainty.py:

    DKT(model_func, n_way, n_support)        train.py:145, test.py:80
    .init_summary()                          train.py:146
    .train_loop(epoch, loader, optimizer)    train.py:50     (optimizer ignored, Adam re-created: DKT.py:114)
    .test_loop(loader, record=None, return_std=False)        train.py:56, test.py:161
    .correct(x, N=0, laplace=False) -> (top1_correct, count, avg_loss)       DKT.py:199-272
        laplace=True: Laplace-approximation GP classification with 1.0 * RBF(0.1), on the device up to 127 support rows (docs/LAPLACE.md);
        laplace="deep": the same with the model's own trained kernel; .laplace_proba(x, kernel) their class probabilities; .laplace the default of test_loop
    .get_logits(x) -> [n_way*n_query, n_way]                 test_uncertainty.py:197
    .set_forward / .set_forward_loss         stubs (DKT.py:73-77)
    .dirichlet_proba(x, samples, seed) -> class probabilities of a model under likelihood="dirichlet" (docs/DIRICHLET.md), whose .correct / .test_loop /
        .get_logits condition on the transformed labels of the support set
    .feature / .feature_extractor / .model / .likelihood / .mll / .normalize / .iteration / .writer

What changed underneath: the n_way GPyTorch ExactGP models + SumMarginalLogLikelihood are replaced by
stacked hyper-parameters (gp.ExactGPHypers) and the HIP kernels behind ops.* -- ONE Gram per episode
instead of one per class, all class Choleskys in one launch, gradients produced in the same launch,
no per-class host syncs (DKT.py:151-154, 180, 190).
"""
from __future__ import annotations

import contextlib
import functools
from time import gmtime, strftime

import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import configs, distributed, ops
from .gp import ExactGPHypers, LINEAR_KINDS, RBF_KINDS
from .meta_template import MetaTemplate

try:  # optional, as in the reference (DKT.py:16-21)
    from tensorboardX import SummaryWriter
    IS_TBX_INSTALLED = True
except ImportError:
    IS_TBX_INSTALLED = False


class _LikelihoodView(nn.Module):
    """`model.likelihood`: the Gaussian noise lives in ExactGPHypers.raw_noise (shared storage)."""

    def __init__(self, hypers: ExactGPHypers):
        super().__init__()
        object.__setattr__(self, "_hypers", hypers)

    @property
    def noise(self):
        return self._hypers.noise


class _MllView(nn.Module):
    """`model.mll`: callable kept for surface parity; evaluates the exact MLL of stored train data."""

    def __init__(self, owner):
        super().__init__()
        object.__setattr__(self, "_owner", owner)

    def forward(self, z, targets):
        loss, _ = self._owner._episode_loss(z, targets)
        return -loss


AMP_MODES = (None, "bf16")


def amp_mode(amp):
    """amp=None | "none" | "bf16" -> None | "bf16" (the only mixed-precision mode the models offer; f16 features from a caller's own
    torch.autocast block are accepted as they come).  None / "none" = fp32."""
    amp = None if amp in (None, "none") else amp
    if amp not in AMP_MODES:
        raise ValueError("amp must be None or 'bf16', got %r" % (amp,))
    return amp


def backbone_autocast(amp):
    """The backbone's autocast region: bf16 under amp="bf16" (cache_enabled=False: the step may be captured into a hipGraph); otherwise nothing --
    a caller's own torch.autocast block then applies as it is."""
    if amp == "bf16":
        return torch.autocast("cuda", dtype=torch.bfloat16, cache_enabled=False)
    return contextlib.nullcontext()


def gp_head(fn):
    """Runs a method of the GP head with autocast disabled (amp="bf16" and a caller's outer torch.autocast alike): its tensors stay fp32."""
    @functools.wraps(fn)
    def wrapped(*args, **kwargs):
        with torch.autocast("cuda", enabled=False):
            return fn(*args, **kwargs)
    return wrapped


def _autocast_active(amp) -> bool:
    return amp is not None or torch.is_autocast_enabled("cuda")


def _set_amp(self, value):
    object.__setattr__(self, "_amp", amp_mode(value))


amp_property = property(lambda self: self._amp, _set_amp)      # `amp` of the classification and the regression models: validated on assignment


def _not_pd(where, note=""):
    raise RuntimeError("%s: kernel matrix not positive definite after jitter retries%s" % (where, note))


# dkt_class_kernel_bwd_f32 takes up to 32 class maps per launch: the `c <= 32` of ops.mll_per_class_supported
CLASS_GROUP = 32


def _class_plan(n, c):
    """How a call over the C class models of an N-row episode is split: (class slices, class-kernel form).  Up to 447 rows the class-kernel form
    (one contraction, the class maps and ONE marginal-likelihood launch per slice): one slice `None` = every class, nothing is cut, or groups of
    CLASS_GROUP classes; N + 1 > 448: the single-model form, one Gram + one launch per class (the blocked path serves those sizes)."""
    if not ops.mll_per_class_supported(n, 1):
        return [slice(k, k + 1) for k in range(c)], False
    if ops.mll_per_class_supported(n, c):
        return [None], True
    return [slice(k, k + CLASS_GROUP) for k in range(0, c, CLASS_GROUP)], True


def _class_cut(s, y, *per_class):
    """The targets y [.., C, N] and the per-class vectors (None stays None) of the class slice s."""
    if s is None:
        return (y,) + per_class
    return (y[..., s, :].contiguous(),) + tuple(None if t is None else t[s] for t in per_class)


def first_argmax(mu, dim, dtype=torch.int64):
    """The arg-max of mu along dim as `dtype`; the first maximum wins, as np.argmax (torch.argmax does not promise which of several equal maxima it returns
    on the GPU)."""
    n = mu.shape[dim]
    idx = torch.arange(n, device=mu.device, dtype=dtype).view([n if k == dim % mu.dim() else 1 for k in range(mu.dim())])
    return torch.where(mu == mu.max(dim, keepdim=True).values, idx, torch.full_like(idx, n)).min(dim).values


class _FusableBatchNorm1d(nn.BatchNorm1d):
    """bn_out (DKT.py:48) with the same parameters / buffers / state-dict keys as nn.BatchNorm1d; `bypass` lets the fused
    front end (ops.episode_loss_bn) take the trunk output in front of it and run the normalisation inside the Gram kernels."""
    bypass = False

    def forward(self, x):
        return x if self.bypass else super().forward(x)


class _MetaBatched:
    """Groups `nb` consecutive episodes of an episodic loader into one item x:[nb, C, S+Q, ch, H, W] (a short tail is dropped)."""

    def __init__(self, loader, nb):
        self.loader, self.nb = loader, nb
        if len(loader) // nb == 0:
            raise ValueError("meta_batch = %d exceeds the %d episodes of the loader: no optimizer step would be taken" % (nb, len(loader)))

    def __len__(self):
        return len(self.loader) // self.nb

    def __iter__(self):
        xs, ys = [], []
        for x, y in self.loader:
            xs.append(x)
            ys.append(y)
            if len(xs) == self.nb:
                yield torch.stack(xs, 0), ys
                xs, ys = [], []


LIKELIHOODS = ("gaussian", "bernoulli", "dirichlet")
OBJECTIVES = ("mll", "loo")


def objective_name(objective):
    """objective=None | "mll" | "loo" -> "mll" | "loo" (None: configs.objective, the drivers' --objective; "mll" by default)."""
    objective = objective or configs.objective or "mll"
    if objective not in OBJECTIVES:
        raise ValueError("objective must be one of %s, got %r" % (OBJECTIVES, objective))
    return objective


def check_loo_rows(n, c=1, rows="n_way * (n_support + n_query)"):
    """The limits of the LDS-resident kernel behind objective="loo" (dkt_loo_f32): 127 rows, 32 classes.  Raised on the host, before any launch."""
    if c > ops._lib.LOO_MAX_C:
        raise ValueError("objective='loo' takes up to %d classes, the episode has %d" % (ops._lib.LOO_MAX_C, c))
    if n > ops._lib.LOO_MAX_N:
        raise ValueError("objective='loo' takes episodes of up to %d rows (%s), this one has %d" % (ops._lib.LOO_MAX_N, rows, n))


class _GraphedTrainStep:
    """One training step (backbone forward / backward, the GP hot path, Adam) captured into a hipGraph (torch.cuda.CUDAGraph):
    three eager warm-up steps on a side stream -- they are real steps on real episodes --, then capture, then one graph launch
    per episode.  Static input buffer `x`; the outputs (loss, aux, z_train) are static tensors overwritten by every replay."""

    WARMUP = 3

    def __init__(self, model, optimizer, x_like, y_targets, nb, n_ep, key):
        self.m, self.opt, self.y, self.nb, self.n_ep, self.key = model, optimizer, y_targets, nb, n_ep, key
        self.x = torch.empty_like(x_like)
        self.bad = torch.zeros((), device=x_like.device, dtype=torch.float32)
        self.graph, self.out, self.steps = None, None, 0
        self.side = torch.cuda.Stream(device=x_like.device)

    def _step(self):
        loss, aux, z_train, fused = self.m._train_forward(self.x, self.y, self.nb, self.n_ep, True)
        loss.backward()
        self.bad.add_(aux["info"].abs().max().float())
        self.opt.step()
        return loss.detach(), aux, z_train, fused

    def run(self, x_dev):
        self.x.copy_(x_dev)
        if self.graph is not None:
            self.graph.replay()
            return self.out
        cur = torch.cuda.current_stream()
        if self.steps < self.WARMUP:
            self.steps += 1
            self.side.wait_stream(cur)
            with torch.cuda.stream(self.side):
                self.opt.zero_grad(set_to_none=True)
                out = self._step()
            cur.wait_stream(self.side)
            return out
        self.opt.zero_grad(set_to_none=True)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self.out = self._step()
        self.graph = g
        g.replay()                       # capture only records: run the step for this episode
        return self.out


class DKT(MetaTemplate):
    def __init__(self, model_func, n_way, n_support, kernel_type=None, amp=None, likelihood=None, objective=None):
        super(DKT, self).__init__(model_func, n_way, n_support)
        if likelihood is None:                                # configs.likelihood: the evaluation drivers' --likelihood (None: "gaussian")
            likelihood = configs.likelihood or "gaussian"
        if likelihood not in LIKELIHOODS:
            raise ValueError("likelihood must be one of %s, got %r" % (LIKELIHOODS, likelihood))
        # "gaussian": regression on +-1 labels (the paper's method, the reference's only objective); "bernoulli": the Laplace approximation of the log marginal
        # likelihood under a Bernoulli likelihood (docs/LAPLACE.md "Training"; up to 127 rows per episode); "dirichlet": the exact marginal likelihood of the class
        # labels as Gaussian targets with a fixed noise per row (docs/DIRICHLET.md; up to 127 rows, any number with the linear kernels on up to 64
        # features).  Not a module, parameter or buffer: the state dict is the same
        self.likelihood_type = likelihood
        # what the Gaussian likelihood is fitted by: "mll", the marginal likelihood (the reference), or "loo", the leave-one-out predictive likelihood of the same
        # model (GPML 5.4.2; docs/LOO.md; up to 127 rows per episode, and the linear kernels with up to 64 features above 128 rows: docs/LOOFS.md).  train_loop and the adaptation of correct(x, N > 0) minimise it; prediction is the same
        self.objective_type = objective_name(objective)
        if self.objective_type == "loo" and likelihood != "gaussian":
            raise ValueError("objective='loo' is the leave-one-out likelihood of the Gaussian model: likelihood must be 'gaussian', got %r" % (likelihood,))
        self.kernel_type = configs.kernel_type if kernel_type is None else kernel_type
        # mixed-precision backbone (opt-in): "bf16" runs the backbone under torch.autocast up to, not including, bn_out; the GP head stays fp32.
        # The fused front end takes the 16-bit trunk features as they are (libdkt_x16.so); every other route converts them once with .float().
        # amp=None takes configs.amp (the drivers' --amp; None by default), "none" is fp32 whatever configs says
        self.amp = configs.amp if amp is None else amp
        self.leghtscale_list = None
        self.noise_list = None
        self.outputscale_list = None
        self.iteration = 0
        self.writer = None
        self.feature_extractor = self.feature          # same module under two names (DKT.py:41)
        self.get_model_likelihood_mll()
        if self.kernel_type == "cossim":
            self.normalize = True
        elif self.kernel_type == "bncossim":
            self.normalize = True
            latent_size = int(np.prod(self.feature_extractor.final_feat_dim))
            self.feature_extractor.trunk.add_module("bn_out", _FusableBatchNorm1d(latent_size))
        else:
            self.normalize = False
        self.jitter0 = 1e-6       # gpytorch psd_safe_cholesky fp32 default
        self.max_tries = 3
        self._target_cache = {}
        self._grad_bucket = None
        self._last = {}
        # what test_loop passes to _correct_device: False (the paper's method), True or "deep" (docs/LAPLACE.md); a model trained under the Bernoulli likelihood
        # predicts with it
        self.laplace = "deep" if self.likelihood_type == "bernoulli" else False

    amp = amp_property

    # ------------------------------------------------------------------ construction
    def init_summary(self):
        if IS_TBX_INSTALLED:
            time_string = strftime("%d%m%Y_%H%M%S", gmtime())
            self.writer = SummaryWriter(log_dir="./log/" + time_string)

    def get_model_likelihood_mll(self, train_x_list=None, train_y_list=None):
        """n_way exact GPs sharing the deep kernel; noise = 0.1 frozen (DKT.py:58-71, 346-347)."""
        self.model = ExactGPHypers(self.n_way, self.kernel_type, fixed_noise=0.1)
        self.likelihood = _LikelihoodView(self.model)
        self.mll = _MllView(self)
        return self.model, self.likelihood, self.mll

    def load_state_dict(self, state_dict, strict=True):
        """Accepts this module's own state dict AND one written by the reference's DKT (train.py:61,65: {'epoch', 'state'} with
        the GPyTorch module tree `model.models.{c}.*`, `likelihood.likelihoods.{c}.*`, `mll.*` next to `feature.*` /
        `feature_extractor.*`): the backbone tensors load by name, the GP hyper-parameters of every class through
        ExactGPHypers.load_reference_state_dict."""
        if not ExactGPHypers.is_reference_state_dict(state_dict):
            return super().load_state_dict(state_dict, strict=strict)
        for prefix in ("feature_extractor.", "feature."):
            fe = {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}
            if fe:
                res = self.feature_extractor.load_state_dict(fe, strict=strict)
                break
        else:
            raise RuntimeError("reference state dict without feature_extractor.* / feature.* tensors")
        if self.model.load_reference_state_dict(state_dict) == 0:
            raise RuntimeError("reference state dict without model.models.{c}.* hyper-parameters")
        return res

    def set_forward(self, x, is_feature=False):
        pass

    def set_forward_loss(self, x):
        pass

    # ------------------------------------------------------------------ helpers
    @property
    def device(self):
        return self.model.mean_constant.device

    def _targets(self, n_way, per_class, device):
        """+-1 one-vs-rest targets [C, N], built on the device once per shape (DKT.py:129-136)."""
        key = (n_way, per_class, str(device))
        y = self._target_cache.get(key)
        if y is None:
            cls = torch.arange(n_way, device=device).repeat_interleave(per_class)
            y = torch.where(cls.unsqueeze(0) == torch.arange(n_way, device=device).unsqueeze(1), 1.0, -1.0)
            y = y.to(torch.float32).contiguous()
            self._target_cache[key] = y
        return y

    @staticmethod
    def _check_resident_rows(n, c=1, likelihood="bernoulli", rows="n_way * (n_support + n_query)"):
        """The limits of the LDS-resident kernels behind the Bernoulli and the Dirichlet likelihood: 127 rows, 32 classes."""
        if c > ops._lib.LAPLACE_MAX_C:
            raise ValueError("likelihood='%s' takes up to %d classes, the episode has %d" % (likelihood, ops._lib.LAPLACE_MAX_C, c))
        if n > ops._lib.LAPLACE_MAX_N:
            more = ("; larger ones run in feature space: linear / cossim / bncossim with up to %d features (a multiple of 4), on the GPU" % ops.LOWRANK_DP
                    if likelihood == "dirichlet" else "")
            raise ValueError("likelihood='%s' takes episodes of up to %d rows (%s), this one has %d%s" % (likelihood, ops._lib.LAPLACE_MAX_N, rows, n, more))

    def _dirichlet_in_feature_space(self, z, c, shape=None):
        """Does a Dirichlet episode on the rows z [.., N, D] (or, before they exist, of rows of shape (N, D) on the device of z) run in feature space
        (ops.rownoise_lowrank_*: the linear kernels, D <= 64, rows on the GPU; by default above the 127 rows of the resident kernel)?  The ONE statement of
        the route: the loss, the conditioning and the fused evaluation all ask here."""
        n, d = z.shape[-2:] if shape is None else shape
        return self.kernel_type in LINEAR_KINDS and ops.rownoise_lowrank_applies(int(n), int(d), c, z.is_cuda)

    def _loo_in_feature_space(self, z, c, shape=None, rows="n_way * (n_support + n_query)"):
        """Does a leave-one-out episode on the rows z [.., N, D] (or, before they exist, of rows of shape (N, D) on the device of z) run in feature space
        (ops.loo_lowrank: the linear kernels, D <= 64, rows on the GPU; by default above 128 rows)?  The ONE statement of the route: the losses and
        loo_accuracy ask here.  Where it does not, the limits of the resident kernel hold (check_loo_rows), and the refusal names the route's condition."""
        n, d = z.shape[-2:] if shape is None else shape
        if self.kernel_type in LINEAR_KINDS and ops.loo_lowrank_applies(int(n), int(d), c, z.is_cuda):
            return True
        try:
            check_loo_rows(int(n), c, rows)
        except ValueError as exc:
            if int(n) <= ops._lib.LOO_MAX_N:
                raise
            raise ValueError("%s; larger ones run in feature space: linear / cossim / bncossim with up to %d features (a multiple of 4), more than %d rows, "
                             "on the GPU" % (exc, ops._lib.LOOFS_MAX_D, ops.FUSED_EP_MAX_N)) from None
        return False

    def _dirichlet_targets(self, y):
        """(ytilde, noise_rows) of the +-1 one-vs-rest targets y (ops.dirichlet_targets), built once per target tensor of `_targets`."""
        key = ("dirichlet", y.data_ptr(), tuple(y.shape), str(y.device))
        t = self._target_cache.get(key)
        if t is None:
            t = ops.dirichlet_targets(y) + (y,)           # (y is kept: its address is the key)
            self._target_cache[key] = t
        return t[0], t[1]

    def _condition(self, e, y, sv, mean, noise, rows=None):
        """The mean cache (alpha) of the class models on a conditioning set with base matrix e and +-1 targets y, under the model's likelihood: the Gaussian
        posterior of ops.mll, or -- likelihood="dirichlet" -- that of the transformed labels with their noise per row (ops.mll_rownoise; no jitter ladder).
        rows [B,N,D] in the place of e (None): the Dirichlet posterior in feature space (ops.rownoise_lowrank), whose `state` ops.rownoise_lowrank_predict reads."""
        if self.likelihood_type != "dirichlet":
            return ops.mll(e, y, sv, mean, noise, jitter0=self.jitter0, max_tries=self.max_tries)
        yt, nr = self._dirichlet_targets(y)
        if rows is not None:
            out = ops.rownoise_lowrank(rows, yt, nr, sv, mean)
        else:
            self._check_resident_rows(e.shape[-1], y.shape[-2], "dirichlet", "the conditioning set")
            out = ops.mll_rownoise(e, yt, nr, sv, mean)
        out["jitter"] = torch.zeros_like(out["logp"])
        return out

    @staticmethod
    def _bernoulli_targets(y):
        """The {0,1} form of the +-1 one-vs-rest targets."""
        return ((y + 1.0) * 0.5).contiguous()

    def _objective(self, rows, y):
        """What the model's (likelihood_type, objective_type) minimises on episodes of rows [B,N,D] (features, or the trunk output in front of the fused front
        end: their shape and device are read) with +-1 targets y [C,N], stated ONCE for both losses: the limits of its kernels, checked on the host before any
        launch, then its name in ops.OBJECTIVES and its arguments, the transformed targets first.  Every one is -(1/C) sum_c logp_c / N through the class
        weights (the reference's SumMarginalLogLikelihood / ExactMarginalLogLikelihood scaling, DKT.py:160-163)."""
        n, c = rows.shape[1], y.shape[-2]
        sv, mean, noise = self._hypers()
        cw = torch.full((c,), -1.0 / (c * n), device=rows.device, dtype=torch.float32)
        if self.likelihood_type == "bernoulli":
            # the Laplace approximation: the Gaussian noise and the constant mean do not enter this model and receive no gradient
            self._check_resident_rows(n, c)
            return "laplace", (self._bernoulli_targets(y), sv, cw, ops.LAPLACE_MAX_ITER)
        if self.likelihood_type == "dirichlet":
            # the C = n_way exact GPs on the transformed labels: outputscale and the constant mean train, the noise is the likelihood's own per row and the
            # frozen Gaussian noise does not enter
            if not self._dirichlet_in_feature_space(rows, c):
                self._check_resident_rows(n, c, "dirichlet")
            return "dirichlet", self._dirichlet_targets(y) + (sv, mean, cw)
        if self.objective_type == "loo":
            self._loo_in_feature_space(rows, c)             # (raises where neither the feature-space route nor the resident kernel takes the episode)
        return ("loo" if self.objective_type == "loo" else "gaussian"), (y, sv, mean, noise, cw, self.jitter0, self.max_tries)

    @staticmethod
    def _aux(out):
        """`aux` of a loss from the named outputs of its episode call: logp, alpha, info, jitter and e (detached; None in feature space) under every objective,
        None where it has none, and what it has beyond them (iters; mu_loo, var_loo)."""
        aux = {k: out.get(k) for k in ("logp", "alpha", "info", "jitter")}
        if aux["info"] is None:                               # (Laplace: B = I + W^1/2 K W^1/2 has eigenvalues >= 1: no jitter ladder, nothing can fail)
            aux["info"] = torch.zeros_like(out["iters"])
        aux["e"] = None if out["e"] is None else out["e"].detach()
        aux.update((k, out[k]) for k in ("iters", "mu_loo", "var_loo") if k in out)
        return aux

    def _check_way(self, n_way):
        if n_way != self.model.n_models:
            raise RuntimeError("DKT was built with %d GP models but the episode has %d classes "
                               "(train_n_way must equal test_n_way for DKT)" % (self.model.n_models, n_way))

    def _embed(self, x):
        if not _autocast_active(self.amp):
            z = self.feature_extractor.forward(x)
            if self.normalize:
                z = F.normalize(z, p=2, dim=1)
            return z
        # mixed precision: the backbone under autocast, then ONE conversion to fp32 at the head boundary and bn_out / F.normalize in fp32
        z = self._trunk_features(x)
        bn = self._bn_out()
        with torch.autocast("cuda", enabled=False):
            z = z.float()
            if bn is not None:
                z = bn(z)
            if self.normalize:
                z = F.normalize(z, p=2, dim=1)
        return z

    def _hypers(self):
        m = self.model
        return m.scale_times_variance(), m.mean, m.noise

    def _hypers_detached(self):
        """(sv, mean, noise, lengthscale, offset) outside autograd, lengthscale / offset None where the kernel has none: what every prediction path reads."""
        m = self.model
        ls, off = m.lengthscale, m.offset
        return (m.scale_times_variance().detach(), m.mean.detach(), m.noise.detach(),
                None if ls is None else ls.detach(), None if off is None else off.detach())

    def _mode(self, train, features=None):
        """Train / eval mode of the GP side (model, likelihood) and of the backbone (`features`; None: the same as the GP side)."""
        self.model.train(train)
        self.likelihood.train(train)
        self.feature_extractor.train(train if features is None else features)

    def _bn_out(self, fused=False):
        """The trunk's bn_out, or None.  fused=True (the two fused front ends): only the bn_out this class appended for "bncossim" is folded into the
        Gram kernels, any other kernel type runs them without one; the torch paths apply or bypass whatever bn_out the trunk carries."""
        if fused and self.kernel_type != "bncossim":
            return None
        return getattr(self.feature_extractor.trunk, "bn_out", None)

    # ---- fused front end: bn_out + F.normalize folded into the Gram kernels (ops.episode_loss_bn) ----
    def _trunk_features(self, x):
        """Backbone output BEFORE bn_out (the module the reference appends to the trunk at DKT.py:48)."""
        bn = self._bn_out()
        with backbone_autocast(self.amp):
            if bn is None:
                return self.feature_extractor.forward(x)
            bn.bypass = True
            try:
                return self.feature_extractor.forward(x)
            finally:
                bn.bypass = False

    def _fused_front_end(self, n, d):
        # (n <= 128: the episode-resident kernels of dkt_frontend.hip; up to 448 rows: the streaming kernels of dkt_frontend_big.hip in front of the large-N Gram kernels)
        return (self.kernel_type in ("bncossim", "cossim") and n <= 448 and d % 4 == 0
                and os.environ.get("DKT_FUSED_FRONTEND", "1") != "0")

    @gp_head
    def _episode_loss_from_trunk(self, x_feat, y, want_z=True):
        """Training loss of ONE episode from the trunk output x_feat:[N,D] (or the mean over a meta-batch [B,N,D]); bn_out runs
        in train mode (batch statistics of EACH episode, running estimates updated exactly as nn.BatchNorm1d would after seeing
        the episodes one by one) inside the fused kernels.
        Returns (loss, aux, z_train) with z_train the normalised train-mode features (detached) of the first episode, which
        the in-loop evaluation conditions on (DKT.py:170-192)."""
        xb = (x_feat if x_feat.dim() == 3 else x_feat.unsqueeze(0)).contiguous()
        name, oargs = self._objective(xb, y)
        bn = self._bn_out(True)                                   # the front end's (x, gamma, beta, eps, use_bn)
        fargs = (xb, None, None, 1e-5, False) if bn is None else (xb, bn.weight, bn.bias, bn.eps, True)
        out = dict(zip(("obj",) + ops.OBJECTIVE_OUTPUTS[name] + ops.BN_TRUNK_OUTPUTS, ops._episode(ops._BnTrunk, fargs, name, oargs)))
        with torch.no_grad():
            if bn is not None and bn.track_running_stats:
                self._update_running_stats(bn, out["batch_mean"], out["batch_var_unbiased"])
            z_train = None
            if want_z:
                d = xb.shape[2]
                z_train = (xb[0].detach() * out["a"].reshape(-1, d)[0] + out["s"].reshape(-1, d)[0]) * out["rnorm"][0].unsqueeze(1)
        return out["obj"].mean(), self._aux(out), z_train

    @staticmethod
    def _update_running_stats(bn, bmean, bvar):
        """bn_out's running estimates after the nb episodes whose batch statistics are bmean / bvar [nb, D], exactly as nn.BatchNorm1d would leave them
        after seeing the episodes one by one (called under torch.no_grad)."""
        mom = bn.momentum if bn.momentum is not None else 1.0 / float(bn.num_batches_tracked.item() + 1)
        nb = bmean.shape[0]
        if bn.momentum is None and nb > 1:
            # cumulative moving average: the factor changes with every episode, 1 / (num_batches_tracked + 1) -- the episodes one by one
            nbt = int(bn.num_batches_tracked.item())
            for bi in range(nb):
                f_ = 1.0 / float(nbt + bi + 1)
                bn.running_mean.mul_(1.0 - f_).add_(bmean[bi], alpha=f_)
                bn.running_var.mul_(1.0 - f_).add_(bvar[bi], alpha=f_)
        elif nb == 1:
            bn.running_mean.mul_(1.0 - mom).add_(bmean[0], alpha=mom)
            bn.running_var.mul_(1.0 - mom).add_(bvar[0], alpha=mom)
        else:       # nb sequential momentum updates in closed form: r <- (1-m)^nb r + m sum_b (1-m)^(nb-1-b) x_b
            wts = mom * (1.0 - mom) ** torch.arange(nb - 1, -1, -1, device=bmean.device, dtype=torch.float32)
            bn.running_mean.mul_((1.0 - mom) ** nb).add_((bmean * wts[:, None]).sum(0))
            bn.running_var.mul_((1.0 - mom) ** nb).add_((bvar * wts[:, None]).sum(0))
        bn.num_batches_tracked += nb

    @gp_head
    def _episode_loss(self, z, y):
        """loss = -(1/C) sum_c logp_c / N for ONE episode z:[N,D] (or a batch [B,N,D] -> mean over B)."""
        zb = z if z.dim() == 3 else z.unsqueeze(0)
        name, oargs = self._objective(zb, y)
        ls, off = self.model.lengthscale, self.model.offset
        if name != "gaussian" or self.kernel_type in LINEAR_KINDS:
            # every kernel through E, one launch over all (episode, class) matrices -- or, the linear kernels where the objective says so, on the rows (no E)
            parts = [ops._episode(*ops._rows_front(zb, self.kernel_type, ls, off, bool(self.normalize)), name, oargs)]
        else:
            # rbf / matern / polynomial: every class model owns its lengthscale / offset (one ExactGPLayer per class,
            # DKT.py:63-66), so the base matrix differs per class
            y, sv, mean, noise, cw, _, _ = oargs
            groups, class_form = _class_plan(zb.shape[1], y.shape[-2])
            parts = []
            for s in groups:
                yk, svk, meank, noisek, cwk, lsk, offk = _class_cut(s, y, sv, mean, noise, cw, ls, off)
                if class_form:
                    # ONE contraction per episode (squared distances / Gram), the class maps in one launch, ONE marginal-likelihood
                    # launch over all (episode, class) matrices (DKT_MLL_E_PER_CLASS), the chain rule back in two launches
                    parts.append(ops.episode_loss_class_kernel(zb, yk, svk, meank, noisek, cwk, self.kernel_type, lsk, offk, self.jitter0, self.max_tries))
                else:       # (E of a single model is not kept: nothing reads it)
                    parts.append(ops.mll_objective(ops.base_matrix(zb, self.kernel_type, lsk, offk), yk, svk, meank, noisek, cwk,
                                                   self.jitter0, self.max_tries) + (None,))
            if len(parts) > 1:           # the class weights already carry 1 / (C N), so the parts' objectives add up
                parts = [(torch.stack([pt[0] for pt in parts], 0).sum(0),) + tuple(torch.cat([pt[i] for pt in parts], 1) for i in range(1, 5))
                         + (torch.cat([pt[5] for pt in parts], 1) if class_form else None,)]
        out = dict(zip(("obj",) + ops.OBJECTIVE_OUTPUTS[name] + ops.ROWS_OUTPUTS, parts[0]))
        return out["obj"].mean(), self._aux(out)

    def _kernel_matrices(self, parts, zc, zq=None, ls=None, off=None, class_form=True):
        """The model's base kernel matrices (no autograd) of a conditioning set zc [B,N,D] and queries zq [B,M,D], the ONE statement of their rule: the linear
        kinds share ops.kernel_matrix [B,.,.], every other kernel has one matrix per class model with its own lengthscale / offset (ops.kernel_matrix_per_class
        [B,C,.,.]; class_form=False: the single model's), and the query diagonal is |zq|^2 or the diagonal of a third per-class call.  parts: which of "e" =
        k(zc, zc), "x" = k(zq, zc), "d" = diag k(zq, zq), one letter each: made in that order (a caller's launches stay where they were) and returned in it."""
        linear = self.kernel_type in LINEAR_KINDS
        kmat = ops.kernel_matrix if linear or not class_form else ops.kernel_matrix_per_class
        make = dict(e=lambda: kmat(zc, None, self.kernel_type, ls, off), x=lambda: kmat(zq, zc, self.kernel_type, ls, off),
                    d=lambda: (zq * zq).sum(-1) if linear else torch.diagonal(kmat(zq, None, self.kernel_type, ls, off), dim1=-2, dim2=-1))
        out = tuple(make[p]() for p in parts)
        return out[0] if len(out) == 1 else out

    @gp_head
    def _posterior(self, z_cond, y, z_star, e_cond=None):
        """Mean cache on the conditioning set, posterior means [C,M] and labels [M] at z_star."""
        sv, mean, noise, ls, off = self._hypers_detached()
        zc = z_cond.detach().unsqueeze(0)
        zs = z_star.detach().unsqueeze(0)
        if self.likelihood_type == "dirichlet" and self._dirichlet_in_feature_space(zc, y.shape[-2]):
            out = self._condition(None, y, sv, mean, noise, rows=zc.float())
            mu, _, labels = ops.rownoise_lowrank_predict(zs.float(), out["state"], sv, mean)
            return mu[0], labels[0], out
        if self.kernel_type in LINEAR_KINDS:
            if e_cond is None:
                e_cond = self._kernel_matrices("e", zc)
            out = self._condition(e_cond, y, sv, mean, noise)
            mu, labels = ops.predict(self._kernel_matrices("x", zc, zs), out["alpha"], sv, mean)
            return mu[0], labels[0], out
        # per-class base matrices (E depends on the class model's own, post-step, lengthscale / offset)
        # class-kernel form: one contraction for the conditioning set, one for the cross kernel, the class maps element-wise ([1, C, N, N], [1, C, M, N]), one
        # marginal-likelihood launch and one dkt_predict_per_class_f32 launch per class slice; single-model form: the same four calls per class
        groups, class_form = _class_plan(zc.shape[1], y.shape[-2])
        mus, outs = [], []
        for s in groups:
            yk, svk, meank, noisek, lsk, offk = _class_cut(s, y, sv, mean, noise, ls, off)
            o = self._condition(self._kernel_matrices("e", zc, None, lsk, offk, class_form), yk, svk, meank, noisek)
            m, labels = ops.predict(self._kernel_matrices("x", zc, zs, lsk, offk, class_form), o["alpha"], svk, meank, want_labels=len(groups) == 1)
            mus.append(m); outs.append(o)
        if len(groups) == 1:                                 # (the labels come from the predict kernel)
            return m[0], labels[0], {key: o[key] for key in ("logp", "alpha", "jitter", "info")}
        mu = torch.cat(mus, 1)
        out = {key: torch.cat([o[key] for o in outs], 1) for key in ("logp", "alpha", "jitter", "info")}
        return mu[0], first_argmax(mu, 1, torch.int32)[0], out

    def _posterior_fused_eval(self, x_support, x_query, y):
        """Test-time episode with bn_out (eval mode: running statistics) + F.normalize folded into ONE Gram launch over the
        stacked [support; query] trunk features (one backbone pass instead of two): E_all = Zn Zn^T, the conditioning matrix is
        its [:ns, :ns] block and the cross kernel its [ns:, :ns] block.  Returns None when the fused kernels do not apply."""
        ns, nq = x_support.shape[0], x_query.shape[0]
        bn = self._bn_out(True)
        if self.feature_extractor.training or (bn is not None and not bn.track_running_stats):
            return None
        if self.likelihood_type == "dirichlet" and self._dirichlet_in_feature_space(
                x_support, y.shape[-2], (ns, int(np.prod(self.feature_extractor.final_feat_dim)))):
            return None                                       # (no E of the support set: the unfused path conditions in feature space, before any trunk pass)
        x_feat = self._trunk_features(torch.cat([x_support, x_query], 0)).detach()
        d = x_feat.shape[1]
        if x_feat.dim() != 2 or not self._fused_front_end(ns + nq, d):
            return None
        with torch.autocast("cuda", enabled=False):          # the GP head: fp32 (16-bit trunk features go to the *_x16 front-end kernels as they are)
            return self._posterior_fused_eval_head(x_feat, ns, nq, y, bn)

    def _posterior_fused_eval_head(self, x_feat, ns, nq, y, bn):
        d = x_feat.shape[1]
        if bn is not None:
            a = bn.weight.detach() * torch.rsqrt(bn.running_var + bn.eps) if bn.affine else torch.rsqrt(bn.running_var + bn.eps)
            s = (bn.bias.detach() if bn.affine else 0.0) - bn.running_mean * a
        else:
            a = torch.ones(d, device=x_feat.device, dtype=torch.float32)
            s = torch.zeros(d, device=x_feat.device, dtype=torch.float32)
        if ns + nq <= ops.FUSED_EP_MAX_N:
            e_all, _ = ops.gram_bn(x_feat.unsqueeze(0).contiguous(), a.contiguous(), s.contiguous())
        else:                                                 # (more than 128 rows: one normalisation kernel in front of the large-N Gram kernel)
            zn, _ = ops.affine_normalize(x_feat.unsqueeze(0).contiguous(), a.contiguous(), s.contiguous())
            e_all = ops.gram(zn, None, ops.KERNEL_LINEAR_UNIT)
        sv, mean, noise, _, _ = self._hypers_detached()
        out = self._condition(e_all[:, :ns, :ns].contiguous(), y, sv, mean, noise)
        mu, labels = ops.predict(e_all[:, ns:, :ns].contiguous(), out["alpha"], sv, mean)
        return mu[0], labels[0], out

    def _train_forward(self, x_all, y_targets, nb, n_ep, want_z=True):
        """Forward of one training step from the uploaded images x_all:[nb * N, ch, H, W]: returns (loss, aux, z_train, fused)."""
        self._mode(True)
        # ONE backbone pass over the nb * N images of the step (meta-batch: the backbone's own BatchNorm2d layers then see
        # all of them as one batch, as any mini-batch training does; bn_out and the GPs stay per episode)
        x_feat = self._trunk_features(x_all)
        with torch.autocast("cuda", enabled=False):          # the GP head: fp32 (see _train_forward_head)
            return self._train_forward_head(x_feat, y_targets, nb, n_ep, want_z)

    def _train_forward_head(self, x_feat, y_targets, nb, n_ep, want_z):
        """The GP side of a training step from the trunk features: the fused front end takes them as they are (fp32, or 16-bit from a backbone under
        autocast: the *_x16 kernels); every other route converts them once to fp32 in front of bn_out ("accepted, not native")."""
        fused = x_feat.dim() == 2 and self._fused_front_end(n_ep, x_feat.shape[1])
        if fused:
            if nb > 1:
                x_feat = x_feat.view(nb, n_ep, -1)
            loss, aux, z_train = self._episode_loss_from_trunk(x_feat, y_targets, want_z=want_z)
            return loss, aux, z_train, True
        x_feat = x_feat.float()
        bn = self._bn_out()                                                 # torch bn_out / F.normalize in front of the Gram kernels
        if bn is None:
            z_train = x_feat
        elif nb == 1:
            z_train = bn(x_feat)
        else:                                                               # per-episode batch statistics, like the fused path
            z_train = torch.cat([bn(x_feat[k * n_ep:(k + 1) * n_ep]) for k in range(nb)], 0)
        if self.normalize:
            z_train = F.normalize(z_train, p=2, dim=1)
        if nb > 1:
            z_train = z_train.view(nb, n_ep, -1)
        loss, aux = self._episode_loss(z_train, y_targets)
        return loss, aux, z_train, False

    def _bucket(self):
        """The flat gradient bucket of the multi-rank step (None outside torch.distributed).  Every fp32 parameter's `.grad` is a VIEW of
        it (`attach`), so the backward writes the bucket directly and the all-reduce needs no pack / unpack copies -- provided the
        training loop clears the gradients with `zero_()` / `set_to_none=False` and masks in place, which `train_loop` does."""
        if not distributed.is_distributed():
            return None
        if self._grad_bucket is None:
            self._grad_bucket = distributed.GradBucket(self.parameters())
        self._grad_bucket.attach()           # (re-attaches a gradient somebody replaced; a no-op when the views are in place)
        return self._grad_bucket

    def _zero_grads(self, optimizer):
        """Start of a step: outside torch.distributed the reference's `optimizer.zero_grad()`; with ranks ONE fill of the flat bucket the
        gradients are views of (set_to_none would drop the views and turn the all-reduce back into pack -> reduce -> scatter)."""
        bucket = self._bucket()
        if bucket is None:
            optimizer.zero_grad()
        else:
            bucket.zero_()

    def _sync_grads(self, flag=None):
        """One all-reduce of the flat gradient bucket; `flag` (max |info| of this rank's step) is summed over the ranks in the
        same collective.  Returns the (global) flag."""
        if distributed.is_distributed():
            if self._grad_bucket is None:
                self._grad_bucket = distributed.GradBucket(self.parameters())
            return self._grad_bucket.allreduce_mean(flag)
        return flag

    # ------------------------------------------------------------------ training
    def _adam(self, **kwargs):
        """The reference's two-group Adam (DKT.py:114): the GP hyper-parameters at 1e-4, the backbone at 1e-3."""
        return torch.optim.Adam([{'params': self.model.parameters(), 'lr': 1e-4},
                                 {'params': self.feature_extractor.parameters(), 'lr': 1e-3}], **kwargs)

    def _check_bad_steps(self):
        """Raises, on every rank alike, when a step since the start of the epoch failed (the accumulated device flag: ONE read-back)."""
        if self._bad_steps is not None and float(self._bad_steps.item()) != 0.0:
            _not_pd("DKT", " (GPyTorch raises NotPSDError here)")

    def train_loop(self, epoch, train_loader, optimizer, print_freq=10):
        # the optimizer argument is ignored and Adam re-created every call, as the reference does
        # (same update rule; on the GPU the fused implementation: one launch per parameter group instead of a dozen element-wise
        # ones, and it takes a device-side `found_inf` flag -- used below to SKIP the update of a step whose factorisation failed)
        fused_adam = os.environ.get("DKT_FUSED_ADAM", "1") == "1" and self.device.type == "cuda"
        dev = self.device
        self._bad_steps = None
        # DKT_TRAIN_GRAPH=1: capture the per-episode step into a hipGraph (the loop is launch-bound: ~150 launches for ~1 ms of
        # GPU work).  Needs static shapes, no TensorBoard writer inside the step and a single process.
        use_graph = os.environ.get("DKT_TRAIN_GRAPH", "0") == "1" and not distributed.is_distributed()
        graph_step = None
        optimizer = self._adam(capturable=True) if use_graph else self._adam(**({"fused": True} if fused_adam else {}))
        mb = max(1, int(getattr(self, "meta_batch", 1) or 1))
        if mb > 1:          # opt-in (train.py --meta_batch B): B episodes per Adam step; 1 = the reference's semantics (DKT.py:160-164)
            train_loader = _MetaBatched(train_loader, mb)
        for i, (x, _) in enumerate(train_loader):
            xe = x if x.dim() == 6 else x.unsqueeze(0)            # [B, C, S+Q, ch, H, W]
            nb = xe.size(0)
            self.n_query = xe.size(2) - self.n_support
            if self.change_way:
                self.n_way = xe.size(1)
            self._check_way(self.n_way)
            per = self.n_support + self.n_query
            n_ep = self.n_way * per
            x_all = xe.contiguous().view(nb * n_ep, *xe.size()[3:]).to(dev, non_blocking=True)
            y_targets = self._targets(self.n_way, per, dev)

            graphed = None
            if use_graph:
                key = (tuple(x_all.shape), nb)
                if graph_step is None or graph_step.key != key:
                    graph_step = _GraphedTrainStep(self, optimizer, x_all, y_targets, nb, n_ep, key)
                graphed = graph_step

            # hyper-parameter means for the log line, read BEFORE the step (DKT.py:145-157); kept on
            # the device, converted to Python floats only when printed
            need_eval = self.writer is not None or i % print_freq == 0 or i == len(train_loader) - 1
            if i % print_freq == 0:
                with torch.no_grad():
                    log_outputscale = self.model.outputscale.mean()
                    log_noise = self.model.noise.mean()
                    ls = self.model.lengthscale
                    log_lengthscale = ls.mean() if ls is not None else torch.zeros((), device=dev)

            if graphed is not None:
                # the whole step (backbone forward / backward, the GP kernels, Adam) as ONE hipGraph launch
                loss, aux, z_train, fused = graphed.run(x_all)
                self._bad_steps = graphed.bad
            else:
                self._zero_grads(optimizer)
                loss, aux, z_train, fused = self._train_forward(x_all, y_targets, nb, n_ep, need_eval)
                loss.backward()
                # failure flag of the step (not positive definite after every jitter retry), kept on the device, summed over the
                # ranks with the gradients and accumulated over the iterations: checked -- on every rank alike -- at the next
                # print point (GPyTorch raises NotPSDError synchronously; a failed step has poisoned the update with NaN)
                bad = self._sync_grads(aux["info"].abs().max().float())
                self._bad_steps = bad if self._bad_steps is None else self._bad_steps + bad
                if fused_adam:
                    optimizer.found_inf = (bad != 0).to(torch.float32).reshape(())    # no NaN ever reaches the weights or Adam's moments
                else:
                    # the default (foreach) implementation has no device-side skip: the poisoned gradients are zeroed IN PLACE (the views
                    # into the gradient bucket survive; no allocation, no host sync), so no NaN reaches the weights or the moments.  This
                    # is NOT a skipped step: Adam still advances its step count, decays its moments and moves the weights by the existing
                    # momentum -- only the fused path (found_inf) leaves the optimizer state untouched.
                    failed = (bad != 0).reshape(())
                    for group in optimizer.param_groups:
                        for p_ in group['params']:
                            if p_.grad is not None:
                                p_.grad.masked_fill_(failed, 0.0)
                optimizer.step()
            x_all = x_all[:n_ep]                          # the in-loop evaluation looks at the step's first episode

            self.iteration = i + (epoch * len(train_loader))
            if self.writer is not None:
                self.writer.add_scalar('loss', loss, self.iteration)

            # (likelihood="bernoulli": this in-loop evaluation, and the Noise it prints, are still the Gaussian posterior's on the +-1 targets -- a cheap
            #  progress indicator with the trained kernel, not the Laplace predictor test_loop uses; docs/LAPLACE.md "Training")
            # evaluation on support / query with eval-mode features, conditioning on the (stale)
            # train-mode features and the post-step hyper-parameters (DKT.py:170-192).  Its only consumers are the TensorBoard
            # writer and the log line, and it has no side effect (eval-mode BatchNorm), so it runs only when one of them will
            # read it (the reference runs it -- with 2C blocking read-backs -- on every iteration)
            if not need_eval:
                self._last = dict(loss=loss.detach(), acc_support=None, acc_query=None, info=aux["info"])
                continue
            if nb > 1 and not fused:
                z_train = z_train[0].detach()
            e_first = None if aux["e"] is None else aux["e"][:1]      # (None: the episode ran in feature space, ops.lowrank_applies)
            with torch.no_grad():
                self._mode(False)
                z_eval = self._embed(x_all).detach().view(self.n_way, per, -1)
                z_support = z_eval[:, :self.n_support].reshape(self.n_way * self.n_support, -1)
                z_query = z_eval[:, self.n_support:].reshape(self.n_way * self.n_query, -1)
                z_star = torch.cat([z_support, z_query], 0)
                _, labels, _ = self._posterior(z_train, y_targets, z_star, e_cond=e_first)
                cls = torch.arange(self.n_way, device=dev, dtype=torch.int32)
                ns = self.n_way * self.n_support
                acc_support = (labels[:ns] == cls.repeat_interleave(self.n_support)).float().mean() * 100.0
                acc_query = (labels[ns:] == cls.repeat_interleave(self.n_query)).float().mean() * 100.0
                if self.writer is not None:
                    self.writer.add_scalar('GP_support_accuracy', acc_support, self.iteration)
                    self.writer.add_scalar('GP_query_accuracy', acc_query, self.iteration)
            self._last = dict(loss=loss.detach(), acc_support=acc_support, acc_query=acc_query, info=aux["info"])

            if i % print_freq == 0:
                if self.writer is not None:
                    self.writer.add_histogram('z_support', z_support, self.iteration)
                self._check_bad_steps()
                print('Epoch [{:d}] [{:d}/{:d}] | Outscale {:f} | Lenghtscale {:f} | Noise {:f} | Loss {:f} | Supp. {:f} | Query {:f}'.format(
                    epoch, i, len(train_loader), log_outputscale.item(), log_lengthscale.item(), log_noise.item(),
                    loss.item(), acc_support.item(), acc_query.item()))
        # failures after the last print point of the epoch (the flag is reset by the next call): raise here, on every rank alike
        self._check_bad_steps()

    # ------------------------------------------------------------------ evaluation
    def _upload(self, x):
        """ONE host-to-device copy of the episode's images (the reference uploads support and query separately, DKT.py:201-203).
        Deliberately a blocking copy: it is the only host/device rendez-vous of a test episode, and it keeps the host from running
        arbitrarily far ahead of the GPU -- measured on MI355X, a fully asynchronous pipeline (pinned staging ring, no blocking call
        at all) is 10x SLOWER (11.8 vs 0.73 ms per Conv4S test episode), while every additional blocking call costs ~1.5 ms."""
        return x if x.is_cuda else x.to(self.device)

    def _split(self, x):
        xd = self._upload(x)
        x_support = xd[:, :self.n_support].contiguous().view(self.n_way * self.n_support, *xd.size()[2:])
        x_query = xd[:, self.n_support:].contiguous().view(self.n_way * self.n_query, *xd.size()[2:])
        return x_support, x_query

    # ---- Laplace-approximation GP classification on the device (libdkt_gpc.so; docs/LAPLACE.md) ----
    def _laplace_targets(self, n_way, per_class, device):
        """{0,1} one-vs-rest targets [C, N]; two classes: ONE binary problem with class 1 positive, as sklearn fits it."""
        key = ("laplace", n_way, per_class, str(device))
        y = self._target_cache.get(key)
        if y is None:
            y = ((self._targets(n_way, per_class, device) + 1.0) * 0.5)[1 if n_way == 2 else 0:].contiguous()
            self._target_cache[key] = y
        return y

    def _laplace_kernels(self, zs, zq, kernel):
        """K, Ks, kss of episodes zs [B,N,D] (support), zq [B,M,D] (queries): "rbf0.1" = the reference's 1.0 * RBF(0.1), shared by the classes;
        "deep" = the model's own kernel outputscale_c * E_c, per class."""
        if kernel == "rbf0.1":
            ls = torch.full((1,), 0.1, device=zs.device, dtype=torch.float32)
            return (ops.gram(zs, None, ops.KERNEL_RBF, ls), ops.gram(zq, zs, ops.KERNEL_RBF, ls),
                    torch.ones(zq.shape[:2], device=zs.device, dtype=torch.float32))
        if kernel != "deep":
            raise ValueError("laplace kernel must be 'rbf0.1' or 'deep', got %r" % (kernel,))
        pick = slice(1, 2) if self.n_way == 2 else slice(None)
        sv, _, _, ls, off = self._hypers_detached()
        sv = sv[pick]
        # (the linear kinds: one matrix for every class model; otherwise the class models picked above)
        e, ex, exx = (t.unsqueeze(1) if self.kernel_type in LINEAR_KINDS else t[:, pick] for t in self._kernel_matrices("exd", zs, zq, ls, off))
        return sv.view(1, -1, 1, 1) * e, sv.view(1, -1, 1, 1) * ex, (sv.view(1, -1, 1) * exx).contiguous()

    def _embed_episodes(self, xd):
        """fp32 embeddings (support [B, ns, D], queries [B, nq, D]) of the episodes xd [B, n_way, n_support + n_query, ...]: one backbone pass per episode
        over its [support; query] rows (called under torch.no_grad)."""
        ns, nq = self.n_way * self.n_support, self.n_way * (xd.shape[2] - self.n_support)
        z = torch.stack([self._embed(torch.cat([xe[:, :self.n_support].reshape(ns, *xe.shape[2:]), xe[:, self.n_support:].reshape(nq, *xe.shape[2:])], 0))
                         for xe in xd], 0).detach().float()
        return z[:, :ns].contiguous(), z[:, ns:].contiguous()

    def _laplace_device(self, x, kernel, batched=False):
        """An episode x [n_way, n_support + n_query, ...] (batched: B of them, [B, n_way, ...]) -> (mu, var, prob [B,C,M], labels [B,M]): one backbone
        pass per episode (so that a batch reproduces its episodes' own results bit for bit, whatever the convolutions do with another batch size), the kernel
        matrices, then ONE mode launch and ONE predict launch for all B x C binary problems."""
        self._check_way(self.n_way)
        xd = self._upload(x if batched else x.unsqueeze(0))
        ns = self.n_way * self.n_support
        if not ops.laplace_supported(ns, self.n_way):
            raise RuntimeError("Laplace GPC on the device takes up to %d support rows and %d classes, the episode has %d and %d"
                               % (ops._lib.GPC_MAX_N, ops._lib.GPC_MAX_C, ns, self.n_way))
        with torch.no_grad():
            zs, zq = self._embed_episodes(xd)
            k, ks, kss = self._laplace_kernels(zs, zq, kernel)
            mode = ops.laplace_mode(k, self._laplace_targets(self.n_way, self.n_support, zs.device))
            self._last["laplace_mode"] = mode
            return ops.laplace_predict(ks, kss, mode)

    def laplace_proba(self, x, kernel="rbf0.1", batched=False):
        """Class probabilities of the Laplace GP classifier, [n_way * n_query, n_way] (batched: x is [B, n_way, ...] and the result [B, n_way * n_query,
        n_way], from one pair of launches), rows normalised to sum 1 as sklearn's multi-class `predict_proba` does; kernel "rbf0.1" (the reference's
        1.0 * RBF(0.1)) or "deep" (the model's own trained kernel)."""
        prob = self._laplace_device(x, kernel, batched)[2].transpose(1, 2)
        prob = torch.cat([1.0 - prob, prob], 2) if self.n_way == 2 else prob / prob.sum(2, keepdim=True)
        return prob.contiguous() if batched else prob[0].contiguous()

    # ---- Dirichlet classification likelihood: class probabilities of the latent posterior (docs/DIRICHLET.md) ----
    def _dirichlet_device(self, x, batched=False):
        """An episode x [n_way, n_support + n_query, ...] (batched: B of them) -> the latent posterior of the queries under the Dirichlet likelihood, conditioned
        on the support set with the model's own kernel: (mu, var [B,C,M]).  One backbone pass per episode, as in `_laplace_device`."""
        self._check_way(self.n_way)
        xd = self._upload(x if batched else x.unsqueeze(0))
        with torch.no_grad():
            self._mode(False)
            zs, zq = self._embed_episodes(xd)
            sv, mean, _, ls, off = self._hypers_detached()
            yt, nr = self._dirichlet_targets(self._targets(self.n_way, self.n_support, zs.device))
            if self._dirichlet_in_feature_space(zs, self.n_way):          # (more than 127 support rows: the D x D models, the latent variance from their state)
                out = ops.rownoise_lowrank(zs, yt, nr, sv, mean)
                return ops.rownoise_lowrank_predict(zq, out["state"], sv, mean)[:2]
            self._check_resident_rows(zs.shape[1], self.n_way, "dirichlet", "n_way * n_support")
            zero = torch.zeros_like(sv)                       # the LATENT variance: no observation noise on the queries
            ex, exx, e = self._kernel_matrices("xde", zs, zq, ls, off)
            out = ops.mll_rownoise(e, yt, nr, sv, mean, want_chol=True)
            mu = ops.predict(ex, out["alpha"], sv, mean, want_labels=False)[0]
            if self.kernel_type in LINEAR_KINDS:
                return mu, ops.predict_var(ex, exx, out["chol"], sv, zero)
            # (dkt_predict_var_f32 takes one cross kernel for the class models it is given: a call per class model here)
            var = torch.cat([ops.predict_var(ex[:, k].contiguous(), exx[:, k].contiguous(), out["chol"][:, k:k + 1].contiguous(), sv[k:k + 1], zero[k:k + 1])
                             for k in range(self.n_way)], 1)
            return mu, var

    def dirichlet_proba(self, x, samples=256, seed=0, batched=False):
        """Class probabilities under the Dirichlet likelihood, [n_way * n_query, n_way] (batched: x is [B, n_way, ...] and the result [B, n_way * n_query, n_way]):
        the mean over `samples` draws of the softmax of the latent posterior, rows summing to 1 (Milios et al. 2018, eq. 8).  The standard normals come from a
        generator seeded with `seed` and are shared by every query and episode (ops.dirichlet_proba), so the result is a deterministic function of x."""
        mu, var = self._dirichlet_device(x, batched)
        eps = torch.randn(int(samples), self.n_way, generator=torch.Generator().manual_seed(int(seed)), dtype=torch.float32).to(mu.device)
        prob = ops.dirichlet_proba(mu, var, eps)[0]
        return prob if batched else prob[0]

    def loo_accuracy(self, x):
        """Leave-one-out accuracy (per cent) of the SUPPORT set of an episode x [n_way, n_support + n_query, ...]: every support row is classified by the arg-max
        over the class models of its leave-one-out predictive mean (mu_loo of ops.loo: the row left out of the conditioning set), the first of several equal maxima.
        One factorisation per class model, no query labels: a validation signal that costs nothing more than the objective.  The call's outputs stay in
        `_last["loo"]`."""
        self.n_query = x.size(1) - self.n_support
        self._check_way(self.n_way)
        x_support, _ = self._split(x)
        with torch.no_grad():
            self._mode(False)
            zs = self._embed(x_support).detach().float().unsqueeze(0)
            sv, mean, noise, ls, off = self._hypers_detached()
            y = self._targets(self.n_way, self.n_support, zs.device)
            if self._loo_in_feature_space(zs, self.n_way, rows="n_way * n_support"):
                out = ops.loo_lowrank(zs, y, sv, mean, noise, jitter0=self.jitter0, max_tries=self.max_tries)
            else:
                out = ops.loo(self._kernel_matrices("e", zs, None, ls, off), y, sv, mean, noise, jitter0=self.jitter0, max_tries=self.max_tries)
            self._last["loo"] = out
            if int(out["info"].abs().max().item()) != 0:
                _not_pd("DKT.loo_accuracy")
            y_s = torch.arange(self.n_way, device=zs.device).repeat_interleave(self.n_support)
            return float((first_argmax(out["mu_loo"][0], 0) == y_s).float().mean().item() * 100.0)

    def correct(self, x, N=0, laplace=False):
        out = self._correct_device(x, N, laplace)
        if not isinstance(out[0], torch.Tensor):
            return out
        stats, count_this, avg_loss = out
        stats = stats.cpu()                                   # the only read-back of the episode
        if stats[1].item() != 0:
            _not_pd("DKT.correct")
        return float(stats[0].item()), count_this, avg_loss

    def _adapt(self, z_train, y_targets, N):
        """Test-time adaptation (DKT.py:242-256): N Adam steps (lr 1e-3) on the GP hyper-parameters only, under the model's own objective of the support set;
        returns the mean loss and leaves the model in eval mode."""
        self._mode(True, False)
        optimizer = torch.optim.Adam([{'params': self.model.parameters()}], lr=1e-3)
        total = 0.0
        for _ in range(N):
            optimizer.zero_grad()
            loss, _ = self._episode_loss(z_train, y_targets)
            loss.backward()
            optimizer.step()
            total = total + loss.item()
        self._mode(False)
        return total / float(N + 1e-10)

    def _episode_posterior(self, x, N=0):
        """The posterior of a test episode x [n_way, n_support + n_query, ...]: (mu [C,M], labels [M], out, avg_loss).  The fused eval front end where it
        applies (N = 0: one backbone pass over support and queries); otherwise embed the support set, adapt (N > 0), eval mode, embed the queries, _posterior."""
        x_support, x_query = self._split(x)
        y_targets = self._targets(self.n_way, self.n_support, self.device)
        fused = None
        if N == 0:
            with torch.no_grad():
                fused = self._posterior_fused_eval(x_support, x_query, y_targets)
        z_train = self._embed(x_support).detach() if fused is None else None
        avg_loss = self._adapt(z_train, y_targets, N) if N > 0 else 0.0
        with torch.no_grad():
            self._mode(False)
            if fused is None:
                fused = self._posterior(z_train, y_targets, self._embed(x_query).detach())
        return fused + (avg_loss,)

    def _correct_device(self, x, N=0, laplace=False):
        """`correct` without the read-back: returns (stats, count, avg_loss) with stats = [top1_correct, max |info|] on the device."""
        self._check_way(self.n_way)
        avg_loss = 0.0
        if self.likelihood_type == "bernoulli":
            # a model trained under the Bernoulli likelihood adapts (N > 0: the GP hyper-parameters only) and predicts under it
            laplace = laplace or "deep"
            if N > 0:
                avg_loss = self._adapt(self._embed(self._split(x)[0]).detach(), self._targets(self.n_way, self.n_support, self.device), N)
        if laplace and (laplace == "deep" or ops.laplace_supported(self.n_way * self.n_support, self.n_way)):
            # Laplace GPC on the device: 1.0 * RBF(0.1) as the reference fits it, or the model's own kernel; top1 counted on the device
            labels = self._laplace_device(x, "deep" if laplace == "deep" else "rbf0.1")[3][0]
            y_q = torch.arange(self.n_way, device=labels.device, dtype=torch.int32).repeat_interleave(self.n_query)
            return torch.stack([(labels == y_q).sum().float(), torch.zeros((), device=labels.device)]), self.n_way * self.n_query, avg_loss

        if laplace:   # more than 127 support rows: sklearn Laplace GPC, "not the method used in the paper" (DKT.py:207-222)
            from sklearn.gaussian_process import GaussianProcessClassifier
            from sklearn.gaussian_process.kernels import RBF
            x_support, x_query = self._split(x)
            y_query = np.repeat(range(self.n_way), self.n_query)
            y_support = np.repeat(range(self.n_way), self.n_support)
            kernel = 1.0 * RBF(length_scale=0.1, length_scale_bounds=(0.1, 10.0))
            gp = GaussianProcessClassifier(kernel=kernel, optimizer=None)
            with torch.no_grad():
                z_support = self._embed(x_support).detach()
                z_query = self._embed(x_query).detach()
            gp.fit(z_support.cpu().numpy(), y_support)
            y_pred = gp.predict(z_query.cpu().numpy())
            return float(np.sum(y_pred == y_query)), len(y_query), 0.0

        _, labels, out, avg_loss = self._episode_posterior(x, N)
        with torch.no_grad():
            y_q = torch.arange(self.n_way, device=self.device, dtype=torch.int32).repeat_interleave(self.n_query)
            stats = torch.stack([(labels == y_q).sum().float(), out["info"].abs().max().float()])
        return stats, self.n_way * self.n_query, avg_loss

    def test_loop(self, test_loader, record=None, return_std=False):
        acc_all, pending = [], []
        iter_num = len(test_loader)

        def flush():          # ONE read-back of the pending per-episode (stats, count)
            got = torch.stack([p[0] for p in pending]).cpu().numpy()
            if (got[:, 1] != 0).any():
                _not_pd("DKT.test_loop")
            acc_all.extend((got[:, 0] / np.asarray([p[1] for p in pending]) * 100).tolist())
            del pending[:]
        for i, (x, _) in enumerate(test_loader):
            self.n_query = x.size(1) - self.n_support
            if self.change_way:
                self.n_way = x.size(0)
            # the per-episode counts stay on the device and are read back in one go at the print points: no blocking call per episode
            stats, count_this, loss_value = self._correct_device(x, 0, self.laplace)
            if not isinstance(stats, torch.Tensor):               # the sklearn route (Laplace, more than 127 support rows) counts on the host
                stats = torch.tensor([stats, 0.0], device=self.device)
            pending.append((stats, count_this))
            if i % 100 == 0 or i == iter_num - 1:
                flush()
            if i % 100 == 0:
                acc_mean = np.mean(np.asarray(acc_all))
                print('Test | Batch {:d}/{:d} | Loss {:f} | Acc {:f}'.format(i, len(test_loader), loss_value, acc_mean))
        if pending:                                            # a loader whose length is unknown / shorter than announced
            flush()
        if distributed.is_distributed():   # every rank evaluated its own shard of the episode list
            acc_all = distributed.gather_accuracies(acc_all)
            iter_num = len(acc_all)
        acc_all = np.asarray(acc_all)
        acc_mean = np.mean(acc_all)
        acc_std = np.std(acc_all)
        print('%d Test Acc = %4.2f%% +- %4.2f%%' % (iter_num, acc_mean, 1.96 * acc_std / np.sqrt(iter_num)))
        if self.writer is not None:
            self.writer.add_scalar('test_accuracy', acc_mean, self.iteration)
        if return_std:
            return acc_mean, acc_std
        return acc_mean

    def get_logits(self, x):
        self.n_query = x.size(1) - self.n_support
        self._check_way(self.n_way)
        return self._episode_posterior(x)[0].t().contiguous()    # [n_way*n_query, n_way] raw posterior means (DKT.py:331-335)
