"""Sine-wave regression (the paper's periodic-function experiment, reference sines/train_DKT.py) on the HIP hot path.

    SineTaskSampler(x_range, family, seed, device)   the task distribution (Task_Distribution + Sine_Task / Cosine_Task, :19-108), drawn on the GPU
    SineFeature()                                    the 1 -> 40 -> 40 ReLU MLP (Feature, :110-121): parameters layer1.*, layer2.*
    SinesDKT()                                       ConstantMean + SpectralMixtureKernel(num_mixtures=4, ard_num_dims=40) + a learned Gaussian
                                                     likelihood (:123-140), on the task-resident spectral-mixture kernels of libdkt_smk.so

The sampler draws B tasks in one vectorised call from a seeded torch generator on the device: amplitude ~ U(0.1, 5.0), phase ~ U(0, pi),
x ~ U(x_range), y = A sin(x + phase) (or cos) + N(0, 0.1^2).  The test draw has 200 sorted points per task, 5 random support points (sorted)
and the other 195 as query (sorted), as sines/train_DKT.py:190-226 does per task.  The draw follows the reference's distribution, not its
numpy random stream: the same seed does not give the reference's tasks, and the targets are computed in fp32 on the device (the reference
evaluates them in float64 before converting).
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .dkt import gp_head
from .dkt_regression import DKT

TRAIN_RANGE = (-5.0, 5.0)
TEST_RANGES = {"in": (-5.0, 5.0), "out": (-5.0, 10.0)}      # the out-of-range condition of sines/train_DKT.py:148
AMPLITUDE = (0.1, 5.0)
PHASE = (0.0, math.pi)
NOISE = 0.1
FAMILIES = ("sine", "cosine")


class SineTaskSampler:
    """B regression tasks per call.  Every tensor comes back on `device` (CPU tensors work too); `generator` state advances per call."""

    def __init__(self, x_range=TRAIN_RANGE, family: str = "sine", seed: int = 0, device="cuda", noise: float = NOISE):
        if family not in FAMILIES:
            raise ValueError("family must be one of %s, got %r" % (FAMILIES, family))
        self.x_range = (float(x_range[0]), float(x_range[1]))
        self.family = family
        self.noise = float(noise)
        self.device = torch.device(device)
        self.generator = torch.Generator(device=self.device)
        self.generator.manual_seed(int(seed))

    def _uniform(self, shape, lo, hi):
        return lo + (hi - lo) * torch.rand(shape, generator=self.generator, device=self.device, dtype=torch.float32)

    def _tasks(self, b: int, n: int, sort: bool):
        amp = self._uniform((b, 1), *AMPLITUDE)
        phase = self._uniform((b, 1), *PHASE)
        x = self._uniform((b, n), *self.x_range)
        if sort:
            x = x.sort(dim=1).values
        fn = torch.sin if self.family == "sine" else torch.cos
        y = amp * fn(phase + x)
        if self.noise > 0:
            y = y + self.noise * torch.randn((b, n), generator=self.generator, device=self.device, dtype=torch.float32)
        return x.unsqueeze(-1), y, amp.squeeze(1), phase.squeeze(1)

    def train_batch(self, b: int, n: int = 10):
        """(x [B,n,1], y [B,n]): n unsorted points per task (sample_data(n, noise=0.1))."""
        x, y, _, _ = self._tasks(b, n, False)
        return x, y

    def test_batch(self, b: int, n_all: int = 200, n_support: int = 5) -> dict:
        """n_all sorted points per task; n_support random ones (sorted) as support, the rest (sorted) as query."""
        if not 0 < n_support < n_all:
            raise ValueError("need 0 < n_support < n_all")
        x, y, amp, phase = self._tasks(b, n_all, True)
        perm = torch.rand((b, n_all), generator=self.generator, device=self.device).argsort(dim=1)
        sup = perm[:, :n_support].sort(dim=1).values
        qry = perm[:, n_support:].sort(dim=1).values
        take = lambda t, idx: torch.gather(t, 1, idx)      # noqa: E731
        return dict(x_all=x, y_all=y, support=sup, query=qry,
                    x_support=take(x[..., 0], sup).unsqueeze(-1), y_support=take(y, sup),
                    x_query=take(x[..., 0], qry).unsqueeze(-1), y_query=take(y, qry), amplitude=amp, phase=phase)

    def true_function(self, amplitude, phase, x):
        fn = torch.sin if self.family == "sine" else torch.cos
        return amplitude * fn(phase + x)


class SineFeature(nn.Module):
    """The reference's feature extractor (sines/train_DKT.py:110-121): relu(layer2(relu(layer1(x)))), 1 -> 40 -> 40."""

    def __init__(self):
        super().__init__()
        self.layer1 = nn.Linear(1, 40)
        self.layer2 = nn.Linear(40, 40)

    def forward(self, x):
        return F.relu(self.layer2(F.relu(self.layer1(x))))


class SinesDKT(DKT):
    """DKT of the sine-wave experiment: spectral mixture of Q = 4 over the 40 MLP features, ConstantMean, learned noise.  The GP head runs on
    libdkt_smk.so (ops.spectral_mixture_matrix_task / ops.smk_task) for a batch of B tasks at once; B = 1 is the reference's loop."""

    def __init__(self, feature=None, num_mixtures: int = 4, n_shot_test: int = 5, sampler: SineTaskSampler = None,
                 test_sampler: SineTaskSampler = None):
        super().__init__(SineFeature() if feature is None else feature, "spectral", num_mixtures=num_mixtures, ard_num_dims=40)
        self.n_shot_test = n_shot_test
        self.sampler, self.test_sampler = sampler, test_sampler      # defaults of train_loop / test_loop

    def _features(self, x):
        """x [B,n,1] -> z [B,n,40]."""
        b, n = x.shape[0], x.shape[1]
        return self.feature_extractor(x.reshape(b * n, -1)).reshape(b, n, -1).float()

    def _mixture(self):
        m = self.model
        return m.mixture_weights, m.mixture_means, m.mixture_scales

    def _base_matrix(self, zb):
        """E [B,N,N] of the tasks zb [B,N,40] on the task-resident kernels."""
        return ops.spectral_mixture_matrix_task(zb, *self._mixture())

    def train_loop(self, step, optimizer, tasks_per_step: int = 1, sampler: SineTaskSampler = None, n_shot: int = 10):
        """One Adam step on the mean over `tasks_per_step` tasks of -logp / N (sines/train_DKT.py:162-180 for B = 1).  Every 100 steps the
        reference's log line; its MSE is that of the train-mode prediction, the PRIOR mean (a constant), against the labels."""
        sampler = self.sampler if sampler is None else sampler
        x, y = sampler.train_batch(tasks_per_step, n_shot)
        optimizer.zero_grad()
        z = self._features(x)
        loss, _ = self._loss(z, y)
        loss.backward()
        optimizer.step()
        if step % 100 == 0:
            mse = self.mse(self.model.mean.detach().expand_as(y), y)
            print('[%d] - Loss: %.3f  MSE: %.3f  lengthscale: %.3f   noise: %.3f' % (step, loss.item(), mse.item(), 0.0, self.model.noise.item()))
        return loss

    @torch.no_grad()
    @gp_head
    def predict(self, x_support, y_support, x_query) -> dict:
        """Condition every task on its support points, posterior at its query points, for B tasks at once.  x_support [B,S,1], y_support [B,S],
        x_query [B,M,1] -> mean, var (of likelihood(gp(x)): noise included) [B,M], lower / upper = mean -+ 2 sqrt(var) (confidence_region)."""
        m = self.model
        zs, zq = self._features(x_support), self._features(x_query)
        mix = self._mixture()
        sv, mean, noise = m.scale_times_variance(), m.mean, m.noise
        e = ops.smk_any(zs, None, *mix)
        out = ops.mll(e, y_support.reshape(zs.shape[0], 1, -1).to(torch.float32), sv, mean, noise, want_chol=True, jitter0=self.jitter0,
                      max_tries=self.max_tries)
        ex = ops.smk_any(zq, zs, *mix)
        mu, _ = ops.predict(ex, out["alpha"], sv, mean, want_labels=False)
        exx = mix[0].sum().reshape(1, 1).expand(zq.shape[0], zq.shape[1]).contiguous()     # k(x, x) = sum of the mixture weights
        var = ops.predict_var(ex, exx, out["chol"], sv, noise)
        mu, var = mu[:, 0], var[:, 0]
        sd = var.sqrt()
        return dict(mean=mu, var=var, lower=mu - 2.0 * sd, upper=mu + 2.0 * sd)

    def test_loop(self, n_tasks: int = 500, sampler: SineTaskSampler = None, n_all: int = 200) -> list:
        """All test tasks in one batch (sines/train_DKT.py:190-222): per-task MSE of the posterior mean against the noisy query targets."""
        sampler = self.test_sampler if sampler is None else sampler
        self.model.eval()
        self.feature_extractor.eval()
        t = sampler.test_batch(n_tasks, n_all, self.n_shot_test)
        pred = self.predict(t["x_support"], t["y_support"], t["x_query"])
        mse = ((pred["mean"] - t["y_query"]) ** 2).mean(dim=1)
        self.model.train()
        self.feature_extractor.train()
        return mse.cpu().tolist()


def summary(mse_list) -> str:
    """The reference's closing block (sines/train_DKT.py:224-226)."""
    return "-------------------\nAverage MSE: " + str(np.mean(mse_list)) + " +- " + str(np.std(mse_list)) + "\n-------------------"
