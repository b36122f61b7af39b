#!/usr/bin/env python
"""Timing of training under the Dirichlet classification likelihood (docs/DIRICHLET.md), in the manner of `tools/laplace_bench.py grad`.

HIP events after --warmup, --reps back-to-back: B in {1, 64, 1024} episodes of (C, N) = (5, 25), (5, 105), (20, 100), unit-norm features D = 64.  Per shape:
  rownoise_ms        `ops.mll_rownoise(want_grad=True)` alone on the shared Gram matrix (dkt_mll_rownoise_f32: both passes)
  dirichlet_step_ms  the full `episode_loss_dirichlet` step (Gram -> marginal likelihood and gradient -> Gram backward; forward + backward)
  gaussian_step_ms   `episode_loss_linear` at the same B, C, N, D on the same box
  bernoulli_step_ms  `episode_loss_laplace` there
No throughput target: the other two likelihoods' steps are the comparison points.  One JSON line per shape."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from dkt_amd import ops


def _events(fn, warmup, reps):
    """ms per call of fn(): `reps` back-to-back calls between two HIP events, after `warmup` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def _features(rng, c, shots, d=64, spread=0.3):
    centres = rng.standard_normal((c, d))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    z = centres[np.repeat(np.arange(c), shots)] + spread * rng.standard_normal((c * shots, d)) / np.sqrt(d)
    return z / np.linalg.norm(z, axis=1, keepdims=True)


def main(args):
    for c, n in ((5, 25), (5, 105), (20, 100)):
        for b_ in (1, 64, 1024):
            rng = np.random.default_rng(n)
            z = torch.tensor(np.stack([_features(rng, c, n // c) for _ in range(min(b_, 8))]), dtype=torch.float32).cuda()
            z = z.repeat((b_ + z.shape[0] - 1) // z.shape[0], 1, 1)[:b_].contiguous().requires_grad_(True)
            cls = torch.arange(c, device="cuda").repeat_interleave(n // c)
            ypm = torch.where(cls.unsqueeze(0) == torch.arange(c, device="cuda").unsqueeze(1), 1.0, -1.0).contiguous()
            y01 = ((ypm + 1.0) * 0.5).contiguous()
            yt, nr = ops.dirichlet_targets(ypm)
            sv = torch.full((c,), 0.6931, device="cuda", requires_grad=True)
            mean, noise = torch.zeros(c, device="cuda", requires_grad=True), torch.full((c,), 0.1, device="cuda")
            cw = torch.full((c,), -1.0 / (c * n), device="cuda")
            e = ops.gram(z.detach(), None, ops.KERNEL_LINEAR_UNIT)

            def dirichlet_step():
                z.grad = sv.grad = mean.grad = None
                ops.episode_loss_dirichlet(z, yt, nr, sv, mean, cw, "bncossim", unit_rows=True)[0].sum().backward()

            def gaussian_step():
                z.grad = sv.grad = mean.grad = None
                ops.episode_loss_linear(z, ypm, sv, mean, noise, cw, unit_rows=True)[0].sum().backward()

            def bernoulli_step():
                z.grad = sv.grad = None
                ops.episode_loss_laplace(z, y01, sv, cw, "bncossim", unit_rows=True)[0].sum().backward()

            row_ms = _events(lambda: ops.mll_rownoise(e, yt, nr, sv.detach(), mean.detach(), want_grad=True, cls_weight=cw), args.warmup, args.reps)
            dir_ms = _events(dirichlet_step, args.warmup, args.reps)
            gauss_ms = _events(gaussian_step, args.warmup, args.reps)
            bern_ms = _events(bernoulli_step, args.warmup, args.reps)
            print(json.dumps(dict(what="Dirichlet training step vs the Gaussian and Bernoulli steps, HIP events", B=b_, C=c, N=n, D=64, rownoise_ms=round(row_ms, 4),
                                  dirichlet_step_ms=round(dir_ms, 4), gaussian_step_ms=round(gauss_ms, 4), bernoulli_step_ms=round(bern_ms, 4),
                                  vs_gaussian=round(dir_ms / gauss_ms, 2), vs_bernoulli=round(dir_ms / bern_ms, 2), reps=args.reps)), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    main(ap.parse_args())
