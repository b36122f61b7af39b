#!/usr/bin/env python
"""Timing of the Dirichlet likelihood in feature space (docs/DIRICHLET.md "Above 127 rows"), in the manner of `tools/dirichlet_bench.py`.

HIP events after --warmup, --reps back-to-back: B in {1, 64, 1024} episodes of (C, N, D) = (20, 420, 64), (20, 400, 64), (5, 105, 64), unit-norm features.
Per shape, one JSON line:
  forward_ms         `ops.rownoise_lowrank(want_grad=True)` (dkt_rownoise_lowrank_f32)
  backward_ms        `ops.rownoise_lowrank_bwd` (dkt_rownoise_lowrank_bwd_f32)
  predict_ms         `ops.rownoise_lowrank_predict` at M = N queries (dkt_rownoise_lowrank_predict_f32)
  dirichlet_step_ms  the `episode_loss_dirichlet` step from the features, forward + backward, on the feature-space route (forced at 105 rows)
  gaussian_step_ms   `episode_loss_linear` at the same shape (its feature-space route above 128 rows): context, not a target
  dkt_step_ms        `DKT(Conv4S, likelihood="dirichlet")` forward + backward of one training step on 28 x 28 images, B <= --max_model_batch
and, last, the resident route for comparison: `ops.mll_rownoise(want_grad=True)` and the resident `episode_loss_dirichlet` step at (1024, 5, 105).
`--rownoise-only RUNS` prints RUNS repetitions of the resident call alone at (1024, 5, 105) and (1024, 5, 25): the figures to compare between two builds."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import dkt_amd
from dkt_amd import ops
from dirichlet_bench import _events, _features


def _inputs(b_, c, n):
    rng = np.random.default_rng(n)
    z = torch.tensor(np.stack([_features(rng, c, n // c) for _ in range(min(b_, 8))]), dtype=torch.float32).cuda()
    z = z.repeat((b_ + z.shape[0] - 1) // z.shape[0], 1, 1)[:b_].contiguous().requires_grad_(True)
    cls = torch.arange(c, device="cuda").repeat_interleave(n // c)
    ypm = torch.where(cls.unsqueeze(0) == torch.arange(c, device="cuda").unsqueeze(1), 1.0, -1.0).contiguous()
    sv = torch.full((c,), 0.6931, device="cuda", requires_grad=True)
    mean = torch.zeros(c, device="cuda", requires_grad=True)
    return z, ypm, sv, mean, torch.full((c,), -1.0 / (c * n), device="cuda")


def _rownoise_ms(b_, c, n, args):
    z, ypm, sv, mean, cw = _inputs(b_, c, n)
    yt, nr = ops.dirichlet_targets(ypm)
    e = ops.gram(z.detach(), None, ops.KERNEL_LINEAR_UNIT)
    return _events(lambda: ops.mll_rownoise(e, yt, nr, sv.detach(), mean.detach(), want_grad=True, cls_weight=cw), args.warmup, args.reps)


def main(args):
    if args.rownoise_only:
        for run in range(args.rownoise_only):
            for c, n in ((5, 105), (5, 25)):
                print(json.dumps(dict(what="dkt_mll_rownoise_f32 with gradients, HIP events", run=run, B=1024, C=c, N=n, rownoise_ms=round(_rownoise_ms(1024, c, n, args), 4),
                                      reps=args.reps)), flush=True)
        return
    for c, n in ((20, 420), (20, 400), (5, 105)):
        for b_ in (1, 64, 1024):
            z, ypm, sv, mean, cw = _inputs(b_, c, n)
            yt, nr = ops.dirichlet_targets(ypm)
            noise = torch.full((c,), 0.1, device="cuda")
            zd, svd, md = z.detach(), sv.detach(), mean.detach()
            gobj = torch.ones(b_, device="cuda")
            out = ops.rownoise_lowrank(zd, yt, nr, svd, md, cw, want_grad=True)

            def dirichlet_step():
                z.grad = sv.grad = mean.grad = None
                ops.episode_loss_dirichlet(z, yt, nr, sv, mean, cw, "bncossim", unit_rows=True)[0].sum().backward()

            def gaussian_step():
                z.grad = sv.grad = mean.grad = None
                ops.episode_loss_linear(z, ypm, sv, mean, noise, cw, unit_rows=True)[0].sum().backward()

            os.environ["DKT_DIRICHLET_LOWRANK"] = "force"
            res = dict(what="Dirichlet likelihood in feature space, HIP events", B=b_, C=c, N=n, D=64,
                       forward_ms=_events(lambda: ops.rownoise_lowrank(zd, yt, nr, svd, md, cw, want_grad=True), args.warmup, args.reps),
                       backward_ms=_events(lambda: ops.rownoise_lowrank_bwd(zd, yt, nr, svd, md, cw, out["state"], gobj), args.warmup, args.reps),
                       predict_ms=_events(lambda: ops.rownoise_lowrank_predict(zd, out["state"], svd, md), args.warmup, args.reps),
                       dirichlet_step_ms=_events(dirichlet_step, args.warmup, args.reps), gaussian_step_ms=_events(gaussian_step, args.warmup, args.reps))
            del os.environ["DKT_DIRICHLET_LOWRANK"]
            if b_ <= args.max_model_batch:
                torch.manual_seed(0)
                m = dkt_amd.DKT(dkt_amd.backbone.Conv4S, n_way=c, n_support=5, likelihood="dirichlet").cuda()
                x = torch.rand(b_ * n, 3, 28, 28, device="cuda")
                y = m._targets(c, n // c, x.device)

                def dkt_step():
                    m.zero_grad(set_to_none=True)
                    m._train_forward(x, y, b_, n, False)[0].backward()

                res["dkt_step_ms"] = _events(dkt_step, max(2, args.warmup // 2), max(3, args.reps // 5))
                del m, x
            print(json.dumps({k: round(v, 4) if isinstance(v, float) else v for k, v in res.items()}), flush=True)
    z, ypm, sv, mean, cw = _inputs(1024, 5, 105)
    yt, nr = ops.dirichlet_targets(ypm)

    def resident_step():
        z.grad = sv.grad = mean.grad = None
        ops.episode_loss_dirichlet(z, yt, nr, sv, mean, cw, "bncossim", unit_rows=True)[0].sum().backward()

    print(json.dumps(dict(what="the resident route (dkt_mll_rownoise_f32), HIP events", B=1024, C=5, N=105, D=64, rownoise_ms=round(_rownoise_ms(1024, 5, 105, args), 4),
                          dirichlet_step_ms=round(_events(resident_step, args.warmup, args.reps), 4))), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--max_model_batch", type=int, default=64, help="largest B at which the DKT training step (Conv4S on B x N images) is timed")
    ap.add_argument("--rownoise-only", type=int, default=0, metavar="RUNS")
    main(ap.parse_args())
