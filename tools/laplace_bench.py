#!/usr/bin/env python
"""Timing of the Laplace GP classifier (docs/LAPLACE.md, libdkt_gpc.so).

  episode   ms per `DKT.correct(x, laplace=True)` episode (Conv4S 28x28, 5-way 5-shot, 16 queries per class), wall clock around a synchronised
            call, median of --reps after --warmup: the device route, and with `--route sklearn` the host route of scikit-learn (what every
            episode took before the device route existed, and what support sets of more than 127 rows still take)
  kernels   the two calls alone, HIP events around --reps back-to-back pairs: B in {1, 64, 1024} episodes of 5 classes, N = 25 and N = 100
            support rows, M = 80 queries; prints ms per pair and episodes per second
  grad      training under the Bernoulli likelihood, HIP events after --warmup, --reps back-to-back: B in {1, 64, 1024} episodes of (C, N) = (5, 25), (5, 105),
            (20, 100), unit-norm features D = 64.  Per shape: the two calls alone (`laplace_mode` on the scaled covariances, `laplace_grad`), the full
            `episode_loss_laplace` step (Gram -> mode -> gradient -> Gram backward; forward + backward), and SIDE BY SIDE the Gaussian
            `episode_loss_linear` step at the same B, C, N, D on the same box.  No throughput target: the Gaussian step is the comparison point
  prof      a short fixed workload of the two calls for `rocprofv3 --kernel-trace --stats -- python tools/laplace_bench.py prof`

One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

import numpy as np
import torch

import dkt_amd
from dkt_amd import ops


def episode(args):
    torch.manual_seed(0)
    m = dkt_amd.DKT(dkt_amd.backbone.Conv4S, n_way=5, n_support=5).cuda()
    m.eval()
    m.n_query = 16
    if args.route == "sklearn":
        ops.laplace_supported = lambda n, c: False
    xs = [torch.rand(5, 21, 3, 28, 28, generator=torch.Generator().manual_seed(s)) for s in range(8)]
    ms = []
    for i in range(args.warmup + args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.correct(xs[i % len(xs)], laplace=True)
        torch.cuda.synchronize()
        if i >= args.warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(what="correct(x, laplace=True) ms per episode", route=args.route, median=round(statistics.median(ms), 4),
                          min=round(min(ms), 4), p90=round(sorted(ms)[int(0.9 * len(ms))], 4), reps=len(ms))))


def _problem(b_, n, m=80, c=5):
    import laplace_model as lm
    rng = np.random.default_rng(n)
    zs, zq = lm.clustered(rng, c, n // c, m, 64, 0.1)
    k = torch.tensor(lm.rbf(zs, zs, 0.1), dtype=torch.float32).cuda().expand(b_, n, n).contiguous()
    ks = torch.tensor(lm.rbf(zq, zs, 0.1), dtype=torch.float32).cuda().expand(b_, m, n).contiguous()
    return k, ks, torch.ones(b_, m, device="cuda"), torch.tensor(lm.one_vs_rest(c, n // c), dtype=torch.float32).cuda()


def kernels(args):
    for n in (25, 100):
        for b_ in (1, 64, 1024):
            k, ks, kss, y = _problem(b_, n)
            for _ in range(args.warmup):
                md = ops.laplace_mode(k, y)
                ops.laplace_predict(ks, kss, md)
            torch.cuda.synchronize()
            ops.kernel_timing(True)
            for _ in range(args.reps):
                md = ops.laplace_mode(k, y)
                ops.laplace_predict(ks, kss, md)
            torch.cuda.synchronize()
            res = ops.kernel_timing_results()
            ops.kernel_timing(False)
            mode_ms, pred_ms = res["dkt_gpc_mode_f32"][1], res["dkt_gpc_predict_f32"][1]
            print(json.dumps(dict(what="mode + predict, HIP events", B=b_, C=5, N=n, M=80, mode_ms=round(mode_ms, 4), predict_ms=round(pred_ms, 4),
                                  episodes_per_s=round(b_ / ((mode_ms + pred_ms) * 1e-3)), iters=int(md["iters"].max()), reps=args.reps)))


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


def grad(args):
    import laplace_model as lm
    for c, n in ((5, 25), (5, 105), (20, 100)):
        for b_ in (1, 64, 1024):
            rng = np.random.default_rng(n)
            z = torch.tensor(np.stack([lm.clustered(rng, c, n // c, 1, 64, 0.3)[0] for _ in range(min(b_, 8))]), dtype=torch.float32).cuda()
            z = z.repeat((b_ + z.shape[0] - 1) // z.shape[0], 1, 1)[:b_].contiguous().requires_grad_(True)
            y01 = torch.tensor(lm.one_vs_rest(c, n // c), dtype=torch.float32).cuda()
            ypm = (2.0 * y01 - 1.0).contiguous()
            sv = torch.full((c,), 0.6931, device="cuda", requires_grad=True)
            mean, noise = torch.zeros(c, device="cuda", requires_grad=True), torch.full((c,), 0.1, device="cuda")
            cw = torch.full((c,), -1.0 / (c * n), device="cuda")
            e = ops.gram(z.detach(), None, ops.KERNEL_LINEAR_UNIT)
            kc = (e.unsqueeze(1) * sv.detach().view(1, -1, 1, 1)).contiguous()
            md = ops.laplace_mode(kc, y01)

            def bernoulli_step():
                z.grad = sv.grad = None
                ops.episode_loss_laplace(z, y01, sv, cw, "bncossim", unit_rows=True)[0].sum().backward()

            def gaussian_step():
                z.grad = sv.grad = mean.grad = None
                ops.episode_loss_linear(z, ypm, sv, mean, noise, cw, unit_rows=True)[0].sum().backward()

            mode_ms = _events(lambda: ops.laplace_mode(kc, y01), args.warmup, args.reps)
            grad_ms = _events(lambda: ops.laplace_grad(e, y01, md["f"], cw, sv.detach()), args.warmup, args.reps)
            bern_ms = _events(bernoulli_step, args.warmup, args.reps)
            gauss_ms = _events(gaussian_step, args.warmup, args.reps)
            print(json.dumps(dict(what="Bernoulli training step vs the Gaussian step, HIP events", B=b_, C=c, N=n, D=64, mode_ms=round(mode_ms, 4),
                                  grad_ms=round(grad_ms, 4), bernoulli_step_ms=round(bern_ms, 4), gaussian_step_ms=round(gauss_ms, 4),
                                  ratio=round(bern_ms / gauss_ms, 2), iters=int(md["iters"].max()), reps=args.reps)), flush=True)


def prof(args):
    for n, b_ in ((25, 1024), (100, 1024)):
        k, ks, kss, y = _problem(b_, n)
        for _ in range(5):
            ops.laplace_predict(ks, kss, ops.laplace_mode(k, y))
    torch.cuda.synchronize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("section", choices=["episode", "kernels", "grad", "prof"])
    ap.add_argument("--route", choices=["device", "sklearn"], default="device")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    {"episode": episode, "kernels": kernels, "grad": grad, "prof": prof}[a.section](a)
