#!/usr/bin/env python
"""Timing of the Laplace GP classifier (docs/LAPLACE.md, libdkt_gpc.so).

  episode   ms per `DKT.correct(x, laplace=True)` episode (Conv4S 28x28, 5-way 5-shot, 16 queries per class), wall clock around a synchronised
            call, median of --reps after --warmup: the device route, and with `--route sklearn` the host route of scikit-learn (what every
            episode took before the device route existed, and what support sets of more than 127 rows still take)
  kernels   the two calls alone, HIP events around --reps back-to-back pairs: B in {1, 64, 1024} episodes of 5 classes, N = 25 and N = 100
            support rows, M = 80 queries; prints ms per pair and episodes per second
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


def prof(args):
    for n, b_ in ((25, 1024), (100, 1024)):
        k, ks, kss, y = _problem(b_, n)
        for _ in range(5):
            ops.laplace_predict(ks, kss, ops.laplace_mode(k, y))
    torch.cuda.synchronize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("section", choices=["episode", "kernels", "prof"])
    ap.add_argument("--route", choices=["device", "sklearn"], default="device")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    {"episode": episode, "kernels": kernels, "prof": prof}[a.section](a)
