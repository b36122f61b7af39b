"""Mixed-precision trunk features through the training step of `from_trunk_features` (bn_out in train mode + F.normalize + Gram + MLL + backward), three
routes alternated in one process after a warm-up (the spread over the rounds is printed):
  fp32     fp32 X through the product kernels (today's from_trunk_features);
  cast     bf16 X, .float() in front of the head (a cast kernel + autograd's cast of dX back), then the product kernels;
  native   bf16 X straight into the *_x16 kernels of libdkt_x16.so (dX written in bf16).
Shapes: the cfg2 shape (N = 105, D = 1600, C = 5) at 2048 and 8192 episodes per step, the 20-way shape (N = 420, D = 512, C = 20) at 1024.
Prints episodes/s per route, the per-kernel HIP-event times of each route and the byte model of the front-end kernels.  Measurement tooling; prints only.
Usage: python tools/time_x16_frontend.py [--rounds R] [--steps K] [--only cfg2_2048|cfg2_8192|20way_1024] [--json PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dkt_amd import ops  # noqa: E402

SHAPES = (("cfg2", 5, 21, 1600, 2048), ("cfg2", 5, 21, 1600, 8192), ("20way", 20, 21, 512, 1024))


def byte_model(n, d, xb):
    """Algorithmic HBM bytes per episode of the front-end kernels (X element size xb; fp32 statistics / E / W / Zn / dZn)."""
    nd, nn = n * d, n * n
    if n <= 128:
        return {"gram_bn_train": nd * xb + nn * 4 + 5 * d * 4,                    # X once, E, the statistics
                "gram_bn_bwd": 2 * nd * xb + nd * xb + 2 * nn * 4 + 6 * d * 4}    # X twice (staging + epilogue, the second mostly an L2 hit), dX, W and E
    return {"bn_stats": nd * xb + 5 * d * 4,
            "affine_normalize": nd * xb + nd * 4,                                   # X -> Zn
            "normalize_bn_bwd": 2 * nd * 4 + 2 * nd * xb + nd * xb}                 # dZn, Zn (row dots + columns), X twice, dX


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--only", default=None, help="one shape, e.g. cfg2_2048 (a counter-collection run)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    report = []
    for tag, c, per, d, b in SHAPES:
        if args.only is not None and args.only != "%s_%d" % (tag, b):
            continue
        n = c * per
        g = torch.Generator(device=dev).manual_seed(1234)
        x32 = (torch.randn(b, n, d, generator=g, device=dev).abs() + 1.0)
        x16 = x32.to(torch.bfloat16)
        gamma = torch.ones(d, device=dev, requires_grad=True)
        beta = torch.zeros(d, device=dev, requires_grad=True)
        sv = torch.ones(c, device=dev, requires_grad=True)
        mean = torch.zeros(c, device=dev, requires_grad=True)
        noise = torch.full((c,), 0.1, device=dev)
        cls = torch.arange(c, device=dev).repeat_interleave(per)
        y = torch.where(cls.unsqueeze(0) == torch.arange(c, device=dev).unsqueeze(1), 1.0, -1.0).contiguous()
        cw = torch.full((c,), -1.0 / (c * n), device=dev)
        leaves = {"fp32": x32.requires_grad_(True), "cast": x16.clone().requires_grad_(True), "native": x16.clone().requires_grad_(True)}

        def step(route):
            x = leaves[route]
            for t in (x, gamma, beta, sv, mean):
                t.grad = None
            xin = x.float() if route == "cast" else x
            obj = ops.episode_loss_bn(xin, gamma, beta, y, sv, mean, noise, cw)[0]
            obj.mean().backward()

        for route in leaves:                       # warm-up: allocator growth, clock ramp, first-launch costs
            for _ in range(3):
                step(route)
        torch.cuda.synchronize()
        times = {r: [] for r in leaves}
        for _ in range(args.rounds):               # alternate the routes: drift of clocks / temperature hits all three alike
            for route in leaves:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    step(route)
                torch.cuda.synchronize()
                times[route].append((time.perf_counter() - t0) / args.steps)
        kernels = {}
        for route in leaves:
            ops.kernel_timing(True)
            for _ in range(args.steps):
                step(route)
            torch.cuda.synchronize()
            kernels[route] = {k: round(v[1], 4) for k, v in ops.kernel_timing_results().items()}
            ops.kernel_timing(False)
        row = dict(shape=tag, n=n, d=d, c=c, episodes=b)
        for route in leaves:
            t = np.asarray(times[route])
            row[route] = dict(eps_per_s=b / float(np.median(t)), ms_median=1e3 * float(np.median(t)), ms_min=1e3 * float(t.min()), ms_max=1e3 * float(t.max()),
                              kernels_ms=kernels[route])
        row["native_over_fp32"] = row["native"]["eps_per_s"] / row["fp32"]["eps_per_s"]
        row["native_over_cast"] = row["native"]["eps_per_s"] / row["cast"]["eps_per_s"]
        row["byte_model_per_episode"] = {"fp32": byte_model(n, d, 4), "bf16": byte_model(n, d, 2)}
        for route in leaves:
            r = row[route]
            print("%-6s N=%3d D=%4d B=%5d  %-6s %10.0f eps/s  step %.3f ms (min %.3f, max %.3f)" % (tag, n, d, b, route, r["eps_per_s"], r["ms_median"], r["ms_min"],
                                                                                               r["ms_max"]))
            for k, v in sorted(r["kernels_ms"].items()):
                print("        %-28s %.4f ms" % (k, v))
        print("        native / fp32 = %.3f   native / cast = %.3f" % (row["native_over_fp32"], row["native_over_cast"]))
        for k in row["byte_model_per_episode"]["fp32"]:
            bf, bh = row["byte_model_per_episode"]["fp32"][k], row["byte_model_per_episode"]["bf16"][k]
            print("        byte model %-18s fp32 %9d B/episode  bf16 %9d B/episode  (%.2f x)" % (k, bf, bh, bh / bf))
        sys.stdout.flush()
        report.append(row)
        del leaves, x32, x16
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(report, fh, indent=1)


if __name__ == "__main__":
    main()
