"""Timing of the feature-space leave-one-out call (ops.loo_lowrank, dkt_loofs_f32; docs/LOOFS.md) at the 20-way and the 5-way Omniglot shapes: forward only and
with gradients; next to it the marginal-likelihood step of the same shapes in feature space (_FeatureSpaceGaussian: ops.episode_loss_linear forward + backward),
and below 128 rows the resident kernel (ops.loo on E = Z Z^T, with gradients).  HIP events, the minimum of 5 timed calls with the median beside it.  Every shape
runs in a child process under its own time limit; the first one that fails ends the run.  Measurement tooling; prints, never asserts.

    python tools/loo_lowrank_bench.py                   # the three shapes of docs/LOOFS.md
    python tools/loo_lowrank_bench.py --one B C N D     # one shape, in this process"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = ((1024, 20, 420, 64), (1, 20, 420, 64), (8192, 5, 105, 64))
LIMIT_S = 240


def _time(fn, reps=5, warmup=2):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return min(ms), statistics.median(ms)


def one(b, c, n, d):
    import torch
    import bench
    from dkt_amd import ops
    dev = torch.device("cuda", 0)
    z = bench.synthetic_batch(b, n, d, 3, dev)
    per = n // c
    y = torch.where(torch.arange(c, device=dev).repeat_interleave(per).unsqueeze(0) == torch.arange(c, device=dev).unsqueeze(1), 1.0, -1.0).contiguous()
    sv = torch.full((c,), 0.7, device=dev)
    mean = torch.zeros(c, device=dev)
    noise = torch.full((c,), 0.1, device=dev)
    cw = torch.full((c,), -1.0 / (c * n), device=dev)
    rows = []
    rows.append(("loo feature space, forward", _time(lambda: ops.loo_lowrank(z, y, sv, mean, noise, want_grad=False, cls_weight=cw))))
    rows.append(("loo feature space, gradients", _time(lambda: ops.loo_lowrank(z, y, sv, mean, noise, want_grad=True, cls_weight=cw))))
    out = ops.loo_lowrank(z, y, sv, mean, noise, want_grad=True, cls_weight=cw)
    assert int(out["info"].abs().max()) == 0
    os.environ["DKT_LOWRANK"] = "force"
    zg = z.clone().requires_grad_(True)

    def mll_step():
        zg.grad = None
        ops.episode_loss_linear(zg, y, sv, mean, noise, cw, unit_rows=True)[0].mean().backward()
    rows.append(("mll feature space, forward + backward", _time(mll_step)))
    if ops.loo_supported(n, c):
        e = ops.gram(z, None, ops.KERNEL_LINEAR_UNIT)
        rows.append(("loo resident (dkt_loo_f32 on E), gradients", _time(lambda: ops.loo(e, y, sv, mean, noise, want_grad=True, cls_weight=cw))))
    base = rows[1][1][0]
    for name, (lo, med) in rows:
        print("LOOFS-BENCH B=%d C=%d N=%d D=%d  %-44s min %9.3f ms  median %9.3f ms  (x %.2f of the gradient call)" % (b, c, n, d, name, lo, med, lo / base), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", nargs=4, type=int, metavar=("B", "C", "N", "D"))
    args = ap.parse_args()
    if args.one:
        return one(*args.one)
    for shape in SHAPES:
        try:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--one"] + [str(v) for v in shape], timeout=LIMIT_S)
        except subprocess.TimeoutExpired:
            print("LOOFS-BENCH %s: no answer within %d s; stopping" % (shape, LIMIT_S))
            return 1
        if res.returncode != 0:
            print("LOOFS-BENCH %s: exit status %d; stopping" % (shape, res.returncode))
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
