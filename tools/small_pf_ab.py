"""Sweep of the workgroups-per-CU cap DKT_GRAM_SMALL_LDS of the N <= 32 Gram forward (dkt_gram_small.hip; twins library).  (Written as the A/B of the forward's
prefetch depth under that cap: the eight-steps-in-flight instances were removed after the measurement, profiles/r06/small_pf_ab.log -- commit 06c82cc has them; what
is left sweeps the cap for the shipped depth.)   python tools/small_pf_ab.py"""
import importlib
import os
import sys

os.environ["DKT_TWINS"] = "1"
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ops = importlib.import_module("deep-kernel-transfer_amd").ops
dev = torch.device("cuda:0")


def timed(fn, reps=10):
    for _ in range(2):
        fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        out = fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps, out


for (b, n, d, kind) in [(8192, 19, 2916, ops.KERNEL_RBF), (8192, 19, 2916, ops.KERNEL_LINEAR), (8192, 25, 2048, ops.KERNEL_LINEAR), (1024, 19, 2916, ops.KERNEL_RBF)]:
    g = torch.Generator(device=dev).manual_seed(n + d)
    z = torch.randn(b, n, d, device=dev, generator=g) * 0.05
    ls = torch.tensor([1.3], device=dev)
    res = {}
    caps = ("0", "33000", "41000", "54000", "81000")
    for rnd in range(3):
        for lds in caps:
            os.environ["DKT_GRAM_SMALL_LDS"] = lds
            ms, _ = timed(lambda: ops.gram(z, None, kind, ls if kind != ops.KERNEL_LINEAR else None))
            res.setdefault(lds, []).append(ms)
    del os.environ["DKT_GRAM_SMALL_LDS"]
    print("B=%d N=%d D=%d kind=%d  (columns: at most all / 4 / 3 / 2 / 1 workgroups per CU)  %s" % (b, n, d, kind, "  ".join("%.4f" % min(res[l]) for l in caps)), flush=True)
