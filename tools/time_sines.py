#!/usr/bin/env python
"""Timings of the sine-wave experiment (docs/SINES.md).  One section per process, so that a job runs each under its own time limit:

  python tools/time_sines.py kernels [out.json]   task-resident kernels (libdkt_smk.so) against the generic pair (ops.smk / ops.smk_bwd + the torch
                                                  reductions of ops.spectral_mixture_matrix) at N = 10, D = 40, Q = 4 for B = 1, 64, 1024 (forward +
                                                  backward), and the test-phase cross matrix M = 195, N = 5 for 500 tasks (forward); outputs compared
  python tools/time_sines.py steps [out.json]     SinesDKT.train_loop, ms per Adam step and tasks/s at B = 1, 64, 1024 tasks per step
  python tools/time_sines.py test [out.json]      the 500-task test phase (SinesDKT.test_loop: sampling, MLP, GP conditioning, prediction, MSE)
  python tools/time_sines.py prof                 a short fixed workload to run under rocprofv3 --kernel-trace --stats

Times: HIP events around the timed loop (kernels) or host clock around work that ends in a device synchronise (steps, test); median of repeats.
Measurement tooling; prints, never asserts."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dkt_amd import ops, sines  # noqa: E402


def _events_ms(fn, reps, inner):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / inner)
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def _hyp(dev, q=4, d=40, seed=0):
    g = torch.Generator().manual_seed(seed)
    w = (torch.rand(q, generator=g) + 0.2).to(dev)
    mu = (torch.rand(q, d, generator=g) * 0.4 + 0.05).to(dev)
    sg = (torch.rand(q, d, generator=g) * 0.2 + 0.02).to(dev)
    return w, mu, sg


def kernels(dev):
    res = {}
    w, mu, sg = _hyp(dev)
    g = torch.Generator(device=dev).manual_seed(1)
    for b in (1, 64, 1024):
        x = torch.rand(b, 10, 40, device=dev, generator=g)
        ge = torch.randn(b, 10, 10, device=dev, generator=g)

        def task():
            ops.smk_task(x, None, w, mu, sg)
            return ops.smk_task_bwd(ge, x, w, mu, sg)

        def generic():
            e, eq = ops.smk(x, None, w, mu, sg, want_terms=True)
            dz, dmb, dsb = ops.smk_bwd(ge, eq, x, w, mu, sg)
            return dz, (ge.unsqueeze(1) * eq).sum((0, 2, 3)), dmb.sum(0), dsb.sum(0)

        t_out, g_out = task(), generic()
        err = {k: float((u - v).abs().max() / v.abs().max().clamp_min(1e-30)) for k, u, v in zip(("dx", "dw", "dmu", "dsg"), t_out, g_out)}
        e_err = float((ops.smk_task(x, None, w, mu, sg) - ops.smk(x, None, w, mu, sg)[0]).abs().max())
        inner = 200 if b < 1024 else 50
        tt = _events_ms(task, 7, inner)
        tg = _events_ms(generic, 7, inner if b < 1024 else 10)
        res["fwd_bwd_B%d" % b] = dict(task_ms=tt, generic_ms=tg, speedup=tg[0] / tt[0], rel_err_vs_generic=err, e_abs_err=e_err)
        print("N=10 D=40 Q=4 B=%-5d fwd+bwd  task %.4f ms  generic %.4f ms  x%.1f   rel diff %s" % (b, tt[0], tg[0], tg[0] / tt[0], err), flush=True)
        tf = _events_ms(lambda: ops.smk_task(x, None, w, mu, sg), 7, inner)
        gf = _events_ms(lambda: ops.smk(x, None, w, mu, sg, want_terms=True), 7, inner)
        res["fwd_B%d" % b] = dict(task_ms=tf, generic_ms=gf, speedup=gf[0] / tf[0])
        print("N=10 D=40 Q=4 B=%-5d fwd      task %.4f ms  generic %.4f ms  x%.1f" % (b, tf[0], gf[0], gf[0] / tf[0]), flush=True)
    xs = torch.rand(500, 5, 40, device=dev, generator=g)
    xq = torch.rand(500, 195, 40, device=dev, generator=g)
    d = float((ops.smk_task(xq, xs, w, mu, sg) - ops.smk(xq, xs, w, mu, sg)[0]).abs().max())
    tt = _events_ms(lambda: ops.smk_task(xq, xs, w, mu, sg), 7, 50)
    tg = _events_ms(lambda: ops.smk(xq, xs, w, mu, sg), 7, 10)
    res["cross_M195_N5_B500"] = dict(task_ms=tt, generic_ms=tg, speedup=tg[0] / tt[0], e_abs_err=d)
    print("cross M=195 N=5 B=500 fwd  task %.4f ms  generic %.4f ms  x%.1f  max |diff| %.2e" % (tt[0], tg[0], tg[0] / tt[0], d), flush=True)
    return res


def steps(dev):
    res = {}
    for b, n_steps in ((1, 500), (64, 200), (1024, 50)):
        torch.manual_seed(0)
        m = sines.SinesDKT(sampler=sines.SineTaskSampler(seed=0, device=dev)).to(dev)
        opt = torch.optim.Adam([{'params': m.model.parameters(), 'lr': 1e-3}, {'params': m.feature_extractor.parameters(), 'lr': 1e-3}])
        for _ in range(20):
            m.train_loop(1, opt, b)              # step 1: no log line (it prints at multiples of 100)
        reps = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n_steps):
                m.train_loop(1, opt, b)
            torch.cuda.synchronize()
            reps.append((time.perf_counter() - t0) * 1e3 / n_steps)
        ms = float(np.median(reps))
        res["B%d" % b] = dict(ms_per_step=ms, spread=[float(min(reps)), float(max(reps))], tasks_per_s=b * 1e3 / ms)
        print("train step B=%-5d %.3f ms/step (%.3f .. %.3f)  %.0f tasks/s" % (b, ms, min(reps), max(reps), b * 1e3 / ms), flush=True)
    return res


def test_phase(dev):
    torch.manual_seed(0)
    m = sines.SinesDKT(test_sampler=sines.SineTaskSampler(seed=1, device=dev)).to(dev)
    for _ in range(5):
        m.test_loop(500)
    reps = []
    for _ in range(21):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.test_loop(500)                         # ends in .cpu(): synchronised
        reps.append((time.perf_counter() - t0) * 1e3)
    t = sines.SineTaskSampler(seed=2, device=dev).test_batch(500)
    pr = _events_ms(lambda: m.predict(t["x_support"], t["y_support"], t["x_query"]), 7, 20)
    res = dict(test_loop_ms=float(np.median(reps)), spread=[float(min(reps)), float(max(reps))], predict_ms=pr)
    print("test phase, 500 tasks: test_loop %.3f ms (%.3f .. %.3f), predict alone %.3f ms" % (res["test_loop_ms"], min(reps), max(reps), pr[0]),
          flush=True)
    return res


def prof(dev):
    """A short workload for rocprofv3 --kernel-trace --stats: 20 training steps at B = 1024, 5 test phases, 20 generic fwd + bwd pairs at
    B = 1024 (the per-kernel split of the step, the test phase and the generic kernels)."""
    torch.manual_seed(0)
    m = sines.SinesDKT(sampler=sines.SineTaskSampler(seed=0, device=dev), test_sampler=sines.SineTaskSampler(seed=1, device=dev)).to(dev)
    opt = torch.optim.Adam([{'params': m.model.parameters(), 'lr': 1e-3}, {'params': m.feature_extractor.parameters(), 'lr': 1e-3}])
    for _ in range(20):
        m.train_loop(1, opt, 1024)
    for _ in range(5):
        m.test_loop(500)
    w, mu, sg = _hyp(dev)
    x = torch.rand(1024, 10, 40, device=dev)
    ge = torch.randn(1024, 10, 10, device=dev)
    for _ in range(20):
        e, eq = ops.smk(x, None, w, mu, sg, want_terms=True)
        ops.smk_bwd(ge, eq, x, w, mu, sg)
    torch.cuda.synchronize()
    return {}


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "kernels"
    dev = torch.device("cuda", 0)
    res = {"kernels": kernels, "steps": steps, "test": test_phase, "prof": prof}[what](dev)
    res["device"] = torch.cuda.get_device_name(0)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
