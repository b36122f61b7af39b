#!/usr/bin/env python
"""Sine-wave regression with DKT on the HIP hot path: the reference's sines/train_DKT.py (its plots aside).

Trains the 1 -> 40 -> 40 MLP and the spectral-mixture GP (Q = 4) on tasks of 10 points from x in (-5, 5), one Adam step per task (lr 1e-3
for both parameter groups), then conditions on 5 support points of each of 500 test tasks and reports the MSE on their 195 query points.

  python train_sines.py [--test_range in|out] [--family sine|cosine] [--iterations 50000] [--tasks_per_step 1] [--seed 0]
                        [--checkpoint PATH] [--test_only]

--tasks_per_step B > 1 averages -logp / N over B tasks per step (this build's batched path).  The task draws are seeded (training and test
from separate streams), so --test_only on a saved checkpoint repeats the test phase exactly.
"""
import time

import numpy as np
import torch

from dkt_amd import sines
from dkt_amd.io_utils import parse_args_sines


def main(argv=None):
    params = parse_args_sines(argv)
    np.random.seed(params.seed)
    torch.manual_seed(params.seed)
    train_sampler = sines.SineTaskSampler(sines.TRAIN_RANGE, params.family, seed=params.seed)
    test_sampler = sines.SineTaskSampler(sines.TEST_RANGES[params.test_range], params.family, seed=params.seed + 1000003)
    model = sines.SinesDKT(n_shot_test=params.n_shot_test, sampler=train_sampler, test_sampler=test_sampler).cuda()
    if params.test_only:
        model.load_checkpoint(params.checkpoint)
    else:
        optimizer = torch.optim.Adam([{'params': model.model.parameters(), 'lr': params.lr},
                                      {'params': model.feature_extractor.parameters(), 'lr': params.lr}])
        model.train()
        t0 = time.time()
        for step in range(params.iterations):
            model.train_loop(step, optimizer, params.tasks_per_step, n_shot=params.n_shot_train)
        torch.cuda.synchronize()
        print("Training: %d steps of %d task(s) in %.1f s" % (params.iterations, params.tasks_per_step, time.time() - t0))
        if params.checkpoint:
            model.save_checkpoint(params.checkpoint)
    print("Test, please wait...")
    mse_list = model.test_loop(params.n_test_tasks)
    print(sines.summary(mse_list))
    return model, mse_list


if __name__ == "__main__":
    main()
