#!/usr/bin/env python
"""test_regression.py's evaluation with the test NLL on request (docs/POSTERIOR.md).  Same flags, checkpoint location and MSE lines as test_regression.py;
`--nll` (off by default) then draws `--n_test_epochs` further test tasks and also prints the mean per-point joint predictive NLL, -logp / M, and its marginal
counterpart, -lpd / M: all M frames of a task are the query set, support frames included, as `test_loop` predicts them, observation noise included.

  python eval_regression.py --method DKT [--spectral] [--n_support 5] [--n_test_epochs 10] [--nll]
"""
import numpy as np
import torch

from dkt_amd.data import SyntheticHeadPoseSampler
from dkt_amd.io_utils import parse_args_regression
from test_regression import evaluate
from train_regression import build_model, checkpoint_path, seed_everything


def _task_nll(model, n_support):
    """One test task -- a random person that is not the last, `n_support` random frames of theirs as the support set, every frame as the query set --
    scored by `DKTRegression.joint_log_likelihood`: (-logp / M, -lpd / M) as floats."""
    inputs, targets = model.batch_fn("test")
    support = torch.as_tensor(np.random.choice(inputs.shape[1], replace=False, size=n_support))
    person = np.random.randint(0, max(inputs.shape[0] - 1, 1))
    x, y = inputs[person].to(model.device), targets[person].to(model.device)
    model.eval()
    with torch.no_grad():
        logp, lpd = model.joint_log_likelihood(model._features(x[support]), y[support], model._features(x), y)
    return -logp.item() / x.shape[0], -lpd.item() / x.shape[0]


def evaluate_nll(model, n_support, n_tasks):
    """([-logp / M], [-lpd / M]) over `n_tasks` test tasks."""
    pairs = [_task_nll(model, n_support) for _ in range(n_tasks)]
    return [j for j, _ in pairs], [m for _, m in pairs]


def main(argv=None):
    params = parse_args_regression('eval_regression', argv)
    seed_everything(params.seed)
    model = build_model(params, SyntheticHeadPoseSampler(seed=params.seed + 1))
    model.load_checkpoint(checkpoint_path(params))
    mse = evaluate(model, params.n_support, params.n_test_epochs)      # (first, with test_regression.py's draws: the MSE lines are its lines)
    bar = "-" * 19
    print("%s\nAverage MSE: %s +- %s\n%s" % (bar, str(np.mean(mse)), str(np.std(mse)), bar))
    if not params.nll:
        return mse
    joint, marginal = evaluate_nll(model, params.n_support, params.n_test_epochs)
    print("Average joint NLL per point: %s +- %s\nAverage marginal NLL per point: %s +- %s\n%s"
          % (str(np.mean(joint)), str(np.std(joint)), str(np.mean(marginal)), str(np.std(marginal)), bar))
    return mse, joint, marginal


if __name__ == '__main__':
    main()
