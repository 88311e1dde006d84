#!/usr/bin/env python3
"""Categorical features benchmark: what set-valued splits cost per round.

1M x 16 synthetic binary classification, depth 6: 8 categorical columns of
32 categories each (the label depends on category membership) and 8 numeric
columns. Three arms in one process invocation, steady-state ms/round each:

  categorical            the columns typed "c": per-level grower, category-set
                         split scan, membership partition
  numeric, per level     the same matrix typed numeric on the same per-level
                         path (SMXGB_NO_DEVICE_GROW=1): what the categorical
                         kernels add to that path
  one-hot, device grower the categorical columns expanded to 0/1 indicator
                         columns (8 + 8 * 32 = 264 columns) on the device
                         grower: what a user without categorical support
                         would train today

Prints one JSON line per arm and a markdown table.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sagemaker_xgboost_container_amd.data.dmatrix import DeviceDMatrix, DMatrix  # noqa: E402
from sagemaker_xgboost_container_amd.models import trainer  # noqa: E402
from sagemaker_xgboost_container_amd.models.callback_api import TrainingCallback  # noqa: E402

N_CAT, N_NUM, CATEGORIES, MAX_DEPTH = 8, 8, 32, 6


class Timer(TrainingCallback):
    def __init__(self, warmup, steps, sync):
        self.warmup, self.steps, self.sync = warmup, steps, sync
        self.t0 = self.t1 = None

    def before_iteration(self, model, epoch, evals_log):
        if epoch == self.warmup:
            self.sync()
            self.t0 = time.perf_counter()
        return False

    def after_iteration(self, model, epoch, evals_log):
        if epoch == self.warmup + self.steps - 1:
            self.sync()
            self.t1 = time.perf_counter()
            return True
        return False


def synth(rows, device, seed):
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    cat = torch.randint(0, CATEGORIES, (rows, N_CAT), generator=g, device=device)
    num = torch.randn((rows, N_NUM), generator=g, device=device)
    # membership in fixed category sets drives the label
    member = ((cat * 7 + torch.arange(N_CAT, device=device)) % 5 < 2).to(torch.float32)
    logit = member[:, 0] * 2.0 - member[:, 1] * 1.5 + member[:, 2] * member[:, 3] + num[:, 0]
    y = (logit + 0.5 * torch.randn(rows, generator=g, device=device) > 0.7).to(torch.float32)
    return cat, num, y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=20, help="timed rounds per arm")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--arms", default="categorical,numeric,onehot")
    args = ap.parse_args()

    use_gpu = torch.cuda.is_available()
    device = torch.device("cuda" if use_gpu else "cpu")
    rows = args.rows if use_gpu else min(args.rows, 20_000)

    def sync():
        if use_gpu:
            torch.cuda.synchronize()

    cat, num, y = synth(rows, device, seed=1234)
    as_float = torch.cat([cat.to(torch.float32), num], 1)
    types = ["c"] * N_CAT + ["q"] * N_NUM

    def matrix(X, feature_types=None):
        if use_gpu:
            return DeviceDMatrix(X, label=y, feature_types=feature_types)
        return DMatrix(X.numpy(), label=y.numpy(), feature_types=feature_types)

    def onehot():
        hot = torch.nn.functional.one_hot(cat, CATEGORIES).reshape(rows, -1).to(torch.float32)
        return torch.cat([hot, num], 1)

    arms = {
        "categorical": (lambda: matrix(as_float, types), {}),
        "numeric": (lambda: matrix(as_float), {"SMXGB_NO_DEVICE_GROW": "1"}),
        "onehot": (lambda: matrix(onehot()), {}),
    }
    table = []
    for arm in args.arms.split(","):
        make, env = arms[arm]
        saved = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            dtrain = make()
            params = {"objective": "binary:logistic", "max_depth": MAX_DEPTH, "eta": 0.3,
                      "tree_method": "gpu_hist" if use_gpu else "hist", "device": str(device)}
            timer = Timer(args.warmup, args.steps, sync)
            res = {}
            trainer.train(params, dtrain, num_boost_round=args.warmup + args.steps,
                          callbacks=[timer], evals=[(dtrain, "train")], evals_result=res,
                          verbose_eval=False)
        finally:
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        row = {
            "metric": f"ms/round ({rows} rows, depth {MAX_DEPTH})", "arm": arm,
            "columns": dtrain.num_col(), "value": (timer.t1 - timer.t0) * 1e3 / args.steps,
            "unit": "ms/round", "steps": args.steps, "warmup": args.warmup,
            "train_logloss_last": res["train"]["logloss"][-1],
        }
        print(json.dumps(row), flush=True)
        table.append(row)
        del dtrain

    print("\n| arm | columns | ms/round | train logloss |")
    print("|---|---|---|---|")
    for r in table:
        print(f"| {r['arm']} | {r['columns']} | {r['value']:.2f} | {r['train_logloss_last']:.4f} |")


if __name__ == "__main__":
    main()
