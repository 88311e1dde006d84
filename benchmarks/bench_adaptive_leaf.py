#!/usr/bin/env python3
"""Adaptive tree leaves benchmark: what the per-leaf quantile pass costs.

Depth 6 on synthetic regression data (the bench.py feature recipe, a
continuous label with heavy-tailed noise). Arms, all in one process
invocation:

  reg:squarederror                   no leaf pass, fused gradient kernel
  reg:absoluteerror                  adaptive leaves (median per leaf)
  reg:absoluteerror, Newton leaves   the objective as it was before adaptive
                                     leaves existed (adaptive_alphas unset):
                                     the same gradients and trees' cost
                                     without the leaf pass

Each arm reports steady-state ms/round. It then times the leaf pass alone
(device events): the traversal that assigns rows to leaves, and
leaf_quantiles (count, scatter, 4 x (hist, select), next, final) on the
leaves of a trained depth-6 tree, unweighted and weighted.

Prints one JSON line per measurement and a markdown table.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sagemaker_xgboost_container_amd.data.dmatrix import DeviceDMatrix, DMatrix  # noqa: E402
from sagemaker_xgboost_container_amd.models import objectives, trainer  # noqa: E402
from sagemaker_xgboost_container_amd.models.callback_api import TrainingCallback  # noqa: E402
from sagemaker_xgboost_container_amd.ops import backend_for  # noqa: E402

FEATURES = 28
MAX_DEPTH = 6
ARMS = ("reg:squarederror", "reg:absoluteerror", "reg:absoluteerror (Newton leaves)")


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
    X = torch.randn((rows, FEATURES), generator=g, device=device, dtype=torch.float32)
    signal = X[:, 0] * 2.0 - X[:, 1] + 0.5 * X[:, 2] * X[:, 3] + 0.25 * X[:, 4]
    noise = torch.randn(rows, generator=g, device=device)
    heavy = noise / torch.rand(rows, generator=g, device=device).clamp_min(0.05).sqrt()
    return X, (signal + 0.5 * heavy).to(torch.float32)


def time_ms(fn, sync, repeats):
    """Mean milliseconds per call over `repeats` calls after one warm call."""
    fn()
    sync()
    if torch.cuda.is_available():
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(repeats):
            fn()
        end.record()
        end.synchronize()
        return start.elapsed_time(end) / repeats
    t0 = time.perf_counter()
    for _ in range(repeats):
        fn()
    return (time.perf_counter() - t0) * 1e3 / repeats


def leaf_pass_timing(bst, X, y, device, sync, repeats=20):
    """The leaf pass alone on the first tree of `bst`."""
    backend = backend_for(device)
    tree = bst.trees[0]
    leaf_ids = np.nonzero(np.asarray(tree.left) < 0)[0]
    slot = np.full(tree.num_nodes, -1, dtype=np.int32)
    slot[leaf_ids] = np.arange(len(leaf_ids), dtype=np.int32)
    slot_dev = torch.from_numpy(slot).to(device)
    if device.type == "cuda":
        flat = backend.make_flat_forest([tree], [0], None, device)

        def traverse():
            return slot_dev[backend.pred_leaf(flat, X)[:, 0].long()]
    else:
        from sagemaker_xgboost_container_amd.ops import torch_ref

        def traverse():
            return slot_dev[torch_ref.tree_leaf_ids(tree, X).long()]

    pos = traverse()
    resid = (y - 0.5).to(torch.float32)
    weight = torch.rand(y.shape[0], device=device) + 0.5
    kwargs = dict(check=False) if device.type == "cuda" else {}
    wkwargs = dict(kwargs, weight_max=float(weight.max())) if device.type == "cuda" else {}
    n_leaves = len(leaf_ids)
    return {
        "metric": f"leaf pass alone ({y.shape[0]} rows, {n_leaves} leaves)", "unit": "ms",
        "backend": backend.NAME,
        "assign_rows_to_leaves": time_ms(traverse, sync, repeats),
        "leaf_quantiles_unweighted": time_ms(
            lambda: backend.leaf_quantiles(pos, resid, n_leaves, 0.5, **kwargs), sync, repeats),
        "leaf_quantiles_weighted": time_ms(
            lambda: backend.leaf_quantiles(pos, resid, n_leaves, 0.5, weight, **wkwargs), sync, repeats),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--steps", type=int, default=30, help="timed rounds per arm")
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()

    use_gpu = torch.cuda.is_available()
    device = torch.device("cuda" if use_gpu else "cpu")
    rows = args.rows if use_gpu else min(args.rows, 50_000)

    def sync():
        if use_gpu:
            torch.cuda.synchronize()

    X, y = synth(rows, device, seed=1234)
    dtrain = DeviceDMatrix(X, label=y) if use_gpu else DMatrix(X.numpy(), label=y.numpy())

    table = []
    adaptive_bst = None
    for arm in ARMS:
        name = arm.split(" ")[0]
        newton = arm.endswith("(Newton leaves)")
        params = {"objective": name, "max_depth": MAX_DEPTH, "eta": 0.3,
                  "tree_method": "gpu_hist" if use_gpu else "hist", "device": str(device)}
        timer = Timer(args.warmup, args.steps, sync)
        saved = objectives.AbsoluteError.adaptive_alphas
        if newton:
            objectives.AbsoluteError.adaptive_alphas = None
        try:
            bst = trainer.train(params, dtrain, num_boost_round=args.warmup + args.steps,
                                callbacks=[timer], verbose_eval=False)
        finally:
            objectives.AbsoluteError.adaptive_alphas = saved
        if name == "reg:absoluteerror" and not newton:
            adaptive_bst = bst
        row = {
            "metric": f"ms/round ({rows}x{FEATURES} depth {MAX_DEPTH})", "arm": arm,
            "value": (timer.t1 - timer.t0) * 1e3 / args.steps, "unit": "ms/round",
            "steps": args.steps, "warmup": args.warmup,
        }
        print(json.dumps(row), flush=True)
        table.append(row)

    alone = leaf_pass_timing(adaptive_bst, X, y, device, sync)
    print(json.dumps(alone), flush=True)

    print("\n| arm | ms/round |")
    print("|---|---|")
    for r in table:
        print(f"| {r['arm']} | {r['value']:.2f} |")
    by_arm = {r["arm"]: r["value"] for r in table}
    print(f"\nleaf pass per round (adaptive - Newton leaves): "
          f"{by_arm[ARMS[1]] - by_arm[ARMS[2]]:.2f} ms; alone: assign "
          f"{alone['assign_rows_to_leaves']:.2f} ms + quantiles "
          f"{alone['leaf_quantiles_unweighted']:.2f} ms "
          f"(weighted {alone['leaf_quantiles_weighted']:.2f} ms)")


if __name__ == "__main__":
    main()
