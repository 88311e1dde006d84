#!/usr/bin/env python3
"""eval_metric=auc benchmark: the torch code (eval_metrics.auc) against the
HIP path (ops/hip.binary_auc), both arms in one process.

Per-call part, at each of --sizes rows, unweighted and weighted: margins
~ N(0, 2^2) rounded to 1/64 (ties, as a model of a few trees gives), labels
drawn from sigmoid(margin). The two arms alternate call by call; each call
ends in its own readback, so a host clock around it times the whole call.
Reported per arm: median, minimum and maximum milliseconds over --repeats
calls after --call-warmup calls. The HIP arm scores with a cached plan, as a
training run does; building the plan, and the key kernel plus torch.sort
alone (device events), are timed next to it.

Training part: binary:logistic, depth 6, Higgs-shape synthetic data (the
bench.py recipe) at the flagship size, rounds/sec for three arms: no eval
set, the training set evaluated on auc by the torch code every round, the
same by the HIP path.

`--no-train --sizes 12500000` keeps a kernel-trace run (rocprofv3
--kernel-trace --stats) short: the auc_* kernels are the new path. Prints one
JSON line per measurement and a markdown table. Needs a GPU.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sagemaker_xgboost_container_amd.data.dmatrix import DeviceDMatrix  # noqa: E402
from sagemaker_xgboost_container_amd.models import eval_metrics, trainer  # noqa: E402
from sagemaker_xgboost_container_amd.models.callback_api import TrainingCallback  # noqa: E402
from sagemaker_xgboost_container_amd.ops import hip  # noqa: E402

FEATURES = 28
MAX_DEPTH = 6


class Timer(TrainingCallback):
    def __init__(self, warmup, steps):
        self.warmup, self.steps = warmup, steps
        self.t0 = self.t1 = None

    def before_iteration(self, model, epoch, evals_log):
        if epoch == self.warmup:
            torch.cuda.synchronize()
            self.t0 = time.perf_counter()
        return False

    def after_iteration(self, model, epoch, evals_log):
        if epoch == self.warmup + self.steps - 1:
            torch.cuda.synchronize()
            self.t1 = time.perf_counter()
            return True
        return False


def synth(rows, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    X = torch.randn((rows, FEATURES), generator=g, device="cuda", dtype=torch.float32)
    logit = X[:, 0] * 2.0 - X[:, 1] + 0.5 * X[:, 2] * X[:, 3] + 0.25 * X[:, 4]
    noise = torch.randn(rows, generator=g, device="cuda") * 0.5
    return X, (logit + noise > 0).to(torch.float32)


def timed_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    value = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, value


def per_call(rows, weighted, repeats, warmup):
    g = torch.Generator(device="cuda")
    g.manual_seed(99)
    margin = torch.round(torch.randn(rows, generator=g, device="cuda") * 2.0 * 64) / 64
    y = (torch.rand(rows, generator=g, device="cuda") < torch.sigmoid(margin)).float()
    w = torch.rand(rows, generator=g, device="cuda") * 1.5 + 0.5 if weighted else None
    hip.auc_plan(y, w)  # warm
    plan_ms, plan = timed_ms(lambda: hip.auc_plan(y, w))
    arms = {"torch": lambda: eval_metrics.auc(margin, y, w),
            "hip": lambda: hip.binary_auc(plan, margin)}
    times = {k: [] for k in arms}
    value = {}
    for i in range(warmup + repeats):
        for name, fn in arms.items():  # alternating
            ms, value[name] = timed_ms(fn)
            if i >= warmup:
                times[name].append(ms)
    sort = []
    for i in range(warmup + repeats):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        hip._K.auc_keys(margin, plan["keys"])
        torch.sort(plan["keys"])
        end.record()
        end.synchronize()
        if i >= warmup:
            sort.append(start.elapsed_time(end))
    row = {"metric": f"auc per call ({rows} rows, {'weighted' if weighted else 'unweighted'})",
           "unit": "ms", "rows": rows, "weighted": weighted, "repeats": repeats,
           "plan_build_ms": plan_ms, "keys_and_sort_median": statistics.median(sort),
           "value_torch": value["torch"], "value_hip": value["hip"]}
    for name, ts in times.items():
        row.update({f"{name}_median": statistics.median(ts), f"{name}_min": min(ts), f"{name}_max": max(ts)})
    return row


def train_arm(arm, dtrain, warmup, steps):
    """Rounds/sec with no eval set ("none") or the training set on auc by
    the torch code ("torch") or by the HIP path ("hip")."""
    device_auc = eval_metrics._device_auc
    if arm == "torch":
        eval_metrics._device_auc = lambda margin, y, weight, plans: eval_metrics.auc(margin, y, weight)
    try:
        timer = Timer(warmup, steps)
        params = {"objective": "binary:logistic", "max_depth": MAX_DEPTH, "eta": 0.3,
                  "tree_method": "gpu_hist", "device": "cuda", "eval_metric": "auc"}
        res = {}
        trainer.train(params, dtrain, num_boost_round=warmup + steps, callbacks=[timer],
                      evals=[] if arm == "none" else [(dtrain, "train")], evals_result=res,
                      verbose_eval=False)
    finally:
        eval_metrics._device_auc = device_auc
    return steps / (timer.t1 - timer.t0), (res["train"]["auc"][-1] if res else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1_000_000, 12_500_000])
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--call-warmup", type=int, default=3)
    ap.add_argument("--train-rows", type=int, default=12_500_000)
    ap.add_argument("--steps", type=int, default=40, help="timed rounds per training arm")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--train-passes", type=int, default=2, help="times the three arms are run, in turn")
    ap.add_argument("--no-train", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_auc.py measures the device: it needs a GPU")

    calls = []
    for rows in args.sizes:
        for weighted in (False, True):
            row = per_call(rows, weighted, args.repeats, args.call_warmup)
            print(json.dumps(row), flush=True)
            calls.append(row)

    trains = []
    if not args.no_train:
        X, y = synth(args.train_rows, seed=1234)
        dtrain = DeviceDMatrix(X, label=y)
        for p in range(args.train_passes):
            for arm in ("none", "torch", "hip"):
                rps, last = train_arm(arm, dtrain, args.warmup, args.steps)
                row = {"metric": f"boost rounds/sec ({args.train_rows}x{FEATURES} binary:logistic depth {MAX_DEPTH})",
                       "eval": arm, "pass": p, "value": rps, "unit": "rounds/sec", "last_auc": last,
                       "steps": args.steps, "warmup": args.warmup}
                print(json.dumps(row), flush=True)
                trains.append(row)

    print("\n| rows | weights | torch ms (min-max) | hip ms (min-max) | keys+sort ms | plan ms | hip - torch value |")
    print("|---|---|---|---|---|---|---|")
    for r in calls:
        print(f"| {r['rows']} | {'yes' if r['weighted'] else 'no'} | "
              f"{r['torch_median']:.3f} ({r['torch_min']:.3f}-{r['torch_max']:.3f}) | "
              f"{r['hip_median']:.3f} ({r['hip_min']:.3f}-{r['hip_max']:.3f}) | "
              f"{r['keys_and_sort_median']:.3f} | {r['plan_build_ms']:.3f} | "
              f"{r['value_hip'] - r['value_torch']:.2e} |")
    if trains:
        print("\n| eval set | pass | rounds/s | last auc |")
        print("|---|---|---|---|")
        for r in trains:
            print(f"| {r['eval']} | {r['pass']} | {r['value']:.2f} | {r['last_auc']} |")


if __name__ == "__main__":
    main()
