"""Ranking on an MSLR-like set, two arms, each comparing two paths in one
process.

gradient: the sampled pair method (one drawn partner per document; on this
data its kernel, lambdarank_mean_tile_kernel) against the top-k LambdaRank
kernels of csrc/smxgb_rank.hip.
eval: ndcg@10, ndcg and map through the per-group Python loop of
models/eval_metrics.py (what SMXGB_FORCE_TORCH_OPS=1 runs) against the
kernels of csrc/smxgb_rank_metric.hip, and a top-k training run that watches
its training set with either.

mean: the default pair method (lambdarank_pair_method=mean) at its defaults,
the per-group Python loop (what SMXGB_FORCE_TORCH_OPS=1 runs, and all there
was before the kernel) against lambdarank_mean_tile_kernel, on 20 000 groups
of 50 documents and on 250 groups of 4 000: the loop pays per group, the
kernel per document. Not part of --arm all.

    python benchmarks/bench_ranking.py [--arm all] [--rows 2400000] [--reps 3] [--rounds 3]

Prints one JSON line: milliseconds per call of each path (median and spread
over the alternating repetitions) and depth-6 training rounds per second
with each path. Needs an MI355X.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sagemaker_xgboost_container_amd.data.dmatrix import DMatrix  # noqa: E402
from sagemaker_xgboost_container_amd.models import eval_metrics, trainer  # noqa: E402
from sagemaker_xgboost_container_amd.models.objectives import create_objective  # noqa: E402


def make_data(rows, features, seed, sizes=None):
    """Seeded, MSLR-like: group sizes in [1, 1300] with a mean near 120
    (lognormal) unless given, labels 0-4 that depend on a few features."""
    rng = np.random.default_rng(seed)
    left = 0 if sizes else rows
    sizes = list(sizes or [])
    while left > 0:
        m = int(min(left, np.clip(rng.lognormal(mean=4.45, sigma=0.8), 1, 1300)))
        sizes.append(m)
        left -= m
    X = rng.standard_normal((rows, features), dtype=np.float32)
    rel = X[:, 0] + 0.5 * X[:, 1] - 0.5 * X[:, 2] + rng.standard_normal(rows, dtype=np.float32)
    y = np.clip(np.floor(rel + 1.5), 0, 4).astype(np.float32)
    return X, y, sizes


def time_gradients(objective, margin, y, reps):
    out = []
    for _ in range(reps):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        objective.gradients(margin, y, None)
        end.record()
        torch.cuda.synchronize()
        out.append(start.elapsed_time(end))
    return out


def time_training(params, dtrain, rounds, evals=None):
    """Seconds per round: (rounds + 1)-round run minus a 1-round run, so that
    the set-up (upload, quantisation) cancels."""
    def run(r):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        trainer.train(params, dtrain, num_boost_round=r, evals=evals, verbose_eval=False)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    one = run(1)
    return (run(rounds + 1) - one) / rounds


def loop_evaluate(metric_name, margin, y, weight, objective, group_ptr=None, rank_plans=None):
    """evaluate() as it runs without the kernels: the per-group loop."""
    base, _, k = metric_name.partition("@")
    fn = {"ndcg": eval_metrics.ndcg, "map": eval_metrics.mean_ap}[base]
    return fn(margin, y, objective, k=int(k) if k else None, group_ptr=group_ptr)


def eval_arm(args, dtrain, sizes, margin, yd):
    """Host milliseconds per evaluate() call, which ends in the readback of
    the value, and rounds per second of a run that watches its training set."""
    objective = create_objective("rank:ndcg", {})
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    plans = {}
    paths = {
        "loop": lambda name: loop_evaluate(name, margin, yd, None, objective, group_ptr=ptr),
        "kernels": lambda name: eval_metrics.evaluate(
            name, margin, yd, None, objective, group_ptr=ptr, rank_plans=plans),
    }
    metrics = ["ndcg@10", "ndcg", "map"]
    values = {p: {} for p in paths}
    ms = {p: {name: [] for name in metrics} for p in paths}
    for rep in range(args.reps + 1):  # the first pass warms up (plans, IDCG, allocator)
        for name in metrics:
            for p, fn in paths.items():  # alternate: both paths see the same machine state
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                values[p][name] = fn(name)
                torch.cuda.synchronize()
                if rep:
                    ms[p][name].append((time.perf_counter() - t0) * 1e3)
    params = {"objective": "rank:ndcg", "lambdarank_pair_method": "topk", "eval_metric": "ndcg",
              "max_depth": 6, "eta": 0.3, "device": "cuda"}
    out = {}
    for p in paths:
        device_evaluate = trainer.evaluate_metric
        if p == "loop":
            trainer.evaluate_metric = loop_evaluate
        try:
            sec = time_training(params, dtrain, args.rounds, evals=[(dtrain, "train")])
        finally:
            trainer.evaluate_metric = device_evaluate
        out[p] = {"round_s": sec, "rounds_per_s": 1.0 / sec}
        for name in metrics:
            t = ms[p][name]
            out[p][name] = {"value": values[p][name], "ms_median": statistics.median(t),
                            "ms_min": min(t), "ms_max": max(t)}
    return out


def mean_arm(args):
    """ms per gradient call and rounds per second of a rank:ndcg run with
    nothing else set, per-group loop against kernel."""
    dev = torch.device("cuda")
    out = {}
    for shape, sizes in (("short_20000x50", [50] * 20000), ("long_250x4000", [4000] * 250)):
        rows = sum(sizes)
        X, y, _ = make_data(rows, args.mean_features, args.seed, sizes)
        dtrain = DMatrix(X, label=y)
        dtrain.set_group(sizes)
        yd = torch.from_numpy(y).to(dev)
        margin = yd * 0.5 + torch.randn(rows, device=dev, generator=torch.Generator(dev).manual_seed(1))
        out[shape] = {}
        for path, force in (("loop", "1"), ("kernel", "0")):
            os.environ["SMXGB_FORCE_TORCH_OPS"] = force  # read by set_info, once per run
            try:
                objective = create_objective("rank:ndcg", {"objective": "rank:ndcg"})
                objective.set_info(dtrain, dev)
                objective.gradients(margin, yd, None)  # warm-up (plan, allocator)
                ms = time_gradients(objective, margin, yd, args.reps)
                sec = time_training({"objective": "rank:ndcg", "max_depth": 6, "eta": 0.3,
                                     "device": "cuda"}, dtrain, args.rounds)
            finally:
                del os.environ["SMXGB_FORCE_TORCH_OPS"]
            out[shape][path] = {
                "grad_ms_median": statistics.median(ms), "grad_ms_min": min(ms),
                "grad_ms_max": max(ms), "round_s": sec, "rounds_per_s": 1.0 / sec,
            }
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=["gradient", "eval", "all", "mean"], default="all")
    ap.add_argument("--mean-features", type=int, default=32)
    ap.add_argument("--rows", type=int, default=2_400_000)
    ap.add_argument("--features", type=int, default=136)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()
    if args.arm == "mean":
        print(json.dumps({"mean": mean_arm(args)}))
        return
    X, y, sizes = make_data(args.rows, args.features, args.seed)
    dtrain = DMatrix(X, label=y)
    dtrain.set_group(sizes)
    dev = torch.device("cuda")
    yd = torch.from_numpy(y).to(dev)
    # margins of a partly trained model: labels plus noise, so ranks are mixed
    margin = (yd * 0.5 + torch.randn(args.rows, device=dev, generator=torch.Generator(dev).manual_seed(1)))
    result = {"rows": args.rows, "groups": len(sizes), "mean_group": args.rows / len(sizes)}
    if args.arm != "gradient":
        result["eval"] = eval_arm(args, dtrain, sizes, margin, yd)
    paths = {
        "sampled": {"objective": "rank:ndcg"},
        "topk": {"objective": "rank:ndcg", "lambdarank_pair_method": "topk"},
    } if args.arm != "eval" else {}
    objectives = {}
    for name, p in paths.items():
        objectives[name] = create_objective(p["objective"], p)
        objectives[name].set_info(dtrain, dev)
        objectives[name].gradients(margin, yd, None)  # warm-up (plan, allocator)
    grad_ms = {name: [] for name in paths}
    for _ in range(args.reps):  # alternate: both paths see the same machine state
        for name in paths:
            grad_ms[name] += time_gradients(objectives[name], margin, yd, 1)
    for name, p in paths.items():
        ms = grad_ms[name]
        sec = time_training(dict(p, max_depth=6, eta=0.3, device="cuda"), dtrain, args.rounds)
        result[name] = {
            "grad_ms_median": statistics.median(ms), "grad_ms_min": min(ms), "grad_ms_max": max(ms),
            "round_s": sec, "rounds_per_s": 1.0 / sec,
            "grad_share_of_round": statistics.median(ms) / 1e3 / sec,
        }
    print(json.dumps(result))


if __name__ == "__main__":
    main()
