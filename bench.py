#!/usr/bin/env python3
"""Flagship benchmark: Higgs-shape binary:logistic hist training on MI355X.

Driver contract:
    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
A plain run sets up, warms up, times the K steps and prints the result line;
--dump-outputs additionally saves the trained model as .npy arrays.
For N > 1 the driver launches this under torch.distributed.run, one rank per
GPU over RCCL. A "step" is one boosting iteration. Weak scaling: each GPU
trains its own 12.5M x 28 row shard (N=8 -> the 100M x 28 BASELINE config;
N=1 covers the 10M x 28 headline config with a 1.25x larger shard) with the
per-level histogram allreduce over xGMI.

Rank 0 prints ONE JSON line with the whole-job metric.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from sagemaker_xgboost_container_amd.data.dmatrix import DeviceDMatrix, DMatrix  # noqa: E402
from sagemaker_xgboost_container_amd.models import trainer  # noqa: E402
from sagemaker_xgboost_container_amd.models.callback_api import TrainingCallback  # noqa: E402
from sagemaker_xgboost_container_amd.parallel import comm as comm_mod  # noqa: E402

ROWS_PER_GPU = 12_500_000
FEATURES = 28


class BenchTimer(TrainingCallback):
    def __init__(self, warmup, steps, sync):
        self.warmup = warmup
        self.steps = steps
        self.sync = sync
        self.t0 = None
        self.t1 = None

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


def synth_shard(rows, features, device, seed):
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    X = torch.randn((rows, features), generator=g, device=device, dtype=torch.float32)
    logit = X[:, 0] * 2.0 - X[:, 1] + 0.5 * X[:, 2] * X[:, 3] + 0.25 * X[:, 4]
    noise = torch.randn(rows, generator=g, device=device) * 0.5
    y = (logit + noise > 0).to(torch.float32)
    return X, y


DUMP_SAMPLE_ROWS = 1 << 16
DUMP_SAMPLE_SEED = 20240521


def dump_outputs(out_dir, booster, X):
    """Write what the timed training run returned to its caller — the
    Booster — as DIR/<name>.npy, so two builds can be compared output for
    output.

    tree_*: every tree's node arrays, concatenated in boosting order
    (tree_num_nodes gives the per-tree lengths; the trees of the last timed
    step come last). Ids, bins and flags are stored as float64 (exact),
    thresholds, leaf values, gains and hessian sums as float32.
    margin_sample: the model's raw margin on a fixed, seeded sample of
    DUMP_SAMPLE_ROWS training rows (float32) — comparable under a
    tolerance even where two builds break a split tie differently.
    A few MB in all at the default sizes.
    """
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    trees = [t.finalize() for t in booster.trees]
    arrays = {"tree_num_nodes": np.asarray([t.num_nodes for t in trees], dtype=np.float64)}
    for name, dtype in (
        ("left", np.float64), ("right", np.float64), ("feature", np.float64),
        ("split_bin", np.float64), ("default_left", np.float64),
        ("threshold", np.float32), ("value", np.float32),
        ("gain", np.float32), ("sum_hess", np.float32),
    ):
        arrays[f"tree_{name}"] = np.concatenate([np.asarray(getattr(t, name)) for t in trees]).astype(dtype)

    g = torch.Generator(device="cpu")
    g.manual_seed(DUMP_SAMPLE_SEED)
    n = X.shape[0]
    idx = torch.randperm(n, generator=g)[: min(n, DUMP_SAMPLE_ROWS)].sort().values
    sample = X[idx.to(X.device)].cpu().numpy()
    arrays["margin_sample_rows"] = idx.numpy().astype(np.float64)
    arrays["margin_sample"] = np.asarray(
        booster.predict(sample, output_margin=True), dtype=np.float32
    )
    for name, arr in arrays.items():
        np.save(os.path.join(out_dir, f"{name}.npy"), arr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100, help="timed boosting rounds")
    ap.add_argument("--warmup", type=int, default=10, help="untimed rounds before the timed ones")
    ap.add_argument("--rows-per-gpu", type=int, default=ROWS_PER_GPU)
    ap.add_argument("--features", type=int, default=FEATURES)
    ap.add_argument("--max-depth", type=int, default=6)
    ap.add_argument("--max-bin", type=int, default=256)
    ap.add_argument(
        "--dump-outputs", metavar="DIR", default=None,
        help="after the timed steps, write the trained model's arrays and its margins on a "
             "fixed row sample as DIR/<name>.npy (rank 0)",
    )
    ap.add_argument(
        "--full", action="store_true",
        help="also run the measurements and checks that the headline figure does not need. "
             "This benchmark has none: everything else is measured by the scripts under "
             "benchmarks/, so the option changes nothing here",
    )
    args = ap.parse_args()

    use_gpu = torch.cuda.is_available()
    comm = comm_mod.init_from_env()
    world = comm.world_size if comm else 1
    rank = comm.rank if comm else 0
    if use_gpu:
        local = int(os.environ.get("LOCAL_RANK", 0)) % max(torch.cuda.device_count(), 1)
        device = torch.device("cuda", local)
        torch.cuda.set_device(device)
    else:
        device = torch.device("cpu")

    rows = args.rows_per_gpu if use_gpu else 200_000  # CPU fallback for smoke runs
    X, y = synth_shard(rows, args.features, device, seed=1234 + rank)
    if use_gpu:
        dtrain = DeviceDMatrix(X, label=y)
    else:
        dtrain = DMatrix(X.numpy(), label=y.numpy())

    def sync():
        if comm:
            comm.barrier()
        if use_gpu:
            torch.cuda.synchronize()

    timer = BenchTimer(args.warmup, args.steps, sync)
    params = {
        "objective": "binary:logistic",
        "tree_method": "gpu_hist" if use_gpu else "hist",
        "max_depth": args.max_depth,
        "max_bin": args.max_bin,
        "eta": 0.3,
        "device": str(device),
    }
    booster = trainer.train(
        params,
        dtrain,
        num_boost_round=args.warmup + args.steps,
        callbacks=[timer],
        verbose_eval=False,
        comm=comm,
    )

    elapsed = timer.t1 - timer.t0
    if comm:
        t = torch.tensor([elapsed], dtype=torch.float64, device=device if use_gpu else "cpu")
        comm.allreduce_max_(t)
        elapsed = float(t[0])

    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, booster, X)

    if rank == 0:
        rounds_per_sec = args.steps / elapsed
        total_rows = rows * world
        result = {
            "metric": "boost rounds/sec (10M×28 Higgs-shape, hist)",
            "value": rounds_per_sec,
            "unit": "rounds/sec",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed * 1000.0 / args.steps,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "fp32",
            "data": "synthetic (randn Higgs-shape, random-init model)",
            "config": {
                "model": "xgboost binary:logistic hist",
                "rows_per_gpu": rows,
                "total_rows": total_rows,
                "features": args.features,
                "max_depth": args.max_depth,
                "max_bin": args.max_bin,
                "global_batch": total_rows,
                "seq_len": None,
                "parallelism": f"dp{world} (row-sharded, RCCL histogram allreduce)",
                "rows_x_rounds_per_sec": rounds_per_sec * total_rows,
            },
        }
        print(json.dumps(result))

    comm_mod.shutdown()


if __name__ == "__main__":
    main()
