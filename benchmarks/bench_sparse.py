#!/usr/bin/env python3
"""Wide sparse (CSR) training on the GPU: device sparse path vs densifying.

Synthetic n x f CSR at a given density (default 500k x 20k at 0.1 %),
binary:logistic, depth 6. Two arms in one invocation, each in a fresh child
process so that peak host RSS and peak device memory belong to that arm
alone:

* ``sparse`` — SMXGB_SPARSE=1: quantized CSR on the device (ops/hip_sparse.py)
* ``dense``  — SMXGB_SPARSE=0: to_dense() on the host, n x f float32 to HBM,
  n x f bin matrix, dense device grower (the only GPU behaviour before the
  device sparse path existed)

Per arm: data-to-first-round seconds (DMatrix in hand -> first round done:
quantization, upload, round 0), steady-state ms per round over the
remaining rounds, torch.cuda.max_memory_allocated() and peak host RSS.
Prints one JSON line per arm and a markdown table.

Values are drawn from --levels distinct levels (default 64, count-like
libsvm features) so both arms use uint8 bins; --levels 0 draws continuous
values (more than 255 cuts per feature -> int16 bins in both arms).
"""
import argparse
import json
import os
import resource
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_data(n, f, density, levels, seed=0):
    import numpy as np
    import scipy.sparse as sp

    rng = np.random.default_rng(seed)
    nnz = int(n * f * density)
    rows = rng.integers(0, n, nnz, dtype=np.int64)
    cols = rng.integers(0, f, nnz, dtype=np.int64)
    csr = sp.csr_matrix(
        (np.ones(nnz, dtype=np.float32), (rows, cols)), shape=(n, f), dtype=np.float32
    )
    csr.sum_duplicates()
    if levels > 0:
        csr.data = rng.integers(1, levels + 1, csr.nnz).astype(np.float32)
    else:
        csr.data = rng.normal(size=csr.nnz).astype(np.float32)
    # label from the first 64 columns so the trees have something to find
    head = csr[:, : min(64, f)]
    score = np.asarray(head.sum(axis=1)).ravel() + rng.normal(scale=0.5, size=n)
    y = (score > np.median(score)).astype(np.float32)
    return csr, y


def run_arm(args):
    os.environ["SMXGB_SPARSE"] = "1" if args.arm == "sparse" else "0"
    import torch

    from sagemaker_xgboost_container_amd.data.dmatrix import DMatrix
    from sagemaker_xgboost_container_amd.models import trainer
    from sagemaker_xgboost_container_amd.models.callback_api import TrainingCallback

    csr, y = make_data(args.rows, args.cols, args.density, args.levels)
    dtrain = DMatrix(csr, label=y)
    rss_data = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0

    class Stamps(TrainingCallback):
        def __init__(self):
            self.t = []

        def after_iteration(self, model, epoch, evals_log):
            torch.cuda.synchronize()
            self.t.append(time.perf_counter())
            return False

    stamps = Stamps()
    torch.cuda.init()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    bst = trainer.train(
        {"objective": "binary:logistic", "max_depth": args.depth, "eta": 0.3, "device": "cuda"},
        dtrain, num_boost_round=args.rounds, verbose_eval=False, callbacks=[stamps],
    )
    torch.cuda.synchronize()
    first = stamps.t[0] - t0
    steady = stamps.t[1:]
    ms_round = (steady[-1] - stamps.t[0]) / len(steady) * 1e3 if steady else float("nan")
    print(json.dumps({
        "arm": args.arm, "rows": args.rows, "cols": args.cols, "nnz": int(csr.nnz),
        "levels": args.levels, "depth": args.depth, "rounds": args.rounds,
        "data_to_first_round_s": round(first, 3),
        "ms_per_round": round(ms_round, 3),
        "device_peak_mb": round(torch.cuda.max_memory_allocated() / 2**20, 1),
        "host_rss_after_data_mb": round(rss_data, 1),
        "host_peak_rss_mb": round(resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0, 1),
        "trees": len(bst.trees),
        "nodes": int(sum(t.num_nodes for t in bst.trees)),
    }), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", type=int, default=500_000)
    ap.add_argument("--cols", type=int, default=20_000)
    ap.add_argument("--density", type=float, default=0.001)
    ap.add_argument("--levels", type=int, default=64)
    ap.add_argument("--depth", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--arms", default="sparse,dense")
    ap.add_argument("--arm", choices=("sparse", "dense"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.arm:
        run_arm(args)
        return 0

    results = []
    for arm in args.arms.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--arm", arm]
        for name in ("rows", "cols", "density", "levels", "depth", "rounds"):
            cmd += [f"--{name}", str(getattr(args, name))]
        proc = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if proc.returncode != 0:
            print(json.dumps({"arm": arm, "error": f"exit status {proc.returncode}"}), flush=True)
            return proc.returncode  # nothing more on the GPU after a failed arm
        line = [ln for ln in proc.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        results.append(json.loads(line))

    print("\n| arm | data -> first round (s) | ms / round | device peak (MB) | host peak RSS (MB) |")
    print("|---|---|---|---|---|")
    for r in results:
        print(f"| {r['arm']} | {r['data_to_first_round_s']} | {r['ms_per_round']} | "
              f"{r['device_peak_mb']} | {r['host_peak_rss_mb']} |")
    if len(results) == 2 and results[0]["nodes"] != results[1]["nodes"]:
        # cut finding runs on the host in one arm and on the device in the
        # other; with quantile cuts the last bit may differ (see
        # tests/test_gpu_sparse_training.py) — reported, not asserted
        print(f"\nnote: total nodes differ ({results[0]['nodes']} vs {results[1]['nodes']})")
    return 0


if __name__ == "__main__":
    sys.exit(main())
