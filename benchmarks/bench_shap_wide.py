#!/usr/bin/env python3
"""A/B exact pred_contribs beyond the dense-slab TreeSHAP kernel's LDS limit:
the compact kernel (chunk-local phi slots, dense or CSR rows) vs what served
these shapes before it, the host recursion.

Arms, each timed in a FRESH child process of this one invocation:
  host     SMXGB_SHAP_COMPACT=0 / SMXGB_SPARSE_EXPLAIN=0: the dense slab does
           not fit, so the request runs Lundberg's recursion on the host (and
           a sparse DMatrix is densified first)
  compact  SMXGB_SHAP_COMPACT=1 / SMXGB_SPARSE_EXPLAIN=1: the new route

Shapes:
  a  dense, 54 columns, 7 classes, 100 rounds of depth 6 (the Covertype
     configuration; synthetic data of that shape), 1k and 100k rows
  b  dense, 500 columns, one output, 100 rounds of depth 6, 1k and 100k rows
  c  CSR, 20000 columns at 0.1 %, 500 hand-built trees of depth 6 with
     consistent covers (no training: the forest's shape is what matters to
     TreeSHAP), 1k and 20k rows

Every timing is end to end, host input to host result: one warm-up call,
then the median of --repeats calls, with the device peak memory
(torch.cuda.max_memory_allocated) and the host peak RSS of the child. The
host arm is linear in rows; it is timed on at most --host-rows-cap rows and
scaled, marked "host_extrapolated": true. The capped host run of the larger
row count repeats the 1k-row measurement in another process, which gives
the spread between two invocations of the same arm.

Prints one JSON line per (shape, rows, arm) and one ratio line per pair.
"""
import argparse
import json
import os
import resource
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = {
    "a": {"f": 54, "k": 7, "rows": (1_000, 100_000), "sparse": False},
    "b": {"f": 500, "k": 1, "rows": (1_000, 100_000), "sparse": False},
    "c": {"f": 20_000, "k": 1, "rows": (1_000, 20_000), "sparse": True},
}
ARM_ENV = {
    "host": {"SMXGB_SHAP_COMPACT": "0", "SMXGB_SPARSE_EXPLAIN": "0"},
    "compact": {"SMXGB_SHAP_COMPACT": "1", "SMXGB_SPARSE_EXPLAIN": "1"},
}


def _dense_data(rng, n, f, k):
    X = rng.normal(size=(n, f)).astype(np.float32)
    X[:, 10:] = (X[:, 10:] > 0.8).astype(np.float32)  # mostly indicator columns
    w = rng.normal(size=(f, max(k, 2))).astype(np.float32)
    score = X @ w + (X[:, :1] * X[:, 1:2])
    y = score.argmax(1) if k > 1 else (score[:, 0] > score[:, 1])
    return X, y.astype(np.float32)


def _sparse_rows(rng, n, f, density=0.001):
    import scipy.sparse as sp

    nnz = int(n * f * density)
    m = sp.coo_matrix(
        (rng.normal(size=nnz).astype(np.float32), (rng.integers(0, n, nnz), rng.integers(0, f, nnz))),
        shape=(n, f),
    ).tocsr()
    m.sum_duplicates()
    return m


def _hand_tree(rng, pool, depth):
    from sagemaker_xgboost_container_amd.models.tree import Tree

    tree = Tree()
    frontier = [(tree.add_node(value=0.0, sum_hess=4096.0), 4096.0)]
    for _ in range(depth):
        nxt = []
        for nid, h in frontier:
            hl = h * float(rng.choice([0.25, 0.5, 0.75]))
            lid, rid = tree.apply_split(
                nid, int(pool[rng.integers(0, len(pool))]), float(rng.normal()), 0,
                bool(rng.integers(0, 2)), 1.0,
                left_value=float(rng.normal() * 0.1), right_value=float(rng.normal() * 0.1),
                left_hess=hl, right_hess=h - hl,
            )
            nxt += [(lid, hl), (rid, h - hl)]
        frontier = nxt
    return tree.finalize()


def child_train(args):
    """Build the model of a shape and save it (a child: the parent never
    opens the GPU)."""
    import torch

    from sagemaker_xgboost_container_amd.data.dmatrix import DMatrix
    from sagemaker_xgboost_container_amd.models import trainer
    from sagemaker_xgboost_container_amd.models.booster import Booster

    shape = SHAPES[args.shape]
    f, k = shape["f"], shape["k"]
    rng = np.random.default_rng(0)
    if shape["sparse"]:
        pool = np.unique(rng.integers(0, f, size=5000))
        bst = Booster({"objective": "binary:logistic"}, num_features=f)
        for _ in range(args.sparse_trees):
            bst.add_iteration([_hand_tree(rng, pool, args.depth)], [0])
    else:
        X, y = _dense_data(rng, args.train_rows, f, k)
        params = {"max_depth": args.depth, "eta": 0.1,
                  "device": "cuda" if torch.cuda.is_available() else "cpu"}
        if k > 1:
            params.update(objective="multi:softprob", num_class=k)
        else:
            params.update(objective="binary:logistic")
        bst = trainer.train(params, DMatrix(X, label=y), num_boost_round=args.rounds,
                            verbose_eval=False)
    bst.save_model(args.model)
    print(json.dumps({"shape": args.shape, "trees": len(bst.trees),
                      "leaves": int(sum(t.num_leaves for t in bst.trees))}), flush=True)


def child_time(args):
    import torch

    from sagemaker_xgboost_container_amd.data.dmatrix import DMatrix
    from sagemaker_xgboost_container_amd.models.booster import Booster

    shape = SHAPES[args.shape]
    f = shape["f"]
    bst = Booster()
    bst.load_model(args.model)
    rng = np.random.default_rng(1)
    n = args.timed_rows
    if shape["sparse"]:
        data = DMatrix(_sparse_rows(rng, n, f))
    else:
        data = DMatrix(_dense_data(rng, n, f, shape["k"])[0])
    have_gpu = torch.cuda.is_available()

    def call():
        out = bst.predict(data, pred_contribs=True)
        if have_gpu:
            torch.cuda.synchronize()
        return out

    out = call()  # warm-up: tables, plans, allocator
    assert out.shape[0] == n and out.shape[-1] == f + 1
    lat = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        call()
        lat.append((time.perf_counter() - t0) * 1000)
    scale = args.rows / n
    line = {
        "shape": args.shape, "rows": args.rows, "arm": args.arm, "trees": len(bst.trees),
        "p50_ms": float(np.median(lat)) * scale, "min_ms": float(min(lat)) * scale,
        "max_ms": float(max(lat)) * scale, "timed_rows": n, "host_extrapolated": n != args.rows,
        "device_peak_mb": torch.cuda.max_memory_allocated() / 2 ** 20 if have_gpu else 0.0,
        "host_peak_rss_mb": resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024,
    }
    if have_gpu and args.arm == "compact":
        from sagemaker_xgboost_container_amd.ops import hip

        flat = bst._device_flat_forest(torch.device("cuda"), with_paths=True)
        plan = hip.shap_compact_plan(flat["shap_paths"], f, 0, len(bst.trees), n)
        line["trees_per_chunk"], line["block"] = plan if plan else (None, None)
        # the tables the timed calls built (cached per device name)
        for name, cache in bst._predict_cache.items():
            if not str(name).startswith("shap_slots:"):
                continue
            for key, tabs in cache.items():
                if key[0] == "slots":
                    line.update(slots=tabs["S"], columns=int(tabs["cols"].shape[0]),
                                max_slots=tabs["max_slots"], chunks=tabs["n_chunks"])
    print(json.dumps(line), flush=True)


def _run_child(extra, env=None, timeout=None):
    cmd = [sys.executable, os.path.abspath(__file__)] + extra
    res = subprocess.run(cmd, env=dict(os.environ, **(env or {})), stdout=subprocess.PIPE,
                         timeout=timeout, check=True, text=True)
    lines = [json.loads(s) for s in res.stdout.splitlines() if s.startswith("{")]
    for line in lines:
        print(json.dumps(line), flush=True)
    return lines[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b,c")
    ap.add_argument("--depth", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--sparse-trees", type=int, default=500)
    ap.add_argument("--train-rows", type=int, default=50_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-rows-cap", type=int, default=1_000,
                    help="time the host arm on at most this many rows and scale (0: all rows)")
    ap.add_argument("--child-timeout", type=float, default=600.0)
    # child-process arguments
    ap.add_argument("--child", choices=("train", "time"))
    ap.add_argument("--shape")
    ap.add_argument("--model")
    ap.add_argument("--arm")
    ap.add_argument("--rows", type=int)
    ap.add_argument("--timed-rows", type=int)
    args = ap.parse_args()
    if args.repeats < 3:
        ap.error("--repeats must be at least 3")
    if args.child == "train":
        return child_train(args)
    if args.child == "time":
        return child_time(args)

    common = ["--depth", str(args.depth), "--rounds", str(args.rounds),
              "--sparse-trees", str(args.sparse_trees), "--train-rows", str(args.train_rows),
              "--repeats", str(args.repeats)]
    with tempfile.TemporaryDirectory() as tmp:
        for name in [s for s in args.shapes.split(",") if s]:
            model = os.path.join(tmp, f"model_{name}.json")
            _run_child(common + ["--child", "train", "--shape", name, "--model", model],
                       timeout=args.child_timeout)
            for rows in SHAPES[name]["rows"]:
                p50 = {}
                for arm in ("host", "compact"):
                    timed = rows
                    if arm == "host" and args.host_rows_cap and rows > args.host_rows_cap:
                        timed = args.host_rows_cap
                    line = _run_child(
                        common + ["--child", "time", "--shape", name, "--model", model,
                                  "--arm", arm, "--rows", str(rows), "--timed-rows", str(timed)],
                        env=ARM_ENV[arm], timeout=args.child_timeout,
                    )
                    p50[arm] = line["p50_ms"]
                print(json.dumps({"shape": name, "rows": rows,
                                  "host_over_compact": p50["host"] / p50["compact"]}), flush=True)


if __name__ == "__main__":
    main()
