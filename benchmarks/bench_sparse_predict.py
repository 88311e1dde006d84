#!/usr/bin/env python3
"""Predict on wide sparse (CSR) data on the GPU: CSR route vs densifying.

A random forest of fixed depth built from Tree objects (no training) over
synthetic n x f CSR data. Two arms on the same model and data, each in a
fresh child process so that peak host RSS and peak device memory belong to
that arm alone, all in one invocation:

* ``csr``   — SMXGB_SPARSE_PREDICT=1: the CSR arrays are uploaded as they are,
  predict_forest_csr_kernel walks them (ops/hip_sparse.py)
* ``dense`` — SMXGB_SPARSE_PREDICT=0: to_dense() on the host, n x f float32
  to HBM, dense predict_kernel (the only behaviour before the CSR route)

Per arm and shape: end-to-end ``Booster.predict(DMatrix)`` wall time and the
traversal alone (data already on the device), each the median of repeated
runs after a warm-up; torch.cuda.max_memory_allocated(); peak host RSS; a
digest of the margins, which the two arms must share. A dense arm whose
image exceeds --dense-max-gb, the free host memory or the free device memory
is reported as not run rather than tried.

``--sweep`` times the CSR traversal alone over LDS tile sizes and items per
block (hip_sparse.PREDICT_CSR_TILE / PREDICT_CSR_BLOCK_ITEMS).

Prints one JSON line per (shape, arm) and a markdown table.
"""
import argparse
import hashlib
import json
import os
import resource
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SWEEP_TILES = (0, 1024, 4096, 8192)
SWEEP_ITEMS = (64, 256, 1024)


def make_data(n, f, density, seed=0):
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
    csr.data = rng.integers(1, 65, csr.nnz).astype(np.float32)  # count-like libsvm values
    return csr


def make_booster(f, trees, depth, seed=1):
    """`trees` full trees of `depth` levels splitting on uniformly drawn
    columns, thresholds inside the value range, random default directions."""
    import numpy as np

    from sagemaker_xgboost_container_amd.models.booster import Booster
    from sagemaker_xgboost_container_amd.models.tree import Tree

    rng = np.random.default_rng(seed)
    bst = Booster({"objective": "binary:logistic"}, num_features=f)
    for _ in range(trees):
        tree = Tree()
        frontier = [tree.add_node(value=0.0)]
        for _level in range(depth):
            nxt = []
            for nid in frontier:
                nxt += tree.apply_split(
                    nid, int(rng.integers(0, f)), float(rng.integers(1, 65)) + 0.5, 0,
                    bool(rng.integers(0, 2)), 1.0,
                    left_value=float(rng.normal() * 0.1), right_value=float(rng.normal() * 0.1),
                    left_hess=1.0, right_hess=1.0,
                )
            frontier = nxt
        bst.add_iteration([tree.finalize()], [0])
    return bst


def _median_ms(fn, repeats, sync):
    fn()  # warm-up
    sync()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        sync()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def _mem_available_bytes():
    try:
        with open("/proc/meminfo") as fh:
            for line in fh:
                if line.startswith("MemAvailable:"):
                    return int(line.split()[1]) * 1024
    except OSError:
        pass
    return None


def run_arm(args):
    os.environ["SMXGB_SPARSE_PREDICT"] = "1" if args.arm == "csr" else "0"
    import numpy as np
    import torch

    from sagemaker_xgboost_container_amd.data.dmatrix import DMatrix
    from sagemaker_xgboost_container_amd.ops import hip, hip_sparse

    n, f = args.rows, args.cols
    base = {"arm": args.arm, "rows": n, "cols": f, "trees": args.trees, "depth": args.depth}
    image = n * f * 4
    torch.cuda.init()
    if args.arm == "dense":
        free_dev, _total = torch.cuda.mem_get_info()
        host = _mem_available_bytes()
        why = None
        if image > args.dense_max_gb * 2**30:
            why = f"dense image {image / 2**30:.1f} GiB above --dense-max-gb"
        elif image > 0.8 * free_dev:
            why = f"dense image {image / 2**30:.1f} GiB does not fit the free device memory"
        elif host is not None and 2 * image > 0.8 * host:
            why = f"dense image {image / 2**30:.1f} GiB (x2 while uploading) does not fit the host"
        if why:
            print(json.dumps(dict(base, ran=False, why=why)), flush=True)
            return

    csr = make_data(n, f, args.density)
    bst = make_booster(f, args.trees, args.depth)
    dmat = DMatrix(csr)
    dev = torch.device("cuda")
    flat = bst._device_flat_forest(dev, with_paths=False)
    sync = torch.cuda.synchronize
    repeats = args.repeats if image < (1 << 30) or args.arm == "csr" else max(2, args.repeats // 3)

    torch.cuda.reset_peak_memory_stats()
    holder = {}

    def e2e():
        holder["margin"] = bst.predict(dmat, output_margin=True)

    e2e_ms = _median_ms(e2e, repeats, sync)
    peak = torch.cuda.max_memory_allocated()
    rss = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0

    if args.arm == "csr":
        dcsr = hip_sparse.DeviceCSR(csr, dev)
        kernel_ms = _median_ms(lambda: hip_sparse.predict_forest_csr(flat, dcsr, 1), args.repeats, sync)
    else:
        X = torch.as_tensor(dmat.to_dense(), dtype=torch.float32, device=dev)
        kernel_ms = _median_ms(lambda: hip.predict_forest_flat(flat, X, 1), args.repeats, sync)
    margin = np.ascontiguousarray(holder["margin"])
    print(json.dumps(dict(
        base, ran=True, nnz=int(csr.nnz), repeats=repeats,
        e2e_ms=round(e2e_ms, 3), kernel_ms=round(kernel_ms, 3),
        device_peak_mb=round(peak / 2**20, 1), host_peak_rss_mb=round(rss, 1),
        digest=hashlib.sha1(margin.tobytes()).hexdigest()[:16],
    )), flush=True)


def run_sweep(args):
    import torch

    from sagemaker_xgboost_container_amd.ops import hip, hip_sparse

    csr = make_data(args.rows, args.cols, args.density)
    bst = make_booster(args.cols, args.trees, args.depth)
    dev = torch.device("cuda")
    flat = bst._device_flat_forest(dev, with_paths=False)
    dcsr = hip_sparse.DeviceCSR(csr, dev)
    n_chunks, _ = hip._predict_chunking(args.rows, args.trees)
    want = None
    for tile in SWEEP_TILES:
        for items in SWEEP_ITEMS:
            hip_sparse.PREDICT_CSR_TILE = tile
            hip_sparse.PREDICT_CSR_BLOCK_ITEMS = items
            ms = _median_ms(
                lambda: hip_sparse.predict_forest_csr(flat, dcsr, 1), args.repeats,
                torch.cuda.synchronize,
            )
            out = hip_sparse.predict_forest_csr(flat, dcsr, 1)
            want = out if want is None else want
            print(json.dumps({
                "sweep": True, "rows": args.rows, "cols": args.cols, "n_chunks": n_chunks,
                "tile": tile, "block_items": items,
                "rows_per_block": hip_sparse._rows_per_group(n_chunks),
                "kernel_ms": round(ms, 3), "same_bits": bool(torch.equal(out, want)),
            }), flush=True)


def _child(args, rows, extra):
    cmd = [sys.executable, os.path.abspath(__file__), "--rows", str(rows)] + extra
    for name in ("cols", "density", "trees", "depth", "repeats", "dense_max_gb"):
        cmd += ["--" + name.replace("_", "-"), str(getattr(args, name))]
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("{")]
    return proc.returncode, [json.loads(ln) for ln in lines]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default="1000,200000,1000000",
                    help="comma-separated row counts (all at --cols columns)")
    ap.add_argument("--rows", type=int, help=argparse.SUPPRESS)
    ap.add_argument("--cols", type=int, default=20_000)
    ap.add_argument("--density", type=float, default=0.001)
    ap.add_argument("--trees", type=int, default=500)
    ap.add_argument("--depth", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--dense-max-gb", type=float, default=64.0)
    ap.add_argument("--arms", default="csr,dense")
    ap.add_argument("--sweep", action="store_true", help="time tile / block-item choices instead")
    ap.add_argument("--arm", choices=("csr", "dense", "sweep"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.arm == "sweep":
        run_sweep(args)
        return 0
    if args.arm:
        run_arm(args)
        return 0

    results = []
    for rows in [int(s) for s in args.shapes.split(",")]:
        for arm in (["sweep"] if args.sweep else args.arms.split(",")):
            code, recs = _child(args, rows, ["--arm", arm])
            for rec in recs:
                print(json.dumps(rec), flush=True)
            if code != 0:
                print(json.dumps({"arm": arm, "rows": rows, "error": f"exit status {code}"}), flush=True)
                return code  # nothing more on the GPU after a failed arm
            results += recs

    if args.sweep:
        print("\n| rows | chunks | tile (entries) | items / block | rows / block | kernel ms | same bits |")
        print("|---|---|---|---|---|---|---|")
        for r in results:
            print(f"| {r['rows']} | {r['n_chunks']} | {r['tile']} | {r['block_items']} | "
                  f"{r['rows_per_block']} | {r['kernel_ms']} | {r['same_bits']} |")
        return 0
    print("\n| rows x cols | arm | predict ms (end to end) | traversal ms | device peak (MB) | host peak RSS (MB) |")
    print("|---|---|---|---|---|---|")
    for r in results:
        shape = f"{r['rows']} x {r['cols']}"
        if not r["ran"]:
            print(f"| {shape} | {r['arm']} | not run: {r['why']} | | | |")
            continue
        print(f"| {shape} | {r['arm']} | {r['e2e_ms']} | {r['kernel_ms']} | "
              f"{r['device_peak_mb']} | {r['host_peak_rss_mb']} |")
    by_shape = {}
    for r in results:
        if r["ran"]:
            by_shape.setdefault(r["rows"], set()).add(r["digest"])
    for rows, digests in by_shape.items():
        if len(digests) > 1:
            print(f"\nERROR: the arms disagree at {rows} rows")
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
