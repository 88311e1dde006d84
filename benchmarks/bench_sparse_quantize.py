#!/usr/bin/env python3
"""CSR quantization alone: scipy matrix in hand -> SparseQuantizedMatrix on the
device, two arms:

* ``torch`` - ops/sparse_ref.quantize_sparse on the host (CSC round trips, a
  Python loop over the features) followed by ``.to("cuda")``: the only path
  before ops/hip_sparse.quantize_csr existed
* ``hip``   - ops/hip_sparse.quantize_csr: upload, then the kernels of
  ops/csrc/smxgb_quantize_csr.hip

Cases: standard-normal values at uniformly random positions, 500k x 20k and
100k x 20k at 0.1 % density (features of about 500 and 100 entries: the LDS
sort) and 200k x 2000 at 5 % (10k entries a feature: the radix select).
Every (case, max_bin, arm) runs in a fresh child process, the arms
alternating, `--repeat` times over; a child warms up with one call and times
`--calls` more, each ended by a device synchronise.

Prints one JSON line per child and a markdown table. `peak` is
torch.cuda.max_memory_allocated over the timed calls; `bound` is what the hip
arm's design promises: the CSR arrays, 4 bytes an entry of keys, the bins, the
padded cuts and QUANTIZE_COUNTER_BYTES. The digests (sums of cuts and bins)
of the two arms of a case must agree.

`--child case,max_bin,arm` runs one child in this process (for a kernel trace).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = {
    "wide500k": (500_000, 20_000, 0.001),
    "wide100k": (100_000, 20_000, 0.001),
    "heavy": (200_000, 2_000, 0.05),
}
RUNS = (("wide500k", 256), ("wide500k", 1024), ("wide100k", 256), ("heavy", 256))


def make_csr(n, f, density, seed=1234):
    import numpy as np
    import scipy.sparse as sp

    rng = np.random.default_rng(seed)
    nnz = int(n * f * density)
    rows = rng.integers(0, n, nnz, dtype=np.int64)
    cols = rng.integers(0, f, nnz, dtype=np.int64)
    csr = sp.csr_matrix((np.ones(nnz, dtype=np.float32), (rows, cols)), shape=(n, f), dtype=np.float32)
    csr.sum_duplicates()
    csr.data = rng.normal(size=csr.nnz).astype(np.float32)
    return csr


def child(case, max_bin, arm, calls):
    import torch

    from sagemaker_xgboost_container_amd.ops import hip, hip_sparse
    from sagemaker_xgboost_container_amd.ops.sparse_ref import quantize_sparse

    if not torch.cuda.is_available():
        sys.exit("bench_sparse_quantize.py measures the device: no GPU found")
    n, f, density = CASES[case]
    csr = make_csr(n, f, density)
    if arm == "hip":
        run = lambda: hip_sparse.quantize_csr(csr, max_bin)  # noqa: E731
    else:
        run = lambda: quantize_sparse(csr, max_bin).to("cuda")  # noqa: E731
    qm = run()  # warm-up: code objects, allocator
    digest = [float(qm.cuts.double().sum()), int(qm.bin_data.long().sum()), int(qm.cut_ptr[-1])]
    bins_bytes = qm.bin_data.numel() * qm.bin_data.element_size()
    del qm
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    times = []
    for _ in range(calls):
        t0 = time.perf_counter()
        qm = run()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        del qm
    nnz = int(csr.nnz)
    csr_bytes = 8 * (n + 1) + 8 * nnz
    bound = csr_bytes + 4 * nnz + bins_bytes + 4 * f * max(max_bin - 1, 1) + hip.QUANTIZE_COUNTER_BYTES
    print(json.dumps({
        "case": case, "rows": n, "cols": f, "nnz": nnz, "max_bin": max_bin, "arm": arm,
        "ms": [round(t * 1e3, 2) for t in times], "ms_min": round(min(times) * 1e3, 2),
        "peak_mb": round(torch.cuda.max_memory_allocated() / 1e6, 1),
        "csr_mb": round(csr_bytes / 1e6, 1), "bound_mb": round(bound / 1e6, 1),
        "digest": digest,
    }), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", default=";".join(f"{c},{b}" for c, b in RUNS), help="case,max_bin;...")
    ap.add_argument("--calls", type=int, default=3, help="timed calls per child")
    ap.add_argument("--repeat", type=int, default=2, help="children per (case, max_bin, arm)")
    ap.add_argument("--child", default="", help="case,max_bin,arm: run one child here")
    args = ap.parse_args()
    if args.child:
        case, max_bin, arm = args.child.split(",")
        return child(case, int(max_bin), arm, args.calls)

    rows = []
    for run in args.runs.split(";"):
        for _ in range(args.repeat):
            for arm in ("torch", "hip"):
                out = subprocess.run(
                    [sys.executable, os.path.abspath(__file__), "--child", f"{run},{arm}",
                     "--calls", str(args.calls)],
                    capture_output=True, text=True,
                )
                if out.returncode != 0:
                    sys.exit(f"{run} {arm} failed:\n{out.stderr[-2000:]}")
                print(out.stdout.strip(), flush=True)
                rows.append(json.loads(out.stdout.strip().splitlines()[-1]))

    print("\n| case | nnz | max_bin | arm | ms (min of all calls) | median | peak MB | CSR MB | "
          "bound MB | same result |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    keys = list(dict.fromkeys((r["case"], r["max_bin"]) for r in rows))
    for case, max_bin in keys:
        mine = [r for r in rows if (r["case"], r["max_bin"]) == (case, max_bin)]
        same = all(r["digest"] == mine[0]["digest"] for r in mine)
        for arm in ("torch", "hip"):
            rs = [r for r in mine if r["arm"] == arm]
            ms = [t for r in rs for t in r["ms"]]
            print(f"| {case} {rs[0]['rows']}x{rs[0]['cols']} | {rs[0]['nnz']} | {max_bin} | {arm} | "
                  f"{min(ms):.1f} | {statistics.median(ms):.1f} | {max(r['peak_mb'] for r in rs):.1f} | "
                  f"{rs[0]['csr_mb']:.1f} | {rs[0]['bound_mb']:.1f} | {same} |")


if __name__ == "__main__":
    main()
