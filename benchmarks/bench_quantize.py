#!/usr/bin/env python3
"""Dense quantization alone: time and peak device memory of ops.quantize.quantize
under SMXGB_QUANTIZE=hip (radix-select cuts + binning kernel,
ops/csrc/smxgb_quantize.hip) and =torch (torch.sort cuts + searchsorted bins,
the path every earlier build ran).

Cases: standard-normal matrices of the flagship (12.5M x 28), Covertype
(581k x 54) and wide (200k x 2000) shapes, and a 12.5M x 28 matrix of binary
columns, where every row of a column lands on one of two counters; max_bin
256 and 1024. Every (case, max_bin, arm) runs in a fresh child process, the
arms alternating, `--repeat` times over; a child warms up with one call and
times `--calls` more, each ended by a device synchronise.

Prints one JSON line per child and a markdown table. `peak` is
torch.cuda.max_memory_allocated over the timed calls; `bound` is what the
hip arm's design promises, X + bins + QUANTIZE_COUNTER_BYTES. The digests
(sums of cuts and bins) of the two arms of a case must agree.

`--child case,max_bin` runs one child in this process (for a kernel trace).
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
    "flagship": (12_500_000, 28, "normal"),
    "covertype": (581_012, 54, "normal"),
    "wide": (200_000, 2000, "normal"),
    "binary": (12_500_000, 28, "binary"),
}


def child(case, max_bin, calls):
    import torch

    from sagemaker_xgboost_container_amd.ops import hip
    from sagemaker_xgboost_container_amd.ops.quantize import quantize

    if not torch.cuda.is_available():
        sys.exit("bench_quantize.py measures the device: no GPU found")
    rows, cols, kind = CASES[case]
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)
    X = torch.randn((rows, cols), generator=g, device="cuda")
    if kind == "binary":
        X = (X > 0.3).to(torch.float32)
    qm = quantize(X, max_bin=max_bin)  # warm-up: code objects, allocator
    digest = [float(qm.cuts.double().sum()), int(qm.bins.long().sum()), int(qm.cut_ptr[-1])]
    bins_bytes = qm.bins.numel() * qm.bins.element_size()
    del qm
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    times = []
    for _ in range(calls):
        t0 = time.perf_counter()
        qm = quantize(X, max_bin=max_bin)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        del qm
    x_bytes = X.numel() * 4
    print(json.dumps({
        "case": case, "rows": rows, "cols": cols, "max_bin": max_bin, "arm": hip.quantize_mode(),
        "ms": [round(t * 1e3, 2) for t in times], "ms_min": round(min(times) * 1e3, 2),
        "peak_gb": round(torch.cuda.max_memory_allocated() / 1e9, 3),
        "x_gb": round(x_bytes / 1e9, 3), "bins_gb": round(bins_bytes / 1e9, 3),
        "bound_gb": round((x_bytes + bins_bytes + hip.QUANTIZE_COUNTER_BYTES) / 1e9, 3),
        "digest": digest,
    }), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--max-bins", default="256,1024")
    ap.add_argument("--calls", type=int, default=3, help="timed calls per child")
    ap.add_argument("--repeat", type=int, default=2, help="children per (case, max_bin, arm)")
    ap.add_argument("--child", default="", help="case,max_bin: run one child here")
    args = ap.parse_args()
    if args.child:
        case, max_bin = args.child.split(",")
        return child(case, int(max_bin), args.calls)

    rows = []
    for case in args.cases.split(","):
        for max_bin in args.max_bins.split(","):
            for _ in range(args.repeat):
                for arm in ("torch", "hip"):
                    out = subprocess.run(
                        [sys.executable, os.path.abspath(__file__), "--child", f"{case},{max_bin}",
                         "--calls", str(args.calls)],
                        env=dict(os.environ, SMXGB_QUANTIZE=arm), capture_output=True, text=True,
                    )
                    if out.returncode != 0:
                        sys.exit(f"{case} max_bin={max_bin} {arm} failed:\n{out.stderr[-2000:]}")
                    print(out.stdout.strip(), flush=True)
                    rows.append(json.loads(out.stdout.strip().splitlines()[-1]))

    print("\n| case | max_bin | arm | ms (min of all calls) | median | peak GB | X GB | bins GB | "
          "bound GB | same result |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    keys = sorted({(r["case"], r["max_bin"]) for r in rows}, key=lambda k: (list(CASES).index(k[0]), k[1]))
    for case, max_bin in keys:
        mine = [r for r in rows if (r["case"], r["max_bin"]) == (case, max_bin)]
        same = all(r["digest"] == mine[0]["digest"] for r in mine)
        for arm in ("torch", "hip"):
            rs = [r for r in mine if r["arm"] == arm]
            ms = [t for r in rs for t in r["ms"]]
            print(f"| {case} {rs[0]['rows']}x{rs[0]['cols']} | {max_bin} | {arm} | {min(ms):.1f} | "
                  f"{statistics.median(ms):.1f} | {max(r['peak_gb'] for r in rs):.3f} | "
                  f"{rs[0]['x_gb']:.3f} | {rs[0]['bins_gb']:.3f} | {rs[0]['bound_gb']:.3f} | {same} |")


if __name__ == "__main__":
    main()
