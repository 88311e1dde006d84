#!/usr/bin/env python3
"""Row-sampling benchmark: full data, uniform and gradient-based sampling.

binary:logistic, depth 6, Higgs-shape synthetic data (the bench.py recipe) at
the flagship size. Arms, all in one process: full data; subsample 0.5 / 0.2 /
0.1 with sampling_method=uniform; the same rates with
sampling_method=gradient_based. Each arm reports steady-state rounds/sec and
the logloss on a held-out set after warmup + steps rounds.

It then times the sampler alone on a logistic gradient tensor of the same
size (device events): the HIP radix-select threshold, the whole
gradient_sample call, and a torch.sort-based threshold
(torch_ref.mvs_threshold on the device) for comparison.

`--arms gradient_based:0.1 --no-sampler-timing` keeps a kernel-trace run
(rocprofv3 --kernel-trace --stats) short: the mvs_* kernels are the sampler.
Prints one JSON line per measurement and a markdown table.
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
from sagemaker_xgboost_container_amd.ops import backend_for, torch_ref  # noqa: E402

FEATURES = 28
MAX_DEPTH = 6
RATES = (0.5, 0.2, 0.1)
ARMS = (
    [("full", 1.0)]
    + [("uniform", r) for r in RATES]
    + [("gradient_based", r) for r in RATES]
)


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
    logit = X[:, 0] * 2.0 - X[:, 1] + 0.5 * X[:, 2] * X[:, 3] + 0.25 * X[:, 4]
    noise = torch.randn(rows, generator=g, device=device) * 0.5
    return X, (logit + noise > 0).to(torch.float32)


def logloss(prob, y):
    prob = prob.double().clamp(1e-15, 1.0 - 1e-15)
    y = y.double()
    return float(-(y * prob.log() + (1.0 - y) * (1.0 - prob).log()).mean())


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


def sampler_timing(rows, device, sync, repeats=20):
    """The sampler alone, on logistic gradients of a model that has learnt
    something (margins ~ N(0, 2^2)), at subsample 0.1 and 0.5."""
    backend = backend_for(device)
    g = torch.Generator(device=device)
    g.manual_seed(99)
    margin = torch.randn(rows, generator=g, device=device) * 2.0
    y = (torch.rand(rows, generator=g, device=device) < torch.sigmoid(margin)).float()
    prob = torch.sigmoid(margin)
    gh = torch.stack([prob - y, prob * (1.0 - prob)], dim=1).contiguous()
    u = torch.rand(rows, generator=g, device=device)
    out = []
    for rate in (0.1, 0.5):
        S = rate * rows
        radix = time_ms(lambda: backend.mvs_threshold(gh, S), sync, repeats)
        whole = time_ms(lambda: backend.gradient_sample(gh, rate, u), sync, repeats)
        sort = time_ms(lambda: torch_ref.mvs_threshold(gh, S), sync, max(2, repeats // 4))
        mu_radix = float(backend.mvs_threshold(gh, S))
        mu_sort = float(torch_ref.mvs_threshold(gh, S))
        out.append({
            "metric": f"sampler time ({rows} rows, subsample {rate})", "unit": "ms",
            "backend": backend.NAME, "threshold_radix_select": radix,
            "gradient_sample_whole_call": whole, "threshold_torch_sort": sort,
            "mu_radix_select": mu_radix, "mu_torch_sort": mu_sort,
        })
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=12_500_000)
    ap.add_argument("--holdout-rows", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=40, help="timed rounds per arm")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--arms", nargs="+", default=None,
                    help="subset of arms as method:rate, e.g. full:1.0 gradient_based:0.1")
    ap.add_argument("--no-sampler-timing", action="store_true")
    args = ap.parse_args()

    use_gpu = torch.cuda.is_available()
    device = torch.device("cuda" if use_gpu else "cpu")
    rows = args.rows if use_gpu else min(args.rows, 50_000)
    holdout_rows = args.holdout_rows if use_gpu else min(args.holdout_rows, 10_000)

    def sync():
        if use_gpu:
            torch.cuda.synchronize()

    arms = ARMS
    if args.arms:
        arms = [(a.split(":")[0], float(a.split(":")[1])) for a in args.arms]

    X, y = synth(rows, device, seed=1234)
    Xh, yh = synth(holdout_rows, device, seed=4321)
    dtrain = DeviceDMatrix(X, label=y) if use_gpu else DMatrix(X.numpy(), label=y.numpy())
    Xh_host = Xh.cpu().numpy()  # Booster.predict takes host arrays

    table = []
    for method, rate in arms:
        params = {"objective": "binary:logistic", "max_depth": MAX_DEPTH, "eta": 0.3,
                  "tree_method": "gpu_hist" if use_gpu else "hist", "device": str(device)}
        if method != "full":
            params.update(subsample=rate, sampling_method=method)
        timer = Timer(args.warmup, args.steps, sync)
        bst = trainer.train(params, dtrain, num_boost_round=args.warmup + args.steps,
                            callbacks=[timer], verbose_eval=False)
        rps = args.steps / (timer.t1 - timer.t0)
        loss = logloss(torch.as_tensor(bst.predict(Xh_host)).to(yh.device), yh)
        row = {
            "metric": f"boost rounds/sec ({rows}x{FEATURES} binary:logistic depth {MAX_DEPTH})",
            "sampling_method": method, "subsample": rate, "value": rps, "unit": "rounds/sec",
            "holdout_logloss": loss, "rounds": bst.num_boosted_rounds(),
            "holdout_rows": holdout_rows, "steps": args.steps, "warmup": args.warmup,
        }
        print(json.dumps(row), flush=True)
        table.append(row)
    del dtrain, X, y

    if not args.no_sampler_timing:
        for row in sampler_timing(rows, device, sync):
            print(json.dumps(row), flush=True)

    full = next((r["value"] for r in table if r["sampling_method"] == "full"), None)
    print("\n| sampling | subsample | rounds/s | vs full data | held-out logloss |")
    print("|---|---|---|---|---|")
    for r in table:
        rel = f"{r['value'] / full:.2f}x" if full else "-"
        print(f"| {r['sampling_method']} | {r['subsample']} | {r['value']:.1f} | {rel} | "
              f"{r['holdout_logloss']:.5f} |")


if __name__ == "__main__":
    main()
