"""HIP binary auc (csrc/smxgb_auc.hip) against the float64 reference
torch_ref.binary_auc: equality where the reference's sums are exact."""
import math

import numpy as np
import pytest
import torch

from sagemaker_xgboost_container_amd.data.dmatrix import DMatrix
from sagemaker_xgboost_container_amd.models import eval_metrics, trainer
from sagemaker_xgboost_container_amd.ops import torch_ref

pytestmark = pytest.mark.gpu

CHUNK = 2048  # asserted against the extension's constant in _hip_auc()
SIZES = [2, CHUNK - 1, CHUNK + 1, 3 * CHUNK + 7]
SCORES = ["mixed", "equal", "separated", "reversed"]


def _data(n, scores, weights, seed=0):
    """Scores, labels, weights in a shuffled row order. "mixed": normal
    scores on a few hundred levels, then by sorted position a tie run across
    every chunk boundary, one over more than a whole chunk, -inf, +inf, two
    scores one bit apart, and -0.0 among the +0.0."""
    rng = np.random.default_rng(seed + n)
    y = (rng.random(n) < 0.4).astype(np.float32)
    y[:2] = [1.0, 0.0]
    if scores == "mixed":
        s = np.sort(np.round(rng.normal(size=n) * 50).astype(np.float32) / 50)
        for b in range(CHUNK, n, CHUNK):
            s[b - 20:b + 20] = s[b - 20]
        if n > 3 * CHUNK:
            s[2 * CHUNK - 96:3 * CHUNK + 6] = s[2 * CHUNK - 96]
        if n > 200:
            s[:2], s[-1] = -np.inf, np.inf
            s[100] = np.nextafter(s[101], np.float32(-np.inf))
            s[np.flatnonzero(s == 0.0)[::2]] = -0.0
        s = s[rng.permutation(n)]
    else:
        s = {"equal": np.full(n, 0.25), "separated": y, "reversed": 1.0 - y}[scores].astype(np.float32)
    w = None
    if weights == "eighths":  # 0, 1/8, ..., 4: every sum of the reference is exact
        w = (rng.integers(0, 33, size=n) / 8).astype(np.float32)
        w[:2] = 1.0
    elif weights == "uniform":
        w = rng.uniform(0.5, 2.0, size=n).astype(np.float32)
    return s, y, w


def _hip_auc(s, y, w):
    from sagemaker_xgboost_container_amd.ops import hip

    assert hip.AUC_CHUNK == CHUNK
    dev = lambda a: None if a is None else torch.as_tensor(a, device="cuda")  # noqa: E731
    plan = hip.auc_plan(dev(y), dev(w))
    return hip.binary_auc(plan, dev(s)), plan


@pytest.mark.parametrize("weights", [None, "eighths"])
@pytest.mark.parametrize("scores", SCORES)
@pytest.mark.parametrize("n", SIZES)
def test_hip_equals_float64_reference(n, scores, weights):
    s, y, w = _data(n, scores, weights)
    want = torch_ref.binary_auc(s, y, w)
    got, _ = _hip_auc(s, y, w)
    print(f"auc n={n} {scores} {weights}: hip {got!r} ref {want!r}")
    assert got == want
    if weights is None and scores in ("separated", "reversed"):
        assert got == (1.0 if scores == "separated" else 0.0)


@pytest.mark.parametrize("weights", [None, "uniform"])
def test_bits_do_not_depend_on_row_order(weights):
    s, y, w = _data(SIZES[-1], "mixed", weights)
    perm = np.random.default_rng(5).permutation(s.size)
    a, _ = _hip_auc(s, y, w)
    b, _ = _hip_auc(s[perm], y[perm], None if w is None else w[perm])
    assert a == b and 0.0 < a < 1.0


@pytest.mark.parametrize("n", SIZES[1:])
def test_float32_weights_stay_within_the_stated_bound(n):
    from sagemaker_xgboost_container_amd.ops import hip

    s, y, w = _data(n, "mixed", "uniform")
    got, plan = _hip_auc(s, y, w)
    want = torch_ref.binary_auc(s, y, w)
    n_pos = int(y.sum())
    unit = math.ldexp(1.0, -plan["s"])
    assert 1.0 / unit == hip.leaf_quantile_weight_scale(n, float(w.max()))
    bound = unit / 2 * (n_pos / (plan["P"] * unit) + (n - n_pos) / (plan["N"] * unit)) + 2.0 ** -50
    print(f"auc n={n} float32 weights: |hip - ref| {abs(got - want):.3e} bound {bound:.3e}")
    assert abs(got - want) <= bound < 1e-9


@pytest.mark.parametrize("weighted", [False, True])
def test_training_reports_the_rule(weighted):
    rng = np.random.default_rng(11)
    sets = {}
    for name, n in (("train", 3000), ("valid", CHUNK + 500)):
        X = rng.normal(size=(n, 5)).astype(np.float32)
        y = (X[:, 0] - X[:, 1] + rng.normal(size=n) > 0).astype(np.float32)
        w = (rng.integers(0, 33, size=n) / 8).astype(np.float32) if weighted else None
        sets[name] = (DMatrix(X, label=y, weight=w), y, w)
    res = {}
    bst = trainer.train(
        {"objective": "binary:logistic", "max_depth": 3, "eta": 0.5, "eval_metric": "auc",
         "seed": 3, "device": "cuda"},
        sets["train"][0], num_boost_round=3, evals=[(sets[k][0], k) for k in sets],
        evals_result=res, verbose_eval=False,
    )
    for name, (dm, y, w) in sets.items():
        for rnd in range(3):
            margin = bst.predict(dm, output_margin=True, iteration_range=(0, rnd + 1))
            assert res[name]["auc"][rnd] == torch_ref.binary_auc(margin, y, w), (name, rnd)


def test_one_plan_serves_every_round_and_one_class_raises():
    s, y, w = _data(SIZES[2], "mixed", "eighths")
    s, y, w = (torch.as_tensor(a, device="cuda") for a in (s, y, w))
    plans = {}
    first = eval_metrics.evaluate("auc", s, y, w, None, rank_plans=plans)
    plan = plans["auc"]
    assert eval_metrics.evaluate("auc", s, y, w, None, rank_plans=plans) == first
    assert plans["auc"] is plan
    with pytest.raises(ValueError, match="the dataset only contains pos or neg samples"):
        eval_metrics.evaluate("auc", s, torch.ones_like(y), w, None)


def test_nan_margin_gives_nan():
    s, y, w = _data(SIZES[2], "mixed", None)
    s[CHUNK // 2] = np.nan
    assert math.isnan(_hip_auc(s, y, w)[0])
