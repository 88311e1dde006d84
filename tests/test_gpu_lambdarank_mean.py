"""HIP sampled (mean) LambdaRank gradients (lambdarank_mean_tile_kernel of
csrc/smxgb_rank.hip) against the float64 reference
torch_ref.lambdarank_gradients(pair_method="mean"), their pair set, their
determinism, and the path from trainer.train."""
import functools
import logging

import numpy as np
import pytest
import torch

from sagemaker_xgboost_container_amd.data.dmatrix import DMatrix
from sagemaker_xgboost_container_amd.models import trainer
from sagemaker_xgboost_container_amd.ops import torch_ref

pytestmark = pytest.mark.gpu

KINDS = ["rank:pairwise", "rank:ndcg", "rank:map"]
MARGINS = ["zero", "eighths", "continuous"]
CAP = 4096  # asserted against the extension's constant in _run_hip
SMALL = [1, 2, 63, 64, 65, 257, 1, 20]
LAYOUTS = {  # (group sizes, P, flags); flags 7: both normalisations and exponential gain
    "small_p1": (SMALL, 1, 7),
    "small_p3": (SMALL, 3, 7),
    "small_p3_plain": (SMALL, 3, 0),
    # groups that end at, and one that fills, a tile
    "tiles": ([2000, CAP - 2000, 1500, CAP - 1500, CAP], 1, 7),
    # 40 draws per document: the plan has to lower tile_docs to 16384 // 40 = 409
    "lowered": ([257, 100, 60, 200, 20, 300, 409], 40, 7),
}

# |g - g_ref| <= TOL * mass and |h - h_ref| <= TOL * h_ref, as for the top-k
# kernels, whose per-pair arithmetic this path shares. Largest ratio observed
# over this matrix on an MI355X: MEASURED_RATIO (rank:map, tiles, continuous
# margins). With the float32 rank:map quotients of the top-k kernels it was
# 1.4e-4 on that layout, which is why this kernel forms them in float64.
MEASURED_RATIO = 6.98e-7
TOL = 2.0 ** -16
assert 4 * MEASURED_RATIO <= TOL


def _inputs(sizes, margins, weighted, kind, seed=11):
    rng = np.random.default_rng(seed)
    n = int(np.sum(sizes))
    s = {
        "zero": np.zeros(n),
        "eighths": np.round(rng.normal(size=n) * 8) / 8,
        "continuous": rng.normal(size=n) * 2,
    }[margins].astype(np.float32)
    y = rng.integers(0, 5, size=n).astype(np.float32)
    if kind == "rank:map":  # three relevant in five: min(y, 1) would keep one draw in three
        y = (y >= 2).astype(np.float32)
    w = rng.uniform(0.25, 4.0, size=n).astype(np.float32) if weighted else None
    return s, y, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), w


def _run_hip(kind, s, y, ptr, w, P, flags, tile_docs=None, seed=5, rnd=2):
    from sagemaker_xgboost_container_amd.ops import hip

    assert hip.LAMBDARANK_CAP == CAP
    plan = hip.lambdarank_plan(ptr, P, "cuda", tile_docs=tile_docs, pair_method="mean")
    dev = lambda a: None if a is None else torch.from_numpy(a).cuda()  # noqa: E731
    gh = hip.lambdarank_mean_gradients(
        plan, dev(s), dev(y), dev(w), torch_ref.LAMBDARANK_KINDS[kind], flags, seed, rnd)
    return gh, plan


@functools.lru_cache(maxsize=None)
def _reference(kind, sizes, margins, weighted, P, flags, seed=5, rnd=2):
    s, y, ptr, w = _inputs(sizes, margins, weighted, kind)
    return torch_ref.lambdarank_gradients(
        torch.from_numpy(s), torch.from_numpy(y), ptr, None if w is None else torch.from_numpy(w),
        kind, P, bool(flags & 1), bool(flags & 2), bool(flags & 4), details=True,
        pair_method="mean", seed=seed, round=rnd)


@pytest.mark.parametrize("margins", MARGINS)
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("kind", KINDS)
def test_hip_matches_float64_reference(kind, layout, margins):
    sizes, P, flags = LAYOUTS[layout]
    weighted = (list(LAYOUTS).index(layout) + MARGINS.index(margins)) % 2 == 1
    s, y, ptr, w = _inputs(sizes, margins, weighted, kind)
    ref = _reference(kind, tuple(sizes), margins, weighted, P, flags)
    gh, plan = _run_hip(kind, s, y, ptr, w, P, flags)
    assert (plan["tile_docs"] < CAP) == (layout == "lowered")
    absmax = gh._smxgb_absmax.cpu().numpy()
    gh = gh.cpu().numpy().astype(np.float64)
    assert np.isfinite(gh).all()
    np.testing.assert_array_equal(absmax, np.abs(gh).max(axis=0).astype(np.float32))
    assert np.all(gh[ref["mass"] == 0, 0] == 0)
    paired = ref["mass"] > 0
    big = np.repeat(np.asarray(sizes) >= 20, sizes)
    assert paired[big].mean() > 0.5  # the ratio below is over the paired rows
    err_g, err_h = np.abs(gh[:, 0] - ref["g"]), np.abs(gh[:, 1] - ref["h"])
    ratio = max(float((err_g[paired] / ref["mass"][paired]).max()), float((err_h / ref["h"]).max()))
    print(f"lambdarank mean ratio {kind} {layout} {margins}: {ratio:.3e}")
    assert ratio <= TOL


@pytest.mark.parametrize("P", [1, 3])
def test_pair_set_is_the_reference_pair_set(P):
    """rank:pairwise on zero margins without normalisation: every kept pair
    adds exactly -+0.5 to g and 0.5 to h, so equal bits mean equal pairs."""
    sizes = [2, 20, 257, 7, 1, 64]
    s, y, ptr, _ = _inputs(sizes, "zero", False, "rank:pairwise")
    y[ptr[3]:ptr[4]] = 2.0  # a group whose labels are all equal
    ref = torch_ref.lambdarank_gradients(
        torch.from_numpy(s), torch.from_numpy(y), ptr, None, "rank:pairwise", P, False, False,
        True, details=True, pair_method="mean", seed=5, round=2)
    gh = _run_hip("rank:pairwise", s, y, ptr, None, P, 0)[0].cpu().numpy()
    assert np.abs(ref["g"][ptr[0]:ptr[3]]).max() > 0 and np.all(ref["g"][ptr[3]:ptr[4]] == 0)
    np.testing.assert_array_equal(gh[:, 0], ref["g"].astype(np.float32))
    np.testing.assert_array_equal(gh[:, 1], ref["h"].astype(np.float32))


@pytest.mark.parametrize("kind", KINDS)
def test_bits_depend_on_the_round_and_not_on_call_or_packing(kind):
    sizes, P = [300, 65, 257, 1, 20, 700, 64], 3
    s, y, ptr, w = _inputs(sizes, "eighths", True, kind)
    first = _run_hip(kind, s, y, ptr, w, P, 7)[0]
    assert torch.equal(first, _run_hip(kind, s, y, ptr, w, P, 7)[0])
    assert torch.equal(first, _run_hip(kind, s, y, ptr, w, P, 7, tile_docs=700)[0])
    other = _run_hip(kind, s, y, ptr, w, P, 7, rnd=3)[0]
    assert not torch.equal(first[ptr[2]:ptr[3]], other[ptr[2]:ptr[3]])  # the group of 257


def test_nan_margin_turns_the_absmax_into_nan():
    s, y, ptr, _ = _inputs([20, 65], "continuous", False, "rank:ndcg")
    s[25] = np.nan
    assert torch.isnan(_run_hip("rank:ndcg", s, y, ptr, None, 1, 7)[0]._smxgb_absmax).all()


def _train(objective, groups, caplog, tmp_path, bad_label=False):
    rng = np.random.default_rng(0)
    n = int(np.sum(groups))
    X = rng.normal(size=(n, 5)).astype(np.float32)
    rel = X[:, 0] + 0.5 * X[:, 1] + rng.normal(scale=0.3, size=n)
    y = np.clip(np.floor(rel + 1.5), 0, 3).astype(np.float32)
    y = np.minimum(y, 1) if objective == "rank:map" else y
    if bad_label:
        y[0] = 1.5
    dtrain = DMatrix(X, label=y)
    dtrain.set_group(groups)
    res = {}
    with caplog.at_level(logging.DEBUG, logger="sagemaker_xgboost_container_amd.models.objectives"):
        bst = trainer.train(
            {"objective": objective, "device": "cuda", "seed": 1, "max_depth": 4, "eta": 0.3,
             "eval_metric": "ndcg"},
            dtrain, num_boost_round=8, evals=[(dtrain, "train")], evals_result=res,
            verbose_eval=False)
    bst.save_model(str(tmp_path / "m.json"))
    return res["train"]["ndcg"], (tmp_path / "m.json").read_text()


@pytest.mark.parametrize("kind", KINDS)
def test_default_pair_method_trains_on_the_device(kind, caplog, tmp_path):
    ndcg, model = _train(kind, [20] * 30, caplog, tmp_path)
    assert "lambdarank_pair_method=mean: device kernel" in caplog.text
    assert ndcg[-1] > ndcg[0]
    assert _train(kind, [20] * 30, caplog, tmp_path)[1] == model


@pytest.mark.parametrize("groups,bad_label", [([CAP + 1, 20], False), ([20] * 30, True)])
def test_long_group_and_float_label_still_train_on_the_loop(groups, bad_label, caplog, tmp_path):
    ndcg, _ = _train("rank:ndcg", groups, caplog, tmp_path, bad_label)
    assert "lambdarank_pair_method=mean: per-group loop" in caplog.text
    assert np.isfinite(ndcg).all()
