"""Adaptive tree leaves on the device: the segmented radix select of
csrc/smxgb_quantile.hip against the numpy oracle of test_adaptive_leaves.py
(exactly), its order independence and bounds, and the leaf values of
reg:absoluteerror / reg:quantileerror models on every device growing path.

All tests require an MI355X (pytest tests -m gpu).
"""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from sagemaker_xgboost_container_amd.data.dmatrix import DMatrix
from sagemaker_xgboost_container_amd.models import trainer

from test_adaptive_leaves import (
    ALPHAS, SHAPES, check_leaf_values, exact_weights, make_pos, make_resid,
    oracle_leaf_quantiles, same_values,
)

pytestmark = pytest.mark.gpu

# the five shapes of the contract, and one past the leaf count up to which
# count / scatter aggregate in LDS (LQ_LDS_LEAVES = 2048)
GPU_SHAPES = SHAPES + ((9000, 2500, "uniform"),)


@pytest.fixture(scope="module")
def hip():
    from sagemaker_xgboost_container_amd.ops import hip as backend

    return backend


def _run(hip, pos, resid, n_leaves, alpha, weight=None):
    out = hip.leaf_quantiles(
        torch.from_numpy(pos).cuda(), torch.from_numpy(resid).cuda(), n_leaves, alpha,
        None if weight is None else torch.from_numpy(weight).cuda(),
    )
    assert out.is_cuda and out.dtype == torch.float32 and out.shape == (n_leaves,)
    return out.cpu().numpy()


@pytest.mark.parametrize("n,n_leaves,layout", GPU_SHAPES)
def test_kernel_equals_oracle(hip, n, n_leaves, layout):
    rng = np.random.default_rng(7 * n + n_leaves)
    pos = make_pos(n, n_leaves, layout, rng)
    for kind in ("continuous", "eighths"):
        resid = make_resid(n, kind, rng)
        for alpha in ALPHAS:
            got = _run(hip, pos, resid, n_leaves, alpha)
            want = oracle_leaf_quantiles(pos, resid, n_leaves, alpha)
            assert same_values(got, want), (kind, alpha, np.nonzero(~(got == want))[0][:8])


@pytest.mark.parametrize("n,n_leaves,layout", GPU_SHAPES)
def test_weighted_exact(hip, n, n_leaves, layout):
    rng = np.random.default_rng(11 * n + n_leaves)
    pos = make_pos(n, n_leaves, layout, rng)
    weight = exact_weights(n, rng)
    for kind in ("continuous", "eighths"):
        resid = make_resid(n, kind, rng)
        for alpha in ALPHAS:
            got = _run(hip, pos, resid, n_leaves, alpha, weight)
            want = oracle_leaf_quantiles(pos, resid, n_leaves, alpha, weight)
            assert same_values(got, want), (kind, alpha, np.nonzero(~(got == want))[0][:8])


@pytest.mark.parametrize("n,n_leaves,layout", (SHAPES[2], SHAPES[4]))
def test_weighted_arbitrary_bracket(hip, n, n_leaves, layout):
    """The value is one of the leaf's residuals and satisfies the bracket of
    the rule in float64, up to the fixed-point slack n * 2^-s / 2 that the
    docstring of hip.leaf_quantiles derives from its scale 2^s."""
    rng = np.random.default_rng(13 * n)
    pos = make_pos(n, n_leaves, layout, rng)
    resid = make_resid(n, "eighths", rng)
    weight = np.exp(rng.normal(size=n) * 2).astype(np.float32)
    scale = hip.leaf_quantile_weight_scale(n, float(weight.max()))
    slack = n * 0.5 / scale
    for alpha in ALPHAS:
        got = _run(hip, pos, resid, n_leaves, alpha, weight)
        for leaf in range(n_leaves):
            rows = pos == leaf
            if not rows.any():
                assert np.isnan(got[leaf])
                continue
            v, w = resid[rows], weight[rows].astype(np.float64)
            assert (v == got[leaf]).any(), (alpha, leaf)
            total = w.sum()
            assert w[v <= got[leaf]].sum() - alpha * total >= -slack, (alpha, leaf)
            assert w[v < got[leaf]].sum() - alpha * total < slack, (alpha, leaf)


@pytest.mark.parametrize("n,n_leaves,layout", (SHAPES[2], SHAPES[3], SHAPES[4]))
def test_order_independence(hip, n, n_leaves, layout):
    rng = np.random.default_rng(17 * n)
    pos = make_pos(n, n_leaves, layout, rng)
    resid = make_resid(n, "eighths", rng)
    weight = np.exp(rng.normal(size=n) * 2).astype(np.float32)
    perm = rng.permutation(n)
    for alpha in (0.5, 0.1):
        for w in (None, weight):
            a = _run(hip, pos, resid, n_leaves, alpha, w)
            b = _run(hip, pos[perm], resid[perm], n_leaves, alpha, None if w is None else w[perm])
            assert a.tobytes() == b.tobytes(), (alpha, w is None)


def test_bounds(hip):
    pos = torch.tensor([0, 1, 4, -1], dtype=torch.int32).cuda()
    resid = torch.zeros(4, dtype=torch.float32).cuda()
    with pytest.raises(ValueError):
        hip.leaf_quantiles(pos, resid, 4, 0.5)
    with pytest.raises(ValueError):
        hip.leaf_quantiles(pos - 2, resid, 8, 0.5)
    with pytest.raises(ValueError):
        hip.leaf_quantiles(pos, resid, 8, 1.0)
    with pytest.raises(ValueError):
        hip.leaf_quantiles(pos, resid, 8, 0.5, torch.tensor([1.0, -1.0, 1.0, 1.0]).cuda())
    assert hip.leaf_quantiles(pos, resid, 5, 0.5).shape == (5,)


# -- training on the device ---------------------------------------------------------
OBJECTIVES = (
    ("reg:absoluteerror", {}),
    ("reg:quantileerror", {"quantile_alpha": [0.2, 0.8]}),
)


def _train_and_check(X, y, params, rounds=3):
    for name, extra in OBJECTIVES:
        p = dict(params, objective=name, eta=0.5, base_score=0.5, **extra)
        bst = trainer.train(p, DMatrix(X, label=y), num_boost_round=rounds, verbose_eval=False)
        alphas = extra.get("quantile_alpha", [0.5])
        assert len(bst.trees) == rounds * len(alphas)
        assert all(t.num_leaves >= 4 for t in bst.trees), [t.num_leaves for t in bst.trees]
        assert check_leaf_values(bst, X, y, 0.5, alphas) >= 4 * len(bst.trees)


def test_training_dense_device_grower():
    rng = np.random.default_rng(3)
    X = rng.normal(size=(4000, 10)).astype(np.float32)
    y = (X[:, 0] * 3 + np.abs(X[:, 1]) + rng.standard_t(3, size=4000)).astype(np.float32)
    _train_and_check(X, y, {"max_depth": 4, "tree_method": "gpu_hist"})


def test_training_dense_per_level(monkeypatch):
    monkeypatch.setenv("SMXGB_NO_DEVICE_GROW", "1")
    rng = np.random.default_rng(4)
    X = rng.normal(size=(4000, 10)).astype(np.float32)
    y = (X[:, 0] * 3 + np.abs(X[:, 1]) + rng.standard_t(3, size=4000)).astype(np.float32)
    _train_and_check(X, y, {"max_depth": 4, "tree_method": "gpu_hist"})


def test_training_sparse(monkeypatch):
    monkeypatch.setenv("SMXGB_SPARSE", "1")
    rng = np.random.default_rng(5)
    X = sp.random(2000, 70, density=0.05, format="csr", dtype=np.float32, random_state=5)
    y = (np.asarray(X[:, :5].sum(axis=1)).ravel() * 4 + rng.standard_t(3, size=2000)).astype(np.float32)
    _train_and_check(X, y, {"max_depth": 4, "tree_method": "gpu_hist"})
