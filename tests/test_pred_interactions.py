"""pred_interactions, iteration_range on the explanation outputs, multiclass
approx_contribs, gblinear contributions and base_margin bias (host paths;
runs everywhere).

Oracles:
* the Shapley interaction index computed from its definition over all
  feature subsets, with the same path-dependent value function
  (`_cond_expectation` of test_treeshap.py) exact TreeSHAP uses;
* invariants: symmetry, rows sum to pred_contribs, grand sum = margin;
* a booster truncated to the requested rounds.
"""
import importlib.util
import math
import os
from itertools import combinations

import numpy as np
import pytest
import torch

from sagemaker_xgboost_container_amd.data.dmatrix import DMatrix
from sagemaker_xgboost_container_amd.models import trainer
from sagemaker_xgboost_container_amd.ops import torch_ref

_spec = importlib.util.spec_from_file_location(
    "_treeshap_oracle", os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_treeshap.py")
)
_oracle = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_oracle)
_train = _oracle._train
_cond_expectation = _oracle._cond_expectation


def _brute_interactions(trees, x, f):
    """Shapley interaction index by definition (off-diagonal cells)."""

    def v(S):
        return sum(_cond_expectation(tree, x, set(S)) for tree in trees)

    phi = np.zeros((f, f))
    feats = list(range(f))
    for i in feats:
        for j in feats:
            if i == j:
                continue
            others = [m for m in feats if m not in (i, j)]
            for size in range(len(others) + 1):
                for S in combinations(others, size):
                    w = (
                        math.factorial(len(S)) * math.factorial(f - len(S) - 2)
                        / (2 * math.factorial(f - 1))
                    )
                    phi[i, j] += w * (
                        v(S + (i, j)) - v(S + (i,)) - v(S + (j,)) + v(S)
                    )
    return phi


def _truncated(bst, rounds):
    b = bst.copy()
    end = b.iteration_indptr[rounds]
    b.trees = b.trees[:end]
    b.tree_info = b.tree_info[:end]
    b.weight_drop = b.weight_drop[:end]
    b.iteration_indptr = b.iteration_indptr[: rounds + 1]
    b._predict_cache = None
    return b


class TestBruteForceInteractions:
    @pytest.mark.parametrize("objective,nan_frac", [("reg:squarederror", 0.0),
                                                    ("binary:logistic", 0.15)])
    def test_off_diagonals_match_definition(self, objective, nan_frac):
        bst, X = _train(objective, n=400, f=4, depth=3, rounds=2, nan_frac=nan_frac)
        rows = X[:4]
        inter = bst.predict(rows, pred_interactions=True)
        assert inter.shape == (4, 5, 5)
        assert inter.dtype == np.float32
        off = ~np.eye(4, dtype=bool)
        for r in range(4):
            expected = _brute_interactions(bst.trees, rows[r], 4)
            np.testing.assert_allclose(
                inter[r, :4, :4][off], expected[off], rtol=1e-4, atol=1e-5
            )


class TestInteractionInvariants:
    def test_symmetric_rows_sum_to_contribs_total_is_margin(self):
        bst, X = _train("binary:logistic", n=400, f=5, depth=4, rounds=4, nan_frac=0.2)
        rows = X[:60]
        inter = bst.predict(rows, pred_interactions=True)
        contribs = bst.predict(rows, pred_contribs=True)
        margin = bst.predict(rows, output_margin=True)
        np.testing.assert_allclose(inter, inter.transpose(0, 2, 1), rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(inter.sum(axis=2), contribs, rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(inter.sum(axis=(1, 2)), margin, rtol=1e-4, atol=1e-4)
        # bias only in the corner cell
        assert not inter[:, -1, :-1].any() and not inter[:, :-1, -1].any()

    def test_multiclass_shape_and_invariants(self):
        bst, X = _train("multi:softprob", n=300, f=5, depth=3, rounds=3, num_class=3)
        rows = X[:30]
        inter = bst.predict(rows, pred_interactions=True)
        assert inter.shape == (30, 3, 6, 6)
        contribs = bst.predict(rows, pred_contribs=True)
        margin = bst.predict(rows, output_margin=True)
        np.testing.assert_allclose(inter, inter.transpose(0, 1, 3, 2), rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(inter.sum(axis=3), contribs, rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(inter.sum(axis=(2, 3)), margin, rtol=1e-4, atol=1e-4)

    def test_cpp_conditional_matches_python_fallback(self):
        bst, X = _train("binary:logistic", n=200, f=4, depth=3, rounds=2, nan_frac=0.15)
        flat = bst._cpu_flat_forest()
        rows = torch.as_tensor(X[:5])
        roots = flat["tree_root"].numpy()
        for condition in (1, -1):
            for feature in range(4):
                fast = torch_ref.tree_shap(
                    flat, rows, 1, condition=condition, condition_feature=feature
                ).numpy()
                slow = np.zeros_like(fast)
                for r in range(5):
                    for t in range(flat["n_trees"]):
                        torch_ref._py_tree_shap_cond_one(
                            flat, X[r], slow[r, 0], int(roots[t]), condition, feature
                        )
                np.testing.assert_allclose(fast, slow, rtol=1e-5, atol=1e-6)


class TestIterationRange:
    @pytest.fixture(scope="class")
    def model(self):
        bst, X = _train("reg:squarederror", n=400, f=5, depth=3, rounds=5)
        return bst, X[:40], _truncated(bst, 2)

    def test_iteration_range_contribs(self, model):
        bst, X, short = model
        got = bst.predict(X, pred_contribs=True, iteration_range=(0, 2))
        np.testing.assert_array_equal(got, short.predict(X, pred_contribs=True))
        assert not np.allclose(got, bst.predict(X, pred_contribs=True))
        margin = bst.predict(X, output_margin=True, iteration_range=(0, 2))
        np.testing.assert_allclose(got.sum(axis=1), margin, rtol=1e-4, atol=1e-4)

    def test_iteration_range_interactions(self, model):
        bst, X, short = model
        got = bst.predict(X, pred_interactions=True, iteration_range=(0, 2))
        np.testing.assert_array_equal(got, short.predict(X, pred_interactions=True))
        assert not np.allclose(got, bst.predict(X, pred_interactions=True))

    def test_iteration_range_leaf(self, model):
        bst, X, short = model
        got = bst.predict(X, pred_leaf=True, iteration_range=(0, 2))
        assert got.shape == (40, 2)
        np.testing.assert_array_equal(got, short.predict(X, pred_leaf=True))
        assert bst.predict(X, pred_leaf=True).shape == (40, 5)

    def test_iteration_range_zero_zero_means_all(self, model):
        bst, X, _ = model
        np.testing.assert_array_equal(
            bst.predict(X, pred_contribs=True, iteration_range=(0, 0)),
            bst.predict(X, pred_contribs=True),
        )

    def test_ntree_limit_alias(self, model):
        bst, X, _ = model
        for flag in ("pred_contribs", "pred_interactions", "pred_leaf"):
            np.testing.assert_array_equal(
                bst.predict(X, ntree_limit=2, **{flag: True}),
                bst.predict(X, iteration_range=(0, 2), **{flag: True}),
            )

    def test_ntree_limit_multiclass_counts_trees(self):
        bst, X = _train("multi:softprob", n=200, f=4, depth=3, rounds=3, num_class=3)
        np.testing.assert_array_equal(
            bst.predict(X[:10], pred_contribs=True, ntree_limit=6),
            bst.predict(X[:10], pred_contribs=True, iteration_range=(0, 2)),
        )


class TestApproxContribs:
    def test_multiclass_shape_and_additivity(self):
        bst, X = _train("multi:softprob", n=300, f=5, depth=3, rounds=3, num_class=3)
        approx = bst.predict(X[:25], pred_contribs=True, approx_contribs=True)
        assert approx.shape == (25, 3, 6)
        margin = bst.predict(X[:25], output_margin=True)
        np.testing.assert_allclose(approx.sum(axis=2), margin, rtol=1e-3, atol=1e-3)

    def test_single_output_matches_per_row_walk(self):
        bst, X = _train("reg:squarederror", n=200, f=4, depth=3, rounds=2)
        approx = bst.predict(X[:10], pred_contribs=True, approx_contribs=True)
        assert approx.shape == (10, 5)
        margin = bst.predict(X[:10], output_margin=True)
        np.testing.assert_allclose(approx.sum(axis=1), margin, rtol=1e-3, atol=1e-3)
        # scalar Saabas walk, the definition
        expected = np.zeros((10, 5))
        expected[:, -1] = bst.objective().base_margin(bst.base_score)
        for tree in bst.trees:
            for i in range(10):
                nid = 0
                while tree.left[nid] >= 0:
                    fv = X[i, tree.feature[nid]]
                    nxt = tree.left[nid] if fv < tree.threshold[nid] else tree.right[nid]
                    expected[i, tree.feature[nid]] += float(tree.value[nxt]) - float(tree.value[nid])
                    nid = nxt
                expected[i, -1] += float(tree.value[0])
        np.testing.assert_allclose(approx, expected, rtol=1e-3, atol=1e-3)


class TestFlagsAndLinear:
    def test_mutually_exclusive_flags(self):
        bst, X = _train("reg:squarederror", n=100, f=4, depth=2, rounds=1)
        for flags in (
            {"pred_contribs": True, "pred_leaf": True},
            {"pred_contribs": True, "pred_interactions": True},
            {"pred_interactions": True, "pred_leaf": True},
        ):
            with pytest.raises(ValueError):
                bst.predict(X[:3], **flags)

    def test_xgboost_shim_passes_keyword_through(self):
        import xgboost as xgb

        rng = np.random.default_rng(1)
        X = rng.normal(size=(120, 3)).astype(np.float32)
        y = (X[:, 0] - X[:, 1]).astype(np.float32)
        bst = xgb.train({"objective": "reg:squarederror", "max_depth": 2, "device": "cpu"},
                        xgb.DMatrix(X, label=y), num_boost_round=2, verbose_eval=False)
        inter = bst.predict(xgb.DMatrix(X[:7]), pred_interactions=True)
        assert inter.shape == (7, 4, 4)

    def test_gblinear_contribs_sum_to_margin(self):
        rng = np.random.default_rng(3)
        X = rng.normal(size=(200, 4)).astype(np.float32)
        y = (X[:, 0] * 2 - X[:, 2]).astype(np.float32)
        bst = trainer.train(
            {"booster": "gblinear", "objective": "reg:squarederror", "device": "cpu"},
            DMatrix(X, label=y), num_boost_round=5, verbose_eval=False,
        )
        rows = X[:20].copy()
        rows[0, 1] = np.nan
        contribs = bst.predict(rows, pred_contribs=True)
        assert contribs.shape == (20, 5)
        margin = bst.predict(rows, output_margin=True)
        np.testing.assert_allclose(contribs.sum(axis=1), margin, rtol=1e-4, atol=1e-4)
        assert contribs[0, 1] == 0.0  # missing value contributes nothing
        inter = bst.predict(rows, pred_interactions=True)
        assert inter.shape == (20, 5, 5)
        np.testing.assert_array_equal(inter[:, np.arange(5), np.arange(5)], contribs)
        assert np.count_nonzero(inter[:, ~np.eye(5, dtype=bool)]) == 0
        with pytest.raises(ValueError):
            bst.predict(rows, pred_leaf=True)


class TestBaseMargin:
    def test_bias_column_is_per_row_base_margin(self):
        bst, X = _train("reg:squarederror", n=300, f=4, depth=3, rounds=3)
        rows = X[:30]
        bm = np.linspace(-1.0, 2.0, 30).astype(np.float32)
        plain = bst.predict(DMatrix(rows), pred_contribs=True)
        base = float(bst.objective().base_margin(bst.base_score))
        expected_value = plain[:, -1] - base
        dm = DMatrix(rows, base_margin=bm)
        contribs = bst.predict(dm, pred_contribs=True)
        np.testing.assert_allclose(contribs[:, -1], bm + expected_value, rtol=1e-5, atol=1e-5)
        np.testing.assert_array_equal(contribs[:, :-1], plain[:, :-1])
        margin = bst.predict(dm, output_margin=True)
        np.testing.assert_allclose(contribs.sum(axis=1), margin, rtol=1e-4, atol=1e-4)
        inter = bst.predict(dm, pred_interactions=True)
        np.testing.assert_allclose(inter[:, -1, -1], bm + expected_value, rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(inter.sum(axis=(1, 2)), margin, rtol=1e-4, atol=1e-4)
