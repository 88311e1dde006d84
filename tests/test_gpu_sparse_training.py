"""Device CSR training (SMXGB_SPARSE=1 on cuda: ops/hip_sparse.py) against the
dense device grower (SMXGB_SPARSE=0) on the same data: every tree array must
be equal, and the sparse run must never densify.

All tests require an MI355X (pytest tests -m gpu).
"""
import copy
import gc
import logging
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from sagemaker_xgboost_container_amd.data.dmatrix import DMatrix
from sagemaker_xgboost_container_amd.models import trainer

pytestmark = pytest.mark.gpu

_TREE_ARRAYS = (
    "left", "right", "parent", "feature", "threshold", "split_bin", "default_left",
    "value", "gain", "sum_hess",
)


def _eighths_csr(n, f, density, seed, blank_rows=()):
    """CSR whose values are multiples of 1/8 (see TestSparseDenseDeviceParity)."""
    rng = np.random.default_rng(seed)
    mask = rng.random((n, f)) < density
    for r in blank_rows:
        mask[r] = False
    vals = np.round(rng.normal(size=(n, f)) * 8).astype(np.float32) / 8
    rows, cols = np.nonzero(mask)
    csr = sp.csr_matrix((vals[rows, cols], (rows, cols)), shape=(n, f), dtype=np.float32)
    signal = np.where(mask[:, 0], vals[:, 0], -0.25) + 0.5 * np.where(mask[:, 1], vals[:, 1], 0.25)
    y = (signal + 0.3 * rng.normal(size=n) > 0).astype(np.float32)
    return csr, y


def _train(mode, csr, y, params, rounds, weight=None, valid=None, growers=None, monkeypatch=None):
    """One run on cuda with SMXGB_SPARSE=mode; the environment is restored."""
    saved = os.environ.get("SMXGB_SPARSE")
    os.environ["SMXGB_SPARSE"] = mode
    try:
        if growers is not None:
            base = trainer.HistGrower

            class _Recording(base):
                def __init__(self, *a, **k):
                    super().__init__(*a, **k)
                    growers.append(self)

            monkeypatch.setattr(trainer, "HistGrower", _Recording)
        res = {}
        dm = DMatrix(csr.copy(), label=y, weight=weight)
        kwargs = {}
        if valid is not None:
            vcsr, vy = valid
            kwargs["evals"] = [(dm, "train"), (DMatrix(vcsr.copy(), label=vy), "validation")]
        p = dict(copy.deepcopy(params), device="cuda")
        bst = trainer.train(p, dm, num_boost_round=rounds, evals_result=res,
                            verbose_eval=False, **kwargs)
        return bst, res
    finally:
        if saved is None:
            os.environ.pop("SMXGB_SPARSE", None)
        else:
            os.environ["SMXGB_SPARSE"] = saved


def _assert_same_trees(a, b):
    assert len(a.trees) == len(b.trees) and len(a.trees) > 0
    for i, (ta, tb) in enumerate(zip(a.trees, b.trees)):
        for name in _TREE_ARRAYS:
            assert np.array_equal(getattr(ta, name), getattr(tb, name)), f"tree {i}: {name} differs"


@pytest.fixture(scope="module")
def data():
    return _eighths_csr(2000, 80, 0.2, seed=11)


class TestSparseDenseDeviceParity:
    """2000 x 80 CSR at density 0.2 whose values are multiples of 1/8: every
    feature then has fewer than max_bin distinct present values, so its cuts
    come from the midpoint branch of ops/quantize._feature_cuts_sorted. That
    branch is exact IEEE arithmetic, the same on the host (quantize_sparse)
    and on the device (quantize). The quantile branch (linspace().round(),
    float32 cumsum) is not guaranteed to round the same on both, and a cut
    that differs in the last bit would be a difference of the two cut
    finders, not of the two training paths compared here."""

    def _both(self, csr, y, params, rounds=4, weight=None):
        sparse, _ = _train("1", csr, y, params, rounds, weight=weight)
        dense, _ = _train("0", csr, y, params, rounds, weight=weight)
        _assert_same_trees(sparse, dense)
        return sparse

    def test_binary_depth6(self, data):
        csr, y = data
        bst = self._both(csr, y, {"objective": "binary:logistic", "max_depth": 6, "eta": 0.3})
        assert max(t.num_nodes for t in bst.trees) > 15  # real trees, not stumps

    def test_weighted_squarederror(self, data):
        csr, y = data
        w = np.random.default_rng(2).uniform(0.5, 2.0, size=csr.shape[0]).astype(np.float32)
        self._both(csr, y, {"objective": "reg:squarederror", "max_depth": 5}, weight=w)

    def test_row_and_column_sampling(self, data):
        csr, y = data
        self._both(csr, y, {"objective": "binary:logistic", "max_depth": 5, "subsample": 0.7,
                            "colsample_bytree": 0.6, "seed": 9})

    def test_lossguide(self, data):
        csr, y = data
        self._both(csr, y, {"objective": "binary:logistic", "grow_policy": "lossguide",
                            "max_leaves": 12})

    def test_monotone_constraint(self, data):
        csr, y = data
        mono = "(" + ",".join(["1", "-1"] + ["0"] * (csr.shape[1] - 2)) + ")"
        self._both(csr, y, {"objective": "binary:logistic", "max_depth": 5,
                            "monotone_constraints": mono})

    def test_stored_zeros_are_values_not_missing(self):
        """A stored 0.0 is a present value; the same cell left out is missing.
        Both runs must agree on each matrix, and the two matrices must not
        train to the same model."""
        csr, y = _eighths_csr(2000, 80, 0.2, seed=12)
        assert (csr.data == 0).sum() > 100  # eighths round to 0 often enough
        params = {"objective": "binary:logistic", "max_depth": 5}
        with_zeros = self._both(csr, y, params)
        pruned = csr.copy()
        pruned.eliminate_zeros()
        assert pruned.nnz < csr.nnz
        without = self._both(pruned, y, params)
        differs = any(
            a.num_nodes != b.num_nodes
            or any(not np.array_equal(getattr(a, name), getattr(b, name)) for name in _TREE_ARRAYS)
            for a, b in zip(with_zeros.trees, without.trees)
        )
        assert differs

    def test_rows_with_no_features(self):
        blank = list(range(0, 2000, 7))
        csr, y = _eighths_csr(2000, 80, 0.2, seed=13, blank_rows=blank)
        assert int((np.diff(csr.indptr) == 0).sum()) >= len(blank)
        self._both(csr, y, {"objective": "binary:logistic", "max_depth": 6})

    def test_eval_metrics_match(self, data):
        csr, y = data
        valid = _eighths_csr(700, 80, 0.2, seed=14)
        params = {"objective": "binary:logistic", "max_depth": 6, "eval_metric": ["logloss", "auc"]}
        _, res_sparse = _train("1", csr, y, params, 4, valid=valid)
        _, res_dense = _train("0", csr, y, params, 4, valid=valid)
        for ds in ("train", "validation"):
            for metric in ("logloss", "auc"):
                assert len(res_sparse[ds][metric]) == 4
                np.testing.assert_allclose(
                    res_sparse[ds][metric], res_dense[ds][metric], rtol=1e-6, atol=1e-7
                )

    def test_warm_start_replays_on_device(self, data):
        csr, y = data
        params = {"objective": "binary:logistic", "max_depth": 4}
        out = {}
        for mode in ("1", "0"):
            first, _ = _train(mode, csr, y, params, 2)
            saved = os.environ.get("SMXGB_SPARSE")
            os.environ["SMXGB_SPARSE"] = mode
            try:
                out[mode] = trainer.train(
                    dict(params, device="cuda"), DMatrix(csr.copy(), label=y),
                    num_boost_round=2, xgb_model=first, verbose_eval=False,
                )
            finally:
                if saved is None:
                    os.environ.pop("SMXGB_SPARSE", None)
                else:
                    os.environ["SMXGB_SPARSE"] = saved
        assert len(out["1"].trees) == 4
        _assert_same_trees(out["1"], out["0"])


class TestNeverDensifies:
    def test_wide_sparse_job_stays_sparse(self, monkeypatch, caplog):
        """100k x 4096 at 0.5 % density, values in {1, 2, 3} (stride 4, tiny
        histograms). The bound is derived, not measured: any densifying path
        allocates at least the n*f-byte uint8 bin matrix (410 MB); the sparse
        footprint is about 25 MB (2 M entries x 5 B, row buffers, gradients,
        margins). n*f/4 (102 MB) separates the two with room on both sides."""
        n, f = 100_000, 4096

        def make(rows, seed):
            rng = np.random.default_rng(seed)
            nnz = int(rows * f * 0.005)
            r = rng.integers(0, rows, nnz)
            c = rng.integers(0, f, nnz)
            csr = sp.csr_matrix(
                (np.ones(nnz, dtype=np.float32), (r, c)), shape=(rows, f), dtype=np.float32
            )
            csr.sum_duplicates()
            csr.data = rng.integers(1, 4, csr.nnz).astype(np.float32)
            col = np.asarray(csr[:, :8].sum(axis=1)).ravel()
            return csr, (col > 0).astype(np.float32)

        csr, y = make(n, 21)
        valid = make(20_000, 22)

        def _no_dense(self):
            raise AssertionError("DMatrix.to_dense() called on the device sparse path")

        monkeypatch.setattr(DMatrix, "to_dense", _no_dense)
        growers = []
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        with caplog.at_level(logging.INFO, logger="sagemaker_xgboost_container_amd"):
            bst, res = _train(
                "1", csr, y, {"objective": "binary:logistic", "max_depth": 4}, 2,
                valid=valid, growers=growers, monkeypatch=monkeypatch,
            )
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
        print(f"peak device memory {peak / 1e6:.1f} MB, bound {n * f / 4 / 1e6:.1f} MB")
        assert peak < n * f / 4
        assert len(bst.trees) == 2 and len(res["validation"]["logloss"]) == 2
        assert len(growers) == 1 and growers[0].grow_path == "per_level"
        assert growers[0].backend.NAME == "hip_sparse"
        engaged = [r.getMessage() for r in caplog.records if "Sparse training path engaged" in r.getMessage()]
        assert engaged and "hip_sparse" in engaged[0]
