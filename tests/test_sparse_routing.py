"""Sparse-path routing (models/trainer.py) and SparseQuantizedMatrix.to():
the pieces of the device CSR path that need no GPU."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from sagemaker_xgboost_container_amd.models import trainer
from sagemaker_xgboost_container_amd.models.trainer import _sparse_path_ok, sparse_auto_engage
from sagemaker_xgboost_container_amd.ops import backend_for_qm, sparse_ref
from sagemaker_xgboost_container_amd.ops.sparse_ref import SparseQuantizedMatrix, quantize_sparse

GB = 1 << 30


class TestAutoEngage:
    def test_host_rule(self):
        assert sparse_auto_engage(1000, 64, 32_000)
        assert not sparse_auto_engage(1000, 63, 10)          # narrow
        assert not sparse_auto_engage(1000, 64, 32_001)      # more than half full

    def test_device_rule_is_memory_driven(self):
        n, f = 500_000, 20_000            # the README shape: 50 GB of staging
        nnz = n * f // 1000
        staging = n * f * 5
        assert sparse_auto_engage(n, f, nnz, free_bytes=2 * staging - 2)
        assert not sparse_auto_engage(n, f, nnz, free_bytes=2 * staging)   # exactly half: fits
        assert not sparse_auto_engage(n, f, nnz, free_bytes=288 * GB)
        assert sparse_auto_engage(5_000_000, f, 10 * nnz, free_bytes=288 * GB)

    @pytest.mark.parametrize("free", [1, GB, 288 * GB])
    def test_never_for_narrow_or_dense(self, free):
        assert not sparse_auto_engage(10**9, 63, 10, free_bytes=free)
        n, f = 10**7, 10**4
        assert not sparse_auto_engage(n, f, n * f // 2 + 1, free_bytes=free)

    def test_small_jobs_keep_the_dense_device_path(self):
        # every shape the existing device tests train: far below half of HBM
        assert not sparse_auto_engage(2000, 80, 32_000, free_bytes=200 * GB)


class _FakeDMatrix:
    is_sparse = True

    def __init__(self, n, f, nnz):
        self._shape = (n, f)
        self._nnz = nnz

    def num_row(self):
        return self._shape[0]

    def num_col(self):
        return self._shape[1]

    def csr(self):
        class _C:
            nnz = self._nnz

        return _C()


class TestSparsePathOk:
    def test_device_forced_and_disabled(self, monkeypatch):
        dm = _FakeDMatrix(100, 8, 10)
        cuda = torch.device("cuda")
        monkeypatch.setenv("SMXGB_SPARSE", "1")
        assert _sparse_path_ok(dm, {}, cuda, None)
        assert _sparse_path_ok(dm, {}, torch.device("cpu"), None)
        assert not _sparse_path_ok(dm, {"booster": "dart"}, cuda, None)
        assert not _sparse_path_ok(dm, {"process_type": "update"}, cuda, None)
        monkeypatch.setenv("SMXGB_SPARSE", "0")
        assert not _sparse_path_ok(dm, {}, cuda, None)

    def test_device_off_with_a_communicator(self, monkeypatch):
        dm = _FakeDMatrix(100, 8, 10)
        comm = object()
        monkeypatch.setenv("SMXGB_SPARSE", "1")
        assert not _sparse_path_ok(dm, {}, torch.device("cuda"), comm)
        assert _sparse_path_ok(dm, {}, torch.device("cpu"), comm)  # host path unchanged

    def test_device_auto_uses_free_memory(self, monkeypatch):
        monkeypatch.delenv("SMXGB_SPARSE", raising=False)
        n, f = 500_000, 20_000
        dm = _FakeDMatrix(n, f, n * f // 1000)
        cuda = torch.device("cuda")
        monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (288 * GB, 288 * GB))
        assert not _sparse_path_ok(dm, {}, cuda, None)
        monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (60 * GB, 288 * GB))
        assert _sparse_path_ok(dm, {}, cuda, None)
        assert not _sparse_path_ok(dm, {}, cuda, object())

        def _no_query(device=None):
            raise AssertionError("device queried for a job the host rule rejects")

        monkeypatch.setattr(torch.cuda, "mem_get_info", _no_query)
        assert not _sparse_path_ok(_FakeDMatrix(1000, 8, 10), {}, cuda, None)

    def test_dense_input_never_engages(self, monkeypatch):
        monkeypatch.setenv("SMXGB_SPARSE", "1")
        dm = _FakeDMatrix(100, 80, 10)
        dm.is_sparse = False
        assert not _sparse_path_ok(dm, {}, torch.device("cuda"), None)


def _rand_csr(n=300, f=40, density=0.2, seed=0):
    rng = np.random.default_rng(seed)
    mask = rng.random((n, f)) < density
    mask[5:9] = False  # rows with no entries
    vals = np.round(rng.normal(size=(n, f)) * 8).astype(np.float32) / 8
    rows, cols = np.nonzero(mask)
    return sp.csr_matrix((vals[rows, cols], (rows, cols)), shape=(n, f), dtype=np.float32)


class TestQuantizedMatrixTo:
    def test_cpu_round_trip(self):
        qm = quantize_sparse(_rand_csr())
        moved = qm.to("cpu")
        assert moved is not qm and moved.device.type == "cpu"
        for name in ("indptr", "indices", "bin_data", "csc_ptr", "csc_rows", "csc_bins",
                     "cuts", "cut_ptr", "nbins"):
            a, b = getattr(qm, name), getattr(moved, name)
            assert a.dtype == b.dtype and torch.equal(a, b), name
        assert (moved.stride, moved.num_row, moved.num_col) == (qm.stride, qm.num_row, qm.num_col)
        assert backend_for_qm(moved) is sparse_ref

    def test_unsorted_indices_come_out_sorted(self):
        qm = quantize_sparse(_rand_csr(seed=1))
        indptr = qm.indptr.numpy()
        indices = qm.indices.clone()
        bins = qm.bin_data.clone()
        rng = np.random.default_rng(3)
        for r in range(qm.num_row):
            s, e = int(indptr[r]), int(indptr[r + 1])
            perm = torch.from_numpy(rng.permutation(e - s))
            indices[s:e] = indices[s:e][perm]
            bins[s:e] = bins[s:e][perm]
        assert not torch.equal(indices, qm.indices)
        shuffled = SparseQuantizedMatrix(
            (qm.indptr, indices, bins), (qm.csc_ptr, qm.csc_rows, qm.csc_bins),
            qm.cuts, qm.cut_ptr, qm.nbins, qm.stride, qm.num_row, qm.num_col,
        )
        fixed = shuffled.to("cpu")
        assert torch.equal(fixed.indptr, qm.indptr)
        assert torch.equal(fixed.indices, qm.indices)   # sorted within each row again
        assert torch.equal(fixed.bin_data, qm.bin_data)  # bins travelled with their columns

    def test_malformed_matrix_is_rejected(self):
        qm = quantize_sparse(_rand_csr(seed=2))
        bad = SparseQuantizedMatrix(
            (qm.indptr, qm.indices + qm.num_col, qm.bin_data),
            (qm.csc_ptr, qm.csc_rows, qm.csc_bins),
            qm.cuts, qm.cut_ptr, qm.nbins, qm.stride, qm.num_row, qm.num_col,
        )
        with pytest.raises(ValueError):
            bad.to("cpu")

    def test_mirror_flag_keys_the_grower(self):
        from sagemaker_xgboost_container_amd.models.grower import HistGrower
        from sagemaker_xgboost_container_amd.ops import torch_ref

        qm = quantize_sparse(_rand_csr(seed=4))
        grower = HistGrower(qm, {"max_depth": 3})
        assert grower.backend is sparse_ref and grower._mirror_device is False
        assert not hasattr(torch_ref, "MIRRORS_DEVICE_GROWER")
        assert trainer.sparse_auto_engage is sparse_auto_engage
