"""Device CSR quantization (ops/hip_sparse.quantize_csr, kernels in
ops/csrc/smxgb_quantize_csr.hip) against ops/sparse_ref.quantize_sparse moved
to the device. The host code defines the rule, so every comparison is exact:
torch.equal, no tolerance."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

pytestmark = pytest.mark.gpu

TREE_ARRAYS = (
    "left", "right", "parent", "feature", "threshold", "split_bin",
    "default_left", "value", "gain", "sum_hess",
)
N_BLANK = 50  # rows 0 .. 49 store nothing, row 50 stores every non-empty column


@pytest.fixture
def hip():
    from sagemaker_xgboost_container_amd.ops import hip as mod

    before = mod.quantize_mode()
    yield mod
    mod.set_quantize_mode(before)


def _contents(n, max_bin, seed=0):
    """(n, 8) float32: one column for each case the cut finder tells apart
    (the columns of tests/test_gpu_device_quantize._columns that can be stored)."""
    rng = np.random.default_rng(seed)
    i = rng.permutation(n)
    specials = np.array(
        [-1.5, -0.0, 0.0, 1e-45, -1e-45, 1e-40, np.inf, -np.inf, -3e38, 2.5], dtype=np.float32
    )
    cols = [
        np.full(n, 3.5),                                      # constant
        (i % max_bin) * 0.25,                                 # exactly max_bin distinct
        (i % (max_bin + 1)) * 0.25,                           # one more than that
        rng.normal(size=n),
        # 60 % of the mass on one value: neighbouring ranks collapse
        np.where(rng.random(n) < 0.6, 0.0, rng.integers(1, 4 * max_bin, size=n)),
        specials[i % len(specials)],
        # keys that share their top 22 bits
        (np.float32(1.0) + (i % 1024).astype(np.float32) * np.float32(2.0 ** -23)),
        np.where(rng.random(n) < 0.7, 0.0, rng.normal(size=n)),  # stored explicit zeros
    ]
    return np.stack([np.asarray(c, dtype=np.float32) for c in cols], axis=1)


def _matrix(max_bin, cap):
    """CSR with one column per (segment length, contents). A column of length
    m stores the first m values of its contents column, so the lengths cap
    and cap + 1 (LDS sort against radix select) hold the same values but one."""
    lengths = [0, 1, 2, max_bin, max_bin + 1, 63, 64, 65, 256, 257, cap - 1, cap, cap + 1, 3 * cap + 5]
    n = 3 * cap + 100
    rng = np.random.default_rng(max_bin)
    contents = _contents(max(lengths), max_bin)
    rows, cols, vals = [], [], []
    for col, (m, k) in enumerate((m, k) for m in lengths for k in range(contents.shape[1])):
        if m == 0:
            continue
        r = N_BLANK + 1 + rng.choice(n - N_BLANK - 1, size=m - 1, replace=False)
        rows.append(np.concatenate([[N_BLANK], r]))
        cols.append(np.full(m, col))
        vals.append(contents[:m, k])
    shape = (n, len(lengths) * contents.shape[1])
    coo = (np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols)))
    return sp.csr_matrix(coo, shape=shape, dtype=np.float32)


@pytest.fixture(scope="module")
def cases():
    """max_bin -> (csr, host result on the device), built once."""
    from sagemaker_xgboost_container_amd.ops import hip_sparse
    from sagemaker_xgboost_container_amd.ops.sparse_ref import quantize_sparse

    made = {}

    def get(max_bin):
        if max_bin not in made:
            csr = _matrix(max_bin, hip_sparse.QUANTIZE_CSR_SORT_CAP)
            made[max_bin] = (csr, quantize_sparse(csr, max_bin).to("cuda"))
        return made[max_bin]

    return get


def _assert_same_qm(got, want):
    for name in ("cuts", "cut_ptr", "nbins", "indptr", "indices", "bin_data"):
        g, w = getattr(got, name), getattr(want, name)
        assert g.dtype == w.dtype and g.device == w.device and torch.equal(g, w), name
    assert got.stride == want.stride and (got.num_row, got.num_col) == (want.num_row, want.num_col)
    assert got.csc_ptr is None and got.csc_rows is None and got.csc_bins is None


@pytest.mark.parametrize("max_bin", [2, 16, 256, 1024])
def test_equals_the_host_rule(cases, max_bin):
    from sagemaker_xgboost_container_amd.ops import hip_sparse

    assert hip_sparse.QUANTIZE_CSR_SORT_CAP >= 4096
    csr, want = cases(max_bin)
    assert csr.nnz == csr.indptr[-1] and (csr.data == 0).any()  # explicit zeros stay stored
    assert (np.diff(csr.indptr)[:N_BLANK] == 0).all()
    got = hip_sparse.quantize_csr(csr, max_bin)
    _assert_same_qm(got, want)
    assert got.to("cuda") is got
    if max_bin == 256:
        assert got.stride == 257 and got.bin_data.dtype == torch.int16

    cuts, ptr = got.cuts.cpu().numpy(), got.cut_ptr.cpu().numpy()
    bins = got.bin_data.cpu().numpy().astype(np.int64)
    for j in range(csr.shape[1]):
        mine = csr.indices == j
        assert np.array_equal(
            bins[mine], np.searchsorted(cuts[ptr[j]:ptr[j + 1]], csr.data[mine], side="right")
        ), j


def test_unsorted_input_changes_nothing(cases):
    from sagemaker_xgboost_container_amd.ops import hip_sparse

    csr, want = cases(16)
    row_of = np.repeat(np.arange(csr.shape[0]), np.diff(csr.indptr))
    order = np.lexsort((np.random.default_rng(3).random(csr.nnz), row_of))
    shuffled = sp.csr_matrix((csr.data[order], csr.indices[order], csr.indptr), shape=csr.shape)
    assert not shuffled.has_sorted_indices
    before = (shuffled.data.copy(), shuffled.indices.copy(), shuffled.indptr.copy())
    _assert_same_qm(hip_sparse.quantize_csr(shuffled, 16), want)
    for now, was in zip((shuffled.data, shuffled.indices, shuffled.indptr), before):
        assert np.array_equal(now, was)


@pytest.mark.parametrize("max_bin", [16, 256])
def test_one_heavy_feature_per_chunk_changes_nothing(cases, hip, monkeypatch, max_bin):
    from sagemaker_xgboost_container_amd.ops import hip_sparse

    csr, want = cases(max_bin)
    monkeypatch.setattr(hip, "QUANTIZE_COUNTER_BYTES", 1)
    _assert_same_qm(hip_sparse.quantize_csr(csr, max_bin), want)


def test_a_stored_nan_gives_the_host_result():
    from sagemaker_xgboost_container_amd.ops import hip_sparse
    from sagemaker_xgboost_container_amd.ops.sparse_ref import quantize_sparse

    # every column has more than max_bin distinct values, so no cut is a NaN
    csr = sp.random(600, 20, density=0.5, random_state=5, dtype=np.float32, format="csr")
    csr.data[7] = np.nan
    _assert_same_qm(hip_sparse.quantize_csr(csr, 16), quantize_sparse(csr, 16).to("cuda"))


def test_trainer_routes_unweighted_csr_to_the_device(hip, monkeypatch):
    from sagemaker_xgboost_container_amd.data.dmatrix import DMatrix
    from sagemaker_xgboost_container_amd.models import trainer
    from sagemaker_xgboost_container_amd.ops import hip_sparse

    monkeypatch.setenv("SMXGB_SPARSE", "1")
    calls = []
    real = hip_sparse.quantize_csr
    monkeypatch.setattr(hip_sparse, "quantize_csr", lambda *a, **k: calls.append(1) or real(*a, **k))
    csr = sp.random(3000, 300, density=0.02, random_state=9, dtype=np.float32, format="csr")
    rng = np.random.default_rng(9)
    y = (csr[:, :5].sum(1).A1 + 0.1 * rng.normal(size=3000)).astype(np.float32)
    w = rng.uniform(0.5, 2.0, size=3000).astype(np.float32)

    def run(mode, weight=None):
        hip.set_quantize_mode(mode)
        return trainer.train(
            {"objective": "reg:squarederror", "max_depth": 4, "device": "cuda"},
            DMatrix(csr.copy(), label=y, weight=weight), 10, verbose_eval=False,
        ).trees

    by_torch = run("torch")
    assert calls == []
    by_hip = run("hip")
    assert calls == [1]
    run("hip", weight=w)
    assert calls == [1]
    assert len(by_hip) == len(by_torch) == 10
    for ta, tb in zip(by_hip, by_torch):
        for name in TREE_ARRAYS:
            assert np.array_equal(getattr(ta, name), getattr(tb, name)), name
