"""Compact TreeSHAP kernel (chunk-local phi slots) over dense and CSR rows
vs the host implementation on the same forest.

Kernel tests call hip.tree_shap_compact directly, so a fallback cannot hide
a broken kernel; booster-level tests make DMatrix.to_dense and the host
TreeSHAP raise. Comparator: torch_ref.tree_shap (fp64 recursion) on the same
forest; for CSR input, on the NaN-densified twin. Both sides compute in fp64
and round once to float32, so rtol 1e-5 / atol 1e-6 on the float32 outputs
(tests/test_gpu_shap.py's tolerance between two fp64 implementations). f = 4
models are also checked against the brute-force Shapley definition at rtol
1e-4 / atol 1e-5. The CSR accessor must be BIT-equal to the dense accessor
on the twin: same kernel, same order, only the lookup differs.

All tests require an MI355X (pytest tests -m gpu).
"""
import gc
import importlib.util
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from sagemaker_xgboost_container_amd.data.dmatrix import DMatrix
from sagemaker_xgboost_container_amd.models import booster as booster_mod
from sagemaker_xgboost_container_amd.models import trainer
from sagemaker_xgboost_container_amd.models.booster import Booster
from sagemaker_xgboost_container_amd.models.tree import Tree
from sagemaker_xgboost_container_amd.ops import torch_ref

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from sagemaker_xgboost_container_amd.ops import hip, hip_sparse
else:  # allow collection on CPU boxes
    hip = hip_sparse = None

_HERE = os.path.dirname(os.path.abspath(__file__))
_RTOL, _ATOL = 1e-5, 1e-6


def _load(name, filename):
    spec = importlib.util.spec_from_file_location(name, os.path.join(_HERE, filename))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _train(objective="reg:squarederror", n=400, f=4, depth=3, rounds=3, nan_frac=0.0,
           num_class=None, seed=0, **extra):
    """Small host-trained model whose target depends on every feature."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, f)).astype(np.float32)
    if nan_frac:
        X[rng.random(size=X.shape) < nan_frac] = np.nan
    Xz = np.nan_to_num(X)
    signal = sum((1.0 + 0.3 * j) * Xz[:, j] * (1 if j % 2 == 0 else -1) for j in range(f))
    signal = signal + Xz[:, 0] * Xz[:, f - 1]
    if objective.startswith("multi"):
        y = np.digitize(signal, np.quantile(signal, [1 / 3, 2 / 3])).astype(np.float32)
    elif objective.startswith("binary"):
        y = (signal > 0).astype(np.float32)
    else:
        y = signal.astype(np.float32)
    params = {"objective": objective, "max_depth": depth, "eta": 0.4, "device": "cpu"}
    if num_class:
        params["num_class"] = num_class
    params.update(extra)
    bst = trainer.train(params, DMatrix(X, label=y), num_boost_round=rounds, verbose_eval=False)
    return bst, X


def _cover_tree(rng, pool, depth, root_feature=None, ragged=True):
    """Ragged hand-built tree with consistent positive covers: every parent's
    cover is the sum of its children's, exactly in float32 (dyadic shares of
    4096). Split features come from `pool`; thresholds are eighths."""
    tree = Tree()
    frontier = [(tree.add_node(value=float(rng.normal()), sum_hess=4096.0), 4096.0)]
    for level in range(depth):
        nxt = []
        for nid, h in frontier:
            if ragged and level > 0 and rng.random() < 0.25:
                continue  # stays a leaf: ragged
            feature = int(pool[rng.integers(0, len(pool))])
            if level == 0 and root_feature is not None:
                feature = root_feature
            hl = h * float(rng.choice([0.25, 0.5, 0.75]))
            lid, rid = tree.apply_split(
                nid, feature, float(np.round(rng.normal() * 8) / 8), 0,
                bool(rng.integers(0, 2)), 1.0,
                left_value=float(rng.normal()), right_value=float(rng.normal()),
                left_hess=hl, right_hess=h - hl,
            )
            nxt += [(lid, hl), (rid, h - hl)]
        frontier = nxt
    return tree.finalize()


def _cover_booster(f, rounds, pool, depth=5, k=1, seed=0, roots=(), full=False):
    """Booster of hand-built trees; `full` makes every tree a complete tree
    of `depth` levels, else depths vary and trees are ragged."""
    rng = np.random.default_rng(seed)
    params = {"objective": "multi:softprob", "num_class": k} if k > 1 else {
        "objective": "binary:logistic"}
    bst = Booster(params, num_features=f)
    roots = list(roots)
    for _ in range(rounds):
        trees = [
            _cover_tree(rng, pool, depth if full else int(rng.integers(1, depth + 1)),
                        roots.pop(0) if roots else None, ragged=not full)
            for _ in range(k)
        ]
        bst.add_iteration(trees, list(range(k)))
    return bst


def _dense_twin(csr):
    n, f = csr.shape
    dense = np.full((n, f), np.nan, dtype=np.float32)
    dense[np.repeat(np.arange(n), np.diff(csr.indptr)), csr.indices] = csr.data
    return dense


def _flats(bst):
    """(host flat forest, device flat forest with path tables)."""
    return bst._cpu_flat_forest(), bst._device_flat_forest(torch.device("cuda"), with_paths=True)


def _scatter(phi, cols, n, k, f):
    """(n, k, f+1) float32 image of a compact result."""
    assert phi.is_cuda and phi.dtype == torch.float64
    assert cols.dtype == torch.int64 and phi.shape == (n, cols.shape[0])
    c = cols.cpu().numpy()
    assert (np.diff(c) > 0).all() and (c.size == 0 or (c[0] >= 0 and c[-1] < k * (f + 1)))
    assert not (c % (f + 1) == f).any()  # the bias column is never produced
    out = np.zeros((n, k * (f + 1)), dtype=np.float64)
    out[:, c] = phi.cpu().numpy()
    return out.reshape(n, k, f + 1).astype(np.float32)


def _host(bst, X, t_begin=0, t_end=None):
    want = torch_ref.tree_shap(
        bst._cpu_flat_forest(), torch.as_tensor(X, dtype=torch.float32), bst.n_outputs,
        t_begin, t_end,
    )
    return want.to(torch.float32).numpy()


def _check_dense(bst, X, t_begin=0, t_end=None, want=None):
    """Direct compact-kernel call on dense rows vs the host path."""
    _, dev = _flats(bst)
    k = bst.n_outputs
    n, f = X.shape
    Xd = torch.as_tensor(X, dtype=torch.float32).cuda()
    phi, cols = hip.tree_shap_compact(dev, Xd, k, t_begin, t_end)
    got = _scatter(phi, cols, n, k, f)
    want = _host(bst, X, t_begin, t_end) if want is None else want
    np.testing.assert_allclose(got, want, rtol=_RTOL, atol=_ATOL)
    return phi, cols


def _plan(bst, n, f, t_begin=0, t_end=None):
    _, dev = _flats(bst)
    t_end = dev["n_trees"] if t_end is None else t_end
    return hip.shap_compact_plan(dev["shap_paths"], f, t_begin, t_end, n)


@pytest.fixture(scope="module")
def depth3():
    return _train("reg:squarederror", n=400, f=4, depth=3, rounds=3)


@pytest.fixture(scope="module")
def depth5():
    return _train("binary:logistic", n=600, f=8, depth=5, rounds=3, nan_frac=0.2)


@pytest.fixture(scope="module")
def wide3():
    """3 classes x 40 columns: k * (f + 1) = 123 cells > 96 at W = 4."""
    return _train("multi:softprob", n=400, f=40, depth=3, rounds=3, num_class=3)


class TestDenseAccessorMatchesHost:
    def test_depth3_group_exactly_full(self, depth3):
        bst, X = depth3
        _, dev = _flats(bst)
        assert hip.shap_limits(dev["shap_paths"], 1, 4, 0, 3)[0] == 4  # W = 4, no idle lane
        _check_dense(bst, X[:67])  # 67: not a multiple of the groups per block

    def test_depth3_brute_force(self, depth3):
        bst, X = depth3
        oracle = _load("_treeshap_oracle", "test_treeshap.py")
        _, dev = _flats(bst)
        rows = X[:4]
        phi, cols = hip.tree_shap_compact(dev, torch.as_tensor(rows).cuda(), 1)
        got = _scatter(phi, cols, 4, 1, 4)[:, 0, :4]
        for r in range(4):
            expected = oracle._brute_shap(bst.trees, rows[r], 4)
            np.testing.assert_allclose(got[r], expected[:4], rtol=1e-4, atol=1e-5)

    def test_brute_force_with_missing_values(self):
        bst, X = _train("binary:logistic", n=400, f=4, depth=3, rounds=2, nan_frac=0.15)
        oracle = _load("_treeshap_oracle", "test_treeshap.py")
        _, dev = _flats(bst)
        rows = X[:4]
        phi, cols = hip.tree_shap_compact(dev, torch.as_tensor(rows).cuda(), 1)
        got = _scatter(phi, cols, 4, 1, 4)[:, 0, :4]
        for r in range(4):
            expected = oracle._brute_shap(bst.trees, rows[r], 4)
            np.testing.assert_allclose(got[r], expected[:4], rtol=1e-4, atol=1e-5)

    @pytest.mark.parametrize("rows", [67, 1])
    def test_depth5_missing_values(self, depth5, rows):
        bst, X = depth5
        _, dev = _flats(bst)
        assert hip.shap_limits(dev["shap_paths"], 1, 8, 0, 3)[0] == 6  # W = 8, idle lanes
        _check_dense(bst, X[:rows])

    def test_two_features_depth4_merged_paths(self):
        bst, X = _train("binary:logistic", n=500, f=2, depth=4, rounds=3, nan_frac=0.2)
        assert max(t.max_depth() for t in bst.trees) == 4
        _check_dense(bst, X[:80])

    def test_dart_weight_drop(self):
        bst, X = _train("reg:squarederror", n=300, f=5, depth=3, rounds=6, booster="dart",
                        rate_drop=0.5, one_drop=1)
        assert any(w != 1.0 for w in bst.weight_drop)
        _check_dense(bst, X[:40])

    def test_tree_range(self):
        bst, X = _train("reg:squarederror", n=300, f=5, depth=3, rounds=5)
        _check_dense(bst, X[:30], 1, 3)

    def test_nan_and_infinite_rows(self, depth5):
        bst, X = depth5
        rows = X[:40].copy()
        rows[0, :] = np.nan
        rows[1, ::2] = np.inf
        rows[1, 1::2] = -np.inf
        rows[2, :] = np.inf
        rows[3, :] = -np.inf
        _check_dense(bst, rows)

    def test_empty_inputs_launch_nothing(self, depth3):
        bst, X = depth3
        _, dev = _flats(bst)
        Xd = torch.as_tensor(X[:5]).cuda()
        phi, cols = hip.tree_shap_compact(dev, Xd[:0], 1)
        assert phi.shape == (0, cols.shape[0])
        phi, cols = hip.tree_shap_compact(dev, Xd, 1, 2, 2)  # empty tree range
        assert phi.shape == (5, 0) and cols.shape == (0,)
        stumps, Xs = _train("reg:squarederror", n=200, f=4, depth=3, rounds=3, gamma=1e9)
        assert all(t.num_nodes == 1 for t in stumps.trees)
        phi, cols = hip.tree_shap_compact(_flats(stumps)[1], torch.as_tensor(Xs[:5]).cuda(), 1)
        assert phi.shape == (5, 0) and cols.shape == (0,)


class TestBeyondTheSlabLimit:
    def test_dense_slab_kernel_refuses_compact_matches_host(self, wide3):
        bst, X = wide3
        _, dev = _flats(bst)
        L, _, fits = hip.shap_limits(dev["shap_paths"], 3, 40, 0, dev["n_trees"])
        assert L == 4 and 3 * 41 == 123 > hip.SHAP_LDS_BUDGET // (8 * 64)
        assert fits is False
        rows = X[:67]
        with pytest.raises(ValueError):
            hip.tree_shap(dev, torch.as_tensor(rows).cuda(), 3)
        _check_dense(bst, rows)


class TestChunkEdges:
    _F = 30  # wide enough that chunks of 1, 2 and 3 trees need different slabs

    @pytest.fixture(scope="class")
    def many(self):
        bst, X = _train("reg:squarederror", n=300, f=self._F, depth=3, rounds=41)
        return bst, X, _host(bst, X[:67])

    def _sizes(self, bst):
        from sagemaker_xgboost_container_amd.ops import shap_paths

        host = _flats(bst)[1]["shap_paths"]["host"]
        return {
            t: shap_paths.make_shap_slots(host, self._F, 0, 41, t)["max_slots"]
            for t in range(1, 42)
        }

    def test_many_chunks_few_rows(self, many):
        bst, X, want = many
        assert _plan(bst, 3, self._F) == (1, 256)  # 41 chunks of one tree
        _check_dense(bst, X[:3], want=want[:3])

    @pytest.mark.parametrize("tpc", [1, 2])
    def test_lds_budget_sets_trees_per_chunk(self, many, tpc, monkeypatch):
        bst, X, want = many
        sizes = self._sizes(bst)
        # the budget holds chunks of `tpc` trees and no larger chunking
        cap = sizes[tpc]
        assert max(t for t, s in sizes.items() if s <= cap) == tpc
        monkeypatch.setattr(hip, "SHAP_LDS_BUDGET", (256 // 4) * cap * 8)
        monkeypatch.setattr(hip, "_SHAP_TARGET_GROUPS", 1)  # occupancy wants one chunk
        bst._predict_cache = None
        assert _plan(bst, 67, self._F) == (tpc, 256)  # tpc = 2: a short last chunk of 1 tree
        _check_dense(bst, X[:67], want=want)
        bst._predict_cache = None

    def test_one_wave_block(self, many, monkeypatch):
        bst, X, want = many
        one_tree = self._sizes(bst)[1]
        monkeypatch.setattr(hip, "SHAP_LDS_BUDGET", (64 // 4) * one_tree * 8)
        bst._predict_cache = None
        tpc, block = _plan(bst, 67, self._F)
        assert block == 64
        _check_dense(bst, X[:67], want=want)
        bst._predict_cache = None

    def test_chunk_of_stumps_between_split_trees(self, monkeypatch):
        bst, X = _train("reg:squarederror", n=300, f=6, depth=3, rounds=6)
        for t in (2, 3):
            stump = Tree()
            stump.add_node(value=0.25 * t, sum_hess=10.0)
            bst.trees[t] = stump.finalize()
        bst._predict_cache = None
        # 40 rows, 120 wanted items: 3 chunks of 2 trees, the middle one all stumps
        monkeypatch.setattr(hip, "_SHAP_TARGET_GROUPS", 120)
        assert _plan(bst, 40, 6) == (2, 256)
        from sagemaker_xgboost_container_amd.ops import shap_paths

        tabs = shap_paths.make_shap_slots(_flats(bst)[1]["shap_paths"]["host"], 6, 0, 6, 2)
        sizes = np.diff(tabs["chunk_slot_ptr"]).tolist()
        assert sizes[1] == 0 and sizes[0] > 0 and sizes[2] > 0
        _check_dense(bst, X[:40])

    def test_row_tiling_under_partial_cap(self, depth3, monkeypatch):
        bst, X = depth3
        _, dev = _flats(bst)
        cols, tiles = hip.tree_shap_compact_tiles(dev, torch.as_tensor(X[:67]).cuda(), 1)
        S = None
        for key, tabs in dev["shap_slot_cache"].items():
            if key[0] == "slots":
                S = tabs["S"]
        assert S
        list(tiles)
        monkeypatch.setattr(hip, "SHAP_PARTIAL_CAP", 25 * S * 8)  # 25 rows of partials
        _, tiles = hip.tree_shap_compact_tiles(dev, torch.as_tensor(X[:67]).cuda(), 1)
        assert [(r0, r1) for r0, r1, _ in tiles] == [(0, 25), (25, 50), (50, 67)]
        _check_dense(bst, X[:67])


def _edge_csr():
    """300 x 70 at ~20 %: an empty row, a full row, rows whose only entry is
    column 0 or column 69, stored zeros and stored NaNs; values in eighths."""
    rng = np.random.default_rng(7)
    n, f = 300, 70
    mask = rng.random(size=(n, f)) < 0.2
    mask[0, :] = False          # empty row
    mask[1, :] = True           # completely full row
    mask[2, :] = False
    mask[2, 0] = True           # only column 0
    mask[3, :] = False
    mask[3, 69] = True          # only column 69
    rows, cols = np.nonzero(mask)
    vals = (np.round(rng.normal(size=rows.size) * 8) / 8).astype(np.float32)
    vals[::7] = 0.0
    vals[3::11] = np.nan
    vals[5::13] = np.inf
    vals[6::17] = -np.inf
    csr = sp.csr_matrix((vals, (rows, cols)), shape=(n, f), dtype=np.float32)
    assert csr.nnz == rows.size and np.isnan(csr.data).any() and (csr.data == 0).any()
    return csr


def _wide_csr(pool):
    """64 x 20000 at ~0.1 %, columns drawn half from the split-feature pool so
    lookups hit; row 5 stores 3000 entries (deeper search than its wave's
    other lanes); columns 0 and 19999 are stored in some rows."""
    rng = np.random.default_rng(11)
    n, f = 64, 20000
    rows, cols = [], []
    for r in range(n):
        m = 3400 if r == 5 else 20
        c = np.unique(np.concatenate([
            rng.choice(pool, size=min(len(pool), 10), replace=False),
            rng.integers(0, f, size=m),
        ]))
        rows.append(np.full(c.size, r))
        cols.append(c)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    vals = (np.round(rng.normal(size=rows.size) * 8) / 8).astype(np.float32)
    vals[::9] = 0.0
    vals[4::23] = np.nan
    csr = sp.csr_matrix((vals, (rows, cols)), shape=(n, f), dtype=np.float32)
    assert np.diff(csr.indptr)[5] >= 3000
    assert (csr.indices == 0).any() and (csr.indices == f - 1).any()
    return csr


def _check_csr(bst, csr, t_begin=0, t_end=None):
    """CSR accessor: bit-equal to the dense accessor on the NaN twin, and
    within tolerance of the host path."""
    _, dev = _flats(bst)
    k = bst.n_outputs
    twin = _dense_twin(csr)
    dcsr = hip_sparse.DeviceCSR(csr, torch.device("cuda"))
    phi_s, cols_s = hip.tree_shap_compact(dev, dcsr, k, t_begin, t_end)
    phi_d, cols_d = _check_dense(bst, twin, t_begin, t_end)
    assert np.array_equal(cols_s.cpu().numpy(), cols_d.cpu().numpy())
    assert np.array_equal(phi_s.cpu().numpy(), phi_d.cpu().numpy())
    return dcsr, phi_s, cols_s


class TestCsrAccessor:
    def test_edge_rows_bit_equal_to_dense(self):
        csr = _edge_csr()
        bst = _cover_booster(70, 6, np.arange(70), depth=5, seed=3, roots=[0, 69])
        _check_csr(bst, csr)

    def test_edge_rows_multiclass_tree_range(self):
        csr = _edge_csr()
        bst = _cover_booster(70, 4, np.arange(70), depth=4, k=3, seed=4)
        _check_csr(bst, csr, 3, 9)

    def test_wide_matrix_and_int64_offsets(self):
        f = 20000
        pool = np.unique(np.concatenate(
            [[0, f - 1], np.random.default_rng(5).integers(0, f, size=38)]))
        csr = _wide_csr(pool)
        bst = _cover_booster(f, 12, pool, depth=5, seed=6, roots=[0, f - 1])
        split_feats = np.concatenate([t.feature[t.left >= 0] for t in bst.trees])
        assert 0 in split_feats and f - 1 in split_feats
        dcsr, phi, cols = _check_csr(bst, csr)
        assert dcsr.indptr.dtype == torch.int64
        # a row slice keeps the parent's index buffers: its offsets start past
        # zero and must be honoured as they are
        sl = object.__new__(hip_sparse.DeviceCSR)
        sl.shape = (24, f)
        sl.indptr = dcsr.indptr[5:30]
        sl.indices = dcsr.indices
        sl.data = dcsr.data
        assert int(sl.indptr[0]) > 0
        phi_sl, cols_sl = hip.tree_shap_compact(_flats(bst)[1], sl, 1)
        assert np.array_equal(cols_sl.cpu().numpy(), cols.cpu().numpy())
        assert np.array_equal(phi_sl.cpu().numpy(), phi[5:29].cpu().numpy())


class TestDeterminism:
    def test_repeated_calls_bit_identical(self, depth5):
        bst, X = depth5
        _, dev = _flats(bst)
        Xd = torch.as_tensor(X[:64]).cuda()
        d = [hip.tree_shap_compact(dev, Xd, 1)[0].cpu().numpy() for _ in range(3)]
        assert np.array_equal(d[0], d[1]) and np.array_equal(d[0], d[2])

    def test_repeated_calls_bit_identical_csr(self):
        csr = _edge_csr()
        bst = _cover_booster(70, 6, np.arange(70), depth=5, seed=3)
        _, dev = _flats(bst)
        dcsr = hip_sparse.DeviceCSR(csr, torch.device("cuda"))
        s = [hip.tree_shap_compact(dev, dcsr, 1)[0].cpu().numpy() for _ in range(3)]
        assert np.array_equal(s[0], s[1]) and np.array_equal(s[0], s[2])


class TestValidation:
    def test_bad_requests_raise_before_any_launch(self, depth3, monkeypatch):
        bst, X = depth3
        _, dev = _flats(bst)

        def _launched(*a, **kw):
            raise AssertionError("a kernel was launched for an invalid request")

        monkeypatch.setattr(hip._K, "tree_shap_compact", _launched, raising=False)
        max_f = int(dev["shap_paths"]["tree_max_feature"].max())
        Xd = torch.as_tensor(X[:5]).cuda()
        with pytest.raises(ValueError):  # narrower than the largest split feature
            hip.tree_shap_compact(dev, Xd[:, :max_f].contiguous(), 1)
        csr = sp.csr_matrix(np.nan_to_num(X[:5, :max_f]))
        with pytest.raises(ValueError):
            hip.tree_shap_compact(dev, hip_sparse.DeviceCSR(csr, torch.device("cuda")), 1)
        with pytest.raises(ValueError):  # host tensors
            hip.tree_shap_compact(dev, torch.as_tensor(X[:5]), 1)
        with pytest.raises(ValueError):  # wrong dtype
            hip.tree_shap_compact(dev, Xd.double(), 1)
        with pytest.raises(ValueError):
            hip.tree_shap_compact(dev, X[:5], 1)
        bad = hip_sparse.DeviceCSR(sp.csr_matrix(np.nan_to_num(X[:5])), torch.device("cuda"))
        bad.indices = bad.indices.to(torch.int64)
        with pytest.raises(ValueError):
            hip.tree_shap_compact(dev, bad, 1)
        bad = hip_sparse.DeviceCSR(sp.csr_matrix(np.nan_to_num(X[:5])), torch.device("cuda"))
        bad.indptr = bad.indptr + 1  # the last offset leaves the index buffer
        with pytest.raises(ValueError):
            hip.tree_shap_compact(dev, bad, 1)
        for t_begin, t_end in ((2, 1), (-1, 2), (0, 4)):  # bad tree ranges
            with pytest.raises(ValueError):
                hip.tree_shap_compact(dev, Xd, 1, t_begin, t_end)


def _forbid_host(monkeypatch):
    def _no_dense(self):
        raise AssertionError("DMatrix.to_dense() called on the sparse explain route")

    def _no_host(*a, **kw):
        raise AssertionError("host TreeSHAP served a device request")

    monkeypatch.setattr(DMatrix, "to_dense", _no_dense)
    monkeypatch.setattr(torch_ref, "tree_shap", _no_host)


@pytest.fixture()
def _no_env(monkeypatch):
    for name in ("SMXGB_SPARSE_EXPLAIN", "SMXGB_SPARSE_PREDICT", "SMXGB_SHAP_COMPACT"):
        monkeypatch.delenv(name, raising=False)


@pytest.mark.usefixtures("_no_env")
class TestBoosterRoute:
    @pytest.mark.parametrize("k", [1, 3])
    def test_sparse_dmatrix_served_over_csr(self, k, monkeypatch):
        csr = _edge_csr()
        n, f = csr.shape
        twin = _dense_twin(csr)
        bst = _cover_booster(f, 4, np.arange(f), depth=4, k=k, seed=8 + k)
        bm = np.random.default_rng(9).normal(size=(n, k)).astype(np.float32)
        bm = bm[:, 0] if k == 1 else bm

        # references first: cpu_predictor on the dense twin (host recursion)
        bst.set_param("predictor", "cpu_predictor")
        want = bst.predict(DMatrix(twin), pred_contribs=True)
        want_bm = bst.predict(DMatrix(twin, base_margin=bm), pred_contribs=True)
        want_rng = bst.predict(DMatrix(twin), pred_contribs=True, iteration_range=(1, 3))
        margin = bst.predict(DMatrix(twin), output_margin=True)
        margin_bm = bst.predict(DMatrix(twin, base_margin=bm), output_margin=True)
        bst.set_param("predictor", None)
        inter = bst.predict(DMatrix(twin[:20]), pred_interactions=True)
        approx_dev = bst.predict(DMatrix(twin), pred_contribs=True, approx_contribs=True)

        monkeypatch.setenv("SMXGB_SPARSE_EXPLAIN", "1")
        with monkeypatch.context() as m:
            _forbid_host(m)
            got = bst.predict(DMatrix(csr), pred_contribs=True)
            got_bm = bst.predict(DMatrix(csr, base_margin=bm), pred_contribs=True)
            got_rng = bst.predict(DMatrix(csr), pred_contribs=True, iteration_range=(1, 3))
        assert got.dtype == np.float32 and got.shape == want.shape
        np.testing.assert_allclose(got, want, rtol=_RTOL, atol=_ATOL)
        np.testing.assert_allclose(got_bm, want_bm, rtol=_RTOL, atol=_ATOL)
        np.testing.assert_allclose(got_rng, want_rng, rtol=_RTOL, atol=_ATOL)
        # additivity: rows sum to the margin
        np.testing.assert_allclose(got.sum(axis=-1), margin, rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(got_bm.sum(axis=-1), margin_bm, rtol=1e-5, atol=1e-5)
        # the other explanation outputs keep their densifying paths, exactly
        assert np.array_equal(
            bst.predict(DMatrix(csr), pred_contribs=True, approx_contribs=True), approx_dev)
        assert np.array_equal(
            bst.predict(DMatrix(csr[:20]), pred_interactions=True), inter)

    def test_dense_model_beyond_the_slab_served_by_compact(self, wide3, monkeypatch):
        bst, X = wide3
        rows = X[:67]
        bst.set_param("predictor", "cpu_predictor")
        want = bst.predict(rows, pred_contribs=True)
        bst.set_param("predictor", None)

        def _no_host(*a, **kw):
            raise AssertionError("host TreeSHAP served a device request")

        monkeypatch.setattr(torch_ref, "tree_shap", _no_host)
        got = bst.predict(rows, pred_contribs=True)
        np.testing.assert_allclose(got, want, rtol=_RTOL, atol=_ATOL)
        margin = bst.predict(rows, output_margin=True)
        np.testing.assert_allclose(got.sum(axis=-1), margin, rtol=1e-5, atol=1e-5)

    def test_knob_forces_and_forbids_compact_on_dense(self, depth5, monkeypatch):
        bst, X = depth5
        rows = X[:50]
        base = bst.predict(rows, pred_contribs=True)  # dense-slab kernel
        calls = []
        real = hip.tree_shap_compact_tiles
        monkeypatch.setattr(hip, "tree_shap_compact_tiles",
                            lambda *a, **kw: calls.append(1) or real(*a, **kw))
        monkeypatch.setenv("SMXGB_SHAP_COMPACT", "1")
        forced = bst.predict(rows, pred_contribs=True)
        assert calls
        np.testing.assert_allclose(forced, base, rtol=_RTOL, atol=_ATOL)
        del calls[:]
        monkeypatch.setenv("SMXGB_SHAP_COMPACT", "0")
        assert np.array_equal(bst.predict(rows, pred_contribs=True), base)
        assert not calls


def _device_bytes(obj, seen=None):
    """Bytes of every distinct device tensor reachable through dicts/lists."""
    seen = set() if seen is None else seen
    if isinstance(obj, torch.Tensor):
        if obj.is_cuda and obj.data_ptr() not in seen:
            seen.add(obj.data_ptr())
            return obj.numel() * obj.element_size()
        return 0
    if isinstance(obj, dict):
        return sum(_device_bytes(v, seen) for v in obj.values())
    if isinstance(obj, (list, tuple)):
        return sum(_device_bytes(v, seen) for v in obj)
    return 0


@pytest.mark.usefixtures("_no_env")
class TestMemory:
    def test_wide_sparse_contribs_never_hold_the_dense_image(self, monkeypatch):
        """A condition, not a measurement: the peak device memory of the
        request stays under a bound computed from the actual arrays, and
        that bound is itself below the dense image."""
        n, f = 4000, 20000
        rng = np.random.default_rng(1)
        pool = np.unique(rng.integers(0, f, size=400))
        nnz = n * f // 1000
        csr = sp.coo_matrix(
            (np.round(rng.normal(size=nnz) * 8).astype(np.float32) / 8,
             (rng.integers(0, n, nnz), rng.choice(pool, size=nnz))),
            shape=(n, f),
        ).tocsr()
        csr.sum_duplicates()
        assert csr.has_canonical_format
        dense_image = n * f * 4
        assert dense_image > booster_mod.SPARSE_PREDICT_DENSE_BUDGET  # 320 MB > 256 MiB
        bst = _cover_booster(f, 50, pool, depth=5, seed=2, full=True)
        cap = 32 << 20
        monkeypatch.setattr(hip, "SHAP_PARTIAL_CAP", cap)

        dense_calls = []
        real_to_dense = DMatrix.to_dense
        monkeypatch.setattr(
            DMatrix, "to_dense", lambda self: dense_calls.append(1) or real_to_dense(self))
        d = DMatrix(csr)
        assert bst._sparse_explain_route(d)  # the automatic rule, no knob set

        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        held = torch.cuda.memory_allocated()  # the forest, other tests' fixtures
        torch.cuda.reset_peak_memory_stats()
        out = bst.predict(d, pred_contribs=True)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
        print(f"allocated before the request: {held}")
        assert not dense_calls
        assert out.shape == (n, f + 1) and np.isfinite(out).all()
        margin = bst.predict(d, output_margin=True)
        np.testing.assert_allclose(out.sum(axis=-1), margin, rtol=1e-5, atol=1e-5)

        csr_bytes = csr.indptr.size * 8 + csr.indices.size * 4 + csr.data.size * 4
        tables = _device_bytes(bst._predict_cache)
        slots = [t for key, t in bst._predict_cache["shap_slots:cuda"].items()
                 if key[0] == "slots"]
        assert len(slots) == 1
        S, U = slots[0]["S"], slots[0]["cols"].shape[0]
        rows_per_tile = max(1, min(n, cap // (S * 8)))
        assert rows_per_tile < n  # more than one row tile
        bound = csr_bytes + 2 * cap + rows_per_tile * U * 8 + tables + (8 << 20)
        print(f"peak {peak} bound {bound} dense image {dense_image} S {S} U {U}")
        assert peak <= bound
        assert bound < dense_image
