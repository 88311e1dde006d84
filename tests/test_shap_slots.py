"""Slot tables of the compact TreeSHAP kernel (ops/shap_paths.py
make_shap_slots), the trees_per_chunk chooser (ops/hip.py shap_compact_plan)
and the sparse explain route of the Booster, all on the host.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from sagemaker_xgboost_container_amd.data.dmatrix import DMatrix
from sagemaker_xgboost_container_amd.models import trainer
from sagemaker_xgboost_container_amd.ops import hip, shap_paths

_F = 6
_K = 3


def _train(**extra):
    rng = np.random.default_rng(0)
    X = rng.normal(size=(300, _F)).astype(np.float32)
    signal = sum((1.0 + 0.3 * j) * X[:, j] * (1 if j % 2 == 0 else -1) for j in range(_F))
    y = np.digitize(signal, np.quantile(signal, [1 / 3, 2 / 3])).astype(np.float32)
    params = {"objective": "multi:softprob", "num_class": _K, "max_depth": 3, "eta": 0.4,
              "device": "cpu"}
    params.update(extra)
    return trainer.train(params, DMatrix(X, label=y), num_boost_round=5, verbose_eval=False)


@pytest.fixture(scope="module")
def bst():
    return _train()


@pytest.fixture(scope="module")
def paths(bst):
    wd = None
    return shap_paths.make_shap_paths(bst.trees, bst.tree_info, wd)


def _elements(paths, t_begin, t_end):
    """(element id, tree, dense output column) of every path element of the range."""
    out = []
    for p in range(paths["tree_path_ptr"][t_begin], paths["tree_path_ptr"][t_end]):
        for e in range(paths["path_offset"][p], paths["path_offset"][p + 1]):
            col = int(paths["path_cls"][p]) * (_F + 1) + int(paths["elem_feature"][e])
            out.append((e, int(paths["path_tree"][p]), col))
    return out


@pytest.mark.parametrize(
    "t_begin,t_end,tpc",
    [(0, 15, 1), (0, 15, 2), (0, 15, 4), (0, 15, 15), (3, 11, 3)],
)
def test_table_invariants(bst, paths, t_begin, t_end, tpc):
    assert len(bst.trees) == 15
    tabs = shap_paths.make_shap_slots(paths, _F, t_begin, t_end, tpc)
    elems = _elements(paths, t_begin, t_end)
    assert elems, "the model must split"
    C = -(-(t_end - t_begin) // tpc)
    ptr = tabs["chunk_slot_ptr"]
    assert tabs["n_chunks"] == C and ptr.shape == (C + 1,) and ptr[0] == 0
    S = int(ptr[-1])
    sizes = np.diff(ptr)
    assert (sizes >= 0).all()
    assert tabs["slot_col"].shape == (S,)
    assert tabs["elem_slot"].dtype == np.int32
    assert tabs["elem_slot"].shape == (len(elems),)
    assert tabs["elem_base"] == elems[0][0]
    # S is at most the number of split nodes of the range
    n_split = sum(int((bst.trees[t].left >= 0).sum()) for t in range(t_begin, t_end))
    assert S <= n_split

    pairs_of_chunk = [set() for _ in range(C)]
    slots_of_chunk = [dict() for _ in range(C)]
    for e, tree, col in elems:
        c = (tree - t_begin) // tpc
        slot = int(tabs["elem_slot"][e - tabs["elem_base"]])
        assert 0 <= slot < sizes[c]
        assert tabs["slot_col"][ptr[c] + slot] == col
        pairs_of_chunk[c].add(col)
        # distinct pairs get distinct slots, one pair always the same slot
        assert slots_of_chunk[c].setdefault(slot, col) == col
    for c in range(C):
        assert len(pairs_of_chunk[c]) == sizes[c] == len(slots_of_chunk[c])
        # pairs are unique within a chunk
        chunk_cols = tabs["slot_col"][ptr[c]:ptr[c + 1]]
        assert len(set(chunk_cols.tolist())) == chunk_cols.shape[0]
    assert tabs["max_slots"] == max(len(s) for s in pairs_of_chunk)

    cols = tabs["cols"]
    assert cols.dtype == np.int64
    assert (np.diff(cols) > 0).all()  # sorted and unique
    assert set(cols.tolist()) == set(tabs["slot_col"].tolist())
    col_ptr, col_slots = tabs["col_ptr"], tabs["col_slots"]
    assert col_ptr.shape == (cols.shape[0] + 1,) and col_ptr[0] == 0 and col_ptr[-1] == S
    slot_chunk = np.repeat(np.arange(C), sizes)
    for j, col in enumerate(cols):
        mine = col_slots[col_ptr[j]:col_ptr[j + 1]]
        assert mine.size > 0
        assert (tabs["slot_col"][mine] == col).all()
        assert (np.diff(slot_chunk[mine]) > 0).all()  # ascending chunks, one slot each
    # together the columns cover the ragged axis exactly once
    assert sorted(col_slots.tolist()) == list(range(S))


def test_single_chunk_slots_are_the_distinct_columns(paths):
    tabs = shap_paths.make_shap_slots(paths, _F, 0, 15, 15)
    assert tabs["n_chunks"] == 1
    assert np.array_equal(tabs["slot_col"], tabs["cols"])
    assert tabs["max_slots"] == tabs["cols"].shape[0]


def test_all_stump_forest_has_no_slots():
    stumps = _train(gamma=1e9)
    assert all(t.num_nodes == 1 for t in stumps.trees)
    paths = shap_paths.make_shap_paths(stumps.trees, stumps.tree_info, None)
    tabs = shap_paths.make_shap_slots(paths, _F, 0, len(stumps.trees), 4)
    assert tabs["slot_col"].shape == (0,) and tabs["cols"].shape == (0,)
    assert tabs["elem_slot"].shape == (0,) and tabs["max_slots"] == 0
    assert tabs["chunk_slot_ptr"].tolist() == [0] * (tabs["n_chunks"] + 1)
    assert tabs["col_ptr"].tolist() == [0]


def test_empty_range_and_bad_arguments(paths):
    tabs = shap_paths.make_shap_slots(paths, _F, 4, 4, 2)
    assert tabs["n_chunks"] == 0 and tabs["chunk_slot_ptr"].tolist() == [0]
    with pytest.raises(ValueError):
        shap_paths.make_shap_slots(paths, _F, 0, 16, 2)
    with pytest.raises(ValueError):
        shap_paths.make_shap_slots(paths, _F, 0, 15, 0)


class TestChooser:
    def _max_slots(self, paths, tpc):
        return shap_paths.make_shap_slots(paths, _F, 0, 15, tpc)["max_slots"]

    def test_unconstrained_takes_what_occupancy_wants(self, paths):
        # 3 rows: one tree per chunk already gives fewer items than wanted
        assert hip.shap_compact_plan(paths, _F, 0, 15, 3) == (1, 256)
        # many rows: a single chunk of all 15 trees
        assert hip.shap_compact_plan(paths, _F, 0, 15, 1 << 20) == (15, 256)

    def test_largest_fitting_trees_per_chunk(self, paths, monkeypatch):
        L, _ = shap_paths.range_limits(paths, 0, 15)
        gpb = 256 // hip.shap_group_width(L)
        sizes = {tpc: self._max_slots(paths, tpc) for tpc in range(1, 16)}
        assert sizes[1] < sizes[15]
        # a budget that holds every chunking up to some tpc but not all 15 trees
        for cap in sorted(set(sizes.values()))[:-1]:
            monkeypatch.setattr(hip, "SHAP_LDS_BUDGET", gpb * cap * 8)
            want = max(tpc for tpc, s in sizes.items() if s <= cap)
            assert hip.shap_compact_plan(paths, _F, 0, 15, 1 << 20) == (want, 256)

    def test_one_wave_block_then_does_not_fit(self, paths, monkeypatch):
        L, _ = shap_paths.range_limits(paths, 0, 15)
        W = hip.shap_group_width(L)
        one_tree = self._max_slots(paths, 1)
        # one tree fits 64 / W groups but not 256 / W
        monkeypatch.setattr(hip, "SHAP_LDS_BUDGET", (64 // W) * one_tree * 8)
        tpc, block = hip.shap_compact_plan(paths, _F, 0, 15, 1 << 20)
        assert block == 64 and tpc >= 1
        assert (64 // W) * self._max_slots(paths, tpc) * 8 <= hip.SHAP_LDS_BUDGET
        # not even one tree in a one-wave block
        monkeypatch.setattr(hip, "SHAP_LDS_BUDGET", (64 // W) * one_tree * 8 - 1)
        assert hip.shap_compact_plan(paths, _F, 0, 15, 1 << 20) is None


class TestSparseExplainRoute:
    @pytest.fixture()
    def dsparse(self):
        rng = np.random.default_rng(2)
        dense = rng.normal(size=(40, _F)).astype(np.float32)
        dense[rng.random(size=dense.shape) < 0.5] = 0.0
        return DMatrix(sp.csr_matrix(dense))

    @pytest.fixture(autouse=True)
    def _no_env(self, monkeypatch):
        monkeypatch.delenv("SMXGB_SPARSE_EXPLAIN", raising=False)
        monkeypatch.delenv("SMXGB_SPARSE_PREDICT", raising=False)

    @staticmethod
    def _pretend_hip(bst, monkeypatch):
        """Make the route believe it predicts on a hip device, with the
        device-side fit check answered on the host."""
        import torch

        monkeypatch.setattr(type(bst), "_predict_device", lambda self: torch.device("cuda"))
        monkeypatch.setattr(
            type(bst), "_compact_explain_flat", lambda self, device, n, f, t0, t1: {}
        )

    def test_off_on_a_cpu_device_even_when_forced(self, bst, dsparse, monkeypatch):
        monkeypatch.setenv("SMXGB_SPARSE_EXPLAIN", "1")
        cpu_bst = bst.copy()
        cpu_bst.params["predictor"] = "cpu_predictor"
        assert not cpu_bst._sparse_explain_route(dsparse)

    def test_follows_its_own_knob(self, bst, dsparse, monkeypatch):
        self._pretend_hip(bst, monkeypatch)
        assert not bst._sparse_explain_route(dsparse)  # 40 x 6: far below the budget
        monkeypatch.setenv("SMXGB_SPARSE_EXPLAIN", "1")
        assert bst._sparse_explain_route(dsparse)
        assert not bst._sparse_explain_route(dsparse, approx_contribs=True)
        assert not bst._sparse_explain_route(dsparse, pred_interactions=True)
        # the predict route's answer for explanations is pinned and independent
        assert bst._sparse_predict_route(dsparse, explain=True) is False
        monkeypatch.setenv("SMXGB_SPARSE_PREDICT", "1")
        assert bst._sparse_predict_route(dsparse, explain=True) is False
        monkeypatch.setenv("SMXGB_SPARSE_PREDICT", "0")
        assert bst._sparse_explain_route(dsparse)
        monkeypatch.setenv("SMXGB_SPARSE_EXPLAIN", "0")
        assert not bst._sparse_explain_route(dsparse)

    def test_off_for_dense_input_and_non_canonical_csr(self, bst, dsparse, monkeypatch):
        self._pretend_hip(bst, monkeypatch)
        monkeypatch.setenv("SMXGB_SPARSE_EXPLAIN", "1")
        assert not bst._sparse_explain_route(DMatrix(np.zeros((4, _F), dtype=np.float32)))
        # a duplicate column id in a row: last-duplicate-wins cannot be searched
        dup = sp.csr_matrix(
            (np.ones(3, dtype=np.float32), np.array([0, 0, 2]), np.array([0, 3, 3])),
            shape=(2, _F),
        )
        assert not dup.has_canonical_format
        assert not bst._sparse_explain_route(DMatrix(dup))

    def test_automatic_rule_is_the_memory_rule(self, monkeypatch):
        from sagemaker_xgboost_container_amd.models import booster as booster_mod
        from sagemaker_xgboost_container_amd.models.booster import Booster
        from sagemaker_xgboost_container_amd.models.tree import Tree

        f = 20000
        tree = Tree()
        root = tree.add_node(value=0.0, sum_hess=2.0)
        tree.apply_split(root, f - 1, 0.5, 0, True, 1.0, left_value=-1.0, right_value=1.0,
                         left_hess=1.0, right_hess=1.0)
        wide = Booster({"objective": "binary:logistic"}, num_features=f)
        wide.add_iteration([tree.finalize()], [0])
        self._pretend_hip(wide, monkeypatch)

        def _wide(n):
            rng = np.random.default_rng(1)
            nnz = n * f // 1000
            return DMatrix(sp.coo_matrix(
                (np.ones(nnz, dtype=np.float32), (rng.integers(0, n, nnz), rng.integers(0, f, nnz))),
                shape=(n, f),
            ).tocsr())

        assert 4000 * f * 4 > booster_mod.SPARSE_PREDICT_DENSE_BUDGET
        assert wide._sparse_explain_route(_wide(4000))
        assert not wide._sparse_explain_route(_wide(1000))  # 80 MB image
