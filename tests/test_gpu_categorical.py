"""Categorical splits on the device: the category-set split scan, the
per-level partition kernels, the forest traversal and training end to end,
each against the host reference."""
import types

import numpy as np
import pytest
import torch

from categorical_oracle import gap, hist_from_rows, node_candidates

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    from sagemaker_xgboost_container_amd.ops import hip as _hip

    return _hip


# -- 9. split_scan_cat_kernel -------------------------------------------------
# two numeric features (7 and 256 bins) and three categorical ones: 3
# categories (one-hot mode at the default max_cat_to_onehot = 4), 17 (a
# partial block) and 255 (a full block)
NBINS = [7, 256, 3, 17, 255]
IS_CAT = [False, False, True, True, True]
K_NODES = 3


def _split_case(has_missing, seed):
    """Integer-valued histograms of K_NODES nodes built from rows, so every
    feature sums to the node's parent and float32 sums are exact; small
    integers give empty categories and exact ratio ties (1/2 and 2/4)."""
    rng = np.random.default_rng(seed)
    f = len(NBINS)
    stride = max(NBINS) + (1 if has_missing else 0)
    hists, parents = [], []
    for node in range(K_NODES):
        n = 1500 + 400 * node
        codes = np.stack([rng.integers(0, nb, n) for nb in NBINS], 1)
        codes[:, 4] = rng.choice(np.arange(0, 255, 2 + node), n)  # leaves categories empty
        g = rng.integers(-1, 2, n).astype(np.float64)
        h = rng.integers(1, 3, n).astype(np.float64)
        # a strong signal on one categorical feature (NODE_MASK hides it)
        # and a weaker one on the next, different per node
        g += (codes[:, 2 + node % 3] % 3 == 0) * 4.0
        g += (codes[:, 2 + (node + 1) % 3] % 2 == 0) * 2.0
        if has_missing:
            for j in range(f):
                codes[rng.random(n) < 0.07, j] = -1
        hists.append(hist_from_rows(codes, g, h, NBINS, stride, has_missing))
        parents.append([g.sum(), h.sum()])
    hist = np.stack(hists)  # (k, f, stride, 2)
    qm = types.SimpleNamespace(
        num_col=f, stride=stride, has_missing=has_missing,
        nbins=torch.tensor(NBINS, dtype=torch.int64),
        is_cat=torch.tensor(IS_CAT, dtype=torch.bool),
    )
    return hist, np.asarray(parents), qm


def _qm_to(qm, device):
    return types.SimpleNamespace(
        num_col=qm.num_col, stride=qm.stride, has_missing=qm.has_missing,
        nbins=qm.nbins.to(device), is_cat=None if qm.is_cat is None else qm.is_cat.to(device),
    )


NODE_MASK = np.array(
    [[1, 1, 0, 1, 1], [1, 0, 1, 0, 1], [0, 1, 1, 1, 0]], dtype=bool
)  # per node: the feature with the node's strong signal is masked


@pytest.mark.parametrize("max_cat_threshold", [64, 3])
@pytest.mark.parametrize("has_missing", [False, True])
def test_split_scan_cat_matches_reference(hip, has_missing, max_cat_threshold):
    from sagemaker_xgboost_container_amd.ops import torch_ref

    # seeds at which the precondition below holds (it is checked on the host)
    hist, parents, qm = _split_case(has_missing, seed=7 if has_missing else 1)
    kw = dict(reg_lambda=1.0, reg_alpha=0.0, gamma=0.0, min_child_weight=1.0,
              max_cat_to_onehot=4, max_cat_threshold=max_cat_threshold)
    hist32 = torch.from_numpy(hist.reshape(K_NODES, -1, 2)).to(torch.float32)
    parent32 = torch.from_numpy(parents).to(torch.float32)
    assert (hist32.to(torch.float64).numpy() == hist.reshape(K_NODES, -1, 2)).all()
    for mask in (None, NODE_MASK):
        # precondition, from the float64 oracle alone: a unique best split
        for node in range(K_NODES):
            cands = node_candidates(
                hist[node], parents[node], NBINS, IS_CAT, has_missing, lam=1.0,
                max_cat_threshold=max_cat_threshold,
                mask=None if mask is None else mask[node],
            )
            assert cands and cands[0][0] > 0
            assert gap(cands, has_missing) > 1e-3, f"node {node}: best two gains too close"
        tmask = None if mask is None else torch.from_numpy(mask)
        ref = torch_ref.find_splits(hist32, parent32, qm, feature_mask=tmask, **kw)
        got = hip.find_splits(
            hist32.to(DEV), parent32.to(DEV), _qm_to(qm, DEV),
            feature_mask=None if tmask is None else tmask.to(DEV), **kw,
        )
        a = ref["packed"].numpy()
        b = got["packed"].cpu().numpy()
        np.testing.assert_array_equal(a[:, 1], b[:, 1])  # feature
        np.testing.assert_array_equal(a[:, 2], b[:, 2])  # bin (0 when categorical)
        np.testing.assert_array_equal(a[:, 3], b[:, 3])  # missing direction
        np.testing.assert_array_equal(ref["cat_bits"].numpy(), got["cat_bits"].cpu().numpy())
        np.testing.assert_allclose(a[:, 0], b[:, 0], rtol=2e-4, atol=1e-5)
        np.testing.assert_allclose(a[:, 4:], b[:, 4:], rtol=2e-4, atol=1e-4)
        # the cases are only worth something if categorical features win
        assert any(IS_CAT[int(v)] for v in a[:, 1])


def test_numeric_matrix_takes_the_numeric_path(hip):
    """Without a categorical column find_splits returns no cat_bits and its
    packed tensor is bit-equal to a direct call of the numeric kernels."""
    from sagemaker_xgboost_container_amd.ops import _smxgb_hip as K

    hist, parents, qm = _split_case(True, seed=5)
    qm.is_cat = None
    dqm = _qm_to(qm, DEV)
    hist32 = torch.from_numpy(hist.reshape(K_NODES, -1, 2)).to(torch.float32).to(DEV)
    parent32 = torch.from_numpy(parents).to(torch.float32).to(DEV)
    got = hip.find_splits(hist32, parent32, dqm)
    assert set(got) == {"packed"}
    f = qm.num_col
    cands = torch.empty((K_NODES, f, 5), dtype=torch.float32, device=DEV)
    out = torch.empty((K_NODES, 6), dtype=torch.float32, device=DEV)
    K.find_splits(
        hist32, parent32, dqm.nbins.to(torch.int32), torch.empty(0, dtype=torch.uint8, device=DEV),
        torch.empty(0, dtype=torch.int8, device=DEV), cands, out, K_NODES, f, qm.stride, 1, 0,
        1.0, 0.0, 0.0, 1.0,
    )
    assert torch.equal(got["packed"], out)


# -- 10. partition ----------------------------------------------------------------
R_SET = [0, 31, 32, 254, 7, 100, 200]
N_ROWS = 10000  # more than two 4096-row tiles of the v1 kernel, the last ragged
SEGS = [(0, 6000), (6000, N_ROWS)]


def _partition_case(f, default_left):
    from sagemaker_xgboost_container_amd.ops.quantize import QuantizedMatrix

    rng = np.random.default_rng(3 + f)
    bins = rng.integers(0, 200, (N_ROWS, f)).astype(np.uint8)
    split_feat = 2
    col = rng.integers(0, 255, N_ROWS)
    col[:40] = np.tile([0, 31, 32, 254, 1, 30, 33, 253], 5)  # both sides of every word edge
    col[rng.random(N_ROWS) < 0.1] = 255  # the missing slot
    col[6000:6040] = np.tile([0, 31, 32, 254, 255, 30, 33, 253], 5)
    bins[:, split_feat] = col
    nbins = torch.tensor([200] * f)
    nbins[split_feat] = 255
    is_cat = torch.zeros(f, dtype=torch.bool)
    is_cat[split_feat] = True
    qm = QuantizedMatrix(
        torch.from_numpy(bins), torch.zeros(0), torch.zeros(f + 1, dtype=torch.int64), nbins,
        256, True, N_ROWS, f, is_cat=is_cat,
    )
    gh = torch.from_numpy(rng.normal(size=(N_ROWS, 2)).astype(np.float32))
    packed = torch.tensor(
        [[1.0, split_feat, 0, float(default_left), 0, 0], [-1.0, -1, -1, 0, 0, 0]],
        dtype=torch.float32,
    )
    bits = np.zeros((2, 8), dtype=np.uint32)
    for c in R_SET:
        bits[0, c >> 5] |= np.uint32(1 << (c & 31))
    return qm, gh, packed, torch.from_numpy(bits.view(np.int32).copy())


def _expected_sides(qm, default_left):
    col = qm.bins[: SEGS[0][1], 2].numpy().astype(np.int64)
    right = np.isin(col, R_SET)
    left = np.where(col == 255, bool(default_left), ~right)
    return set(np.flatnonzero(left).tolist()), set(np.flatnonzero(~left).tolist())


@pytest.mark.parametrize("default_left", [0, 1])
@pytest.mark.parametrize("f", [5, 8])  # scalar and uchar4 copy paths
def test_partition_compact_category_set(hip, f, default_left):
    from sagemaker_xgboost_container_amd.ops import torch_ref

    qm, gh, packed, bits = _partition_case(f, default_left)
    ref_state = torch_ref.TreeState(qm, gh)
    ref_counts = ref_state.partition_level(SEGS, [0, 1], packed, 0, cat_bits=bits)
    state = hip.TreeState(qm.to(DEV), gh.to(DEV))
    counts = state.partition_level(SEGS, [0, 1], packed.to(DEV), 0, cat_bits=bits.to(DEV))
    counts = counts.cpu()
    left, right = _expected_sides(qm, default_left)
    assert counts.tolist() == ref_counts.tolist() == [[len(left), len(right)], [0, 0]]
    nl = len(left)
    rows = state._rows[1].cpu().numpy()[: SEGS[0][1]]
    ref_rows = ref_state._bufs[1].numpy()[: SEGS[0][1]]
    assert set(rows[:nl].tolist()) == set(ref_rows[:nl].tolist()) == left
    assert set(rows[nl:].tolist()) == set(ref_rows[nl:].tolist()) == right
    # the payload copied with every row is that row's
    np.testing.assert_array_equal(
        state._bins[1].cpu().numpy()[: SEGS[0][1]], qm.bins.numpy()[rows]
    )
    np.testing.assert_array_equal(state._gh[1].cpu().numpy()[: SEGS[0][1]], gh.numpy()[rows])


@pytest.mark.parametrize("default_left", [0, 1])
def test_partition_v1_category_set(hip, default_left):
    from sagemaker_xgboost_container_amd.ops import torch_ref

    qm, gh, packed, bits = _partition_case(5, default_left)
    ref_state = torch_ref.TreeState(qm, gh)
    ref_counts = ref_state.partition_level(SEGS, [0, 1], packed, 0, cat_bits=bits)
    state = hip._V1TreeState(qm.to(DEV), gh.to(DEV))
    counts = state.partition_level(SEGS, [0, 1], packed.to(DEV), 0, cat_bits=bits.to(DEV))
    left, right = _expected_sides(qm, default_left)
    assert counts.tolist() == ref_counts.tolist() == [[len(left), len(right)], [0, 0]]
    rows = state._bufs[1].cpu().numpy()[: SEGS[0][1]]
    assert set(rows[: len(left)].tolist()) == left
    assert set(rows[len(left):].tolist()) == right


# -- 11. predict and pred_leaf ---------------------------------------------------
def _forest():
    """Three trees with mixed node types; leaf values are multiples of 1/4,
    so float32 sums are exact in any order."""
    from sagemaker_xgboost_container_amd.models.tree import Tree, cat_bits_from_members

    def leaf_vals(i):
        return 0.25 * (i + 1), -0.5 * (i + 1)

    trees = []
    # tree 0: categorical root {1, 33, 255}, numeric left child, categorical right child
    t = Tree()
    t.add_node()
    l, r = t.apply_split(0, 0, float("nan"), 0, True, 1.0, 0.25, -0.5, 1, 1,
                         cat_bits=cat_bits_from_members([1, 33, 255]))
    t.apply_split(l, 1, 0.5, 0, False, 1.0, 1.0, 2.0, 1, 1)
    t.apply_split(r, 2, 2.0, 0, False, 1.0, 3.0, 4.0, 1, 1, cat_bits=cat_bits_from_members([2]))
    trees.append(t.finalize())
    # tree 1: numeric root, categorical child on the same column as tree 0's root
    t = Tree()
    t.add_node()
    l, r = t.apply_split(0, 1, -0.25, 0, False, 1.0, 0.0, 0.0, 1, 1)
    t.apply_split(l, 0, float("nan"), 0, False, 1.0, 8.0, 16.0, 1, 1,
                  cat_bits=cat_bits_from_members([0, 31, 32, 254]))
    trees.append(t.finalize())
    # tree 2: numeric only
    t = Tree()
    t.add_node()
    t.apply_split(0, 3, 0.0, 0, True, 1.0, 32.0, 64.0, 1, 1)
    trees.append(t.finalize())
    return trees


def _predict_rows():
    rng = np.random.default_rng(9)
    X = rng.normal(size=(257, 4)).astype(np.float32)
    X[:, 0] = rng.integers(0, 256, 257)
    X[:, 2] = rng.integers(0, 5, 257)
    special = [np.nan, -1.0, 2.7, 255.0, 256.0, 1e9, 1.0, 33.0, 0.0, 31.0, 32.0, 254.0, 1.9, -0.5]
    X[: len(special), 0] = special
    X[: len(special), 2] = special
    X[20:30, 1] = np.nan
    return X


def test_predict_and_pred_leaf_match_host(hip):
    from sagemaker_xgboost_container_amd.ops import _smxgb_hip as K
    from sagemaker_xgboost_container_amd.ops import torch_ref

    trees = _forest()
    X = _predict_rows()
    n = X.shape[0]
    by_row = np.array(
        [[t.predict_row(x) for t in trees] for x in X], dtype=np.float32
    )  # the scalar host traversal
    host_flat = torch_ref.make_flat_forest(trees, [0, 0, 0], None, torch.device("cpu"))
    host = torch_ref.predict_forest_flat(host_flat, torch.from_numpy(X), 1).numpy()[:, 0]
    np.testing.assert_array_equal(host, by_row.sum(1))
    host_leaf = torch_ref.pred_leaf(host_flat, torch.from_numpy(X)).numpy()

    flat = hip.make_flat_forest(trees, [0, 0, 0], None, torch.device(DEV))
    assert flat["has_cat"] and flat["cat_table"].shape == (3, 8)
    Xd = torch.from_numpy(X).to(DEV)
    np.testing.assert_array_equal(hip.predict_forest_flat(flat, Xd, 1).cpu().numpy()[:, 0], host)
    for n_chunks, tpc in ((1, 3), (3, 1), (2, 2)):
        out = torch.zeros((n_chunks, n, 1), dtype=torch.float32, device=DEV)
        K.predict_forest_cat(
            Xd, flat["left"], flat["right"], flat["feature"], flat["threshold"],
            flat["default_left"], flat["value"], flat["tree_root"], flat["tree_cls"],
            0, 3, 3, 0, out, 1, n_chunks, tpc, flat["cat_slot"], flat["cat_table"],
            flat["cat_max_slot"],
        )
        np.testing.assert_array_equal(out.sum(0).cpu().numpy()[:, 0], host)
    np.testing.assert_array_equal(hip.pred_leaf(flat, Xd).cpu().numpy(), host_leaf)
    # a single tree through predict_tree: the eval-set margin path
    for i, t in enumerate(trees):
        np.testing.assert_array_equal(hip.predict_tree(t, Xd).cpu().numpy(), by_row[:, i])


def test_numeric_forest_keeps_the_numeric_kernel(hip):
    trees = _forest()[2:]
    X = _predict_rows()
    flat = hip.make_flat_forest(trees, [0], None, torch.device(DEV))
    assert "has_cat" not in flat and "cat_slot" not in flat
    got = hip.predict_forest_flat(flat, torch.from_numpy(X).to(DEV), 1).cpu().numpy()[:, 0]
    want = np.array([trees[0].predict_row(x) for x in X], dtype=np.float32)
    np.testing.assert_array_equal(got, want)


# -- 12. end to end -----------------------------------------------------------------
def _dataset(n_class):
    rng = np.random.default_rng(0)
    n = 600
    c = rng.integers(0, 12, n).astype(np.float32)
    X = np.stack([c, rng.normal(size=n).astype(np.float32)], 1)
    if n_class == 2:
        y = np.isin(c, [1, 4, 7, 10]).astype(np.float32)
    else:
        y = (c % n_class).astype(np.float32)
    return X, y


@pytest.mark.parametrize("n_class", [2, 5])
def test_train_on_device_matches_cpu_backend(n_class):
    from sagemaker_xgboost_container_amd.data.dmatrix import DMatrix
    from sagemaker_xgboost_container_amd.models import trainer
    from sagemaker_xgboost_container_amd.models.grower import HistGrower
    from sagemaker_xgboost_container_amd.ops.quantize import quantize

    X, y = _dataset(n_class)
    params = {"max_depth": 1, "eta": 1.0, "lambda": 0.0, "max_cat_to_onehot": 1}
    if n_class == 2:
        params["objective"] = "binary:logistic"
        rounds = 1
    else:
        # the classes are c % 5: depth 2 with a gain floor that keeps the
        # noise column's chance gains out of both backends' trees
        params.update(objective="multi:softprob", num_class=n_class, max_depth=2, gamma=0.5)
        rounds = 2
    boosters, results = {}, {}
    for device in ("cpu", DEV):
        dtrain = DMatrix(X, y, feature_types=["c", "q"])
        dval = DMatrix(X[:200], y[:200], feature_types=["c", "q"])
        results[device] = {}
        boosters[device] = trainer.train(
            dict(params, device=device), dtrain, rounds, evals=[(dtrain, "train"), (dval, "val")],
            evals_result=results[device], verbose_eval=False,
        )
    cpu, gpu = boosters["cpu"], boosters[DEV]
    assert len(cpu.trees) == len(gpu.trees) == rounds * (1 if n_class == 2 else n_class)
    assert any(t.has_categorical for t in gpu.trees)
    for a, b in zip(cpu.trees, gpu.trees):
        np.testing.assert_array_equal(a.left, b.left)
        np.testing.assert_array_equal(a.feature, b.feature)
        np.testing.assert_array_equal(a.default_left, b.default_left)
        np.testing.assert_array_equal(a.split_type, b.split_type)
        np.testing.assert_array_equal(a.cat_bits, b.cat_bits)
    np.testing.assert_allclose(cpu.predict(DMatrix(X)), gpu.predict(DMatrix(X)), rtol=1e-5)
    # the eval set that is not the training matrix goes through hip.predict_tree
    metric = "logloss" if n_class == 2 else "mlogloss"
    assert len(results[DEV]["val"][metric]) == rounds
    np.testing.assert_allclose(results[DEV]["val"][metric], results["cpu"]["val"][metric], rtol=1e-4)

    # the grower itself: categorical columns grow per level, never on the device grower
    Xd = torch.from_numpy(X).to(DEV)
    qm = quantize(Xd, is_cat=[True, False])
    grower = HistGrower(qm, dict(params, device=DEV))
    assert not grower.device_async_ok()
    gh = torch.stack([torch.from_numpy(0.5 - y.clip(0, 1)).to(DEV), torch.full((600,), 0.25, device=DEV)], 1)
    tree, _ = grower.grow(gh.to(torch.float32).contiguous())
    assert grower.grow_path == "per_level"
    assert tree.has_categorical
