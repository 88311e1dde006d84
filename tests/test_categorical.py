"""Categorical features on the host: data intake, the set-valued split
search against an independent oracle, traversal, model IO and refusals."""
import itertools
import json
import multiprocessing as mp
import os
import pickle
import socket
import types

import numpy as np
import pandas as pd
import pytest
import torch

from categorical_oracle import bits_of, gap, hist_from_rows, node_candidates
from sagemaker_xgboost_container_amd.data.dmatrix import DMatrix
from sagemaker_xgboost_container_amd.models import trainer
from sagemaker_xgboost_container_amd.models.booster import Booster
from sagemaker_xgboost_container_amd.models.tree import Tree, cat_bits_from_members, cat_members
from sagemaker_xgboost_container_amd.ops import torch_ref

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "categorical_model.json")
MEMBERS = [1, 4, 7, 10]


def _dataset(n=600, seed=0):
    """One categorical column of 12 categories, y = 1 iff the category is in
    {1, 4, 7, 10}, and one noise numeric column."""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 12, n).astype(np.float32)
    X = np.stack([c, rng.normal(size=n).astype(np.float32)], 1)
    return X, np.isin(c, MEMBERS).astype(np.float32)


STUMP = {"objective": "binary:logistic", "max_depth": 1, "eta": 1.0, "lambda": 0.0,
         "max_cat_to_onehot": 1, "device": "cpu"}


def _train(params, dtrain, rounds=1, **kw):
    return trainer.train(params, dtrain, rounds, verbose_eval=False, **kw)


# -- 1. intake and the depth-1 separation ------------------------------------
def test_categorical_stump_separates_what_a_threshold_cannot():
    X, y = _dataset()
    by_types = DMatrix(X, y, feature_types=["c", "q"])
    frame = pd.DataFrame({"colour": pd.Categorical(X[:, 0].astype(int), categories=range(12)),
                          "noise": X[:, 1]})
    by_frame = DMatrix(frame, y, enable_categorical=True)
    assert by_frame.feature_types == ["c", "q"]
    np.testing.assert_array_equal(by_frame.to_dense(), X)
    assert by_types.slice([0, 5, 7]).feature_types == ["c", "q"]
    for dtrain in (by_types, by_frame):
        bst = _train(STUMP, dtrain)
        assert bst.feature_types == ["c", "q"]
        tree = bst.trees[0]
        assert tree.num_nodes == 3 and tree.split_type[0] == 1 and tree.feature[0] == 0
        members = cat_members(tree.cat_bits[0])
        assert members in (MEMBERS, [c for c in range(12) if c not in MEMBERS])
        assert ((bst.predict(dtrain) > 0.5) == (y > 0.5)).all()
    # the same column read as an ordered number cannot do that at depth 1
    numeric = DMatrix(X, y)
    bst = _train(STUMP, numeric)
    assert not bst.trees[0].has_categorical
    assert ((bst.predict(numeric) > 0.5) != (y > 0.5)).any()


def test_missing_code_of_a_category_column_is_nan():
    frame = pd.DataFrame({"c": pd.Categorical(["a", None, "b", "a"]), "x": [1.0, 2.0, 3.0, 4.0]})
    dense = DMatrix(frame, enable_categorical=True).to_dense()
    np.testing.assert_array_equal(dense[:, 0], np.array([0, np.nan, 1, 0], dtype=np.float32))


# -- 2. torch_ref.find_splits against the oracle -----------------------------------
def _qm(nbins, is_cat, stride, has_missing):
    return types.SimpleNamespace(
        num_col=len(nbins), stride=stride, has_missing=has_missing,
        nbins=torch.tensor(nbins, dtype=torch.int64),
        is_cat=torch.tensor(is_cat, dtype=torch.bool),
    )


def _random_nodes(rng, nbins, k, has_missing, n=400):
    """k nodes' float64 histograms from rows with real-valued gradients."""
    stride = max(nbins) + (1 if has_missing else 0)
    hists, parents = [], []
    for _ in range(k):
        codes = np.stack([rng.integers(0, nb, n) for nb in nbins], 1)
        g = rng.normal(size=n) + 0.8 * np.sin(codes[:, rng.integers(0, len(nbins))])
        h = rng.uniform(0.5, 2.0, n)
        if has_missing:
            for j in range(len(nbins)):
                codes[rng.random(n) < 0.1, j] = -1
        hists.append(hist_from_rows(codes, g, h, nbins, stride, has_missing))
        parents.append([g.sum(), h.sum()])
    return np.stack(hists), np.asarray(parents), stride


@pytest.mark.parametrize("has_missing", [False, True])
@pytest.mark.parametrize(
    "nbins,is_cat,onehot,threshold",
    [
        ([9, 5, 14, 3], [False, True, True, True], 4, 64),   # one-hot (3 < 4) and partition
        ([6, 12, 7], [False, True, True], 16, 64),            # every categorical one-hot
        ([5, 20, 8], [False, True, False], 1, 3),             # m = 20 capped at 3
    ],
)
def test_find_splits_matches_float64_oracle(nbins, is_cat, onehot, threshold, has_missing):
    rng = np.random.default_rng(17 + len(nbins) + threshold)
    k = 6
    hist, parents, stride = _random_nodes(rng, nbins, k, has_missing)
    params = dict(lam=1.3, alpha=0.2, gamma=0.1, min_child_weight=2.0)
    best = []
    for node in range(k):
        cands = node_candidates(hist[node], parents[node], nbins, is_cat, has_missing,
                                max_cat_to_onehot=onehot, max_cat_threshold=threshold, **params)
        # precondition, from the oracle alone
        assert gap(cands, has_missing) > 1e-6, "best and second-best gains too close: change the seed"
        best.append(cands[0])
    got = torch_ref.find_splits(
        torch.from_numpy(hist.reshape(k, -1, 2)), torch.from_numpy(parents),
        _qm(nbins, is_cat, stride, has_missing),
        reg_lambda=1.3, reg_alpha=0.2, gamma=0.1, min_child_weight=2.0,
        max_cat_to_onehot=onehot, max_cat_threshold=threshold,
    )
    packed = got["packed"].numpy()
    for node, (gain, feat, _cand, d, R, gl, hl) in enumerate(best):
        assert int(packed[node, 1]) == feat
        assert int(packed[node, 3]) == d
        np.testing.assert_array_equal(got["cat_bits"][node].numpy().view(np.uint32), bits_of(R))
        if R is not None:
            assert packed[node, 2] == 0
            if threshold == 3:
                assert len(R) <= 3
    # both sides float64: gain64 is the winner's gain before the float32 store
    gains = np.array([b[0] for b in best])
    assert got["gain64"].dtype == torch.float64
    np.testing.assert_allclose(got["gain64"].numpy(), gains, rtol=1e-9)
    np.testing.assert_allclose(got["gain"].numpy(), gains, rtol=1e-6)
    assert any(b[4] is not None for b in best), "no categorical winner: the case shows nothing"


# -- 3. exhaustive optimality of the sorted partition ---------------------------------
@pytest.mark.parametrize("m", [2, 5, 10])
def test_partition_mode_is_optimal_over_all_subsets(m):
    """Conditions of the ordered-partition theorem: lambda = alpha = 0,
    min_child_weight = 0, no missing values, every h_c > 0, no cap."""
    rng = np.random.default_rng(100 + m)
    for _ in range(4):
        G = rng.normal(size=m)
        H = rng.uniform(0.2, 3.0, m)
        hist = np.zeros((1, 1, m, 2))
        hist[0, 0, :, 0], hist[0, 0, :, 1] = G, H
        parent = np.array([[G.sum(), H.sum()]])
        got = torch_ref.find_splits(
            torch.from_numpy(hist.reshape(1, -1, 2)), torch.from_numpy(parent),
            _qm([m], [True], m, False), reg_lambda=0.0, reg_alpha=0.0, gamma=0.0,
            min_child_weight=0.0, max_cat_to_onehot=1, max_cat_threshold=256,
        )
        R = cat_members(got["cat_bits"][0].numpy().view(np.uint32))
        rg, rh = G[R].sum(), H[R].sum()
        pg, ph = parent[0]
        found = 0.5 * (rg * rg / rh + (pg - rg) ** 2 / (ph - rh) - pg * pg / ph)
        best = -np.inf
        for size in range(1, m):  # every proper subset; complements repeat, which is harmless
            for S in itertools.combinations(range(m), size):
                sg, sh = G[list(S)].sum(), H[list(S)].sum()
                best = max(best, 0.5 * (sg * sg / sh + (pg - sg) ** 2 / (ph - sh) - pg * pg / ph))
        np.testing.assert_allclose(found, best, rtol=1e-9)


# -- 4. empty categories and routing -----------------------------------------------------
def test_empty_categories_are_never_members():
    rng = np.random.default_rng(4)
    nbins = [16]
    codes = rng.choice([0, 3, 4, 9, 15], 300)[:, None]  # 11 of 16 categories empty
    g = rng.normal(size=300) + (codes[:, 0] > 3)
    h = np.ones(300)
    hist = hist_from_rows(codes, g, h, nbins, 16, False)[None]
    for onehot in (1, 64):
        got = torch_ref.find_splits(
            torch.from_numpy(hist.reshape(1, -1, 2)), torch.tensor([[g.sum(), h.sum()]]),
            _qm(nbins, [True], 16, False), max_cat_to_onehot=onehot,
        )
        R = cat_members(got["cat_bits"][0].numpy().view(np.uint32))
        assert R and set(R) <= {0, 3, 4, 9, 15}
    # fewer than two non-empty categories: no candidate
    one = np.zeros((1, 16, 2))
    one[0, 5] = (3.0, 7.0)
    got = torch_ref.find_splits(
        torch.from_numpy(one), torch.tensor([[3.0, 7.0]]), _qm(nbins, [True], 16, False)
    )
    assert float(got["gain"][0]) <= 0 and not got["cat_bits"].any()


def _routing_tree():
    t = Tree()
    t.add_node()
    t.apply_split(0, 0, float("nan"), 0, False, 1.0, 1.0, 2.0, 1, 1,
                  cat_bits=cat_bits_from_members([2, 5, 255]))
    return t.finalize()


def test_routing_of_unseen_negative_large_and_fractional_values():
    tree = _routing_tree()
    #        member  unseen  neg.   >= 256        2.7 -> 2  5.999 -> 5  255   missing
    values = [2.0, 7.0, -1.0, 256.0, 1e9, 2.7, 5.999, 255.0, np.nan, -0.5, 0.0]
    expect = [2.0, 1.0, 1.0, 1.0, 1.0, 2.0, 2.0, 2.0, 2.0, 1.0, 1.0]  # default: right
    X = np.array(values, dtype=np.float32)[:, None]
    by_row = [tree.predict_row(x) for x in X]
    assert by_row == expect
    np.testing.assert_array_equal(torch_ref.predict_tree(tree, torch.from_numpy(X)).numpy(), expect)
    leaf = torch_ref.tree_leaf_ids(tree, torch.from_numpy(X)).numpy()
    np.testing.assert_array_equal(leaf, np.where(np.array(expect) == 1.0, 1, 2))
    flat = torch_ref.make_flat_forest([tree], [0], None, torch.device("cpu"))
    out = torch_ref.predict_forest_flat(flat, torch.from_numpy(X), 1).numpy()[:, 0]
    np.testing.assert_array_equal(out, expect)
    np.testing.assert_array_equal(torch_ref.pred_leaf(flat, torch.from_numpy(X)).numpy()[:, 0], leaf)
    # the C++ host traversal called directly: a missing extension is a failure
    from sagemaker_xgboost_container_amd.ops import _smxgb_hip as K

    i32 = torch_ref._flat_i32(flat)
    Xt = torch.from_numpy(X).contiguous()
    margins = torch.zeros((len(values), 1), dtype=torch.float32)
    K.predict_forest_cat_cpu(
        Xt, i32["left"], i32["right"], i32["feature"], flat["threshold"], i32["default_left"],
        flat["value"], i32["tree_root"], i32["tree_cls"], 0, 1, 0, 0, margins, 1,
        i32["cat_slot"], i32["cat_table"],
    )
    np.testing.assert_array_equal(margins.numpy()[:, 0], expect)
    leaves = torch.zeros((len(values), 1), dtype=torch.int32)
    K.pred_leaf_cat_cpu(
        Xt, i32["left"], i32["right"], i32["feature"], flat["threshold"], i32["default_left"],
        i32["tree_root"], 0, 1, 0, leaves, i32["cat_slot"], i32["cat_table"],
    )
    np.testing.assert_array_equal(leaves.numpy()[:, 0], leaf)
    with pytest.raises(ValueError, match="cat_slot"):
        K.pred_leaf_cat_cpu(
            Xt, i32["left"], i32["right"], i32["feature"], flat["threshold"], i32["default_left"],
            i32["tree_root"], 0, 1, 0, leaves, i32["cat_slot"] + 5, i32["cat_table"],
        )


# -- 5. model IO ----------------------------------------------------------------------------
def _trained(max_depth=3, rounds=3, **extra):
    X, y = _dataset()
    X[::17, 0] = np.nan
    dtrain = DMatrix(X, y, feature_types=["c", "q"])
    params = dict(STUMP, max_depth=max_depth, eta=0.5, max_cat_to_onehot=1, **extra)
    params["lambda"] = 1.0
    return _train(params, dtrain, rounds), X, dtrain


def test_json_ubjson_and_pickle_round_trips(tmp_path):
    bst, X, dtrain = _trained()
    assert any(t.has_categorical for t in bst.trees)
    probe = np.concatenate([X, [[np.nan, 0.0], [300.0, 1.0], [-2.0, 1.0], [3.5, np.nan]]]).astype(np.float32)
    want = bst.predict(probe, output_margin=True)
    saved = bst.save_json()
    tree0 = saved["learner"]["gradient_booster"]["model"]["trees"][0]
    assert saved["learner"]["feature_types"] == ["c", "q"]
    assert tree0["split_type"][0] == 1 and tree0["categories_nodes"][0] == 0
    assert tree0["categories_nodes"] == [i for i, t in enumerate(tree0["split_type"]) if t == 1]
    assert tree0["categories_segments"][0] == 0
    assert sum(tree0["categories_sizes"]) == len(tree0["categories"])
    for nid, start, size in zip(tree0["categories_nodes"], tree0["categories_segments"],
                                tree0["categories_sizes"]):
        members = tree0["categories"][start:start + size]
        assert members and members == sorted(members)
        assert members == cat_members(bst.trees[0].cat_bits[nid])
        assert np.isnan(tree0["split_conditions"][nid])  # partition mode: no single category
    bst.save_model(str(tmp_path / "m.json"))
    bst.save_model_ubj(str(tmp_path / "m.ubj"))
    for name in ("m.json", "m.ubj"):
        loaded = Booster()
        loaded.load_model(str(tmp_path / name))
        assert loaded.feature_types == ["c", "q"]
        np.testing.assert_array_equal(loaded.predict(probe, output_margin=True), want)
        np.testing.assert_array_equal(loaded.predict(probe, pred_leaf=True), bst.predict(probe, pred_leaf=True))
    np.testing.assert_array_equal(pickle.loads(pickle.dumps(bst)).predict(probe, output_margin=True), want)


def test_one_hot_split_stores_its_category():
    X, y = _dataset()
    y = (X[:, 0] == 4).astype(np.float32)
    bst = _train(dict(STUMP, max_cat_to_onehot=64), DMatrix(X, y, feature_types=["c", "q"]))
    tree = bst.save_json()["learner"]["gradient_booster"]["model"]["trees"][0]
    assert tree["split_type"][0] == 1 and tree["categories"] == [4]
    assert tree["split_conditions"][0] == 4.0


def test_old_trees_without_the_new_fields_load_as_numeric():
    tree = Tree()
    tree.add_node()
    tree.apply_split(0, 0, 0.5, 0, False, 1.0, 1.0, 2.0, 1, 1)
    tree.finalize()
    state = dict(tree.__dict__)
    del state["split_type"], state["cat_bits"]
    old = Tree.__new__(Tree)
    old.__setstate__(state)
    assert not old.has_categorical and old.cat_bits.shape == (3, 8)
    arrays = {k: v for k, v in tree.to_arrays().items() if k not in ("split_type", "cat_bits")}
    assert not Tree.from_arrays(arrays).has_categorical
    assert old.predict_row(np.array([0.25], dtype=np.float32)) == 1.0


def test_hand_written_upstream_model_gives_hand_computed_margins():
    """tests/golden/categorical_model.json was written by hand to upstream's
    schema: tree 0 is a one-hot node {2} on feature 0 (missing goes right);
    tree 1 splits feature 1 at 1.5 (missing left), its left child is the set
    {1, 3, 40} on feature 0 (missing left). Margin = 0.5 + both leaves."""
    bst = Booster()
    bst.load_model(GOLDEN)
    assert bst.feature_types == ["c", "q"]
    assert [int(v) for v in bst.trees[1].split_type] == [0, 1, 0, 0, 0]
    assert cat_members(bst.trees[1].cat_bits[1]) == [1, 3, 40]
    nan = np.nan
    X = np.array(
        [[2, 1.0], [3, 1.0], [nan, 2.0], [40.9, nan], [-1, 0.0], [300, nan]], dtype=np.float32
    )
    #           -0.5+2   0.25+4  -0.5+1  0.25+4  0.25+2  0.25+2
    want = [2.0, 4.75, 1.0, 4.75, 2.75, 2.75]
    np.testing.assert_array_equal(bst.predict(X, output_margin=True), np.float32(want))
    for i, x in enumerate(X):
        assert 0.5 + sum(t.predict_row(x) for t in bst.trees) == want[i]
    # and what it saves is what it read
    again = bst.save_json()["learner"]["gradient_booster"]["model"]["trees"]
    with open(GOLDEN) as fh:
        source = json.load(fh)["learner"]["gradient_booster"]["model"]["trees"]
    for a, b in zip(again, source):
        for key in ("split_type", "categories", "categories_nodes", "categories_segments",
                    "categories_sizes", "split_indices", "default_left"):
            assert a[key] == b[key]


# -- 6. refusals ------------------------------------------------------------------------------
def test_refusals():
    X, y = _dataset()
    types_ = ["c", "q"]
    with pytest.raises(ValueError, match="monotone"):
        _train(dict(STUMP, monotone_constraints="(1,0)"), DMatrix(X, y, feature_types=types_))
    _train(dict(STUMP, monotone_constraints="(0,1)"), DMatrix(X, y, feature_types=types_))
    for bad in (255.0, -1.0, 2.5):
        Xb = X.copy()
        Xb[3, 0] = bad
        with pytest.raises(ValueError, match=r"categorical column colour.*\[0, 254\]"):
            _train(STUMP, DMatrix(Xb, y, feature_types=types_, feature_names=["colour", "noise"]))
    frame = pd.DataFrame({"c": pd.Categorical(X[:, 0].astype(int)), "x": X[:, 1]})
    with pytest.raises(ValueError, match="enable_categorical"):
        DMatrix(frame, y)
    with pytest.raises(ValueError, match="feature_types"):
        DMatrix(X, y, feature_types=["c"])
    bst = _train(dict(STUMP, max_depth=2), DMatrix(X, y, feature_types=types_), 2)
    for kw in ({"pred_contribs": True}, {"pred_interactions": True},
               {"pred_contribs": True, "approx_contribs": True}):
        with pytest.raises(NotImplementedError, match="categorical splits"):
            bst.predict(DMatrix(X), **kw)
    # dumps print `feature < threshold`: refused, not answered wrongly
    for dump in (bst.get_dump, lambda: bst.get_dump(dump_format="json"), bst.trees_to_dataframe):
        with pytest.raises(NotImplementedError, match="categorical splits"):
            dump()
    flat = torch_ref.make_flat_forest(bst.trees, bst.tree_info, None, torch.device("cpu"))
    Xt = torch.from_numpy(X)
    for fn in (torch_ref.tree_shap, torch_ref.tree_shap_interactions, torch_ref.saabas_contribs):
        with pytest.raises(NotImplementedError, match="categorical splits"):
            fn(flat, Xt, 1)
    from sagemaker_xgboost_container_amd.ops import shap_paths

    with pytest.raises(NotImplementedError, match="categorical splits"):
        shap_paths.make_shap_paths(bst.trees, bst.tree_info, None)
    # a numeric-only model is unaffected
    plain = _train(dict(STUMP, max_depth=2), DMatrix(X, y), 2)
    contribs = plain.predict(DMatrix(X), pred_contribs=True)
    np.testing.assert_allclose(
        contribs.sum(1), plain.predict(DMatrix(X), output_margin=True), rtol=1e-4, atol=1e-5
    )
    assert len(plain.get_dump()) == 2 and len(plain.trees_to_dataframe()) > 0
    assert plain.predict(DMatrix(X), pred_interactions=True).shape == (600, 3, 3)
    assert plain.predict(DMatrix(X), pred_contribs=True, approx_contribs=True).shape == (600, 3)


def test_sparse_input_takes_the_dense_route(monkeypatch):
    import scipy.sparse as sp

    from sagemaker_xgboost_container_amd.models.trainer import _sparse_path_ok

    X, y = _dataset()
    csr = sp.csr_matrix(X)
    monkeypatch.setenv("SMXGB_SPARSE", "1")
    monkeypatch.setenv("SMXGB_SPARSE_PREDICT", "1")
    cpu = torch.device("cpu")
    assert _sparse_path_ok(DMatrix(csr, y), {}, cpu, None)
    dcat = DMatrix(csr, y, feature_types=["c", "q"])
    assert not _sparse_path_ok(dcat, {}, cpu, None)
    bst = _train(STUMP, dcat)
    assert bst.trees[0].has_categorical
    assert not bst._sparse_predict_route(dcat)
    np.testing.assert_array_equal(bst.predict(dcat), bst.predict(DMatrix(dcat.to_dense())))


# -- 7. other paths -------------------------------------------------------------------------------
@pytest.mark.parametrize(
    "extra",
    [
        {"max_depth": 3},
        {"grow_policy": "lossguide", "max_leaves": 8, "max_depth": 0},
        {"objective": "reg:absoluteerror", "max_depth": 3},
        {"objective": "multi:softprob", "num_class": 3, "max_depth": 2},
    ],
    ids=["depthwise", "lossguide", "absoluteerror", "multiclass"],
)
def test_growers_and_adaptive_leaves_train_on_categorical_data(extra):
    X, y = _dataset()
    if extra.get("num_class"):
        y = (X[:, 0] % 3).astype(np.float32)
    X[::13, 0] = np.nan
    dtrain = DMatrix(X, y, feature_types=["c", "q"])
    res = {}
    params = dict(STUMP, eta=0.5, **extra)
    params["lambda"] = 1.0
    bst = _train(params, dtrain, 4, evals=[(dtrain, "train")], evals_result=res)
    assert any(t.has_categorical for t in bst.trees)
    metric = next(iter(res["train"].values()))
    assert metric[-1] < metric[0]
    # the margins the trainer kept equal a fresh prediction
    pred = bst.predict(dtrain, output_margin=True)
    assert np.isfinite(pred).all()
    if "max_leaves" in extra:
        assert max(t.num_leaves for t in bst.trees) <= 8


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _dist_data():
    """Rows sorted by category, so rank 0 never sees the upper categories:
    the category count must come from all ranks. The numeric column has few
    distinct values, so local and global cuts are the same midpoints."""
    rng = np.random.default_rng(2)
    n = 800
    c = np.sort(rng.integers(0, 12, n)).astype(np.float32)
    x = rng.integers(0, 6, n).astype(np.float32)
    y = (np.isin(c, MEMBERS) ^ (x > 4)).astype(np.float32)
    return np.stack([c, x], 1), y


DIST_PARAMS = {"objective": "binary:logistic", "max_depth": 3, "eta": 0.5, "device": "cpu",
               "max_cat_to_onehot": 1}


def _dist_worker(rank, world, port, q):
    os.environ["GLOO_SOCKET_IFNAME"] = os.environ.get("GLOO_SOCKET_IFNAME", "lo")
    import datetime

    import torch.distributed as dist

    from sagemaker_xgboost_container_amd.parallel.comm import Communicator

    dist.init_process_group(backend="gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank,
                            world_size=world, timeout=datetime.timedelta(seconds=120))
    X, y = _dist_data()
    half = len(y) // 2
    rows = slice(0, half) if rank == 0 else slice(half, None)
    assert X[:half, 0].max() < 11  # rank 0 alone would count too few categories
    bst = trainer.train(DIST_PARAMS, DMatrix(X[rows], y[rows], feature_types=["c", "q"]), 3,
                        verbose_eval=False, comm=Communicator())
    q.put((rank, bst.save_json()["learner"]["gradient_booster"]["model"]["trees"]))
    dist.destroy_process_group()


def test_two_ranks_grow_the_single_process_trees():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dist_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=180) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    X, y = _dist_data()
    single = _train(DIST_PARAMS, DMatrix(X, y, feature_types=["c", "q"]), 3)
    want = single.save_json()["learner"]["gradient_booster"]["model"]["trees"]
    assert any(t["categories"] for t in want)
    for rank in (0, 1):
        for a, b in zip(got[rank], want):
            for key in ("left_children", "right_children", "split_indices", "split_type",
                        "default_left", "categories", "categories_nodes", "categories_sizes"):
                assert a[key] == b[key], key
            np.testing.assert_allclose(a["base_weights"], b["base_weights"], rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(
                np.nan_to_num(a["split_conditions"], nan=-7.0),
                np.nan_to_num(b["split_conditions"], nan=-7.0), rtol=1e-5, atol=1e-6,
            )


# -- 8. the xgboost shim ----------------------------------------------------------------------------
def test_xgboost_shim_classifier_with_a_category_column():
    import xgboost as xgb

    X, y = _dataset()
    frame = pd.DataFrame({"colour": pd.Categorical(X[:, 0].astype(int)), "noise": X[:, 1]})
    clf = xgb.XGBClassifier(
        enable_categorical=True, max_cat_to_onehot=1, n_estimators=2, max_depth=2, device="cpu"
    )
    clf.fit(frame, y)
    assert clf.get_booster().trees[0].has_categorical
    assert (clf.predict(frame) == y).all()
    with pytest.raises(ValueError, match="enable_categorical"):
        xgb.XGBClassifier(n_estimators=1, device="cpu").fit(frame, y)
    dmat = xgb.DMatrix(frame, label=y, enable_categorical=True)
    bst = xgb.train({"objective": "binary:logistic", "max_cat_to_onehot": 1, "max_cat_threshold": 8,
                     "device": "cpu"}, dmat, 2, verbose_eval=False)
    assert bst.trees[0].has_categorical
