"""Device-autonomous grower under monotone / interaction constraints and
per-level / per-node column sampling.

Every check compares the device path with the per-level path of the same
build (SMXGB_NO_DEVICE_GROW=1): same kernels, same float math, same draws
from the shared generator, so the trees must be structurally identical.
"""
import json

import numpy as np
import pytest
import torch

from sagemaker_xgboost_container_amd.data.dmatrix import DMatrix
from sagemaker_xgboost_container_amd.models import trainer
from sagemaker_xgboost_container_amd.models.grower import HistGrower

pytestmark = pytest.mark.gpu

N, F = 20000, 70  # 70 features: two full 32-bit bitset words and a 6-bit tail
MAX_DEPTH = 4
ROUNDS = 8
MONO = tuple([1, -1] + [0] * (F - 2))
# overlapping sets, one spanning both full words and the tail, most features in none
INTER = [[0, 1, 2, 33], [2, 64, 65], [40, 41]]
BASE = {"objective": "binary:logistic", "max_depth": MAX_DEPTH, "eta": 0.5, "seed": 7,
        "device": "cuda"}

SINGLE = {
    "monotone": {"monotone_constraints": MONO},
    "interaction": {"interaction_constraints": INTER},
    "bylevel": {"colsample_bylevel": 0.6},
    "bynode": {"colsample_bynode": 0.7},
}


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(21)
    X = rng.normal(size=(N, F)).astype(np.float32)
    X[rng.random(size=X.shape) < 0.05] = np.nan
    Z = np.nan_to_num(X)
    y = (2 * Z[:, 0] - Z[:, 1] + 0.5 * Z[:, 2] * Z[:, 33] + 0.3 * Z[:, 64] * Z[:, 65]
         + 0.5 * rng.normal(size=N) > 0).astype(np.float32)
    return X, y, Z


@pytest.fixture
def paths(monkeypatch):
    """Records HistGrower.grow_path after every tree grown."""
    seen = []
    for name in ("grow", "grow_finish"):
        orig = getattr(HistGrower, name)

        def spy(self, *args, _orig=orig, **kwargs):
            out = _orig(self, *args, **kwargs)
            seen.append(self.grow_path)
            return out

        monkeypatch.setattr(HistGrower, name, spy)
    return seen


def _sig(bst):
    return json.dumps(
        [{"f": t.feature.tolist(), "b": t.split_bin.tolist(), "l": t.left.tolist()}
         for t in bst.trees]
    )


def _depth(tree, nid=0):
    if tree.left[nid] < 0:
        return 0
    return 1 + max(_depth(tree, int(tree.left[nid])), _depth(tree, int(tree.right[nid])))


def _train_pair(monkeypatch, params, X, y, rounds=ROUNDS):
    """(per-level model, device model) of one configuration."""
    monkeypatch.setenv("SMXGB_NO_DEVICE_GROW", "1")
    ref = trainer.train(dict(params), DMatrix(X, label=y), rounds, verbose_eval=False)
    monkeypatch.delenv("SMXGB_NO_DEVICE_GROW")
    dev = trainer.train(dict(params), DMatrix(X, label=y), rounds, verbose_eval=False)
    return ref, dev


def _assert_identical(ref, dev, X):
    assert _sig(ref) == _sig(dev), "device grower diverged from per-level path"
    np.testing.assert_allclose(ref.predict(X[:2000]), dev.predict(X[:2000]), rtol=1e-4, atol=1e-5)


def _assert_interaction_respected(bst, groups, f):
    """No split feature outside its ancestors' allowed sets (allowed sets
    recomputed here from the constraint lists)."""
    groups = [set(g) for g in groups]
    for tree in bst.trees:
        def walk(nid, allowed):
            if tree.left[nid] < 0:
                return
            feat = int(tree.feature[nid])
            assert feat in allowed, f"feature {feat} split outside allowed set {sorted(allowed)}"
            follow = {feat}
            for g in groups:
                if feat in g:
                    follow |= g
            child = allowed & follow
            walk(int(tree.left[nid]), child)
            walk(int(tree.right[nid]), child)

        walk(0, set(range(f)))


@pytest.mark.parametrize("name", list(SINGLE))
def test_device_path_taken(name, data, paths, monkeypatch):
    X, y, _ = data

    def no_per_level(self, *args, **kwargs):
        raise AssertionError("per-level grower used")

    monkeypatch.setattr(HistGrower, "_grow_depthwise", no_per_level)
    trainer.train(dict(BASE, **SINGLE[name]), DMatrix(X, label=y), 1, verbose_eval=False)
    assert paths == ["device"]


@pytest.mark.parametrize("name", list(SINGLE))
def test_tree_identity_single(name, data, paths, monkeypatch):
    X, y, _ = data
    ref, dev = _train_pair(monkeypatch, dict(BASE, **SINGLE[name]), X, y)
    assert paths == ["per_level"] * ROUNDS + ["device"] * ROUNDS
    _assert_identical(ref, dev, X)


def test_tree_identity_combined(data, paths, monkeypatch):
    X, y, _ = data
    params = dict(BASE, subsample=0.8, colsample_bytree=0.8)
    for extra in SINGLE.values():
        params.update(extra)
    ref, dev = _train_pair(monkeypatch, params, X, y)
    assert paths == ["per_level"] * ROUNDS + ["device"] * ROUNDS
    _assert_identical(ref, dev, X)
    _assert_interaction_respected(dev, INTER, F)


def test_rng_rewind_after_early_stop(data, paths, monkeypatch):
    """A tree that stops above max_depth draws fewer level masks on the
    per-level path; the device path pre-draws all levels and must rewind the
    generator, or the first tree after an early stop diverges."""
    X, y, _ = data
    params = dict(BASE, monotone_constraints=MONO, colsample_bylevel=0.6, colsample_bynode=0.7,
                  gamma=6)
    ref, dev = _train_pair(monkeypatch, params, X, y)
    depths = [_depth(t) for t in ref.trees]
    # precondition: an early-stopped tree is followed by one that splits
    assert any(
        depths[i] < MAX_DEPTH and any(d > 0 for d in depths[i + 1:]) for i in range(len(depths))
    ), f"recipe no longer exercises the rewind: depths {depths}"
    assert paths == ["per_level"] * ROUNDS + ["device"] * ROUNDS
    _assert_identical(ref, dev, X)


def test_empty_allowed_set(data, paths, monkeypatch):
    """Interaction constraints with both colsamples: paths through
    ungrouped features run out of candidates (node mask all zero)."""
    X, y, _ = data
    params = dict(BASE, interaction_constraints=INTER, colsample_bylevel=0.6, colsample_bynode=0.7)
    ref, dev = _train_pair(monkeypatch, params, X, y)
    assert any(_depth(t) < MAX_DEPTH for t in ref.trees)
    assert paths == ["per_level"] * ROUNDS + ["device"] * ROUNDS
    _assert_identical(ref, dev, X)
    _assert_interaction_respected(dev, INTER, F)


@pytest.mark.parametrize("with_level_mask", [True, False])
def test_node_mask_kernel(with_level_mask):
    """The bitset kernel alone on a hand-built level of 8 slots."""
    from sagemaker_xgboost_container_amd.ops import hip

    k, f = 8, F
    W = (f + 31) // 32
    dev = "cuda"

    def follow(feature):  # _interaction_allowed's rule from the raw lists
        out = np.zeros(f, dtype=bool)
        out[feature] = True
        for group in INTER:
            if feature in group:
                out[[i for i in group if i < f]] = True
        return out

    def pack(bits):
        words = np.zeros(W, dtype=np.uint32)
        for j in np.nonzero(bits)[0]:
            words[j >> 5] |= np.uint32(1 << (j & 31))
        return words

    # parents: 0 split on 2 (two overlapping sets); 1 dead (no rows); 2 holds
    # rows but did not split; 3 split on 65 (third word's tail) under an
    # already narrowed allowed set
    par_nodes = np.array([[0, 100, 1], [100, 100, 0], [100, 180, 1], [180, 300, 0]], dtype=np.int32)
    par_splits = np.array(
        [[1.5, 2, 7, 0, 0.1, 0.2], [-1, -1, -1, 0, 0, 0], [-1, -1, -1, 0, 0, 0],
         [0.25, 65, 3, 1, 0.3, 0.4]], dtype=np.float32)
    par_bits = [np.ones(f, dtype=bool), np.ones(f, dtype=bool), np.ones(f, dtype=bool), follow(2)]
    par_allowed = np.stack([pack(b) for b in par_bits])
    par_allowed[:3] = 0xFFFFFFFF  # root-style rows carry tail bits past f
    level_mask = np.ones(f, dtype=np.uint8)
    level_mask[[1, 33, 64, 69]] = 0

    want_bits = np.zeros((k, f), dtype=bool)
    for p, feature in ((0, 2), (3, 65)):
        want_bits[2 * p] = want_bits[2 * p + 1] = par_bits[p] & follow(feature)
    want_allowed = np.stack([pack(b) for b in want_bits])
    want_mask = want_bits & (level_mask.astype(bool) if with_level_mask else True)
    assert want_bits[6].sum() == 3 and want_bits[0].sum() == 6  # {2,64,65}, {0,1,2,33,64,65}

    union = torch.from_numpy(hip.interaction_union_bitsets([set(g) for g in INTER], f).view(np.int32))
    allowed = torch.full((k, W), -1, dtype=torch.int32, device=dev)  # 0xFF poison
    node_mask = torch.full((k, f), 0xFF, dtype=torch.uint8, device=dev)
    lm = torch.from_numpy(level_mask).to(dev) if with_level_mask else torch.empty(
        0, dtype=torch.uint8, device=dev)
    hip._K.grow_node_mask(
        torch.from_numpy(par_nodes).to(dev), torch.from_numpy(par_splits).to(dev),
        torch.from_numpy(par_allowed.view(np.int32)).to(dev), union.to(dev), lm,
        allowed, node_mask, k, f,
    )
    torch.cuda.synchronize()
    np.testing.assert_array_equal(node_mask.cpu().numpy(), want_mask.astype(np.uint8))
    np.testing.assert_array_equal(allowed.cpu().numpy().view(np.uint32), want_allowed)


def test_multiclass_pipelined(data, paths, monkeypatch):
    """Monotone + interaction keep the per-class stream pipeline; adding a
    level colsample drops to the sequential device path. Both match the
    per-level model."""
    X, _, Z = data
    y = np.digitize(2 * Z[:, 0] - Z[:, 1] + 0.5 * Z[:, 2] * Z[:, 33], [-1.0, 1.0]).astype(np.float32)
    async_ok = []
    orig = HistGrower.device_async_ok

    def spy(self):
        out = orig(self)
        async_ok.append(out)
        return out

    monkeypatch.setattr(HistGrower, "device_async_ok", spy)
    base = {"objective": "multi:softprob", "num_class": 3, "max_depth": MAX_DEPTH, "eta": 0.4,
            "seed": 7, "device": "cuda", "monotone_constraints": MONO,
            "interaction_constraints": INTER}
    rounds = 4
    for extra, want_async in (({}, True), ({"colsample_bylevel": 0.6}, False)):
        del paths[:], async_ok[:]
        params = dict(base, **extra)
        dev = trainer.train(dict(params), DMatrix(X, label=y), rounds, verbose_eval=False)
        assert async_ok and all(ok == want_async for ok in async_ok)
        assert paths == ["device"] * (3 * rounds)
        monkeypatch.setenv("SMXGB_NO_DEVICE_GROW", "1")
        ref = trainer.train(dict(params), DMatrix(X, label=y), rounds, verbose_eval=False)
        monkeypatch.delenv("SMXGB_NO_DEVICE_GROW")
        assert _sig(ref) == _sig(dev)
        np.testing.assert_allclose(dev.predict(X[:5000]), ref.predict(X[:5000]), rtol=1e-5, atol=1e-6)


def test_monotone_enforced_on_device_path(paths):
    rng = np.random.default_rng(0)
    X = rng.normal(size=(3000, 5)).astype(np.float32)
    y = (np.sin(X[:, 0] * 2) + X[:, 0] + X[:, 1] + rng.normal(scale=0.3, size=3000)).astype(np.float32)
    bst = trainer.train(
        {"objective": "reg:squarederror", "max_depth": 5, "eta": 0.5, "device": "cuda",
         "monotone_constraints": (1, 0, 0, 0, 0)},
        DMatrix(X, label=y), num_boost_round=10, verbose_eval=False,
    )
    assert paths == ["device"] * 10
    probe = np.random.default_rng(0).normal(size=(30, 5)).astype(np.float32)
    grid = np.linspace(-3, 3, 60, dtype=np.float32)
    violations = 0
    for row in probe:
        tiled = np.tile(row, (60, 1))
        tiled[:, 0] = grid
        pred = bst.predict(tiled, output_margin=True)
        violations += int((np.diff(pred) < -1e-7).sum())
    assert violations == 0


def test_interaction_respected_on_device_path(paths):
    rng = np.random.default_rng(3)
    X = rng.normal(size=(3000, 4)).astype(np.float32)
    y = (X[:, 0] * X[:, 1] + X[:, 2] * X[:, 3]).astype(np.float32)
    bst = trainer.train(
        {"objective": "reg:squarederror", "max_depth": 4, "device": "cuda",
         "interaction_constraints": [[0, 1], [2, 3]]},
        DMatrix(X, label=y), num_boost_round=5, verbose_eval=False,
    )
    assert paths == ["device"] * 5
    groups = [{0, 1}, {2, 3}]
    for tree in bst.trees:
        def walk(nid, path_feats):
            if tree.left[nid] < 0:
                if path_feats:
                    assert any(path_feats <= g for g in groups), f"path {path_feats} crosses groups"
                return
            feats = path_feats | {int(tree.feature[nid])}
            walk(int(tree.left[nid]), feats)
            walk(int(tree.right[nid]), feats)

        walk(0, set())
