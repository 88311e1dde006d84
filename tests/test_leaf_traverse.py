"""Margin update by streaming tree traversal vs the row-id leaf scatter.

Both modes add the same host-computed float32 leaf value to every row's
margin cell with one float add, so every comparison here is exact: the full
training margin after 3 rounds (`torch.equal`) and every array of every
tree. SMXGB_LEAF_UPDATE selects the mode per tree, so both run in one
process. Shapes are the smallest that reach the tile tail, more than one
tile, the in-place (non-staged) path and int16 bins.
"""
import multiprocessing as mp
import os
import socket

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROUNDS = 3
TREE_ARRAYS = (
    "left", "right", "parent", "feature", "threshold", "split_bin",
    "default_left", "value", "gain", "sum_hess",
)


def _data(n, f, seed=0, nan_frac=0.0):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, f)).astype(np.float32)
    score = X[:, 0] * 2 - X[:, 1 % f] + 0.5 * X[:, 2 % f] * X[:, 3 % f]
    if nan_frac:
        # missing feature 0 behaves like a large value (default right),
        # missing feature 1 like a small one (default left)
        m0 = rng.random(n) < nan_frac
        m1 = rng.random(n) < nan_frac
        score = np.where(m0, 2.0, X[:, 0]) + np.where(m1, -2.0, X[:, 1])
        X[rng.random(size=X.shape) < nan_frac] = np.nan
        X[m0, 0] = np.nan
        X[m1, 1] = np.nan
    y = (score + rng.normal(scale=0.3, size=n) > 0).astype(np.float32)
    return X, y


class _Calls:
    """Counts launches of the two margin-update kernels."""

    def __init__(self, monkeypatch):
        from sagemaker_xgboost_container_amd.ops import hip

        self.traverse = 0
        self.scatter = 0
        real_traverse = hip._K.leaf_update_traverse
        real_scatter = hip._K.leaf_update_compact

        def traverse(*args):
            self.traverse += 1
            return real_traverse(*args)

        def scatter(*args):
            self.scatter += 1
            return real_scatter(*args)

        monkeypatch.setattr(hip._K, "leaf_update_traverse", traverse)
        monkeypatch.setattr(hip._K, "leaf_update_compact", scatter)

    def take(self):
        out = (self.traverse, self.scatter)
        self.traverse = self.scatter = 0
        return out


def _train(params, X, y, comm=None):
    """(booster, training margin after the last round as a CPU tensor)."""
    from sagemaker_xgboost_container_amd.data.dmatrix import DMatrix
    from sagemaker_xgboost_container_amd.models import trainer

    seen = []

    def capture(margin, _dmatrix):
        seen.append(np.array(margin, copy=True))
        return "captured", 0.0

    dtrain = DMatrix(X, label=y)
    bst = trainer.train(
        dict(params, device="cuda"), dtrain, ROUNDS, evals=[(dtrain, "train")],
        feval=capture, verbose_eval=False, comm=comm,
    )
    assert len(seen) == ROUNDS
    return bst, torch.from_numpy(seen[-1])


def _assert_same(a, b, ma, mb):
    assert len(a.trees) == len(b.trees)
    for i, (ta, tb) in enumerate(zip(a.trees, b.trees)):
        for name in TREE_ARRAYS:
            assert np.array_equal(getattr(ta, name), getattr(tb, name)), f"tree {i}: {name} differs"
    assert ma.dtype == torch.float32 and ma.shape == mb.shape
    assert torch.equal(ma, mb), "margins differ between scatter and traverse"


def _both_modes(monkeypatch, params, X, y, expect_traverse=True, comm=None):
    """Train in scatter and in traverse mode, compare exactly, check which
    kernel ran. Returns the traverse-mode booster and margin."""
    calls = _Calls(monkeypatch)
    monkeypatch.setenv("SMXGB_LEAF_UPDATE", "scatter")
    ref, m_ref = _train(params, X, y, comm)
    n_traverse, n_scatter = calls.take()
    assert n_traverse == 0, "scatter mode ran the traversal kernel"
    monkeypatch.setenv("SMXGB_LEAF_UPDATE", "traverse")
    bst, m = _train(params, X, y, comm)
    n_traverse, n_scatter = calls.take()
    if expect_traverse:
        assert n_traverse == len(bst.trees) and n_scatter == 0
    else:
        assert n_traverse == 0, "this configuration must keep the leaf scatter"
    _assert_same(ref, bst, m_ref, m)
    return bst, m


def _leaf_depths(tree):
    depth = np.zeros(tree.num_nodes, dtype=np.int64)
    for nid in range(1, tree.num_nodes):
        depth[nid] = depth[tree.parent[nid]] + 1
    return depth[tree.left < 0]


BINARY = {"objective": "binary:logistic", "max_depth": 6, "eta": 0.3}


@pytest.mark.parametrize("n", [1, 255, 257, 4099])
def test_u8_staged_tiles(monkeypatch, n):
    """f = 28 u8 bins: one partial tile, a tile less one row, a tile plus
    one row, and many tiles with a tail."""
    X, y = _data(n, 28, seed=n)
    _both_modes(monkeypatch, BINARY, X, y)


def test_in_place_path_odd_feature_count(monkeypatch):
    X, y = _data(4099, 5, seed=5)
    bst, _ = _both_modes(monkeypatch, BINARY, X, y)
    assert min(t.num_nodes for t in bst.trees) > 1


def test_int16_bins(monkeypatch):
    """The device grower's split scan covers features of up to 256 bins, so
    these trees may be single leaves; test_kernel_against_torch_walk drives
    the int16 path through a deep synthetic tree."""
    X, y = _data(4099, 8, seed=6)
    _both_modes(monkeypatch, dict(BINARY, max_bin=512), X, y)


@pytest.mark.parametrize(
    "dtype, f, depth, top_bin",
    [
        (torch.int16, 8, 4, 512),   # in place, bins beyond the u8 range
        (torch.uint8, 5, 4, 255),   # in place, f not a multiple of 4
        (torch.uint8, 28, 4, 255),  # staged, odd dword row stride
        (torch.uint8, 8, 4, 255),   # staged, even dword row stride
        (torch.uint8, 28, 10, 255),  # staged, largest split/value tables
    ],
)
def test_kernel_against_torch_walk(dtype, f, depth, top_bin):
    """leaf_update_traverse on a synthetic split heap (random features, bins
    and default directions, a fifth of the nodes leaves above `depth`) vs a
    plain torch walk of the same heap; `top_bin` is the missing bin."""
    from sagemaker_xgboost_container_amd.ops import hip

    n = 4099
    g = torch.Generator().manual_seed(depth * 100 + f)
    heap = (1 << depth) - 1
    splits = torch.zeros((heap, 6), dtype=torch.float32)
    splits[:, 0] = torch.where(torch.rand(heap, generator=g) < 0.2, -1.0, 1.0)
    splits[0, 0] = 1.0
    splits[:, 1] = torch.randint(0, f, (heap,), generator=g).float()
    splits[:, 2] = torch.randint(0, top_bin, (heap,), generator=g).float()
    splits[:, 3] = torch.randint(0, 2, (heap,), generator=g).float()
    values = torch.randn(2 * heap + 1, generator=g)
    bins = torch.randint(0, top_bin + 1, (n, f), generator=g).to(dtype)
    start = torch.randn(n, generator=g)

    margin = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    margin[:, 2] = start.cuda()
    hip._K.leaf_update_traverse(
        bins.cuda(), splits.cuda(), values.cuda(), margin[:, 2], depth, top_bin, 3
    )

    node = torch.zeros(n, dtype=torch.long)
    wide = bins.long()
    for _ in range(depth):
        inner = (node < heap) & (splits[node.clamp(max=heap - 1), 0] > 0)
        rec = splits[node.clamp(max=heap - 1)]
        b = wide.gather(1, rec[:, 1].long().unsqueeze(1)).squeeze(1)
        go_left = torch.where(b == top_bin, rec[:, 3] > 0.5, b <= rec[:, 2].long())
        node = torch.where(inner, 2 * node + torch.where(go_left, 1, 2), node)
    assert node.max() >= heap, "no row reached the deepest level"
    assert (node < heap).any(), "no row stopped above the deepest level"
    assert torch.equal(margin[:, 2].cpu(), start + values[node])
    assert float(margin[:, :2].abs().sum()) == 0.0


def test_missing_values_both_default_directions(monkeypatch):
    X, y = _data(4099, 28, seed=7, nan_frac=0.2)
    bst, _ = _both_modes(monkeypatch, BINARY, X, y)
    # default direction of the splits that actually see missing values
    dirs = {
        (int(t.feature[i]), bool(t.default_left[i]))
        for t in bst.trees for i in range(t.num_nodes) if t.left[i] >= 0
    }
    assert any(d for _f, d in dirs) and any(not d for _f, d in dirs), dirs


def test_depth_one(monkeypatch):
    X, y = _data(4099, 28, seed=8)
    bst, _ = _both_modes(monkeypatch, dict(BINARY, max_depth=1), X, y)
    assert all(t.num_nodes == 3 for t in bst.trees)


def test_root_does_not_split(monkeypatch):
    X, y = _data(4099, 28, seed=9)
    bst, m = _both_modes(monkeypatch, dict(BINARY, gamma=1e9), X, y)
    assert all(t.num_nodes == 1 for t in bst.trees)
    # every row got the root value of every tree: one constant column
    assert torch.equal(m, m[:1].expand_as(m))
    assert float(m[0]) != 0.0


def test_leaves_above_max_depth(monkeypatch):
    X, y = _data(4099, 28, seed=10)
    bst, _ = _both_modes(monkeypatch, dict(BINARY, min_child_weight=8.0), X, y)
    depths = np.concatenate([_leaf_depths(t) for t in bst.trees])
    assert depths.min() < 6 and depths.max() == 6, (depths.min(), depths.max())


def test_multiclass_async_class_streams(monkeypatch):
    X, _ = _data(4099, 28, seed=11)
    y = (np.digitize(X[:, 0] + 0.5 * X[:, 1], [-0.5, 0.5])).astype(np.float32)
    params = {"objective": "multi:softprob", "num_class": 3, "max_depth": 6, "eta": 0.3}
    bst, m = _both_modes(monkeypatch, params, X, y)
    assert m.shape == (4099, 3) and len(bst.trees) == 3 * ROUNDS


def test_dart_rescaled_leaf_values(monkeypatch):
    X, y = _data(4099, 28, seed=12)
    params = dict(BINARY, booster="dart", rate_drop=0.5, one_drop=1, seed=5)
    bst, _ = _both_modes(monkeypatch, params, X, y)
    assert any(w != 1.0 for w in bst.weight_drop), "no tree was dropped: new_tree_scale stayed 1"


@pytest.mark.parametrize(
    "params, env",
    [
        (dict(BINARY, subsample=0.5, seed=3), {}),
        (dict(BINARY), {"SMXGB_NO_DEVICE_GROW": "1"}),
        (dict(BINARY, grow_policy="lossguide", max_leaves=16), {}),
        (dict(BINARY), {"SMXGB_PIPELINE": "v1", "SMXGB_NO_DEVICE_GROW": "1"}),
    ],
    ids=["subsample", "per_level", "lossguide", "pipeline_v1"],
)
def test_other_paths_keep_the_scatter(monkeypatch, params, env):
    for key, value in env.items():
        monkeypatch.setenv(key, value)
    X, y = _data(4099, 28, seed=13)
    _both_modes(monkeypatch, params, X, y, expect_traverse=False)


def test_against_torch_traversal(monkeypatch):
    """One tree grown directly, its margin update checked against a plain
    torch walk of the finished tree over the quantized matrix."""
    from sagemaker_xgboost_container_amd.models.grower import HistGrower
    from sagemaker_xgboost_container_amd.ops.quantize import quantize

    monkeypatch.setenv("SMXGB_LEAF_UPDATE", "traverse")
    n = 4099
    X, y = _data(n, 28, seed=14, nan_frac=0.2)
    qm = quantize(torch.tensor(X, device="cuda"), max_bin=256)
    assert qm.has_missing
    yt = torch.tensor(y, device="cuda")
    gh = torch.stack([0.5 - yt, torch.full_like(yt, 0.25)], dim=1).contiguous()
    grower = HistGrower(qm, {"max_depth": 6, "eta": 0.3})
    tree, leaf_jobs = grower.grow(gh)
    assert grower.grow_path == "device" and grower.state._traverse is not None
    start = torch.arange(n, dtype=torch.float32, device="cuda") * 0.125
    margin = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
    margin[:, 1] = start
    grower.state.update_margins(margin[:, 1], leaf_jobs)

    bins = qm.bins.long()
    missing_bin = qm.stride - 1
    node = torch.zeros(n, dtype=torch.long, device="cuda")
    left = torch.tensor(tree.left, dtype=torch.long, device="cuda")
    right = torch.tensor(tree.right, dtype=torch.long, device="cuda")
    feature = torch.tensor(tree.feature, dtype=torch.long, device="cuda")
    split_bin = torch.tensor(tree.split_bin, dtype=torch.long, device="cuda")
    default_left = torch.tensor(tree.default_left, dtype=torch.bool, device="cuda")
    for _ in range(6):
        b = bins.gather(1, feature[node].unsqueeze(1)).squeeze(1)
        go_left = torch.where(b == missing_bin, default_left[node], b <= split_bin[node])
        nxt = torch.where(go_left, left[node], right[node])
        node = torch.where(left[node] >= 0, nxt, node)
    value = torch.tensor(np.asarray(tree.value, dtype=np.float32), device="cuda")
    assert int((left >= 0).sum()) > 1
    assert torch.equal(margin[:, 1], start + value[node])
    assert float(margin[:, 0].abs().sum()) == 0.0, "the neighbouring column was touched"


def _find_open_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _comm_worker(port, q):
    """Both modes through the communicator's per-level device loop under a
    1-rank nccl group (the pattern of tests/test_rccl_rehearsal.py)."""
    try:
        import datetime

        import torch.distributed as dist

        from sagemaker_xgboost_container_amd.parallel.comm import Communicator

        torch.cuda.set_device(0)
        dist.init_process_group(
            backend="nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
            timeout=datetime.timedelta(seconds=120),
        )
        from sagemaker_xgboost_container_amd.ops import hip

        comm = Communicator()
        launches = []
        real_traverse = hip._K.leaf_update_traverse
        hip._K.leaf_update_traverse = lambda *a: (launches.append(1), real_traverse(*a))[1]
        X, y = _data(4099, 28, seed=15)
        os.environ["SMXGB_LEAF_UPDATE"] = "scatter"
        ref, m_ref = _train(BINARY, X, y, comm)
        assert not launches
        os.environ["SMXGB_LEAF_UPDATE"] = "traverse"
        bst, m = _train(BINARY, X, y, comm)
        assert len(launches) == ROUNDS
        _assert_same(ref, bst, m_ref, m)
        q.put(("ok", sum(t.num_nodes for t in bst.trees)))
        dist.barrier()
        dist.destroy_process_group()
    except BaseException as e:  # noqa: BLE001 - relayed to the test process
        q.put(("error", f"{type(e).__name__}: {e}"))


def test_communicator_device_loop():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_comm_worker, args=(_find_open_port(), q))
    p.start()
    result = q.get(timeout=420)
    p.join(timeout=120)
    assert result[0] == "ok", f"communicator path failed: {result[1]}"
    assert result[1] > ROUNDS, "the trees did not split"
    assert p.exitcode == 0
