"""Deepest-level histograms built by filtering the level above.

A tree whose margins are updated by traversal does not partition levels D-2
and D-1: level D-1's histogram launch streams the row ranges level D-2 read
and keeps, per build child, the rows its parent's split sends there.
Histograms are sums of fixed-point integers, so which pass contributes a row
cannot change a bit: every comparison here is exact (`np.array_equal` on
every tree array, `torch.equal` on margins and accumulators).

The modes ("filter" compacts the kept rows per wave where its queues fit
behind the histogram slab, "filter-predicate" holds it to plain predication)
run in one process: `hip._DEEPEST_HIST` is the value
SMXGB_DEEPEST_HIST was read into at import, SMXGB_LEAF_UPDATE is read per
tree. Shapes are the smallest that reach one row, a tile tail, more than one
row block (2048 rows below 4M), the vec4 and the scalar feature loops, and
the depths at which the filtered level reads the original matrix (2), a
partitioned buffer (3, 6) or does not exist (1).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROUNDS = 3
TREE_ARRAYS = (
    "left", "right", "parent", "feature", "threshold", "split_bin",
    "default_left", "value", "gain", "sum_hess",
)
# (SMXGB_DEEPEST_HIST, SMXGB_LEAF_UPDATE); the first is the reference
MODES = (
    ("partition", "scatter"), ("partition", "traverse"),
    ("filter-predicate", "traverse"), ("filter", "traverse"),
)
BINARY = {"objective": "binary:logistic", "max_depth": 6, "eta": 0.3}


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


def _set_mode(monkeypatch, deepest, leaf_update):
    from sagemaker_xgboost_container_amd.ops import hip

    monkeypatch.setattr(hip, "_DEEPEST_HIST", deepest)
    monkeypatch.setenv("SMXGB_LEAF_UPDATE", leaf_update)


def _train(params, X, y):
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
        feval=capture, verbose_eval=False,
    )
    assert len(seen) == ROUNDS
    return bst, torch.from_numpy(seen[-1])


def _assert_same_trees(trees_a, trees_b, what):
    assert len(trees_a) == len(trees_b)
    for i, (ta, tb) in enumerate(zip(trees_a, trees_b)):
        for name in TREE_ARRAYS:
            assert np.array_equal(getattr(ta, name), getattr(tb, name)), (
                f"{what}: tree {i}: {name} differs"
            )


def _three_modes(monkeypatch, params, X, y):
    """Train in every mode, compare each exactly with the scatter run.
    Returns the filter-mode booster and margin."""
    ref = m_ref = bst = m = None
    for deepest, leaf_update in MODES:
        _set_mode(monkeypatch, deepest, leaf_update)
        bst, m = _train(params, X, y)
        if ref is None:
            ref, m_ref = bst, m
            continue
        what = f"{deepest}/{leaf_update} vs scatter"
        _assert_same_trees(ref.trees, bst.trees, what)
        assert m.dtype == torch.float32 and m.shape == m_ref.shape
        assert torch.equal(m, m_ref), f"{what}: margins differ"
    return bst, m


def _depths(tree):
    depth = np.zeros(tree.num_nodes, dtype=np.int64)
    for nid in range(1, tree.num_nodes):
        depth[nid] = depth[tree.parent[nid]] + 1
    return depth


@pytest.mark.parametrize("max_depth", [1, 2, 3, 6])
@pytest.mark.parametrize("f", [8, 5])
@pytest.mark.parametrize("n", [1, 255, 257, 2 * 2048 + 3])
def test_training_three_modes(monkeypatch, n, f, max_depth):
    X, y = _data(n, f, seed=n + f)
    bst, _ = _three_modes(monkeypatch, dict(BINARY, max_depth=max_depth), X, y)
    if n > 4096:
        # enough rows to split down to the filtered level
        assert max(int(_depths(t).max()) for t in bst.trees) == max_depth


def test_missing_values_both_default_directions(monkeypatch):
    D = 6
    X, y = _data(4099, 28, seed=7, nan_frac=0.2)
    bst, _ = _three_modes(monkeypatch, BINARY, X, y)
    # the splits the filter applies are those of depth D-2
    dirs = set()
    for t in bst.trees:
        depth = _depths(t)
        for i in range(t.num_nodes):
            if t.left[i] >= 0 and depth[i] == D - 2:
                dirs.add(bool(t.default_left[i]))
    assert dirs == {True, False}, dirs


def test_dead_branches_above_the_filtered_level(monkeypatch):
    D = 6
    X, y = _data(4099, 28, seed=10)
    bst, _ = _three_modes(monkeypatch, dict(BINARY, min_child_weight=8.0), X, y)
    leaves = splits = 0
    for t in bst.trees:
        depth = _depths(t)
        at = depth == D - 2
        leaves += int((at & (np.asarray(t.left) < 0)).sum())
        splits += int((at & (np.asarray(t.left) >= 0)).sum())
    assert leaves > 0 and splits > 0, (leaves, splits)


def test_multiclass_class_slots_and_streams(monkeypatch):
    X, _ = _data(4099, 28, seed=11)
    y = (np.digitize(X[:, 0] + 0.5 * X[:, 1], [-0.5, 0.5])).astype(np.float32)
    params = {"objective": "multi:softprob", "num_class": 3, "max_depth": 6, "eta": 0.3}
    bst, m = _three_modes(monkeypatch, params, X, y)
    assert m.shape == (4099, 3) and len(bst.trees) == 3 * ROUNDS


@pytest.mark.parametrize(
    "dtype, f, stride, rows_per_block",
    [
        (torch.uint8, 8, 256, 2048),   # vec4 loop, one full-feature slab
        (torch.uint8, 5, 256, 2048),   # scalar loop
        (torch.uint8, 40, 256, 2048),  # grouped slabs: the split feature lies outside most groups
        (torch.int16, 8, 300, 2048),   # int16 bins beyond the u8 range
        # one block per parent: a wave of the larger one sees 625 rows, so
        # its queue of kept rows fills and drains before the remainder
        (torch.uint8, 8, 256, 1 << 16),
        (torch.uint8, 5, 256, 1 << 16),
        (torch.int16, 8, 300, 1 << 16),
    ],
)
def test_kernels_against_torch_histogram(dtype, f, stride, rows_per_block):
    """grow_make_level + grow_hist_level in filter mode on a synthetic level
    of two parents (300 and 5000 rows; at 2048 rows per block one block with
    only the tail loop and three blocks through the 4-rows-in-flight loop)
    vs a torch int64 histogram of the rows the same predicate selects."""
    from sagemaker_xgboost_container_amd.ops import hip

    g = torch.Generator().manual_seed(f * 1000 + stride)
    n = 5300
    missing_bin = stride - 1
    bins = torch.randint(0, stride, (n, f), generator=g)
    # both split features see missing values in both parents
    bins[3::40, 1] = missing_bin
    bins[7::40, f - 1] = missing_bin
    gh = torch.stack([torch.randn(n, generator=g), torch.rand(n, generator=g)], dim=1)
    gh_max = gh.abs().amax(0)
    ranges = [(0, 300), (300, n)]
    # (gain, feature, split_bin, default_left, left G, left H): the first
    # parent builds its left child, the second its right one
    node_gh = torch.tensor([[1.0, 10.0], [2.0, 20.0]])
    splits = torch.tensor([
        [1.0, 1.0, float(stride // 3), 1.0, 0.5, 4.0],
        [1.0, float(f - 1), float(stride // 2), 0.0, 1.5, 15.0],
    ])
    build_side = [0, 1]

    dev = "cuda"
    cur = torch.tensor([[0, 300, 1], [300, n, 0]], dtype=torch.int32, device=dev)
    counts = torch.zeros((2, 2), dtype=torch.int32, device=dev)
    nxt = torch.full((4, 3), -7, dtype=torch.int32, device=dev)
    nxt_gh = torch.zeros((4, 2), dtype=torch.float32, device=dev)
    hp = torch.zeros(5, dtype=torch.int32, device=dev)
    pp = torch.zeros(5, dtype=torch.int32, device=dev)
    work = torch.zeros(2, dtype=torch.int32, device=dev)
    splits_dev = splits.to(dev)
    hip._K.grow_make_level(
        cur, splits_dev, counts, node_gh.to(dev), nxt, nxt_gh, hp, pp, work,
        2, rows_per_block, hip._MAX_BLOCKS_PER_JOB, 1,
    )
    expect_nodes = [[0, 300, 1], [0, 300, 0], [300, n, 0], [300, n, 1]]
    assert nxt.cpu().tolist() == expect_nodes
    # the build child's block count comes from the parent's row count
    big = -(-5000 // rows_per_block)
    assert hp.cpu().tolist() == [0, 1, 1, 1, 1 + big]
    assert nxt_gh.cpu().tolist() == [[0.5, 4.0], [0.5, 6.0], [1.5, 15.0], [0.5, 5.0]]

    groups, lds_words, hist_block = hip._device_hist_plan(f, stride)
    accs = []
    for predicate_only in (0, 1):  # compaction where it fits, plain predication
        acc = torch.zeros((4, f * stride * 2), dtype=torch.int64, device=dev)
        hip._K.grow_hist_level(
            bins.to(dtype).to(dev), gh.to(dev), nxt, hp, work, acc,
            4, f, stride, len(groups), groups[0][1] - groups[0][0], gh_max.to(dev),
            rows_per_block, hip._GROW_HIST_GRID, lds_words, hist_block, 0, 1 << 30,
            splits_dev, missing_bin, predicate_only,
        )
        accs.append(acc.cpu().view(4, f * stride, 2))

    # fixed point exactly as the kernel: float32 scale, float32 product,
    # round half to even, summed as int64
    scale = torch.tensor(8589934592.0) / gh_max.clamp(min=1e-30)
    fixed = torch.round(gh * scale).to(torch.int64)
    expect = torch.zeros((4, f * stride, 2), dtype=torch.int64)
    cols = torch.arange(f) * stride
    kept_rows = []
    for p, (start, end) in enumerate(ranges):
        feat, sbin, dleft = int(splits[p, 1]), int(splits[p, 2]), bool(splits[p, 3] > 0.5)
        b = bins[start:end, feat]
        left = torch.where(b == missing_bin, torch.tensor(dleft), b <= sbin)
        keep = left if build_side[p] == 0 else ~left
        assert (b == missing_bin).any() and keep.any() and (~keep).any()
        kept_rows.append(int(keep.sum()))
        rows = torch.arange(start, end)[keep]
        idx = (bins[rows] + cols).reshape(-1)
        for c in range(2):
            expect[2 * p + build_side[p], :, c].index_add_(
                0, idx, fixed[rows, c].repeat_interleave(f)
            )
    for got in accs:
        assert torch.equal(got, expect), kept_rows
        assert int(got[1].abs().sum()) == 0 and int(got[2].abs().sum()) == 0


class _OneRank:
    """Identity communicator: sends DeviceGrower.grow through the per-level
    Python loop (the distributed path) inside the test process."""

    rank = 0
    world_size = 1
    is_master = True

    def allreduce_(self, tensor):
        return tensor

    allreduce_max_ = allreduce_min_ = allreduce_

    def broadcast_(self, tensor, src=0):
        return tensor

    def barrier(self):
        pass


def test_comm_loop_launch_counts_and_results(monkeypatch):
    """The per-level loop partitions a depth-6 tree D-2 = 4 times with the
    filter, 5 times with traversal alone and 6 times with the scatter, and
    grows in every mode the tree the whole-tree enqueue grows."""
    from sagemaker_xgboost_container_amd.models.grower import HistGrower
    from sagemaker_xgboost_container_amd.ops import hip
    from sagemaker_xgboost_container_amd.ops.quantize import quantize

    D = 6
    n = 2 * 2048 + 3
    X, y = _data(n, 28, seed=14, nan_frac=0.2)
    qm = quantize(torch.tensor(X, device="cuda"), max_bin=256)
    yt = torch.tensor(y, device="cuda")
    gh = torch.stack([0.5 - yt, torch.full_like(yt, 0.25)], dim=1).contiguous()

    calls = []
    real = hip._K.grow_partition_level

    def counted(*args):
        calls.append(args[-1])  # copy_rows
        return real(*args)

    monkeypatch.setattr(hip._K, "grow_partition_level", counted)

    def grow(comm):
        grower = HistGrower(qm, {"max_depth": D, "eta": 0.3}, comm=comm)
        tree, leaf_jobs = grower.grow(gh)
        assert grower.grow_path == "device"
        margin = torch.zeros(n, dtype=torch.float32, device="cuda")
        grower.state.update_margins(margin, leaf_jobs)
        return tree, margin.cpu()

    expected_calls = {"scatter": [1] * D, "traverse": [0] * (D - 1), "filter": [0] * (D - 2)}
    ref = None
    for deepest, leaf_update in MODES:
        _set_mode(monkeypatch, deepest, leaf_update)
        tree, margin = grow(None)
        assert not calls, "the whole-tree enqueue launches its partitions itself"
        tree_c, margin_c = grow(_OneRank())
        key = "scatter" if leaf_update == "scatter" else (
            "traverse" if deepest == "partition" else "filter"
        )
        assert calls == expected_calls[key], (key, calls)
        del calls[:]
        if ref is None:
            ref = (tree, margin)
            assert int(_depths(tree).max()) == D
        for what, (t, m) in (("enqueue", (tree, margin)), ("comm loop", (tree_c, margin_c))):
            _assert_same_trees([ref[0]], [t], f"{deepest}/{leaf_update} {what}")
            assert torch.equal(m, ref[1]), f"{deepest}/{leaf_update} {what}: margins differ"
