"""The staged (single-read) partition kernel against the classic one.

`partition_device_staged_kernel` loads a tile's bin rows, gradient pairs and
row ids into registers once, classifies from the register that holds the
split feature's byte and stores from the same registers; the classic kernel
reads the source a second time for the copy. Both move the same rows to the
same child ranges, in atomic-arrival order inside a child, and everything
downstream sums fixed-point integers, so every comparison here is exact:
records are compared as sorted multisets per child, trees with
`np.array_equal`, margins with `torch.equal`.

Kernel-level cases call `hip._K.grow_partition_level` on hand-built level
tables, once per mode, and check both against the rows numpy selects.
`hip.set_partition_mode` switches the kernel inside the process;
"staged-512/1024/2048" pin the tile ("staged" itself runs 2048 rows on a
512-thread block; the smaller tiles are 256-thread geometries kept for A/B
sweeps), so the row counts below are taken relative to each geometry's own
tile.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL_BIN = 0x5A
SENTINEL_ROW = -77
SENTINEL_GH = -12345.5
ROWS_PER_BLOCK = 2048  # virtual-block granularity of the hand-built levels


@pytest.fixture
def hip():
    from sagemaker_xgboost_container_amd.ops import hip as mod

    before = mod._PARTITION
    yield mod
    mod.set_partition_mode(before)


class Level:
    """One level's inputs on the host: k nodes over n source rows."""

    def __init__(self, ranges, splits, f, dtype=torch.uint8, stride=256, seed=0,
                 blocks_per_node=None):
        self.ranges = ranges
        self.k = len(ranges)
        self.f = f
        self.dtype = dtype
        self.stride = stride
        self.missing_bin = stride - 1
        n = max([e for _, e in ranges] + [1])
        self.n = n
        g = torch.Generator().manual_seed(seed)
        self.bins = torch.randint(0, stride - 1, (n, f), generator=g)
        # every feature sees missing values
        self.bins[torch.rand((n, f), generator=g) < 0.1] = self.missing_bin
        self.gh = torch.randn((n, 2), generator=g)
        self.rows = torch.randperm(n, generator=g).to(torch.int32)
        self.splits = torch.tensor(splits, dtype=torch.float32).reshape(self.k, 6)
        prefix = [0]
        for i, (s, e) in enumerate(ranges):
            nb = -(-(e - s) // ROWS_PER_BLOCK) if blocks_per_node is None else blocks_per_node[i]
            prefix.append(prefix[-1] + (nb if e > s else 0))
        self.prefix = prefix

    def live(self, i):
        s, e = self.ranges[i]
        return e > s and float(self.splits[i, 0]) > 0.0

    def left_mask(self, i):
        s, e = self.ranges[i]
        feat, sbin = int(self.splits[i, 1]), int(self.splits[i, 2])
        dleft = bool(self.splits[i, 3] > 0.5)
        b = self.bins[s:e, feat]
        return torch.where(b == self.missing_bin, torch.tensor(dleft), b <= sbin)

    def run(self, hip, mode, copy_rows, grid=64):
        hip.set_partition_mode(mode)
        dev = "cuda"
        n, f = self.n, self.f
        nodes = torch.tensor([[s, e, 1] for s, e in self.ranges], dtype=torch.int32, device=dev)
        pp = torch.tensor(self.prefix, dtype=torch.int32, device=dev)
        work = torch.tensor([0, self.prefix[-1]], dtype=torch.int32, device=dev)
        counters = torch.zeros((self.k, 2), dtype=torch.int32, device=dev)
        dst_bins = torch.full((n, f), SENTINEL_BIN, dtype=self.dtype, device=dev)
        dst_gh = torch.full((n, 2), SENTINEL_GH, dtype=torch.float32, device=dev)
        dst_rows = torch.full((n,), SENTINEL_ROW, dtype=torch.int32, device=dev)
        hip._K.grow_partition_level(
            self.bins.to(self.dtype).to(dev), self.gh.to(dev), self.rows.to(dev),
            dst_bins, dst_gh, dst_rows, nodes, pp, work, self.splits.to(dev), counters,
            self.k, f, self.missing_bin, grid, 1, copy_rows,
        )
        torch.cuda.synchronize()
        return counters.cpu(), dst_bins.cpu().to(torch.int64), dst_gh.cpu(), dst_rows.cpu()


def _records(bins, gh, rows):
    """Rows of (bins..., gh bits, row id), sorted lexicographically."""
    rec = np.concatenate(
        [bins.numpy().astype(np.int64),
         gh.numpy().view(np.int32).astype(np.int64),
         rows.numpy().astype(np.int64)[:, None]], axis=1,
    )
    return rec[np.lexsort(rec.T[::-1])]


def _check(level, out, copy_rows, what):
    counters, dst_bins, dst_gh, dst_rows = out
    touched = torch.zeros(level.n, dtype=torch.bool)
    for i, (s, e) in enumerate(level.ranges):
        if not level.live(i):
            assert counters[i].tolist() == [0, 0], (what, i)
            continue
        left = level.left_mask(i)
        nl, nr = int(left.sum()), int((~left).sum())
        assert counters[i].tolist() == [nl, nr], (what, i, counters[i].tolist(), nl, nr)
        touched[s:e] = True
        src = slice(s, e)
        for side, keep, dst in (("left", left, slice(s, s + nl)), ("right", ~left, slice(e - nr, e))):
            src_rows = level.rows[src][keep] if copy_rows else torch.full((int(keep.sum()),), SENTINEL_ROW)
            want = _records(level.bins[src][keep], level.gh[src][keep], src_rows)
            got = _records(dst_bins[dst], dst_gh[dst], dst_rows[dst])
            assert np.array_equal(got, want), f"{what}: node {i} {side} child differs"
    rest = ~touched
    assert bool((dst_bins[rest] == SENTINEL_BIN).all()), f"{what}: bins written outside live nodes"
    assert bool((dst_gh[rest] == SENTINEL_GH).all()), f"{what}: gh written outside live nodes"
    assert bool((dst_rows[rest] == SENTINEL_ROW).all()), f"{what}: rows written outside live nodes"
    if not copy_rows:
        assert bool((dst_rows == SENTINEL_ROW).all()), f"{what}: row ids written with copy_rows=0"


def _both_modes(hip, level, staged_mode, copy_rows, grid=64):
    ref = level.run(hip, "classic", copy_rows, grid)
    _check(level, ref, copy_rows, "classic")
    out = level.run(hip, staged_mode, copy_rows, grid)
    _check(level, out, copy_rows, staged_mode)
    assert torch.equal(ref[0], out[0]), "counters differ between the kernels"


# (gain, feature, split_bin, default_left, left G, left H)
def _split(feature, split_bin=120, default_left=1, gain=1.0):
    return [gain, float(feature), float(split_bin), float(default_left), 0.0, 0.0]


TILES = {"staged-512": 512, "staged-1024": 1024, "staged-2048": 2048}


def test_tile_rule(hip):
    """Where the staged kernel applies and which tile it runs."""
    hip.set_partition_mode("staged")
    for f in (4, 8, 28, 32):
        assert hip._K.partition_tile(f, 1, 1) == 2048
    assert hip._K.partition_tile(36, 1, 1) == 0   # beyond the 8-lane row group
    assert hip._K.partition_tile(5, 1, 1) == 0    # odd width
    assert hip._K.partition_tile(8, 0, 1) == 0    # int16 bins
    assert hip._K.partition_tile(28, 1, 0) == 0   # payload-free last level
    for mode, tile in TILES.items():
        hip.set_partition_mode(mode)
        assert hip._K.partition_tile(28, 1, 1) == tile
    hip.set_partition_mode("classic")
    assert hip._K.partition_tile(28, 1, 1) == 0
    with pytest.raises(ValueError):
        hip.set_partition_mode("lds")
    assert hip._PARTITION == "classic"


@pytest.mark.parametrize("copy_rows", [0, 1])
@pytest.mark.parametrize("which", ["1", "T-1", "T", "T+1", "2T+3"])
@pytest.mark.parametrize("mode", sorted(TILES))
def test_row_counts_around_the_tile(hip, mode, which, copy_rows):
    T = TILES[mode]
    n = {"1": 1, "T-1": T - 1, "T": T, "T+1": T + 1, "2T+3": 2 * T + 3}[which]
    # the node starts at an offset so that tile bases are not multiples of T
    level = Level([(5, 5 + n)], [_split(9)], 28, seed=n)
    _both_modes(hip, level, mode, copy_rows)


@pytest.mark.parametrize("copy_rows", [0, 1])
@pytest.mark.parametrize("mode", sorted(TILES) + ["staged"])
def test_block_walks_several_virtual_blocks_and_tiles(hip, mode, copy_rows):
    """3 virtual blocks on a grid of 2: block 0 walks virtual blocks 0 and 2,
    and each virtual block walks two tiles (the last one a tail)."""
    T = TILES.get(mode, 2048)
    level = Level([(0, 5 * T + 7)], [_split(26, split_bin=60, default_left=0)], 28, seed=3,
                  blocks_per_node=[3])
    _both_modes(hip, level, mode, copy_rows, grid=2)


@pytest.mark.parametrize("copy_rows", [0, 1])
@pytest.mark.parametrize("layout", ["a", "b", "all"])
def test_level_of_mixed_nodes(hip, layout, copy_rows):
    """Live, empty, unsplit (gain <= 0), all-left and all-right nodes in one
    level; 10% of every feature's bins are missing, sent both ways."""
    mixed_l = ((0, 1500), _split(5, 100, 1))
    mixed_r = ((0, 1500), _split(14, 140, 0))
    empty = ((0, 0), _split(0))
    zero_gain = ((0, 700), _split(3, gain=0.0))
    neg_gain = ((0, 700), _split(3, gain=-1.0))
    # every bin <= 254, the missing ones follow default_left = 1
    all_left = ((0, 1100), _split(27, 254, 1))
    # no bin <= -1, the missing ones follow default_left = 0
    all_right = ((0, 1100), _split(0, -1, 0))
    kinds = {
        "a": [mixed_l, empty, zero_gain, all_left],
        "b": [all_right, neg_gain, mixed_r, empty],
        "all": [mixed_l, empty, zero_gain, all_left, all_right, mixed_r, neg_gain, mixed_l],
    }[layout]
    ranges, splits, at = [], [], 0
    for (s, e), sp in kinds:
        ranges.append((at, at + (e - s)) if e > s else (0, 0))
        splits.append(sp)
        at += e - s
    level = Level(ranges, splits, 28, seed=11)
    assert len(ranges) == (8 if layout == "all" else 4)
    # the level is what it is meant to be
    for i, kind in enumerate(kinds):
        if not level.live(i):
            continue
        s0, e0 = ranges[i]
        assert bool((level.bins[s0:e0, int(level.splits[i, 1])] == level.missing_bin).any())
        went_left = level.left_mask(i)
        if kind is all_left:
            assert bool(went_left.all())
        elif kind is all_right:
            assert not bool(went_left.any())
        else:
            assert bool(went_left.any()) and not bool(went_left.all())
    _both_modes(hip, level, "staged", copy_rows)


@pytest.mark.parametrize("copy_rows", [0, 1])
@pytest.mark.parametrize(
    "dtype, f, stride, staged",
    [
        (torch.uint8, 4, 256, True),     # nd = 1
        (torch.uint8, 28, 256, True),    # nd = 7: one idle lane per row group
        (torch.uint8, 32, 256, True),    # nd = 8: the whole row group
        (torch.uint8, 36, 256, False),   # beyond the row group: classic kernel
        (torch.uint8, 5, 256, False),    # odd width: classic kernel, scalar copy
        (torch.int16, 8, 300, False),    # int16 bins: classic kernel
    ],
)
def test_split_feature_in_every_dword_and_byte(hip, dtype, f, stride, staged, copy_rows):
    """One node per split feature: each byte of the first, a middle and the
    last dword of the row. Widths the staged kernel does not cover fall back
    to the classic kernel and still agree."""
    nd = max(f // 4, 1)
    feats = sorted({d * 4 + b for d in (0, nd // 2, nd - 1) for b in range(4) if d * 4 + b < f}
                   | {f - 1})
    ranges, splits, at = [], [], 0
    for j, feat in enumerate(feats):
        rows = 600 + 37 * j
        ranges.append((at, at + rows))
        splits.append(_split(feat, stride // 3 + j, j & 1))
        at += rows
    level = Level(ranges, splits, f, dtype=dtype, stride=stride, seed=f)
    hip.set_partition_mode("staged")
    tile = hip._K.partition_tile(f, 1 if dtype == torch.uint8 else 0, 1)
    assert (tile > 0) == staged
    _both_modes(hip, level, "staged", copy_rows)


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------

ROUNDS = 3
TREE_ARRAYS = (
    "left", "right", "parent", "feature", "threshold", "split_bin",
    "default_left", "value", "gain", "sum_hess",
)
BINARY = {"objective": "binary:logistic", "max_depth": 6, "eta": 0.3}
BIG_TILE = 2048


def _data(n, f, seed=0, nan_frac=0.0):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, f)).astype(np.float32)
    score = X[:, 0] * 2 - X[:, 1 % f] + 0.5 * X[:, 2 % f] * X[:, 3 % f]
    if nan_frac:
        m0 = rng.random(n) < nan_frac
        m1 = rng.random(n) < nan_frac
        score = np.where(m0, 2.0, X[:, 0]) + np.where(m1, -2.0, X[:, 1])
        X[rng.random(size=X.shape) < nan_frac] = np.nan
        X[m0, 0] = np.nan
        X[m1, 1] = np.nan
    y = (score + rng.normal(scale=0.3, size=n) > 0).astype(np.float32)
    return X, y


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


def _train_both(hip, params, X, y):
    hip.set_partition_mode("classic")
    ref, m_ref = _train(params, X, y)
    hip.set_partition_mode("staged")
    bst, m = _train(params, X, y)
    _assert_same_trees(ref.trees, bst.trees, "staged vs classic")
    assert m.dtype == torch.float32 and m.shape == m_ref.shape
    assert torch.equal(m, m_ref), "margins differ"
    return bst


@pytest.mark.parametrize("max_depth", [2, 3, 6])
@pytest.mark.parametrize("f", [8, 28, 5])
@pytest.mark.parametrize("n", [1, 255, 2 * 2048 + 3, 3 * BIG_TILE + 5])
def test_training_both_modes(hip, n, f, max_depth):
    X, y = _data(n, f, seed=n + f)
    _train_both(hip, dict(BINARY, max_depth=max_depth), X, y)


def test_training_missing_values(hip):
    X, y = _data(4099, 28, seed=7, nan_frac=0.2)
    bst = _train_both(hip, BINARY, X, y)
    assert {bool(d) for t in bst.trees for d, l in zip(t.default_left, t.left) if l >= 0} == {True, False}


def test_training_leaf_scatter_copies_row_ids(hip, monkeypatch):
    monkeypatch.setenv("SMXGB_LEAF_UPDATE", "scatter")
    X, y = _data(3 * BIG_TILE + 5, 28, seed=8)
    _train_both(hip, BINARY, X, y)


def test_training_subsample(hip):
    X, y = _data(3 * BIG_TILE + 5, 28, seed=9)
    _train_both(hip, dict(BINARY, subsample=0.6, seed=5), X, y)


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


@pytest.mark.parametrize("leaf_update", ["traverse", "scatter"])
def test_per_level_path_selects_the_same_kernel(hip, monkeypatch, leaf_update):
    """The loop taken with a communicator grows, in both modes, the tree the
    whole-tree enqueue grows."""
    from sagemaker_xgboost_container_amd.models.grower import HistGrower
    from sagemaker_xgboost_container_amd.ops.quantize import quantize

    monkeypatch.setenv("SMXGB_LEAF_UPDATE", leaf_update)
    D = 6
    n = 3 * BIG_TILE + 5
    X, y = _data(n, 28, seed=14, nan_frac=0.2)
    qm = quantize(torch.tensor(X, device="cuda"), max_bin=256)
    yt = torch.tensor(y, device="cuda")
    gh = torch.stack([0.5 - yt, torch.full_like(yt, 0.25)], dim=1).contiguous()

    levels = []
    real = hip._K.grow_partition_level

    def counted(*args):
        levels.append(args[-1])
        return real(*args)

    def grow(comm):
        grower = HistGrower(qm, {"max_depth": D, "eta": 0.3}, comm=comm)
        tree, leaf_jobs = grower.grow(gh)
        assert grower.grow_path == "device"
        margin = torch.zeros(n, dtype=torch.float32, device="cuda")
        grower.state.update_margins(margin, leaf_jobs)
        return tree, margin.cpu()

    monkeypatch.setattr(hip._K, "grow_partition_level", counted)
    ref = None
    for mode in ("classic", "staged"):
        hip.set_partition_mode(mode)
        for comm in (None, _OneRank()):
            del levels[:]
            tree, margin = grow(comm)
            assert bool(levels) == (comm is not None)
            if ref is None:
                ref = (tree, margin)
                continue
            _assert_same_trees([ref[0]], [tree], f"{mode} comm={comm is not None}")
            assert torch.equal(margin, ref[1]), f"{mode} comm={comm is not None}: margins differ"
