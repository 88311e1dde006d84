"""Level histograms with the slab resident across a block's virtual blocks.

`hist_device_kernel` deals a level's virtual blocks out in contiguous ranges,
feature-group-major, and flushes its LDS slab to `acc` only where the (slot,
feature group) changes. The sums are int64 fixed point, so every grid must
give the same bits: each comparison is `torch.equal` against an int64
histogram computed with torch on the CPU from the same
`llrintf(g * 2^33 / max)` values.

The level is the smallest that crosses every boundary: four slots of 5000, 0,
1 and 9000 rows at 2048 rows per block are 3 + 0 + 1 + 5 = 9 virtual blocks
(times the feature groups of a grouped layout), run at grids below, at and
above that count. Grid 1 crosses every slot and group boundary in one block,
grid 64 leaves most blocks without work, grid 0 is the extension's own rule.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 14001
ROWS_PER_BLOCK = 2048
GRIDS = (1, 2, 7, 9, 64, 0)
SENTINEL = -7
# (bin type, features, stride)
LAYOUTS = {
    "u8_28_vec4_single_slab": (torch.uint8, 28, 256),
    "u8_5_scalar": (torch.uint8, 5, 256),
    "int16_28": (torch.int16, 28, 300),
    "u8_54_grouped": (torch.uint8, 54, 256),
}


@functools.lru_cache(maxsize=None)
def _level(layout):
    """Inputs of one layout, shared and left unchanged by every test: CPU
    bins, the fixed-point (g, h) of every row, and the device tensors."""
    from sagemaker_xgboost_container_amd.ops import hip

    dtype, f, stride = LAYOUTS[layout]
    g = torch.Generator().manual_seed(f * 1000 + stride)
    missing_bin = stride - 1
    bins = torch.randint(0, stride, (N, f), generator=g)
    bins[3::40, 1] = missing_bin
    bins[7::40, f - 1] = missing_bin
    gh = torch.stack([torch.randn(N, generator=g), torch.rand(N, generator=g)], dim=1)
    gh_max = gh.abs().amax(0)
    # fixed point exactly as the kernel: float32 scale, float32 product,
    # round half to even, summed as int64
    scale = torch.tensor(8589934592.0) / gh_max.clamp(min=1e-30)
    fixed = torch.round(gh * scale).to(torch.int64)
    groups, lds_words, hist_block = hip._device_hist_plan(f, stride)
    return {
        "dtype": dtype, "f": f, "stride": stride, "missing_bin": missing_bin,
        "bins": bins, "fixed": fixed,
        "bins_dev": bins.to(dtype).cuda(), "gh_dev": gh.cuda(), "gh_max_dev": gh_max.cuda(),
        "n_groups": len(groups), "feats_per_group": groups[0][1] - groups[0][0],
        "lds_words": lds_words, "hist_block": hist_block,
    }


def _hist_of(lv, rows):
    """int64 [f * stride, 2] histogram of the given rows."""
    f, stride = lv["f"], lv["stride"]
    out = torch.zeros((f * stride, 2), dtype=torch.int64)
    idx = (lv["bins"][rows] + torch.arange(f) * stride).reshape(-1)
    for c in range(2):
        out[:, c].index_add_(0, idx, lv["fixed"][rows, c].repeat_interleave(f))
    return out


def _launch(lv, nodes, hp, work, acc, k, grid, slot_lo=0, slot_hi=1 << 30, par_splits=None,
            predicate_only=0):
    from sagemaker_xgboost_container_amd.ops import hip

    if par_splits is None:
        par_splits = torch.empty(0, dtype=torch.float32, device="cuda")
    hip._K.grow_hist_level(
        lv["bins_dev"], lv["gh_dev"], nodes, hp, work, acc, k, lv["f"], lv["stride"],
        lv["n_groups"], lv["feats_per_group"], lv["gh_max_dev"], ROWS_PER_BLOCK, grid,
        lv["lds_words"], lv["hist_block"], slot_lo, slot_hi, par_splits, lv["missing_bin"],
        predicate_only,
    )
    return acc.cpu().view(k, lv["f"] * lv["stride"], 2)


# the plain level: every slot builds from its own rows
PLAIN_RANGES = [(0, 5000), (5000, 5000), (5000, 5001), (5001, N)]
PLAIN_PREFIX = [0, 3, 3, 4, 9]


def _plain_tables():
    nodes = torch.tensor([[s, e, 1] for s, e in PLAIN_RANGES], dtype=torch.int32, device="cuda")
    hp = torch.tensor(PLAIN_PREFIX, dtype=torch.int32, device="cuda")
    work = torch.tensor([PLAIN_PREFIX[-1], PLAIN_PREFIX[-1]], dtype=torch.int32, device="cuda")
    return nodes, hp, work


@functools.lru_cache(maxsize=None)
def _plain_expect(layout):
    lv = _level(layout)
    return torch.stack([_hist_of(lv, torch.arange(s, e)) for s, e in PLAIN_RANGES])


def test_layouts_take_the_paths_they_are_named_for():
    assert _level("u8_28_vec4_single_slab")["hist_block"] == 512
    assert _level("u8_28_vec4_single_slab")["n_groups"] == 1
    assert _level("u8_5_scalar")["n_groups"] == 1
    assert _level("int16_28")["bins_dev"].dtype == torch.int16
    grouped = _level("u8_54_grouped")
    assert grouped["n_groups"] > 1 and grouped["hist_block"] == 256
    assert [-(-(e - s) // ROWS_PER_BLOCK) for s, e in PLAIN_RANGES] == [3, 0, 1, 5]


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_plain_level_every_grid(layout):
    lv = _level(layout)
    nodes, hp, work = _plain_tables()
    expect = _plain_expect(layout)
    assert int(expect[1].abs().sum()) == 0 and int(expect[2].abs().sum()) > 0
    for grid in GRIDS:
        acc = torch.zeros((4, lv["f"] * lv["stride"] * 2), dtype=torch.int64, device="cuda")
        got = _launch(lv, nodes, hp, work, acc, 4, grid)
        assert torch.equal(got, expect), f"grid {grid}"


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_slot_window_leaves_the_rest_of_acc_alone(layout):
    lv = _level(layout)
    nodes, hp, work = _plain_tables()
    expect = _plain_expect(layout).clone()
    expect[0] = 0
    expect[3] = 0
    expect += SENTINEL
    for grid in GRIDS:
        acc = torch.full((4, lv["f"] * lv["stride"] * 2), SENTINEL, dtype=torch.int64,
                         device="cuda")
        got = _launch(lv, nodes, hp, work, acc, 4, grid, slot_lo=1, slot_hi=3)
        assert torch.equal(got, expect), f"grid {grid}"


# the filtered level: four parents; (range, (gain, feature, split_bin,
# default_left, left G, left H), node H, build side)
def _filter_parents(lv):
    f, stride = lv["f"], lv["stride"]
    return [
        ((0, 5000), [1.0, 1.0, float(stride // 3), 1.0, 0.5, 4.0], 10.0, 0),
        # dead: holds rows, has no split
        ((5000, 5300), [0.0, 0.0, 0.0, 0.0, 0.0, 0.0], 10.0, None),
        ((5300, 5301), [1.0, float(f - 1), float(stride // 2), 0.0, 1.5, 8.0], 10.0, 1),
        # every row goes left and the right child builds: its filter keeps none
        ((5301, N), [1.0, 0.0, float(stride - 1), 1.0, 1.5, 15.0], 20.0, 1),
    ]


@functools.lru_cache(maxsize=None)
def _filter_expect(layout):
    lv = _level(layout)
    expect = torch.zeros((8, lv["f"] * lv["stride"], 2), dtype=torch.int64)
    kept = []
    for p, ((start, end), sp, _, side) in enumerate(_filter_parents(lv)):
        if side is None:
            continue
        b = lv["bins"][start:end, int(sp[1])]
        left = torch.where(b == lv["missing_bin"], torch.tensor(sp[3] > 0.5), b <= int(sp[2]))
        keep = left if side == 0 else ~left
        kept.append(int(keep.sum()))
        expect[2 * p + side] = _hist_of(lv, torch.arange(start, end)[keep])
    assert kept[0] > 0 and kept[2] == 0, kept
    return expect


@pytest.mark.parametrize("predicate_only", [0, 1])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_filtered_level_every_grid(layout, predicate_only):
    from sagemaker_xgboost_container_amd.ops import hip

    lv = _level(layout)
    parents = _filter_parents(lv)
    cur = torch.tensor([[s, e, 1] for (s, e), _, _, _ in parents], dtype=torch.int32,
                       device="cuda")
    splits = torch.tensor([sp for _, sp, _, _ in parents], dtype=torch.float32, device="cuda")
    node_gh = torch.tensor([[1.0, h] for _, _, h, _ in parents], dtype=torch.float32,
                           device="cuda")
    counts = torch.zeros((4, 2), dtype=torch.int32, device="cuda")
    nxt = torch.full((8, 3), -7, dtype=torch.int32, device="cuda")
    nxt_gh = torch.zeros((8, 2), dtype=torch.float32, device="cuda")
    hp = torch.zeros(9, dtype=torch.int32, device="cuda")
    pp = torch.zeros(9, dtype=torch.int32, device="cuda")
    work = torch.zeros(2, dtype=torch.int32, device="cuda")
    hip._K.grow_make_level(cur, splits, counts, node_gh, nxt, nxt_gh, hp, pp, work, 4,
                           ROWS_PER_BLOCK, hip._MAX_BLOCKS_PER_JOB, 1)
    # blocks are counted from the parent's rows; only the build child has any
    assert hp.cpu().tolist() == [0, 3, 3, 3, 3, 3, 4, 4, 9]
    assert nxt.cpu().tolist() == [
        [0, 5000, 1], [0, 5000, 0], [0, 0, 0], [0, 0, 0],
        [5300, 5301, 0], [5300, 5301, 1], [5301, N, 0], [5301, N, 1],
    ]
    expect = _filter_expect(layout)
    for grid in GRIDS:
        acc = torch.zeros((8, lv["f"] * lv["stride"] * 2), dtype=torch.int64, device="cuda")
        got = _launch(lv, nxt, hp, work, acc, 8, grid, par_splits=splits,
                      predicate_only=predicate_only)
        assert torch.equal(got, expect), f"grid {grid}"


def test_tree_levels_start_from_the_acc_the_convert_launch_zeroed():
    """Two depth-3 trees on 20 000 rows through grow_tree_enqueue: each built
    slot of levels 0, 1 and 2 holds the float32 image of the reference sums
    of exactly its rows, which it cannot if the level before it (or the tree
    before it) left anything in `acc`; `acc` is all zero afterwards."""
    from sagemaker_xgboost_container_amd.models.grower import HistGrower
    from sagemaker_xgboost_container_amd.ops.quantize import quantize

    D, n, f = 3, 20000, 28
    rng = np.random.default_rng(5)
    X = rng.normal(size=(n, f)).astype(np.float32)
    y = (X[:, 0] * 2 - X[:, 1] + 0.5 * X[:, 2] * X[:, 3] > 0).astype(np.float32)
    qm = quantize(torch.tensor(X, device="cuda"), max_bin=256)
    assert qm.bins.dtype == torch.uint8
    stride = qm.stride
    missing_bin = stride - 1 if qm.has_missing else -1
    bins = qm.bins.cpu().long()
    cols = torch.arange(f) * stride
    yt = torch.tensor(y, device="cuda")
    grower = HistGrower(qm, {"max_depth": D, "eta": 0.3})

    for tree_no, shift in enumerate((0.5, 0.3)):
        gh = torch.stack([shift - yt, torch.full_like(yt, 0.25) + 0.1 * yt * tree_no],
                         dim=1).contiguous()
        grower.grow(gh)
        assert grower.grow_path == "device"
        dg = grower._device_grower_for(0)
        torch.cuda.synchronize()
        assert int(dg.acc.abs().sum()) == 0

        gh_cpu = gh.cpu()
        gh_max = gh_cpu.abs().amax(0)
        fixed = torch.round(gh_cpu * (torch.tensor(8589934592.0) / gh_max.clamp(min=1e-30)))
        fixed = fixed.to(torch.int64)
        inv = gh_max.clamp(min=1e-30).double() / 8589934592.0
        nodes = dg.nodes.cpu()
        splits = dg.splits.cpu()
        hist = dg.hist_f32.cpu().view(-1, f * stride, 2)

        rows_of = {0: torch.arange(n)}
        built = 0
        for d in range(D):
            for slot in range(1 << d):
                heap = (1 << d) - 1 + slot
                rows = rows_of.get(heap)
                if rows is None:
                    continue
                start, end, build = nodes[heap].tolist()
                assert end > start
                if build:
                    acc_ref = torch.zeros((f * stride, 2), dtype=torch.int64)
                    idx = (bins[rows] + cols).reshape(-1)
                    for c in range(2):
                        acc_ref[:, c].index_add_(0, idx, fixed[rows, c].repeat_interleave(f))
                    want = (acc_ref.double() * inv).float()
                    built += 1
                else:
                    sibling = heap + 1 if slot % 2 == 0 else heap - 1
                    want = hist[(heap - 1) // 2] - hist[sibling]
                assert torch.equal(hist[heap], want), f"tree {tree_no} level {d} slot {slot}"
                gain, feat, sbin, dleft = splits[heap, :4].tolist()
                if gain > 0 and d < D - 1:
                    b = bins[rows, int(feat)]
                    left = torch.where(b == missing_bin, torch.tensor(dleft > 0.5), b <= int(sbin))
                    rows_of[2 * heap + 1] = rows[left]
                    rows_of[2 * heap + 2] = rows[~left]
        # the root and one child of every pair below it
        assert built == 1 + 1 + 2, built
