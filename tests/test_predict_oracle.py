"""Dense forest prediction (margins and leaf ids) against a float64 oracle.

The dense kernels (predict_kernel / pred_leaf_kernel in
ops/csrc/smxgb_kernels.hip) and their host twins (predict_forest_cpu /
pred_leaf_cpu) are what the CSR kernels, the booster routes and the SHAP
additivity checks are compared with, so they are pinned here by an oracle that
shares no code with ops/: plain numpy, level by level, float64.

* Forests are exact by construction: leaf values i/1024 (|i| <= 1024), DART
  weights in eighths, T <= 500. Every partial sum is a multiple of 2^-13 below
  2^9, hence a float32 in any summation order, and the comparison is
  np.array_equal.
* Trees never repeat a feature on a path, so a row can be built that reaches
  any given node. For every internal node of a targeted tree three rows are
  built: x == thr (must go right), x == nextafter(thr, -inf) (must go left)
  and x == NaN (must follow default_left). The coverage this promises is
  asserted from the oracle's counters before any kernel is compared.

GPU tests are marked one by one; the host-backend half runs on a CPU box.
"""
import gc

import numpy as np
import pytest
import torch

from sagemaker_xgboost_container_amd.data.dmatrix import DMatrix
from sagemaker_xgboost_container_amd.models.booster import Booster
from sagemaker_xgboost_container_amd.models.tree import Tree
from sagemaker_xgboost_container_amd.ops import torch_ref

if torch.cuda.is_available():
    from sagemaker_xgboost_container_amd.ops import hip
else:  # allow collection on CPU boxes
    hip = None

_GPU = pytest.param("gpu", marks=pytest.mark.gpu)
_BACKENDS = ["host", _GPU]

_F32_MAX = np.finfo(np.float32).max
# thresholds beyond the eighths: both zeros, both smallest denormals, the
# largest float and a value that is no dyadic fraction
_SPECIAL_THR = np.array([0.0, -0.0, 1e-45, -1e-45, _F32_MAX, 0.1], dtype=np.float32)
_NEG_INF = np.float32(-np.inf)
_POS_INF = np.float32(np.inf)


# -- the oracle ----------------------------------------------------------------
def _walk(tree, X):
    """One tree over all rows, level by level, in float64. Returns the
    tree-local leaf id per row and the per-node counters."""
    n = X.shape[0]
    X64 = X.astype(np.float64)  # exact: every comparison equals the fp32 one
    thr = np.asarray(tree.threshold, dtype=np.float32).astype(np.float64)
    left = np.asarray(tree.left, dtype=np.int64)
    right = np.asarray(tree.right, dtype=np.int64)
    feat = np.asarray(tree.feature, dtype=np.int64)
    defl = np.asarray(tree.default_left, dtype=bool)
    m = left.shape[0]
    counts = {name: np.zeros(m, dtype=np.int64) for name in ("left", "right", "equal", "nan")}
    node = np.zeros(n, dtype=np.int64)
    rows = np.nonzero(left[node] >= 0)[0]
    while rows.size:
        cur = node[rows]
        x = X64[rows, feat[cur]]
        missing = np.isnan(x)
        with np.errstate(invalid="ignore"):
            go_left = np.where(missing, defl[cur], x < thr[cur])
            equal = ~missing & (x == thr[cur])
        counts["left"] += np.bincount(cur[go_left], minlength=m)
        counts["right"] += np.bincount(cur[~go_left], minlength=m)
        counts["equal"] += np.bincount(cur[equal], minlength=m)
        counts["nan"] += np.bincount(cur[missing], minlength=m)
        node[rows] = np.where(go_left, left[cur], right[cur])
        rows = rows[left[node[rows]] >= 0]
    return node.astype(np.int32), counts


def _oracle(trees, tree_info, weight_drop, X, k, t_begin, t_end, walks=None):
    """(sums (n, k) f64, leaf ids (n, T) i32, sums of |value| (n, k) f64,
    per-tree node counters) of trees [t_begin, t_end). `walks` caches
    _walk(tree, X) per tree index for an X that never changes."""
    n = X.shape[0]
    T = max(0, t_end - t_begin)
    sums = np.zeros((n, k), dtype=np.float64)
    mags = np.zeros((n, k), dtype=np.float64)
    leaves = np.zeros((n, T), dtype=np.int32)
    counters = []
    for j, t in enumerate(range(t_begin, t_end)):
        if walks is not None and t in walks:
            leaf, counts = walks[t]
        else:
            leaf, counts = _walk(trees[t], X)
            if walks is not None:
                walks[t] = (leaf, counts)
        w = np.float64(weight_drop[t]) if weight_drop else np.float64(1.0)
        v = np.asarray(trees[t].value, dtype=np.float32).astype(np.float64)[leaf] * w
        sums[:, tree_info[t]] += v
        mags[:, tree_info[t]] += np.abs(v)
        leaves[:, j] = leaf
        counters.append(counts)
    return sums, leaves, mags, counters


# -- forests ---------------------------------------------------------------------
def _draw_threshold(rng):
    if rng.random() < 0.35:
        return float(_SPECIAL_THR[rng.integers(0, _SPECIAL_THR.size)])
    return float(np.round(rng.normal() * 8) / 8)


def _exact_value(rng):
    return float(rng.integers(-1024, 1025)) / 1024.0


def _make_tree(rng, f, depth, value):
    """Ragged tree of at most `depth` <= f levels (a stump for depth 0) that
    never repeats a feature along a root-to-leaf path."""
    assert depth <= f
    tree = Tree()
    frontier = [(tree.add_node(value=value(rng)), ())]
    for level in range(depth):
        nxt = []
        for nid, used in frontier:
            if level > 0 and rng.random() < 0.25:
                continue  # stays a leaf: ragged
            free = [j for j in range(f) if j not in used]
            feature = int(free[rng.integers(0, len(free))])
            lid, rid = tree.apply_split(
                nid, feature, _draw_threshold(rng), 0, bool(rng.integers(0, 2)), 1.0,
                left_value=value(rng), right_value=value(rng), left_hess=1.0, right_hess=1.0,
            )
            nxt += [(lid, used + (feature,)), (rid, used + (feature,))]
        frontier = nxt
    return tree.finalize()


def _make_trees(f, n_trees, depth_cap, seed, value=_exact_value):
    """Depths 1..8 in turn (capped), every 9th tree a stump."""
    rng = np.random.default_rng(seed)
    depths = [min((i + 1) % 9, depth_cap) for i in range(n_trees)]
    if n_trees == 1:
        depths = [min(5, depth_cap)]
    return [_make_tree(rng, f, d, value) for d in depths]


def _eighths(n_trees):
    """DART weights as _forest(..., weights=True) of test_gpu_sparse_predict."""
    return [0.5 + 0.125 * (i % 5) for i in range(n_trees)]


# -- probe rows --------------------------------------------------------------------
def _below(x):
    return np.nextafter(np.float32(x), _NEG_INF)


def _threshold_pool(trees):
    pool = [np.asarray(t.threshold, dtype=np.float32)[np.asarray(t.left) >= 0] for t in trees]
    pool = np.concatenate(pool) if pool else np.zeros(0, dtype=np.float32)
    return pool if pool.size else np.zeros(1, dtype=np.float32)


def _random_probes(rng, pool, shape):
    """Draws from {thr, nextafter(thr, +-inf), NaN, +-inf, +-0}."""
    thr = pool[rng.integers(0, pool.size, size=shape)]
    kind = rng.integers(0, 8, size=shape)
    out = thr.copy()
    out = np.where(kind == 1, np.nextafter(thr, _NEG_INF), out)
    with np.errstate(over="ignore"):  # above the largest float lies +inf
        out = np.where(kind == 2, np.nextafter(thr, _POS_INF), out)
    out = np.where(kind == 3, np.float32(np.nan), out)
    out = np.where(kind == 4, _POS_INF, out)
    out = np.where(kind == 5, _NEG_INF, out)
    out = np.where(kind == 6, np.float32(0.0), out)
    out = np.where(kind == 7, np.float32(-0.0), out)
    return out.astype(np.float32)


def _rows_for_tree(rng, tree, f, pool):
    """Three rows per internal node that reach it (x == thr, x just below thr,
    x NaN): each ancestor's feature is set just below its threshold to go left
    or to the threshold itself to go right; every other feature is a random
    probe."""
    internal = np.nonzero(np.asarray(tree.left) >= 0)[0]
    rows = _random_probes(rng, pool, (3 * internal.size, f))
    for i, v in enumerate(internal):
        blk = rows[3 * i:3 * i + 3]
        node = int(v)
        while tree.parent[node] >= 0:
            p = int(tree.parent[node])
            thr = np.float32(tree.threshold[p])
            blk[:, tree.feature[p]] = _below(thr) if tree.left[p] == node else thr
            node = p
        thr = np.float32(tree.threshold[v])
        blk[0, tree.feature[v]] = thr
        blk[1, tree.feature[v]] = _below(thr)
        blk[2, tree.feature[v]] = np.nan
    return rows


def _assert_coverage(trees, blocks):
    """Every internal node of a targeted tree sees, among the rows built for
    that tree, both directions, an exact-equality visit and a NaN visit. A
    failure is a mistake in this file, never a reason to skip."""
    for t, rows in blocks.items():
        _, counts = _walk(trees[t], rows)
        internal = np.asarray(trees[t].left) >= 0
        for name in ("left", "right", "equal", "nan"):
            missed = np.nonzero(internal & (counts[name] == 0))[0]
            assert missed.size == 0, f"tree {t}: nodes {missed.tolist()} see no '{name}' visit"
        leaf_visits = counts["left"] + counts["right"]
        assert (leaf_visits[~internal] == 0).all()


class _Case:
    """A forest, its matrix and the cached oracle walks; built once, shared by
    the GPU and the host tests, never modified."""

    def __init__(self, n, n_trees, f, depth_cap=8, seed=0, value=_exact_value):
        self.n, self.T, self.f = n, n_trees, f
        self.trees = _make_trees(f, n_trees, min(depth_cap, f), seed + 7 * n_trees, value)
        rng = np.random.default_rng(seed + n)
        pool = _threshold_pool(self.trees)
        self.targeted = {}
        used = 0
        for t in rng.permutation(n_trees):
            need = 3 * int((np.asarray(self.trees[t].left) >= 0).sum())
            if need == 0 or used + need > n:
                continue
            self.targeted[int(t)] = _rows_for_tree(rng, self.trees[t], f, pool)
            used += need
        parts = list(self.targeted.values()) + [_random_probes(rng, pool, (n - used, f))]
        self.X = np.concatenate(parts, axis=0)[rng.permutation(n)] if n else np.zeros((0, f), np.float32)
        assert self.X.shape == (n, f) and self.X.dtype == np.float32
        self.walks = {}
        self._oracles = {}
        self._flats = {}
        self._X = {}

    def info(self, k):
        return [i % k for i in range(self.T)]

    def oracle(self, k, weights, t_begin=0, t_end=None):
        t_end = self.T if t_end is None else t_end
        key = (k, weights, t_begin, t_end)
        if key not in self._oracles:
            wd = _eighths(self.T) if weights else None
            self._oracles[key] = _oracle(
                self.trees, self.info(k), wd, self.X, k, t_begin, t_end, self.walks
            )
        return self._oracles[key]

    def flat(self, backend, k, weights):
        key = (backend, k, weights)
        if key not in self._flats:
            wd = _eighths(self.T) if weights else None
            mod, dev = _backend(backend)
            self._flats[key] = mod.make_flat_forest(self.trees, self.info(k), wd, dev)
        return self._flats[key]

    def tensor(self, backend):
        if backend not in self._X:
            self._X[backend] = torch.from_numpy(self.X).to(_backend(backend)[1])
        return self._X[backend]


def _backend(backend):
    if backend == "gpu":
        return hip, torch.device("cuda")
    return torch_ref, torch.device("cpu")


# (n, T, f, depth cap) -> the regime the shape is named for, as a predicate
# over hip._predict_chunking(n, T) = (n_chunks, trees_per_chunk)
_PREDICT_SHAPES = {
    "n1-T1-minimal": ((1, 1, 8, 8), lambda c, tpc, n, T: c == 1),
    "n1-T500-one-tree-per-chunk": ((1, 500, 8, 8), lambda c, tpc, n, T: c == T and tpc == 1),
    "n255-T7-below-block": ((255, 7, 8, 8), lambda c, tpc, n, T: n < 256 and c == T),
    "n257-T300-above-block": ((257, 300, 8, 8), lambda c, tpc, n, T: n > 256 and c == T and tpc == 1),
    "n3000-T100-ragged-last-chunk": (
        (3000, 100, 8, 8), lambda c, tpc, n, T: tpc == 3 and T - (c - 1) * tpc == 1),
    "n1000-T500-several-per-chunk": (
        (1000, 500, 8, 8), lambda c, tpc, n, T: tpc > 1 and c > 1),
    "n131075-T3-single-chunk": ((131075, 3, 4, 4), lambda c, tpc, n, T: c == 1),
    "n1048579-T2-grid-stride-tail": (
        (1048579, 2, 2, 2), lambda c, tpc, n, T: c == 1 and n * c > 4096 * 256),
}
# pred_leaf has one item per (row, tree): its own grid-stride tail
_LEAF_ONLY_SHAPES = {
    "n4099-T257-leaf-grid-stride-tail": ((4099, 257, 8, 8), None),
}
_RANGE_SHAPES = [
    "n1-T500-one-tree-per-chunk", "n257-T300-above-block",
    "n3000-T100-ragged-last-chunk", "n1000-T500-several-per-chunk",
]
_cases = {}


def _case(name):
    if name not in _cases:
        spec = {**_PREDICT_SHAPES, **_LEAF_ONLY_SHAPES, **_EXTRA_SHAPES}[name][0]
        n, T, f, cap = spec[:4]
        _cases[name] = _Case(n, T, f, cap, seed=len(name), **(spec[4] if len(spec) > 4 else {}))
    return _cases[name]


def _normal_value(rng):
    return float(rng.normal())


_EXTRA_SHAPES = {
    # a range inside a larger forest whose last chunk is ragged: dropping the
    # min() of the chunk end would add trees 105 and 106 (in bounds, wrong sum)
    "n3000-T120-inner-range": ((3000, 120, 8, 8), None),
    "n1000-T500-normal": ((1000, 500, 8, 8, {"value": _normal_value}), None),
    "n3000-T100-normal": ((3000, 100, 8, 8, {"value": _normal_value}), None),
}


@pytest.fixture(scope="module", autouse=True)
def _release_caches():
    yield
    _cases.clear()
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


def _ranges(T):
    return [(0, T), (3, 11), (T - 1, T), (7, 7)]


def _assert_exact(got, want64):
    """Bit equality with the float64 oracle, which must itself be a float32."""
    want = want64.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), want64), "oracle sum is no float32"
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(got, want)


def _assert_leaves(got, want):
    got = got.cpu().numpy()
    assert got.dtype == np.int32 and got.shape == want.shape
    assert np.array_equal(got, want)


# -- the construction keeps its promises ----------------------------------------------
class TestConstruction:
    @pytest.mark.parametrize("name", list(_PREDICT_SHAPES) + list(_LEAF_ONLY_SHAPES))
    def test_coverage(self, name):
        case = _case(name)
        _assert_coverage(case.trees, case.targeted)
        if case.n >= 255:
            assert case.targeted, "no tree fits the row budget"
            defl = np.concatenate([
                np.asarray(case.trees[t].default_left)[np.asarray(case.trees[t].left) >= 0]
                for t in case.targeted
            ])
            assert defl.any() and not defl.all(), "one default direction never occurs"
        # the whole matrix, all trees: the counters of the full oracle agree
        # with the leaf ids (every row ends in a leaf, visits add up)
        _, leaves, _, counters = case.oracle(1, False)
        for t, counts in enumerate(counters):
            left = np.asarray(case.trees[t].left)
            assert (left[leaves[:, t]] < 0).all()
            root_visits = counts["left"][0] + counts["right"][0]
            assert root_visits == (case.n if left[0] >= 0 else 0)

    def test_forests_are_ragged_and_special(self):
        case = _case("n1000-T500-several-per-chunk")
        depths = {t.max_depth() for t in case.trees}
        assert depths >= set(range(0, 9))
        thr = _threshold_pool(case.trees)
        for special in _SPECIAL_THR:
            hit = (thr == special) & (np.signbit(thr) == np.signbit(special))
            assert hit.any(), f"threshold {special!r} never drawn"
        for t in case.trees:  # no feature twice on a path
            for leaf in np.nonzero(np.asarray(t.left) < 0)[0]:
                seen, node = [], int(leaf)
                while t.parent[node] >= 0:
                    node = int(t.parent[node])
                    seen.append(int(t.feature[node]))
                assert len(seen) == len(set(seen))

    def test_oracle_on_a_hand_made_tree(self):
        """The oracle itself, on a tree small enough to check by eye."""
        tree = Tree()
        root = tree.add_node(value=0.0)
        lid, rid = tree.apply_split(root, 1, 0.5, 0, True, 1.0, left_value=0.25,
                                    right_value=-0.5, left_hess=1.0, right_hess=1.0)
        tree.apply_split(rid, 0, -0.0, 0, False, 1.0, left_value=1.0, right_value=0.125,
                         left_hess=1.0, right_hess=1.0)
        tree.finalize()
        X = np.array([
            [9.0, 0.5],            # 0.5 < 0.5 is false -> right; 9 >= -0 -> right: 0.125
            [9.0, _below(0.5)],    # left: 0.25
            [9.0, np.nan],         # default left: 0.25
            [0.0, 1.0],            # right; 0.0 < -0.0 is false -> right: 0.125
            [-1e-45, 1.0],         # right; denormal below zero -> left: 1.0
            [np.nan, np.inf],      # right; NaN, default right: 0.125
            [-np.inf, -np.inf],    # left: 0.25
        ], dtype=np.float32)
        sums, leaves, mags, counters = _oracle([tree], [1], [0.5], X, 2, 0, 1)
        want = np.array([0.125, 0.25, 0.25, 0.125, 1.0, 0.125, 0.25]) * 0.5
        assert np.array_equal(sums[:, 1], want) and not sums[:, 0].any()
        assert np.array_equal(mags[:, 1], np.abs(want))
        assert leaves[:, 0].tolist() == [4, 1, 1, 4, 3, 4, 1]
        assert counters[0]["left"].tolist() == [3, 0, 1, 0, 0]
        assert counters[0]["right"].tolist() == [4, 0, 3, 0, 0]
        assert counters[0]["equal"].tolist() == [1, 0, 1, 0, 0]
        assert counters[0]["nan"].tolist() == [1, 0, 1, 0, 0]


# -- margins -----------------------------------------------------------------------
@pytest.mark.parametrize("backend", _BACKENDS)
class TestPredictExact:
    @pytest.mark.parametrize("weights", [False, True], ids=["plain", "dart"])
    @pytest.mark.parametrize("k", [1, 3])
    @pytest.mark.parametrize("name", list(_PREDICT_SHAPES))
    def test_shapes(self, backend, name, k, weights):
        case = _case(name)
        mod, _ = _backend(backend)
        if backend == "gpu":
            regime = _PREDICT_SHAPES[name][1]
            assert regime(*hip._predict_chunking(case.n, case.T), case.n, case.T)
        got = mod.predict_forest_flat(case.flat(backend, k, weights), case.tensor(backend), k)
        _assert_exact(got, case.oracle(k, weights)[0])

    @pytest.mark.parametrize("weights", [False, True], ids=["plain", "dart"])
    @pytest.mark.parametrize("name", _RANGE_SHAPES)
    def test_tree_ranges(self, backend, name, weights):
        case = _case(name)
        mod, _ = _backend(backend)
        flat, X = case.flat(backend, 3, weights), case.tensor(backend)
        for tb, te in _ranges(case.T):
            got = mod.predict_forest_flat(flat, X, 3, tb, te)
            _assert_exact(got, case.oracle(3, weights, tb, te)[0])
            if tb == te:
                assert not got.cpu().numpy().any()
        # trees 3 and 4 belong to classes 0 and 1: class 2 owns no tree
        got = mod.predict_forest_flat(flat, X, 3, 3, 5).cpu().numpy()
        _assert_exact(got, case.oracle(3, weights, 3, 5)[0])
        assert (got[:, :2].any() or case.n == 1) and not got[:, 2].any()
        assert not np.signbit(got[:, 2]).any()

    def test_range_with_ragged_last_chunk_inside_a_forest(self, backend):
        case = _case("n3000-T120-inner-range")
        mod, _ = _backend(backend)
        if backend == "gpu":
            n_chunks, tpc = hip._predict_chunking(case.n, 100)
            assert tpc == 3 and 100 - (n_chunks - 1) * tpc == 1
        got = mod.predict_forest_flat(case.flat(backend, 3, True), case.tensor(backend), 3, 5, 105)
        _assert_exact(got, case.oracle(3, True, 5, 105)[0])
        # the trees just past the range do change the sums: a chunk that ran
        # over t_end would be seen
        assert not np.array_equal(case.oracle(3, True, 5, 105)[0], case.oracle(3, True, 5, 107)[0])

    def test_no_rows(self, backend):
        case = _case("n255-T7-below-block")
        mod, dev = _backend(backend)
        empty = torch.zeros((0, case.f), dtype=torch.float32, device=dev)
        for k in (1, 3):
            out = mod.predict_forest_flat(case.flat(backend, k, False), empty, k)
            assert out.shape == (0, k) and out.dtype == torch.float32
        assert mod.pred_leaf(case.flat(backend, 1, False), empty).shape == (0, case.T)

    def test_strided_input(self, backend):
        case = _case("n257-T300-above-block")
        _, dev = _backend(backend)
        mod = _backend(backend)[0]
        wide = torch.full((case.n, 2 * case.f), 123.0, dtype=torch.float32, device=dev)
        wide[:, ::2] = case.tensor(backend)
        X = wide[:, ::2]
        assert not X.is_contiguous()
        flat = case.flat(backend, 3, True)
        _assert_exact(mod.predict_forest_flat(flat, X, 3), case.oracle(3, True)[0])
        _assert_leaves(mod.pred_leaf(flat, X), case.oracle(3, True)[1])

    def test_repeated_call_is_bit_identical(self, backend):
        case = _case("n1000-T500-normal")
        mod, _ = _backend(backend)
        flat, X = case.flat(backend, 3, True), case.tensor(backend)
        first = mod.predict_forest_flat(flat, X, 3).cpu().numpy()
        again = mod.predict_forest_flat(flat, X, 3).cpu().numpy()
        assert np.array_equal(first.view(np.uint32), again.view(np.uint32))

    @pytest.mark.parametrize("name", ["n1000-T500-normal", "n3000-T100-normal"])
    def test_arbitrary_values(self, backend, name):
        """Normal leaf values and weights. Bound per cell: 2 T u sum|v|,
        u = 2^-24: the recursive-summation bound gamma_{T-1} sum|v| doubled,
        which holds for any chunk order and covers the rounding of
        value * weight to float32."""
        case = _case(name)
        mod, dev = _backend(backend)
        rng = np.random.default_rng(5)
        wd = [float(w) for w in rng.normal(size=case.T).astype(np.float32)]
        info = case.info(3)
        flat = mod.make_flat_forest(case.trees, info, wd, dev)
        got = mod.predict_forest_flat(flat, case.tensor(backend), 3).cpu().numpy()
        sums, _, mags, _ = _oracle(case.trees, info, wd, case.X, 3, 0, case.T, case.walks)
        bound = 2.0 * case.T * 2.0 ** -24 * mags
        err = np.abs(got.astype(np.float64) - sums)
        print(f"{name} [{backend}]: max |err| {err.max():.3e}, max err/bound "
              f"{(err / np.maximum(bound, 1e-300)).max():.3e}")
        assert (err <= bound).all()


@pytest.mark.gpu
class TestLegacyWrappers:
    def test_predict_forest_and_predict_tree(self):
        case = _case("n257-T300-above-block")
        X = case.tensor("gpu")
        info = case.info(3)
        got = hip.predict_forest(case.trees, info, X, 3)
        _assert_exact(got, case.oracle(3, False)[0])
        start = (np.arange(case.n * 3).reshape(case.n, 3) % 17 - 8) / 8.0
        out = torch.from_numpy(start.astype(np.float32)).cuda()
        res = hip.predict_forest(case.trees, info, X, 3, 3, 11, out=out)
        assert res is out
        _assert_exact(out, case.oracle(3, False, 3, 11)[0] + start)
        deep = max(range(case.T), key=lambda t: case.trees[t].num_nodes)
        got = hip.predict_tree(case.trees[deep], X)
        _assert_exact(got, case.oracle(1, False, deep, deep + 1)[0][:, 0])


# -- leaf ids --------------------------------------------------------------------------
@pytest.mark.parametrize("backend", _BACKENDS)
class TestPredLeaf:
    @pytest.mark.parametrize("name", list(_PREDICT_SHAPES) + list(_LEAF_ONLY_SHAPES))
    def test_shapes(self, backend, name):
        case = _case(name)
        mod, _ = _backend(backend)
        if name in _LEAF_ONLY_SHAPES:
            assert case.n * case.T > 4096 * 256
        got = mod.pred_leaf(case.flat(backend, 1, False), case.tensor(backend))
        _assert_leaves(got, case.oracle(1, False)[1])

    @pytest.mark.parametrize("name", _RANGE_SHAPES)
    def test_tree_ranges(self, backend, name):
        case = _case(name)
        mod, _ = _backend(backend)
        flat, X = case.flat(backend, 3, True), case.tensor(backend)
        for tb, te in _ranges(case.T):
            got = mod.pred_leaf(flat, X, tb, te)
            assert got.shape == (case.n, te - tb)
            _assert_leaves(got, case.oracle(3, True, tb, te)[1])


# -- the booster route --------------------------------------------------------------------
def _booster(case, objective, k, rounds, weights):
    params = {"objective": objective, "base_score": 0.5}
    if k > 1:
        params["num_class"] = k
    bst = Booster(params, num_features=case.f)
    wd = _eighths(case.T)
    for r in range(rounds):
        ids = list(range(r * k, (r + 1) * k))
        bst.add_iteration(
            [case.trees[t] for t in ids], [t % k for t in ids],
            [wd[t] for t in ids] if weights else None,
        )
    return bst


@pytest.mark.parametrize("backend", _BACKENDS)
@pytest.mark.parametrize("objective,k", [("reg:squarederror", 1), ("multi:softprob", 3)])
class TestBoosterRoute:
    def test_margin_equals_oracle_plus_start(self, backend, objective, k):
        case = _case("n257-T300-above-block")
        rounds = 30
        bst = _booster(case, objective, k, rounds, weights=True)
        if backend == "host":
            bst.set_param("predictor", "cpu_predictor")
        assert str(bst._predict_device().type) == ("cuda" if backend == "gpu" else "cpu")

        def want(lo, hi, start):
            sums = case.oracle(k, True, lo * k, hi * k)[0] + start
            return sums[:, 0] if k == 1 else sums

        _assert_exact(bst.predict(case.X, output_margin=True), want(0, rounds, 0.5))
        _assert_exact(
            bst.predict(case.X, output_margin=True, iteration_range=(2, 9)), want(2, 9, 0.5)
        )
        base = ((np.arange(case.n * k).reshape(case.n, k) % 33) - 16) / 8.0
        dm = DMatrix(case.X, base_margin=base.astype(np.float32))
        _assert_exact(
            bst.predict(dm, output_margin=True, iteration_range=(2, 9)), want(2, 9, base)
        )
        _assert_exact(bst.predict(dm, output_margin=True), want(0, rounds, base))


# -- narrow and malformed input is refused before anything runs -------------------------------
def _narrow_case():
    """Nine trees over eight features; the first three are rebuilt to split
    on features 0..2 only, so a three-column matrix serves range (0, 3)."""
    if "narrow" not in _cases:
        case = _Case(300, 9, 8, 8, seed=3)
        small = _make_trees(3, 3, 3, seed=4)
        case.trees[:3] = small
        case.walks.clear()
        assert case.targeted  # rows built for the trees that stayed
        for t in list(case.targeted):
            if t < 3:
                del case.targeted[t]
        _cases["narrow"] = case
    return _cases["narrow"]


def _narrow_message(width, max_f):
    return f"X has {width} columns but the forest splits on feature {max_f}"


@pytest.mark.parametrize("backend", _BACKENDS)
class TestNarrowInputIsRefused:
    def _setup(self, backend):
        case = _narrow_case()
        mod, dev = _backend(backend)
        flat = mod.make_flat_forest(case.trees, case.info(1), None, dev)
        maxf = np.asarray(flat["tree_max_feature"])
        assert maxf[:3].max() <= 2 and maxf.max() >= 3
        narrow = np.ascontiguousarray(case.X[:, :3])
        return case, mod, dev, flat, narrow, int(maxf.max())

    def test_kernel_level(self, backend, monkeypatch):
        case, mod, dev, flat, narrow, max_f = self._setup(backend)
        Xn = torch.from_numpy(narrow).to(dev)

        class _NoLaunch:
            def __getattr__(self, name):
                raise AssertionError(f"{name} reached the native layer")

        def _no_native(*args):
            raise AssertionError("the native traversal was reached")

        # the Python wrapper refuses before it touches the extension
        with monkeypatch.context() as m:
            if backend == "gpu":
                m.setattr(hip, "_K", _NoLaunch())
            else:
                m.setattr(torch_ref, "_native_predict", _no_native)
            with pytest.raises(ValueError, match=_narrow_message(3, max_f)):
                mod.predict_forest_flat(flat, Xn, 1)
        with pytest.raises(ValueError, match=_narrow_message(3, max_f)):
            mod.pred_leaf(flat, Xn)
        # trees that fit the narrow matrix still predict
        sums, leaves, _, _ = _oracle(case.trees, case.info(1), None, narrow, 1, 0, 3)
        _assert_exact(mod.predict_forest_flat(flat, Xn, 1, 0, 3), sums)
        _assert_leaves(mod.pred_leaf(flat, Xn, 0, 3), leaves)
        # tree ranges outside the forest
        for tb, te in [(-1, 2), (0, case.T + 1), (5, 4)]:
            with pytest.raises(ValueError, match="out of bounds"):
                mod.predict_forest_flat(flat, torch.from_numpy(case.X).to(dev), 1, tb, te)
        # a class id beyond k, a wrong dtype
        flat3 = mod.make_flat_forest(case.trees, case.info(3), None, dev)
        with pytest.raises(ValueError, match="class id"):
            mod.predict_forest_flat(flat3, torch.from_numpy(case.X).to(dev), 2)
        with pytest.raises(ValueError):
            mod.predict_forest_flat(flat, torch.from_numpy(case.X.astype(np.float64)).to(dev), 1)

    def test_stumps_accept_no_columns(self, backend):
        mod, dev = _backend(backend)
        trees = _make_trees(8, 4, 0, seed=9)
        assert all(t.num_nodes == 1 for t in trees)
        flat = mod.make_flat_forest(trees, [0, 1, 0, 1], _eighths(4), dev)
        X = torch.zeros((5, 0), dtype=torch.float32, device=dev)
        sums, leaves, _, _ = _oracle(trees, [0, 1, 0, 1], _eighths(4), np.zeros((5, 0), np.float32), 2, 0, 4)
        _assert_exact(mod.predict_forest_flat(flat, X, 2), sums)
        _assert_leaves(mod.pred_leaf(flat, X), leaves)

    def test_through_the_booster(self, backend):
        case, _, _, _, narrow, max_f = self._setup(backend)
        # num_features = 0: a model loaded without the count, the case in which
        # the serving code cannot pad and validate_features=False checks nothing
        for num_features in (0, case.f):
            bst = Booster({"objective": "reg:squarederror", "base_score": 0.5},
                          num_features=num_features)
            for t in range(case.T):
                bst.add_iteration([case.trees[t]], [0])
            if backend == "host":
                bst.set_param("predictor", "cpu_predictor")
            with pytest.raises(ValueError, match=_narrow_message(3, max_f)):
                bst.predict(narrow, validate_features=False)
            with pytest.raises(ValueError, match=_narrow_message(3, max_f)):
                bst.predict(DMatrix(narrow), validate_features=False)
            got = bst.predict(narrow, validate_features=False, output_margin=True,
                              iteration_range=(0, 3))
            sums = _oracle(case.trees, case.info(1), None, narrow, 1, 0, 3)[0]
            _assert_exact(got, sums[:, 0] + 0.5)


def _launcher_args(flat32, X, t_begin, t_end, max_f, out, k=1):
    return (
        X, flat32["left"], flat32["right"], flat32["feature"], flat32["threshold"],
        flat32["default_left"], flat32["value"], flat32["tree_root"], flat32["tree_cls"],
        t_begin, t_end, max_f, 0, out, k,
    )


class TestLaunchersRefuse:
    """The native entry points themselves: every refusal is a ValueError
    raised on the host, before a row is read."""

    def test_host(self):
        from sagemaker_xgboost_container_amd.ops import _smxgb_hip as K

        case = _narrow_case()
        flat = torch_ref.make_flat_forest(case.trees, case.info(1), None, torch.device("cpu"))
        i32 = dict(torch_ref._flat_i32(flat), threshold=flat["threshold"], value=flat["value"])
        max_f = int(flat["tree_max_feature"].max())
        X = torch.from_numpy(case.X)
        narrow = torch.from_numpy(np.ascontiguousarray(case.X[:, :3]))
        out = torch.zeros((case.n, 1), dtype=torch.float32)
        leaf = torch.zeros((case.n, case.T), dtype=torch.int32)
        leaf_args = lambda x, tb, te, mf, o: (  # noqa: E731
            x, i32["left"], i32["right"], i32["feature"], i32["threshold"],
            i32["default_left"], i32["tree_root"], tb, te, mf, o,
        )
        with pytest.raises(ValueError, match=_narrow_message(3, max_f)):
            K.predict_forest_cpu(*_launcher_args(i32, narrow, 0, case.T, max_f, out))
        with pytest.raises(ValueError, match=_narrow_message(3, max_f)):
            K.pred_leaf_cpu(*leaf_args(narrow, 0, case.T, max_f, leaf))
        with pytest.raises(ValueError, match="expected dtype"):
            K.predict_forest_cpu(*_launcher_args(i32, X.double(), 0, case.T, max_f, out))
        with pytest.raises(ValueError, match="expected dtype"):
            K.pred_leaf_cpu(*leaf_args(X.double(), 0, case.T, max_f, leaf))
        with pytest.raises(ValueError, match=r"X must be \(n, f\)"):
            K.predict_forest_cpu(*_launcher_args(i32, X.reshape(-1), 0, case.T, max_f, out))
        for tb, te in [(-1, 2), (0, case.T + 1), (5, 4)]:
            with pytest.raises(ValueError, match="out of bounds"):
                K.predict_forest_cpu(*_launcher_args(i32, X, tb, te, max_f, out))
            with pytest.raises(ValueError, match="out of bounds"):
                K.pred_leaf_cpu(*leaf_args(X, tb, te, max_f, leaf))
        with pytest.raises(ValueError, match=r"out must be \(n, k\)"):
            K.predict_forest_cpu(*_launcher_args(i32, X, 0, case.T, max_f, out[:5].clone()))
        with pytest.raises(ValueError, match=r"out must be \(n, T\)"):
            K.pred_leaf_cpu(*leaf_args(X, 0, 3, max_f, leaf))
        assert not out.any() and not leaf.any()  # nothing was written

    @pytest.mark.gpu
    def test_device(self):
        case = _narrow_case()
        flat = hip.make_flat_forest(case.trees, case.info(1), None, torch.device("cuda"))
        max_f = int(flat["tree_max_feature"].max())
        X = torch.from_numpy(case.X).cuda()
        narrow = torch.from_numpy(np.ascontiguousarray(case.X[:, :3])).cuda()
        n_chunks, tpc = hip._predict_chunking(case.n, case.T)
        out = torch.zeros((n_chunks, case.n, 1), dtype=torch.float32, device="cuda")

        def launch(x, tb=0, te=case.T, mf=max_f, o=out, cls_max=0, k=1, c=n_chunks, per=tpc):
            hip._K.predict_forest(
                x, flat["left"], flat["right"], flat["feature"], flat["threshold"],
                flat["default_left"], flat["value"], flat["tree_root"], flat["tree_cls"],
                tb, te, mf, cls_max, o, k, c, per,
            )

        with pytest.raises(ValueError, match=_narrow_message(3, max_f)):
            launch(narrow)
        with pytest.raises(ValueError, match="expected dtype"):
            launch(X.double())
        with pytest.raises(ValueError, match="expected dtype"):
            launch(X.cpu())
        with pytest.raises(ValueError, match=r"X must be \(n, f\)"):
            launch(X.reshape(-1))
        for tb, te in [(-1, 2), (0, case.T + 1), (5, 4)]:
            with pytest.raises(ValueError, match="out of bounds"):
                launch(X, tb, te)
        with pytest.raises(ValueError, match="out must be"):
            launch(X, o=out[:, :5].contiguous())
        with pytest.raises(ValueError, match="class id"):
            launch(X, cls_max=1)
        with pytest.raises(ValueError, match="chunking"):
            launch(X, c=1, per=case.T - 1, o=out[:1].contiguous())
        torch.cuda.synchronize()
        assert not out.any()  # nothing was launched
        launch(X)  # and the same arguments, unbroken, run
        _assert_exact(out.sum(0), case.oracle(1, False)[0])
