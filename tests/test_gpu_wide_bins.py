"""Features of more than 256 bins (max_bin > 256) on the HIP backends: the
wide split scan against a float64 gain table, its tie rule, the device grower
against the per-level path, and the sparse backend. Needs an MI355X."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NBINS = [2, 17, 256, 257, 512, 513, 1025, 3000]  # 256c, 256c + 1 and a non-multiple
TREE_ARRAYS = ("left", "right", "parent", "feature", "threshold", "split_bin",
               "default_left", "value", "gain", "sum_hess")
LAM = 1.0


def _stub_qm(nbins, stride, has_missing):
    return types.SimpleNamespace(num_col=len(nbins), stride=stride, nbins=torch.tensor(nbins),
                                 has_missing=bool(has_missing), is_cat=None)


def _case(nbins, has_missing, seed, k=3):
    """Integer-valued histograms [k, f, stride, 2] (exact float32 prefix sums), parents
    [k, 2], stub qm. One random bin of every row takes what the row lacks of the node's
    (G, H), so that all features of a node sum to its parent."""
    rng = np.random.default_rng(seed)
    f, stride = len(nbins), max(nbins) + has_missing
    hist = np.stack([rng.integers(-8, 9, (k, f, stride)), rng.integers(0, 5, (k, f, stride))], -1)
    hist = hist.astype(np.float32)
    for j, nb in enumerate(nbins):
        hist[:, j, nb:stride - has_missing] = 0
    total = hist.sum(2)
    parent = np.stack([total[:, -1, 0], total[..., 1].max(1)], axis=1)
    node, feat = np.indices((k, f))
    hist[node, feat, rng.integers(0, np.asarray(nbins), (k, f))] += parent[:, None] - total
    return hist, parent, _stub_qm(nbins, stride, has_missing)


def _gain_table(hist, parent, qm, mcw=1.0, mono=None, mask=None):
    """float64 gain [k, f, bin, dir] (-inf: no candidate) and left sums [k, f, bin, dir, 2]."""
    k, f, stride, _ = hist.shape
    nreal = stride - qm.has_missing
    h = hist.astype(np.float64)
    scan = np.cumsum(h[:, :, :nreal], axis=2)
    miss = h[:, :, -1] if qm.has_missing else np.zeros((k, f, 2))
    left = np.stack([scan, scan + miss[:, :, None]], axis=3)
    par = parent.astype(np.float64)[:, None, None, None]
    right = par - left
    score = lambda s: s[..., 0] ** 2 / (s[..., 1] + LAM)  # noqa: E731
    gain = 0.5 * (score(left) + score(right) - score(par))
    ok = (left[..., 1] >= mcw) & (right[..., 1] >= mcw)
    ok &= (np.arange(nreal)[None, :] <= qm.nbins.numpy()[:, None] - 2)[None, :, :, None]
    if mono is not None:
        wl, wr = (-s[..., 0] / (s[..., 1] + LAM) for s in (left, right))
        m = np.asarray(mono)[None, :, None, None]
        ok &= ~(((m > 0) & (wl > wr)) | ((m < 0) & (wl < wr)))
    if mask is not None:
        ok &= np.broadcast_to(mask, (k, f))[:, :, None, None]
    return np.where(ok, gain, -np.inf), left


def _barred(*a, **k):
    raise AssertionError("torch_ref.find_splits reached from a HIP backend")


def _find(monkeypatch, hist, parent, qm, **kw):
    """hip.find_splits with the torch reference barred: packed [k, 6], twice the same."""
    from sagemaker_xgboost_container_amd.ops import hip, torch_ref

    monkeypatch.setattr(torch_ref, "find_splits", _barred)
    kw = {n: torch.as_tensor(v).cuda() if isinstance(v, np.ndarray) else v for n, v in kw.items()}
    args = (torch.from_numpy(hist.reshape(len(hist), -1, 2)).cuda(), torch.from_numpy(parent).cuda(), qm)
    a, b = (hip.find_splits(*args, reg_lambda=LAM, **kw)["packed"].cpu().numpy() for _ in range(2))
    assert np.array_equal(a, b), "split search differs between two calls"
    return a


def _check(packed, gain, left):
    """Every node's candidate is valid, as good as the float64 best within the tolerance
    of tests/test_gpu_kernels.py::TestFindSplits, and carries the exact left sums."""
    for node, (g, feat, b, d, lg, lh) in enumerate(packed):
        best = gain[node].max()
        print(f"node {node}: device gain {g!r} at {(feat, b, d)}, float64 best {best!r}")
        if not best > 0:  # no candidate, or none worth a split
            assert g == -1.0
            continue
        got = gain[node, int(feat), int(b), int(d)]
        assert np.isfinite(got), "the chosen candidate is not a valid one"
        np.testing.assert_allclose(got, best, rtol=2e-4, atol=1e-5)
        np.testing.assert_allclose(g, got, rtol=2e-4, atol=1e-5)
        assert (lg, lh) == tuple(left[node, int(feat), int(b), int(d)])


@pytest.mark.parametrize("has_missing", [0, 1])
def test_wide_scan_matches_float64_table(monkeypatch, has_missing):
    hist, parent, qm = _case(NBINS, has_missing, seed=has_missing)
    _check(_find(monkeypatch, hist, parent, qm), *_gain_table(hist, parent, qm))
    for j in range(len(NBINS)):  # each feature's own candidate, narrow and wide
        mask = np.arange(len(NBINS)) == j
        table = _gain_table(hist, parent, qm, mask=mask)
        _check(_find(monkeypatch, hist, parent, qm, feature_mask=mask), *table)


@pytest.mark.parametrize("constraint", ["node_mask", "monotone", "min_child_weight"])
def test_wide_scan_constraints(monkeypatch, constraint):
    hist, parent, qm = _case([17, 513, 1025, 3000], 1, seed=8)
    free, left = _gain_table(hist, parent, qm)
    win = [np.unravel_index(free[n].argmax(), free[n].shape) for n in range(len(free))]
    assert all(w[0] > 0 for w in win)  # the unconstrained winners are wide features
    if constraint == "node_mask":  # hide every node's best feature
        mask = np.ones(free.shape[:2], dtype=bool)
        mask[np.arange(len(win)), [w[0] for w in win]] = False
        kw, ref = {"feature_mask": mask}, {"mask": mask}
    elif constraint == "monotone":  # the direction that rejects node 0's winner
        lg, lh = left[0][win[0]]
        wl, wr = -lg / (lh + LAM), -(parent[0, 0] - lg) / (parent[0, 1] - lh + LAM)
        mono = np.zeros(4, dtype=np.int8)
        mono[win[0][0]] = 1 if wl > wr else -1
        kw, ref = {"monotone": mono}, {"mono": mono}
    else:
        mcw = float(parent[:, 1].min() * 0.45)
        kw, ref = {"min_child_weight": mcw}, {"mcw": mcw}
    table = _gain_table(hist, parent, qm, **ref)
    assert table[0][0].max() < free[0].max()  # the constraint binds on node 0
    _check(_find(monkeypatch, hist, parent, qm, **kw), *table)


@pytest.mark.parametrize("has_missing", [0, 1])
def test_exact_ties_lowest_bin_then_lowest_feature(monkeypatch, has_missing):
    """Only bins a and b hold rows: every cut in [a, b - 1] has the same sums, over three
    tiles of the scan. The same column twice: feature 0, bin a, missing right."""
    a, b = 300, 2500
    hist = np.zeros((1, 2, 3000 + has_missing, 2), dtype=np.float32)
    hist[0, :, a], hist[0, :, b] = (-4, 2), (4, 2)
    parent = np.array([[0, 4]], dtype=np.float32)
    packed = _find(monkeypatch, hist, parent, _stub_qm([3000, 3000], hist.shape[2], has_missing))
    assert packed[0, 1:].tolist() == [0, a, 0, -4, 2] and packed[0, 0] > 5


def test_stride_beyond_the_histogram_slab_is_refused():
    from sagemaker_xgboost_container_amd.ops import hip

    hip.check_hist_stride(_stub_qm([3184], 3185, 1))
    with pytest.raises(ValueError, match="max_bin too large"):
        hip.make_tree_state(_stub_qm([3185], 3186, 1), None)


def _train(monkeypatch, X, y, env=()):
    from sagemaker_xgboost_container_amd.data.dmatrix import DMatrix
    from sagemaker_xgboost_container_amd.models import trainer

    with monkeypatch.context() as patch:
        for name, value in env:
            patch.setenv(name, value)
        res = {}
        dm = DMatrix(X.copy(), label=y)
        params = {"objective": "binary:logistic", "max_depth": 6, "max_bin": 512, "device": "cuda"}
        bst = trainer.train(params, dm, 3, evals=[(dm, "train")], evals_result=res, verbose_eval=False)
    return bst, res["train"]["logloss"]


def _same_trees(a, b, what):
    assert len(a) == len(b) > 0
    for i, (ta, tb) in enumerate(zip(a, b)):
        for name in TREE_ARRAYS:
            assert np.array_equal(getattr(ta, name), getattr(tb, name)), f"{what}: tree {i}: {name}"


@pytest.mark.parametrize("nan_frac", [0.0, 0.2])
def test_device_grower_splits_wide_features(monkeypatch, nan_frac):
    from sagemaker_xgboost_container_amd.models.grower import HistGrower
    from sagemaker_xgboost_container_amd.ops.quantize import quantize

    rng, n = np.random.default_rng(3), 4099
    X = rng.normal(size=(n, 5)).astype(np.float32)
    y = (X[:, 0] * 2 - X[:, 1] + rng.normal(scale=0.3, size=n) > 0).astype(np.float32)
    X[rng.random(X.shape) < nan_frac] = np.nan
    qm = quantize(torch.tensor(X, device="cuda"), max_bin=512)
    assert int(qm.nbins.max()) > 256 and qm.bins.dtype == torch.int16
    gh = torch.tensor(np.stack([0.5 - y, np.full_like(y, 0.25)], 1), device="cuda")

    def grow(path, comm=None):
        with monkeypatch.context() as patch:
            if path == "per_level":
                patch.setenv("SMXGB_NO_DEVICE_GROW", "1")
            grower = HistGrower(qm, {"max_depth": 6, "eta": 0.3}, comm=comm)
            tree, leaf_jobs = grower.grow(gh)
            assert grower.grow_path == path
            margin = torch.zeros(n, dtype=torch.float32, device="cuda")
            grower.state.update_margins(margin, leaf_jobs)
        return tree, margin.cpu()

    same = lambda t, src=0: t  # noqa: E731
    one_rank = types.SimpleNamespace(rank=0, world_size=1, is_master=True, barrier=lambda: None,
                                     allreduce_=same, allreduce_max_=same,
                                     allreduce_min_=same, broadcast_=same)
    tree, margin = grow("device")
    splits = np.asarray(tree.left) >= 0
    assert splits.sum() > 1, "the tree is the root alone"
    assert (np.asarray(tree.split_bin)[splits] >= 256).any(), "no split above a 256th cut"
    for what, other in (("per-level", grow("per_level")), ("one-rank hook", grow("device", one_rank))):
        _same_trees([tree], [other[0]], what)
        assert torch.equal(margin, other[1]), f"{what}: margins differ"

    bst, loss = _train(monkeypatch, X, y)
    assert all((np.asarray(t.left) >= 0).any() for t in bst.trees)
    assert all(b < a for a, b in zip(loss, loss[1:])), loss


def test_sparse_backend_trains_wide_feature_on_device(monkeypatch):
    """Column 0: 400 distinct multiples of 1/8 (midpoint cuts, exact on both cut finders)."""
    import scipy.sparse as sp
    from sagemaker_xgboost_container_amd.ops import torch_ref

    rng, n, f = np.random.default_rng(9), 3000, 6
    dense = rng.integers(-12, 13, (n, f)).astype(np.float32) / 8
    dense[:, 0] = rng.integers(0, 400, n).astype(np.float32) / 8
    keep = rng.random((n, f)) < 0.6
    rows, cols = np.nonzero(keep)
    csr = sp.csr_matrix((dense[rows, cols], (rows, cols)), shape=(n, f), dtype=np.float32)
    y = (np.where(keep[:, 0], dense[:, 0], 45.0) > 40.0).astype(np.float32)  # cut 320 of 399
    ref, _ = _train(monkeypatch, csr, y, env=[("SMXGB_SPARSE", "0"), ("SMXGB_NO_DEVICE_GROW", "1")])
    monkeypatch.setattr(torch_ref, "find_splits", _barred)
    got, _ = _train(monkeypatch, csr, y, env=[("SMXGB_SPARSE", "1")])
    _same_trees(got.trees, ref.trees, "sparse vs dense per-level")
    assert any((np.asarray(t.split_bin)[np.asarray(t.left) >= 0] >= 256).any() for t in got.trees)
