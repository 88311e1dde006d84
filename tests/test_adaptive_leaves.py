"""Adaptive tree leaves (reg:absoluteerror, reg:quantileerror): the per-leaf
quantile rule against an independent numpy oracle, and the objective,
trainer, model-file and distributed layers above it, on the CPU.

The oracle below (a per-leaf np.sort with the rule in float64) is written
out here on purpose: it shares no code with ops/torch_ref.leaf_quantiles.
The device tests (test_gpu_adaptive_leaves.py) import it.
"""
import json
import math
import os
import pickle

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from sagemaker_xgboost_container_amd.data.dmatrix import DMatrix
from sagemaker_xgboost_container_amd.models import trainer
from sagemaker_xgboost_container_amd.models.booster import Booster
from sagemaker_xgboost_container_amd.ops import torch_ref

ALPHAS = (0.5, 0.1, 0.9, 1e-4, 0.9999)


# -- the oracle ---------------------------------------------------------------
def oracle_quantile(values, alpha, weights=None):
    """The rule for one leaf: float32 values in, one float32 (or NaN) out."""
    m = len(values)
    if m == 0:
        return np.float32(np.nan)
    order = np.argsort(values, kind="stable")
    v = np.asarray(values, dtype=np.float32)[order].astype(np.float64)
    if weights is not None:
        cs = np.cumsum(np.asarray(weights, dtype=np.float32)[order].astype(np.float64))
        if not cs[-1] > 0.0:
            return np.float32(np.nan)
        reached = np.nonzero(cs >= alpha * cs[-1])[0]
        return np.float32(v[reached[0] if len(reached) else m - 1])
    if alpha <= 1.0 / (m + 1):
        return np.float32(v[0])
    if alpha >= m / (m + 1):
        return np.float32(v[m - 1])
    x = alpha * (m + 1)
    k = int(math.floor(x)) - 1
    d = x - 1 - k
    return np.float32(v[k] + d * (v[min(k + 1, m - 1)] - v[k]))


def oracle_leaf_quantiles(pos, resid, n_leaves, alpha, weight=None):
    out = np.empty(n_leaves, dtype=np.float32)
    order = np.argsort(pos, kind="stable")
    ps = pos[order]
    lo = np.searchsorted(ps, np.arange(n_leaves), side="left")
    hi = np.searchsorted(ps, np.arange(n_leaves), side="right")
    for leaf in range(n_leaves):
        rows = order[lo[leaf]:hi[leaf]]
        out[leaf] = oracle_quantile(
            resid[rows], alpha, None if weight is None else weight[rows]
        )
    return out


def same_values(a, b):
    """Exact equality by value: NaN matches NaN, -0 matches +0."""
    return np.array_equal(np.asarray(a, np.float32), np.asarray(b, np.float32), equal_nan=True)


# -- inputs ---------------------------------------------------------------------
# (n, n_leaves, layout): the shapes of the kernel tests, reused here
SHAPES = (
    (1, 1, "uniform"),
    (257, 3, "one_empty"),
    (5000, 64, "uniform"),
    (20000, 1024, "sparse_leaves"),
    (70000, 2, "all_but_three"),
)


def make_pos(n, n_leaves, layout, rng):
    if layout == "one_empty":
        pos = rng.choice([0, 2], size=n).astype(np.int32)
    elif layout == "sparse_leaves":
        # sixteen busy leaves, 300 leaves of one row, the other leaves empty
        pos = rng.integers(0, 16, size=n).astype(np.int32)
        single = 16 + rng.choice(n_leaves - 16, size=300, replace=False)
        pos[rng.choice(n, size=300, replace=False)] = single
    elif layout == "all_but_three":
        pos = np.zeros(n, dtype=np.int32)
        pos[rng.choice(n, size=3, replace=False)] = 1
        return pos
    else:
        pos = rng.integers(0, n_leaves, size=n).astype(np.int32)
    if n > 1:
        pos[rng.random(n) < 0.07] = -1
    return pos


def make_resid(n, kind, rng):
    if kind == "continuous":
        return (rng.normal(size=n) * np.exp(rng.normal(size=n) * 3)).astype(np.float32)
    if kind == "eighths":  # ties, and both zeros
        r = (np.round(rng.normal(size=n) * 16) / 8).astype(np.float32)
        r[r == 0] = np.where(rng.random(int((r == 0).sum())) < 0.5, -0.0, 0.0)
        return r
    if kind == "equal":
        return np.full(n, -3.25, dtype=np.float32)
    raise ValueError(kind)


def exact_weights(n, rng):
    """Multiples of 1/8 up to 1024 (zero included): every partial sum is
    exact in any order, in float64 and in fixed point."""
    return (rng.integers(0, 8193, size=n) / 8.0).astype(np.float32)


# -- the reference against the oracle -------------------------------------------
@pytest.mark.parametrize("n,n_leaves,layout", SHAPES[:4])
@pytest.mark.parametrize("kind", ("continuous", "eighths", "equal"))
def test_reference_equals_oracle(n, n_leaves, layout, kind):
    rng = np.random.default_rng(n + len(kind))
    pos = make_pos(n, n_leaves, layout, rng)
    resid = make_resid(n, kind, rng)
    weight = exact_weights(n, rng)
    for alpha in ALPHAS:
        for w in (None, weight, rng.random(n).astype(np.float32)):
            got = torch_ref.leaf_quantiles(
                torch.from_numpy(pos), torch.from_numpy(resid), n_leaves, alpha,
                None if w is None else torch.from_numpy(w),
            )
            assert got.dtype == torch.float32 and got.shape == (n_leaves,)
            want = oracle_leaf_quantiles(pos, resid, n_leaves, alpha, w)
            assert same_values(got.numpy(), want), (alpha, w is None)


def test_reference_edge_leaves():
    pos = np.array([0, 2, 2, -1, 3, 3, 3, 3], dtype=np.int32)
    resid = np.array([7.5, -1.0, 2.0, 99.0, 0.0, -0.0, 4.0, -4.0], dtype=np.float32)
    for alpha in ALPHAS:
        got = torch_ref.leaf_quantiles(torch.from_numpy(pos), torch.from_numpy(resid), 5, alpha).numpy()
        assert np.isnan(got[1]) and np.isnan(got[4])  # empty leaves
        assert got[0] == np.float32(7.5)  # one row: both clamps give it
        assert same_values(got, oracle_leaf_quantiles(pos, resid, 5, alpha))
    # median of two rows interpolates half way; alpha (m + 1) = 1.5, k = 0
    got = torch_ref.leaf_quantiles(torch.from_numpy(pos), torch.from_numpy(resid), 5, 0.5).numpy()
    assert got[2] == np.float32(0.5)
    # zero total weight is an empty leaf
    w = np.array([0, 1, 1, 1, 0, 0, 0, 0], dtype=np.float32)
    got = torch_ref.leaf_quantiles(
        torch.from_numpy(pos), torch.from_numpy(resid), 5, 0.5, torch.from_numpy(w)
    ).numpy()
    assert np.isnan(got[0]) and np.isnan(got[3]) and got[2] == np.float32(-1.0)
    with pytest.raises(ValueError):
        torch_ref.leaf_quantiles(torch.from_numpy(pos), torch.from_numpy(resid), 3, 0.5)


# -- leaf values of a trained model ------------------------------------------------
def check_leaf_values(bst, data, y, eta, alphas, weight=None, rows=None):
    """Every leaf of every tree holds float32(float64(q) * eta), q the oracle
    quantile of y - (the margin before the tree's round, rebuilt from the
    earlier trees' leaf values) over the rows of the leaf, grouped by
    pred_leaf. `rows`: per tree, the boolean mask of the rows it was grown
    on (all rows when None). Returns the number of leaves checked."""
    n = len(y)
    k = len(alphas)
    leaves = bst.predict(DMatrix(data), pred_leaf=True).reshape(n, -1)
    assert leaves.shape[1] == len(bst.trees) and len(bst.trees) % k == 0
    base = np.float32(bst.objective().base_margin(bst.base_score))
    # the trainer's own margins: float32, one tree after the other, a round's
    # trees all reading the margin the round began with
    margin = np.full((n, k), base, dtype=np.float32)
    next_margin = margin.copy()
    checked = 0
    for t, tree in enumerate(bst.trees):
        cls = bst.tree_info[t]
        if t % k == 0:
            margin = next_margin.copy()
        resid = (y.astype(np.float32) - margin[:, cls]).astype(np.float32)
        leaf_ids = np.nonzero(np.asarray(tree.left) < 0)[0]
        slot = np.full(tree.num_nodes, -1, dtype=np.int32)
        slot[leaf_ids] = np.arange(len(leaf_ids), dtype=np.int32)
        pos = slot[leaves[:, t]]
        assert (pos >= 0).all()
        if rows is not None:
            pos = np.where(rows[t], pos, -1).astype(np.int32)
        q = oracle_leaf_quantiles(pos, resid, len(leaf_ids), alphas[cls], weight)
        for s, nid in enumerate(leaf_ids):
            if np.isnan(q[s]):
                continue  # no row of the sample: the Newton value stays
            want = np.float32(np.float64(q[s]) * eta)
            assert np.float32(tree.value[nid]) == want, (t, nid, tree.value[nid], want)
            checked += 1
        next_margin[:, cls] += np.asarray(tree.value, dtype=np.float32)[leaves[:, t]]
    return checked


# -- trainer ---------------------------------------------------------------------------
CPU = {"device": "cpu"}


def _regression_data(n=1500, f=6, seed=0):
    """Labels on both sides of base_score = 0.5, heavy-tailed noise."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, f)).astype(np.float32)
    y = (0.5 + 3 * X[:, 0] + np.abs(X[:, 1]) * X[:, 2] + rng.standard_t(3, size=n)).astype(np.float32)
    return X, y


def test_absolute_error_reaches_far_labels():
    """Newton leaves (|value| < eta) cannot move a prediction beyond
    0.5 + 20 * 0.3 from labels near 1000; adaptive leaves can."""
    rng = np.random.default_rng(1)
    X = rng.normal(size=(800, 4)).astype(np.float32)
    y = (1000 + 50 * X[:, 0]).astype(np.float32)
    bst = trainer.train(
        dict(CPU, objective="reg:absoluteerror", eta=0.3, max_depth=3),
        DMatrix(X, label=y), num_boost_round=20, verbose_eval=False,
    )
    mae = np.abs(bst.predict(DMatrix(X)) - y).mean()
    assert mae < np.abs(y - np.median(y)).mean(), mae


LEAF_CASES = {
    "depthwise": dict(max_depth=3),
    "lossguide": dict(grow_policy="lossguide", max_leaves=7, max_depth=0),
    "subsample": dict(max_depth=3, subsample=0.5),
    "weighted": dict(max_depth=3),
    "sparse": dict(max_depth=3),
}


@pytest.mark.parametrize("case", sorted(LEAF_CASES))
@pytest.mark.parametrize("objective,extra", (
    ("reg:absoluteerror", {}),
    ("reg:quantileerror", {"quantile_alpha": [0.25, 0.8]}),
))
def test_leaf_values_after_one_round(case, objective, extra, monkeypatch):
    X, y = _regression_data()
    n = len(y)
    weight = rows = None
    data = X
    if case == "weighted":
        weight = exact_weights(n, np.random.default_rng(5))
    if case == "subsample":
        # the trainer's generator (seed 0 -> 2016) draws one rand(n) per tree
        gen = torch.Generator(device="cpu")
        gen.manual_seed(2016)
        rows = [(torch.rand(n, generator=gen) < 0.5).numpy() for _ in extra.get("quantile_alpha", [0])]
    if case == "sparse":
        monkeypatch.setenv("SMXGB_SPARSE", "1")
        data = sp.random(n, 70, density=0.05, format="csr", dtype=np.float32, random_state=3)
        y = (0.5 + 4 * np.asarray(data[:, :6].sum(axis=1)).ravel()
             + np.random.default_rng(2).standard_t(3, size=n)).astype(np.float32)
    params = dict(CPU, objective=objective, eta=0.7, base_score=0.5, **LEAF_CASES[case], **extra)
    bst = trainer.train(params, DMatrix(data, label=y, weight=weight), num_boost_round=1,
                        verbose_eval=False)
    alphas = extra.get("quantile_alpha", [0.5])
    assert len(bst.trees) == len(alphas)
    assert all(t.num_leaves >= 3 for t in bst.trees)
    if case == "lossguide":
        assert all(t.num_leaves == 7 for t in bst.trees)
    checked = check_leaf_values(bst, data, y, 0.7, alphas, weight=weight, rows=rows)
    assert checked >= 3 * len(alphas)


def _pinball(pred, y, alpha):
    d = y.astype(np.float64) - pred.astype(np.float64)
    return float(np.mean(alpha * np.maximum(d, 0) + (1 - alpha) * np.maximum(-d, 0)))


@pytest.mark.parametrize("alpha", (0.1, 0.9))
def test_quantile_error_metric_decreases(alpha):
    X, y = _regression_data(seed=4)
    dtrain = DMatrix(X, label=y)
    res = {}
    bst = trainer.train(
        dict(CPU, objective="reg:quantileerror", quantile_alpha=alpha, max_depth=3, eta=0.3),
        dtrain, num_boost_round=5, evals=[(dtrain, "train")], evals_result=res, verbose_eval=False,
    )
    hist = res["train"]["quantile"]  # the objective's default metric
    assert len(hist) == 5 and all(b < a for a, b in zip(hist, hist[1:])), hist
    pred = bst.predict(dtrain)
    assert pred.shape == (len(y),)
    assert hist[-1] == pytest.approx(_pinball(pred, y, alpha), rel=1e-6)
    constant = np.full(len(y), np.quantile(y, alpha), dtype=np.float32)
    assert hist[-1] < _pinball(constant, y, alpha)


def test_multi_alpha_columns_equal_single_alpha_models():
    X, y = _regression_data(seed=6)
    alphas = [0.1, 0.5, 0.9]
    common = dict(CPU, objective="reg:quantileerror", max_depth=3, eta=0.4, base_score=0.25)
    multi = trainer.train(dict(common, quantile_alpha=alphas), DMatrix(X, label=y), 4, verbose_eval=False)
    pred = multi.predict(DMatrix(X))
    assert pred.shape == (len(y), 3) and pred.dtype == np.float32
    for j, alpha in enumerate(alphas):
        single = trainer.train(dict(common, quantile_alpha=alpha), DMatrix(X, label=y), 4, verbose_eval=False)
        assert np.array_equal(pred[:, j], single.predict(DMatrix(X))), alpha


@pytest.mark.parametrize("bad", (0, 1, 0.0, 1.0, -0.1, 1.5, [0.5, 1.5], [], "abc", [0.5, "x"],
                                 float("nan"), None, True))
def test_invalid_quantile_alpha_raises(bad):
    from sagemaker_xgboost_container_amd.models.objectives import create_objective

    with pytest.raises(ValueError):
        create_objective("reg:quantileerror", {"quantile_alpha": bad})


def test_quantile_objective_surface():
    from sagemaker_xgboost_container_amd.models.objectives import create_objective

    with pytest.raises(ValueError):
        create_objective("reg:quantileerror", {})
    obj = create_objective("reg:quantileerror", {"quantile_alpha": [0.2, 0.7]})
    assert obj.n_outputs == 2 and obj.adaptive_alphas == [0.2, 0.7] and obj.default_metric == "quantile"
    assert create_objective("reg:absoluteerror", {}).adaptive_alphas == [0.5]
    assert create_objective("reg:squarederror", {}).adaptive_alphas is None
    margin = torch.tensor([[0.0, 2.0], [1.0, 1.0], [3.0, -1.0]])
    y = torch.tensor([1.0, 1.0, 1.0])
    gh = obj.gradients(margin, y, torch.tensor([1.0, 2.0, 0.5]))
    assert gh.shape == (3, 2, 2)
    want_g = np.array([[-0.2, 0.3], [2 * 0.8, 2 * 0.3], [0.5 * 0.8, 0.5 * -0.7]], dtype=np.float32)
    assert np.allclose(gh[:, :, 0].numpy(), want_g, rtol=1e-6)
    assert np.array_equal(gh[:, :, 1].numpy(), np.array([[1, 1], [2, 2], [0.5, 0.5]], dtype=np.float32))
    assert torch.equal(obj.transform(margin), margin)
    single = create_objective("reg:quantileerror", {"quantile_alpha": "0.3"})
    assert single.n_outputs == 1 and single.gradients(margin[:, 0], y).shape == (3, 2)


def test_sklearn_wrapper_passes_quantile_alpha():
    import xgboost as xgb

    X, y = _regression_data(n=400, seed=7)
    model = xgb.XGBRegressor(
        objective="reg:quantileerror", quantile_alpha=np.array([0.1, 0.9]), n_estimators=3,
        max_depth=2, device="cpu",
    ).fit(X, y)
    assert model.get_booster().objective().alphas == [0.1, 0.9]
    pred = model.predict(X)
    assert pred.shape == (400, 2)
    assert (pred[:, 0] <= pred[:, 1]).mean() > 0.9


# -- model files --------------------------------------------------------------------
@pytest.mark.parametrize("alpha", (0.3, [0.1, 0.5, 0.9]))
def test_model_file_round_trips(alpha, tmp_path):
    X, y = _regression_data(n=500, seed=8)
    bst = trainer.train(
        dict(CPU, objective="reg:quantileerror", quantile_alpha=alpha, max_depth=3),
        DMatrix(X, label=y), num_boost_round=3, verbose_eval=False,
    )
    want = bst.predict(DMatrix(X))
    alphas = alpha if isinstance(alpha, list) else [alpha]
    block = bst.save_json()["learner"]["objective"]["quantile_loss_param"]
    assert json.loads(block["quantile_alpha"]) == alphas

    path = str(tmp_path / "model.json")
    bst.save_model(path)
    with open(path) as f:
        assert "quantile_loss_param" in json.load(f)["learner"]["objective"]
    loaded = Booster()
    loaded.load_model(path)
    assert loaded.objective().alphas == alphas
    assert np.array_equal(loaded.predict(DMatrix(X)), want)

    path = str(tmp_path / "model.ubj")
    bst.save_model_ubj(path)
    loaded = Booster()
    loaded.load_model(path)
    assert loaded.objective().alphas == alphas
    assert np.array_equal(loaded.predict(DMatrix(X)), want)

    loaded = pickle.loads(pickle.dumps(bst))
    assert np.array_equal(loaded.predict(DMatrix(X)), want)

    # a scalar (not an array string) in the block loads too
    model = bst.save_json()
    if len(alphas) == 1:
        model["learner"]["objective"]["quantile_loss_param"]["quantile_alpha"] = str(alphas[0])
        loaded = Booster().load_json(model)
        assert loaded.objective().alphas == alphas
        assert np.array_equal(loaded.predict(DMatrix(X)), want)


# -- other objectives are untouched --------------------------------------------------
def test_other_objectives_never_enter_the_adaptive_step(monkeypatch):
    X, y = _regression_data(n=600, seed=9)
    params = dict(CPU, objective="reg:squarederror", max_depth=3, subsample=0.8)

    def signature():
        bst = trainer.train(params, DMatrix(X, label=y), num_boost_round=3, verbose_eval=False)
        return json.dumps(bst.save_json(), sort_keys=True), bst.predict(DMatrix(X))

    before = signature()

    class Refuses:
        def __init__(self, *args, **kwargs):
            raise AssertionError("the adaptive leaf step ran for reg:squarederror")

    monkeypatch.setattr(trainer, "_AdaptiveLeaves", Refuses)
    after = signature()
    assert before[0] == after[0] and np.array_equal(before[1], after[1])
    with pytest.raises(AssertionError):  # the patch does guard the step
        trainer.train(dict(params, objective="reg:absoluteerror"), DMatrix(X, label=y), 1, verbose_eval=False)


# -- distributed ---------------------------------------------------------------------
def _dist_data(rank):
    """Two shards; x0 > 0.5 exists on rank 1 only, where the labels jump."""
    rng = np.random.default_rng(20 + rank)
    n = 400
    X = rng.uniform(-1.0, 0.5 if rank == 0 else 1.0, size=(n, 3)).astype(np.float32)
    # the sign of y - 0.5 is the gradient: it has to change at both edges
    y = (np.where(X[:, 0] > 0.5, -40.0, np.where(X[:, 0] > -0.2, 6.0, -5.0))
         + rng.standard_t(3, size=n)).astype(np.float32)
    return X, y


def _dist_worker(rank, world, port, q):
    os.environ["GLOO_SOCKET_IFNAME"] = os.environ.get("GLOO_SOCKET_IFNAME", "lo")
    import datetime

    import torch.distributed as dist

    from sagemaker_xgboost_container_amd.parallel.comm import Communicator

    dist.init_process_group(
        backend="gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world,
        timeout=datetime.timedelta(seconds=120),
    )
    comm = Communicator()
    X, y = _dist_data(rank)
    bst = trainer.train(
        dict(CPU, objective="reg:absoluteerror", eta=0.7, max_depth=2, base_score=0.5),
        DMatrix(X, label=y), num_boost_round=1, verbose_eval=False, comm=comm,
    )
    tree = bst.trees[0]
    leaf_ids = np.nonzero(np.asarray(tree.left) < 0)[0]
    slot = np.full(tree.num_nodes, -1, dtype=np.int32)
    slot[leaf_ids] = np.arange(len(leaf_ids), dtype=np.int32)
    pos = slot[bst.predict(DMatrix(X), pred_leaf=True).reshape(len(y))]
    local_q = oracle_leaf_quantiles(pos, (y - np.float32(0.5)).astype(np.float32), len(leaf_ids), 0.5)
    structure = json.dumps(bst.save_json()["learner"]["gradient_booster"]["model"]["trees"], sort_keys=True)
    q.put((rank, structure, np.asarray(tree.value)[leaf_ids].tolist(), local_q.tolist()))
    dist.barrier()
    dist.destroy_process_group()


def test_distributed_leaf_is_mean_of_rank_quantiles():
    import multiprocessing as mp
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dist_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = sorted(q.get(timeout=300) for _ in range(2))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    (_, tree0, values0, q0), (_, tree1, values1, q1) = results
    assert tree0 == tree1 and values0 == values1, "ranks hold different trees"
    q0, q1 = np.asarray(q0, dtype=np.float64), np.asarray(q1, dtype=np.float64)
    assert len(q0) >= 3
    assert (np.isnan(q0) & ~np.isnan(q1)).any(), "no leaf is empty on rank 0 only"
    for v, a, b in zip(values0, q0, q1):
        have = [x for x in (a, b) if not np.isnan(x)]
        assert have, "a leaf without rows on either rank"
        assert np.float32(v) == np.float32(sum(have) / len(have) * 0.7)
