"""HIP ranking metrics (csrc/smxgb_rank_metric.hip) against the float64
reference torch_ref.rank_metric, and their determinism."""
import numpy as np
import pytest
import torch

from sagemaker_xgboost_container_amd.data.dmatrix import DMatrix
from sagemaker_xgboost_container_amd.models import trainer
from sagemaker_xgboost_container_amd.ops import torch_ref

pytestmark = pytest.mark.gpu

KINDS = ["ndcg", "map"]
KS = [None, 1, 10, 5000]
CAP = 4096  # asserted against the extension's constant in case()

# |hip - ref| <= TOL for every group value and for the mean; both sides work
# in float64. Largest difference observed over this matrix on an MI355X:
# MEASURED_DIFF. TOL is 4x that, rounded up to a power of two, and may not
# pass 1e-9.
MEASURED_DIFF = 2.220e-16  # one unit in the last place of a value near 1
TOL = 2.0 ** -50
assert 4 * MEASURED_DIFF <= TOL <= 1e-9

# The run of 300 one- and two-document groups crosses the 256 groups of a
# tile; 4096 is the largest tiled group; 4097 the smallest streamed one (five
# chunks, so a carry); 7169 a streamed one that k = 5000 cuts inside a chunk.
SIZES = ([0, 1, 2, 63, 64, 65] + [1, 2] * 150 + [CAP, CAP + 1, 0, 3 * 1024 + 1, CAP + 3 * 1024 + 1]
         + [50, 40, 30, 30, 30, 700])
CAP_GROUP = SIZES.index(CAP)
STREAM_GROUPS = [g for g, m in enumerate(SIZES) if m > CAP]
ZERO_LABELS, TIED, INFS, NANS, FRACTIONAL = (len(SIZES) - 6 + i for i in range(5))


@pytest.fixture(scope="module")
def case():
    from sagemaker_xgboost_container_amd.ops import hip

    assert hip.RANK_METRIC_CAP == CAP
    rng = np.random.default_rng(23)
    ptr = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    n = int(ptr[-1])
    s = (rng.normal(size=n) * 2).astype(np.float32)
    s[ptr[CAP_GROUP]:ptr[CAP_GROUP + 1]:3] = 0.25  # ties inside the full tile
    y = rng.integers(0, 5, size=n).astype(np.float32)
    seg = lambda g: slice(ptr[g], ptr[g + 1])  # noqa: E731
    y[seg(ZERO_LABELS)] = 0.0
    s[seg(TIED)] = 1.5
    s[seg(INFS)][::4] = np.inf
    s[seg(INFS)][1::4] = -np.inf
    s[seg(NANS)][7] = np.nan
    s[seg(NANS)][8] = np.inf
    s[seg(INFS)][2::4] = -0.0
    s[seg(INFS)][3::8] = 0.0  # ranks equal to -0.0, by row
    y[seg(FRACTIONAL)] = rng.uniform(-1.0, 3.5, size=30).astype(np.float32)
    for g in STREAM_GROUPS:  # the stream path builds its own keys
        s[seg(g)][::5] = 0.25
        s[seg(g)][1::97] = -0.0
        s[seg(g)][2::97] = 0.0
        s[seg(g)][[3, 4000]] = np.nan
        s[seg(g)][[8, 9, 3000]] = np.inf
        s[seg(g)][[13, 2000]] = -np.inf
    labels = {"ndcg": y, "map": (y >= 1).astype(np.float32)}
    ref = {(kind, k): torch_ref.rank_metric(kind, s, labels[kind], ptr, k).numpy()
           for kind in KINDS for k in KS}
    return s, labels, ptr, ref


def _run(kind, s, y, ptr, k, tile_docs=None):
    from sagemaker_xgboost_container_amd.ops import hip

    plan = hip.rank_metric_plan(ptr, k, torch.from_numpy(y), "cuda", tile_docs=tile_docs)
    mean, per_group = hip.rank_metric(plan, kind, torch.from_numpy(s).cuda())
    return mean, per_group.cpu().numpy(), plan["tiles"].cpu().tolist()


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("kind", KINDS)
def test_hip_matches_float64_reference(case, kind, k):
    s, labels, ptr, ref = case
    mean, got, _ = _run(kind, s, labels[kind], ptr, k)
    want = ref[kind, k]
    diff = max(float(np.abs(got - want).max()), abs(mean - float(want.mean())))
    print(f"rank metric diff {kind} k={k}: {diff:.3e}")
    assert got.dtype == np.float64 and diff <= TOL


@pytest.mark.parametrize("k", [None, 10])
@pytest.mark.parametrize("kind", KINDS)
def test_bits_do_not_depend_on_call_or_packing(kind, k):
    # no tiled group above 700 documents: tiles of 700 cut both runs of tiled
    # groups (2639 and 1753 documents) where one tile of 4096 holds each
    sizes = [700, 300, 65, 257, 1, 20, 0, 64, 500, 2, 130, 600, CAP + 1, 400, 700, 3, 650]
    rng = np.random.default_rng(31)
    n = int(np.sum(sizes))
    s = (np.round(rng.normal(size=n) * 8) / 8).astype(np.float32)  # many ties
    y = rng.integers(0, 5 if kind == "ndcg" else 2, size=n).astype(np.float32)
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    mean, first, tiles = _run(kind, s, y, ptr, k, tile_docs=CAP)
    assert _run(kind, s, y, ptr, k, tile_docs=CAP)[1].tobytes() == first.tobytes()
    small_mean, small, small_tiles = _run(kind, s, y, ptr, k, tile_docs=700)
    assert len(small_tiles) > len(tiles) == 2
    assert small.tobytes() == first.tobytes() and small_mean == mean


@pytest.mark.parametrize("k", KS)
def test_ndcg_of_the_labels_as_margin_is_exactly_one(case, k):
    """The cached IDCG is the DCG kernel run on the labels."""
    _, labels, ptr, _ = case
    y = labels["ndcg"]
    _, got, _ = _run("ndcg", y, y, ptr, k)
    some_gain = np.array([(y[a:b] > 0).any() for a, b in zip(ptr[:-1], ptr[1:])])
    assert some_gain.sum() > 200 and np.all(got[some_gain] == 1.0)


def test_training_reports_the_rule_for_its_own_and_a_validation_set():
    rng = np.random.default_rng(4)
    sets = {}
    for name, sizes in (("train", rng.integers(20, 81, size=40)), ("valid", rng.integers(5, 60, size=25))):
        n = int(sizes.sum())
        X = rng.normal(size=(n, 6)).astype(np.float32)
        y = np.clip(np.floor(X[:, 0] + 0.5 * X[:, 1] + rng.normal(scale=0.5, size=n) + 1.5), 0, 4)
        dm = DMatrix(X, label=y.astype(np.float32), qid=np.repeat(np.arange(len(sizes)), sizes))
        sets[name] = (dm, X, y.astype(np.float32), np.concatenate([[0], np.cumsum(sizes)]))
    res = {}
    bst = trainer.train(
        {"objective": "rank:ndcg", "lambdarank_pair_method": "topk", "max_depth": 4, "eta": 0.3,
         "eval_metric": ["ndcg@5", "map"], "seed": 3, "device": "cuda"},
        sets["train"][0], num_boost_round=5, evals=[(sets[k][0], k) for k in sets],
        evals_result=res, verbose_eval=False,
    )
    for name, (dm, X, y, ptr) in sets.items():
        for rnd in range(5):
            margin = bst.predict(dm, output_margin=True, iteration_range=(0, rnd + 1))
            for metric, kind, k in (("ndcg@5", "ndcg", 5), ("map", "map", None)):
                want = torch_ref.rank_metric(kind, margin, y, ptr, k).mean().item()
                print(f"rank metric diff {name} {metric} round {rnd}: {abs(res[name][metric][rnd] - want):.3e}")
                assert abs(res[name][metric][rnd] - want) <= TOL, (name, metric, rnd)
