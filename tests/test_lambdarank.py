"""torch_ref.lambdarank_gradients (the rule of lambdarank_pair_method=topk)
against a brute-force oracle that swaps every pair literally."""
import json

import numpy as np
import pytest
import torch

from sagemaker_xgboost_container_amd.data.dmatrix import DMatrix
from sagemaker_xgboost_container_amd.models import trainer
from sagemaker_xgboost_container_amd.models.objectives import create_objective
from sagemaker_xgboost_container_amd.ops import torch_ref

KINDS = ["rank:pairwise", "rank:ndcg", "rank:map"]
SIZES = [1, 2, 3, 7, 20, 7, 20, 3, 20, 7]  # groups 6 and 8: equal labels, equal margins


def _metric(kind, lab, k, exp_gain=True):
    """DCG over the list / IDCG@k (the quantity the rule's delta swaps), or
    AP over the whole list."""
    pos = np.arange(len(lab))
    if kind == "rank:map":
        rel = lab > 0
        return float((np.cumsum(rel)[rel] / (pos[rel] + 1.0)).sum() / rel.sum())
    gain = 2.0 ** lab - 1.0 if exp_gain else lab.astype(np.float64)
    idcg = (np.sort(gain)[::-1][:k] / np.log2(pos[:k] + 2.0)).sum()
    return float((gain / np.log2(pos + 2.0)).sum() / idcg) if idcg > 0 else 0.0


def _oracle(kind, s, lab, ptr, w, k, norm, score_norm, exp_gain):
    n = len(s)
    g, h = np.zeros(n), np.zeros(n)
    for g0, g1 in zip(ptr[:-1], ptr[1:]):
        order = g0 + np.array(sorted(range(g1 - g0), key=lambda i: (-s[g0 + i], i)), dtype=int)
        m = len(order)
        gg, hh, sig = np.zeros(m), np.zeros(m), 0.0
        for r in range(min(k, m)):
            for q in range(r + 1, m):
                if lab[order[r]] == lab[order[q]]:
                    continue
                hi, lo = (r, q) if lab[order[r]] > lab[order[q]] else (q, r)
                delta = 1.0
                if kind != "rank:pairwise":
                    swapped = order.copy()
                    swapped[[r, q]] = swapped[[q, r]]
                    delta = abs(_metric(kind, lab[swapped], k, exp_gain)
                                - _metric(kind, lab[order], k, exp_gain))
                d = float(s[order[hi]]) - float(s[order[lo]])
                rho = 1.0 / (1.0 + np.exp(d))
                if score_norm and s[order[0]] != s[order[-1]]:
                    delta /= abs(d) + 0.01
                lam, eta = rho * delta, max(rho * (1.0 - rho), 1e-16) * delta * 2.0
                gg[hi] -= lam
                gg[lo] += lam
                hh[[hi, lo]] += eta
                sig += 2.0 * lam
        fac = np.log2(1.0 + sig) / sig if (norm and sig > 0) else 1.0
        g[order], h[order] = gg * fac, hh * fac
    return g * w, np.maximum(h, 1e-16) * w


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(5)
    ptr = np.concatenate([[0], np.cumsum(SIZES)])
    n = int(ptr[-1])
    s = np.round(rng.normal(size=n) * 4) / 4  # quarter steps: ties inside groups
    s[3] = -0.0
    lab = rng.integers(0, 4, size=n)
    lab[ptr[6]:ptr[7]] = 2
    s[ptr[8]:ptr[9]] = 0.5
    w = rng.uniform(0.5, 2.0, size=n)
    return s.astype(np.float32), lab, ptr, w.astype(np.float32)


@pytest.mark.parametrize("score_norm", [False, True])
@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("k", [1, 3, 32])
@pytest.mark.parametrize("kind", KINDS + ["rank:ndcg/linear_gain"])
def test_reference_matches_brute_force(data, kind, k, norm, score_norm):
    s, lab, ptr, w = data
    kind, exp_gain = kind.split("/")[0], "/" not in kind
    lab = np.minimum(lab, 1) if kind == "rank:map" else lab
    want_g, want_h = _oracle(kind, s, lab, ptr, w.astype(np.float64), k, norm, score_norm, exp_gain)
    got = torch_ref.lambdarank_gradients(
        torch.from_numpy(s), torch.from_numpy(lab.astype(np.float32)), ptr, torch.from_numpy(w),
        kind, k, norm, score_norm, exp_gain, details=True,
    )
    assert np.abs(want_g).max() > 0
    # g cancels: relative to the largest |g|; h does not: purely relative
    np.testing.assert_allclose(got["g"], want_g, rtol=1e-12, atol=1e-12 * np.abs(want_g).max())
    np.testing.assert_allclose(got["h"], want_h, rtol=1e-12, atol=0)
    assert np.all(want_g[ptr[6]:ptr[7]] == 0) and np.all(got["g"][ptr[6]:ptr[7]] == 0)


@pytest.mark.parametrize("kind,label", [("rank:ndcg", 32.0), ("rank:ndcg", 1.5), ("rank:map", 2.0)])
def test_bad_label_is_refused(kind, label):
    y = torch.tensor([0.0, label, 1.0])
    with pytest.raises(ValueError, match=str(label)):
        torch_ref.lambdarank_gradients(torch.zeros(3), y, None, None, kind)
    with pytest.raises(ValueError, match=str(label)):
        create_objective(kind, {"lambdarank_pair_method": "topk"}).validate_labels(y)


def _tiny_rank_set():
    rng = np.random.default_rng(0)
    X = rng.normal(size=(40, 3)).astype(np.float32)
    dtrain = DMatrix(X, label=rng.integers(0, 3, size=40).astype(np.float32))
    dtrain.set_group([20, 20])
    return X, dtrain


@pytest.mark.parametrize("extra,match", [
    ({"lambdarank_unbiased": 1}, "lambdarank_unbiased"),
    ({"lambdarank_num_pair_per_sample": 5000}, "lambdarank_num_pair_per_sample"),
])
def test_training_refuses_what_it_does_not_build(extra, match):
    params = {"objective": "rank:ndcg", "lambdarank_pair_method": "topk", "device": "cpu", **extra}
    with pytest.raises(ValueError, match=match):
        trainer.train(params, _tiny_rank_set()[1], num_boost_round=1, verbose_eval=False)


def test_model_with_refused_training_settings_still_predicts(tmp_path):
    """A model file may carry topk settings that training here refuses (as
    files written elsewhere do); loading it and predicting is not training."""
    X, dtrain = _tiny_rank_set()
    bst = trainer.train({"objective": "rank:ndcg", "device": "cpu", "max_depth": 2}, dtrain,
                        num_boost_round=2, verbose_eval=False)
    path = tmp_path / "m.json"
    bst.save_model(str(path))
    model = json.loads(path.read_text())
    model["learner"]["objective"]["lambdarank_param"].update(
        lambdarank_pair_method="topk", lambdarank_unbiased="1",
        lambdarank_num_pair_per_sample="100000")
    path.write_text(json.dumps(model))
    from sagemaker_xgboost_container_amd.models.booster import Booster

    loaded = Booster()
    loaded.load_model(str(path))
    np.testing.assert_array_equal(loaded.predict(X), bst.predict(X))


def test_topk_trains_deterministically_and_round_trips(tmp_path):
    rng = np.random.default_rng(0)
    X = rng.normal(size=(200, 4)).astype(np.float32)
    y = np.clip(np.round(X[:, 0] + rng.normal(scale=0.3, size=200) + 1.5), 0, 3).astype(np.float32)
    params = {"objective": "rank:ndcg", "lambdarank_pair_method": "topk", "ndcg_exp_gain": 0,
              "max_depth": 3, "eval_metric": "ndcg", "device": "cpu"}
    texts = []
    for _ in range(2):
        dtrain = DMatrix(X, label=y)
        dtrain.set_group([20] * 10)
        res = {}
        bst = trainer.train(params, dtrain, num_boost_round=5, evals=[(dtrain, "train")],
                            evals_result=res, verbose_eval=False)
        path = tmp_path / "m.json"
        bst.save_model(str(path))
        texts.append(path.read_text())
    assert res["train"]["ndcg"][-1] > res["train"]["ndcg"][0]
    assert texts[0] == texts[1]
    block = json.loads(texts[0])["learner"]["objective"]["lambdarank_param"]
    assert block["lambdarank_pair_method"] == "topk" and block["ndcg_exp_gain"] == "0"
    assert block["lambdarank_num_pair_per_sample"] == "32"
