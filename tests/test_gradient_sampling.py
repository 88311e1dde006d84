"""Gradient-based row sampling (sampling_method=gradient_based) on the CPU
reference backend: the threshold against an independent float64 oracle, the
keep / rescale rule, and the trainer's margins."""
import json
import math

import numpy as np
import pytest
import torch

from sagemaker_xgboost_container_amd.data.dmatrix import DMatrix
from sagemaker_xgboost_container_amd.models import trainer
from sagemaker_xgboost_container_amd.ops import torch_ref

SUBSAMPLES = (0.1, 0.5, 0.9)


def _pairs_with_norm(r, rng):
    """(n, 2) float32 pairs whose norms are about r, split at a random angle."""
    theta = rng.uniform(0.0, 0.5 * np.pi, size=r.shape)
    g = r * np.cos(theta) * rng.choice([-1.0, 1.0], size=r.shape)
    return np.stack([g, r * np.sin(theta)], axis=1).astype(np.float32)


def make_gh(kind, n, seed=0):
    """The distributions the sampler must handle; `n` is ignored by the two
    with a fixed shape."""
    rng = np.random.default_rng(seed)
    if kind == "constant":
        return np.tile(np.array([[0.3, 0.4]], dtype=np.float32), (n, 1))
    if kind == "lognormal3":
        return _pairs_with_norm(rng.lognormal(0.0, 3.0, size=n), rng)
    if kind == "zeros70":
        r = rng.uniform(0.1, 1.0, size=n)
        r[rng.random(n) < 0.7] = 0.0
        return _pairs_with_norm(r, rng)
    if kind == "logistic":
        margin = rng.normal(scale=3.0, size=n)
        y = (rng.random(n) < 0.5).astype(np.float64)
        prob = 1.0 / (1.0 + np.exp(-margin))
        return np.stack([prob - y, prob * (1.0 - prob)], axis=1).astype(np.float32)
    if kind == "single":
        return np.array([[0.25, 0.5]], dtype=np.float32)
    if kind == "huge_beside_tiny":
        r = np.concatenate([np.full(10, 1e6), rng.uniform(1e-6, 1e-3, size=4097)])
        return _pairs_with_norm(r, rng)
    if kind == "all_zero":
        return np.zeros((n, 2), dtype=np.float32)
    raise ValueError(kind)


DISTRIBUTIONS = ("constant", "lognormal3", "zeros70", "logistic", "single", "huge_beside_tiny")


def norms64(gh):
    g = gh[:, 0].astype(np.float64)
    h = gh[:, 1].astype(np.float64)
    return np.sqrt(g * g + h * h)


def F(r, mu):
    """sum_i min(1, r_i / mu) in float64; mu = 0 counts the rows with r > 0."""
    if mu == 0.0:
        return float((r > 0).sum())
    return float(np.minimum(1.0, r / mu).sum())


def oracle_mu(r, S):
    """Independent solution: bisect the monotone F in float64 (no closed form)."""
    if (r > 0).sum() <= S:
        return 0.0
    lo, hi = 0.0, max(float(r.max()), float(r.sum()) / S) * 2.0
    for _ in range(300):
        mid = 0.5 * (lo + hi)
        if F(r, mid) > S:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def oracle_p(r, mu):
    if mu == 0.0:
        return (r > 0).astype(np.float64)
    return np.minimum(1.0, r / mu)


def check_threshold(mu, gh, subsample):
    """mu (a float32 value) against the issue's bound |F(mu) - S| <= 2^-20 S,
    and mu = 0 exactly where the oracle says so."""
    r = norms64(gh)
    S = subsample * len(r)
    want = oracle_mu(r, S)
    if want == 0.0:
        assert mu == 0.0
        return
    assert mu > 0.0
    err = abs(F(r, float(mu)) - S)
    print(f"n={len(r)} subsample={subsample} mu={mu!r} oracle={want!r} |F-S|/S={err / S:.3e}")
    assert err <= 2.0 ** -20 * S


def non_borderline_u(gh, subsample, seed):
    """Uniform draws with no row near its keep probability (the oracle's)."""
    r = norms64(gh)
    p = oracle_p(r, oracle_mu(r, subsample * len(r)))
    u = np.random.default_rng(seed).random(len(r)).astype(np.float32)
    near = np.abs(u.astype(np.float64) - p) < 1e-4
    u[near] = (p[near] / 2).astype(np.float32)
    return u, p


def check_sample(rows, gh_scaled, gh, u, p):
    """Kept set, rescale, certain rows, dropped rows and the attached absmax
    of one gradient_sample result (numpy inputs) against the oracle's p."""
    keep = u.astype(np.float64) < p
    assert rows.dtype == torch.int32
    np.testing.assert_array_equal(rows.cpu().numpy(), np.nonzero(keep)[0])
    out = gh_scaled.cpu().numpy()
    assert out.dtype == np.float32 and out.shape == gh.shape
    want = gh.astype(np.float64)[keep] / p[keep][:, None]
    np.testing.assert_allclose(out[keep], want, rtol=1e-6, atol=0.0)
    certain = keep & (p == 1.0)
    np.testing.assert_array_equal(out[certain].view(np.uint32), gh[certain].view(np.uint32))
    assert not out[~keep].any()
    absmax = getattr(gh_scaled, "_smxgb_absmax", None)
    if absmax is not None:
        np.testing.assert_array_equal(absmax.cpu().numpy(), np.abs(out).max(axis=0))
    assert getattr(gh_scaled, "_smxgb_rootsum", None) is None


@pytest.mark.parametrize("subsample", SUBSAMPLES)
@pytest.mark.parametrize("kind", DISTRIBUTIONS)
def test_threshold_matches_bisection_oracle(kind, subsample):
    gh = make_gh(kind, 5000)
    mu = torch_ref.mvs_threshold(torch.from_numpy(gh), subsample * len(gh))
    assert mu.dtype == torch.float32
    check_threshold(float(mu), gh, subsample)


def test_threshold_is_zero_when_few_rows_have_gradients():
    # 30 % of 5000 rows are non-zero: mu = 0 at 0.5 and 0.9, positive at 0.1
    gh = make_gh("zeros70", 5000)
    npos = int((norms64(gh) > 0).sum())
    assert 0.1 * len(gh) < npos < 0.5 * len(gh)
    assert float(torch_ref.mvs_threshold(torch.from_numpy(gh), 0.5 * len(gh))) == 0.0
    assert float(torch_ref.mvs_threshold(torch.from_numpy(gh), 0.1 * len(gh))) > 0.0
    assert float(torch_ref.mvs_threshold(torch.from_numpy(make_gh("all_zero", 64)), 6.4)) == 0.0


@pytest.mark.parametrize("subsample", SUBSAMPLES)
@pytest.mark.parametrize("kind", DISTRIBUTIONS)
def test_keep_and_rescale(kind, subsample):
    gh = make_gh(kind, 5000)
    u, p = non_borderline_u(gh, subsample, seed=1)
    rows, gh_scaled = torch_ref.gradient_sample(torch.from_numpy(gh), subsample, torch.from_numpy(u))
    check_sample(rows, gh_scaled, gh, u, p)


@pytest.mark.parametrize("subsample", SUBSAMPLES)
def test_sample_size_and_gradient_sum_are_unbiased(subsample):
    gh = make_gh("logistic", 20000, seed=3)
    n = len(gh)
    r = norms64(gh)
    S = subsample * n
    p = oracle_p(r, oracle_mu(r, S))
    u = torch.rand(n, generator=torch.Generator().manual_seed(7))
    rows, gh_scaled = torch_ref.gradient_sample(torch.from_numpy(gh), subsample, u)
    assert abs(rows.numel() - S) <= 5.0 * math.sqrt(float((p * (1.0 - p)).sum())) + 1.0
    g = gh[:, 0].astype(np.float64)
    bound = 5.0 * math.sqrt(float((g * g * (1.0 / p - 1.0)).sum()))
    assert abs(float(gh_scaled[:, 0].double().sum()) - g.sum()) <= bound


# -- trainer ----------------------------------------------------------------

def trainer_data(n=3000, f=6, classes=2, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, f)).astype(np.float32)
    score = X[:, 0] * 1.5 - X[:, 1] + 0.5 * X[:, 2] * X[:, 3] + rng.normal(scale=0.5, size=n)
    if classes == 2:
        y = (score > 0).astype(np.float32)
    else:
        y = np.digitize(score, np.quantile(score, np.linspace(0, 1, classes + 1)[1:-1])).astype(np.float32)
    return X, y


def check_trainer_margins(params, dtrain, rounds=5):
    """After every round the trainer's own training margin (handed to feval
    for the training watchlist) must equal the model's prediction on ALL
    rows: a gradient-sampled tree updates the rows it dropped too."""
    seen = []

    def feval(margin, dmatrix):
        seen.append(np.array(margin, dtype=np.float64, copy=True))
        return "seen", 0.0

    bst = trainer.train(params, dtrain, num_boost_round=rounds, evals=[(dtrain, "train")],
                        feval=feval, verbose_eval=False)
    assert len(seen) == rounds
    for r, got in enumerate(seen):
        want = np.asarray(
            bst.predict(dtrain, output_margin=True, iteration_range=(0, r + 1)), dtype=np.float64
        ).reshape(got.shape)
        tol = 1e-5 * (1.0 + np.abs(want).max())
        worst = np.abs(got - want).max()
        print(f"round {r}: max |trainer margin - predict| = {worst:.3e} (tol {tol:.3e})")
        assert worst <= tol
    return bst


BASE = {"objective": "binary:logistic", "max_depth": 4, "eta": 0.3, "seed": 11, "device": "cpu"}


def model_json(bst):
    """The trees (not the recorded hyperparameters) as canonical JSON."""
    return json.dumps(bst.save_json()["learner"]["gradient_booster"], sort_keys=True)


def test_trainer_margin_covers_every_row():
    X, y = trainer_data()
    params = dict(BASE, subsample=0.3, sampling_method="gradient_based")
    check_trainer_margins(params, DMatrix(X, label=y))


def test_trainer_margin_covers_every_row_lossguide():
    X, y = trainer_data()
    params = dict(BASE, subsample=0.3, sampling_method="gradient_based",
                  grow_policy="lossguide", max_leaves=8)
    check_trainer_margins(params, DMatrix(X, label=y))


def test_trees_differ_from_uniform_sampling():
    X, y = trainer_data()
    dtrain = DMatrix(X, label=y)
    gradient = trainer.train(dict(BASE, subsample=0.3, sampling_method="gradient_based"),
                             dtrain, num_boost_round=3, verbose_eval=False)
    uniform = trainer.train(dict(BASE, subsample=0.3, sampling_method="uniform"),
                            dtrain, num_boost_round=3, verbose_eval=False)
    absent = trainer.train(dict(BASE, subsample=0.3), dtrain, num_boost_round=3, verbose_eval=False)
    assert model_json(gradient) != model_json(uniform)
    assert model_json(uniform) == model_json(absent)


def test_no_sampling_at_subsample_one():
    X, y = trainer_data()
    dtrain = DMatrix(X, label=y)
    with_option = trainer.train(dict(BASE, subsample=1.0, sampling_method="gradient_based"),
                                dtrain, num_boost_round=3, verbose_eval=False)
    without = trainer.train(dict(BASE), dtrain, num_boost_round=3, verbose_eval=False)
    assert model_json(with_option) == model_json(without)


def test_unknown_sampling_method_is_refused():
    X, y = trainer_data(n=200)
    with pytest.raises(ValueError, match="sampling_method"):
        trainer.train(dict(BASE, subsample=0.5, sampling_method="importance"),
                      DMatrix(X, label=y), num_boost_round=1, verbose_eval=False)
