"""Gradient-based row sampling on the device: the HIP radix-select threshold
and the keep / rescale kernel (csrc/smxgb_sampling.hip) against the float64
oracle and the reference backend, bit-determinism, and the trainer's margins
on every device growing path.

All tests require an MI355X (pytest tests -m gpu).
"""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from sagemaker_xgboost_container_amd.data.dmatrix import DMatrix
from sagemaker_xgboost_container_amd.models import trainer
from sagemaker_xgboost_container_amd.ops import torch_ref

from test_gradient_sampling import (
    DISTRIBUTIONS, SUBSAMPLES, check_sample, check_threshold, check_trainer_margins, make_gh,
    model_json, non_borderline_u, trainer_data,
)

pytestmark = pytest.mark.gpu

# one lane, the wave edges, more than one block, many blocks with a ragged tail
SIZES = (1, 63, 64, 65, 4097, 100003)
KINDS = DISTRIBUTIONS + ("all_zero",)


@pytest.fixture(scope="module")
def hip():
    from sagemaker_xgboost_container_amd.ops import hip as backend

    return backend


def _cases():
    """Distinct (kind, n) inputs: two of the distributions have a fixed shape."""
    seen = set()
    for kind in KINDS:
        for n in SIZES:
            gh = make_gh(kind, n)
            if (kind, len(gh)) not in seen:
                seen.add((kind, len(gh)))
                yield kind, gh


@pytest.mark.parametrize("kind", KINDS)
def test_threshold_against_oracle_and_reference(hip, kind):
    for _kind, gh in (c for c in _cases() if c[0] == kind):
        dev = torch.from_numpy(gh).cuda()
        for subsample in SUBSAMPLES:
            S = subsample * len(gh)
            mu = hip.mvs_threshold(dev, S)
            assert mu.is_cuda and mu.dtype == torch.float32 and mu.numel() == 1
            mu = float(mu)
            check_threshold(mu, gh, subsample)
            ref = float(torch_ref.mvs_threshold(torch.from_numpy(gh), S))
            assert abs(mu - ref) <= 2.0 ** -20 * ref, (kind, len(gh), subsample, mu, ref)


@pytest.mark.parametrize("kind", KINDS)
def test_keep_and_rescale(hip, kind):
    for _kind, gh in (c for c in _cases() if c[0] == kind):
        dev = torch.from_numpy(gh).cuda()
        for subsample in SUBSAMPLES:
            u, p = non_borderline_u(gh, subsample, seed=len(gh))
            rows, gh_scaled = hip.gradient_sample(dev, subsample, torch.from_numpy(u).cuda())
            assert gh_scaled._smxgb_absmax is not None
            check_sample(rows, gh_scaled, gh, u, p)


def test_two_calls_give_identical_bits(hip):
    for kind in ("lognormal3", "logistic", "huge_beside_tiny"):
        gh = torch.from_numpy(make_gh(kind, 100003)).cuda()
        u = torch.rand(gh.shape[0], device="cuda", generator=torch.Generator("cuda").manual_seed(5))
        first = None
        for _ in range(2):
            mu = hip.mvs_threshold(gh, 0.2 * gh.shape[0])
            rows, scaled = hip.gradient_sample(gh, 0.2, u)
            got = (mu.view(torch.int32).cpu(), rows.cpu(), scaled.view(torch.int32).cpu())
            if first is None:
                first = got
            else:
                for a, b in zip(first, got):
                    assert torch.equal(a, b)


# -- trainer ----------------------------------------------------------------

BASE = {"max_depth": 4, "eta": 0.3, "seed": 11, "device": "cuda",
        "subsample": 0.3, "sampling_method": "gradient_based"}


@pytest.fixture
def growers(monkeypatch):
    """Every HistGrower the trainer builds during the test."""
    made = []
    base = trainer.HistGrower

    class _Recording(base):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

    monkeypatch.setattr(trainer, "HistGrower", _Recording)
    return made


def test_trainer_margin_device_grower(growers):
    X, y = trainer_data()
    check_trainer_margins(dict(BASE, objective="binary:logistic"), DMatrix(X, label=y))
    assert growers[-1].grow_path == "device"
    assert growers[-1].state._traverse is not None  # margins went by traversal


def test_trainer_margin_per_level_loop(growers, monkeypatch):
    monkeypatch.setenv("SMXGB_NO_DEVICE_GROW", "1")
    X, y = trainer_data()
    check_trainer_margins(dict(BASE, objective="binary:logistic"), DMatrix(X, label=y))
    assert growers[-1].grow_path == "per_level"


def test_trainer_margin_multiclass_pipeline(growers):
    X, y = trainer_data(classes=3)
    params = dict(BASE, objective="multi:softprob", num_class=3)
    check_trainer_margins(params, DMatrix(X, label=y))
    assert growers[-1].device_async_ok() and growers[-1].grow_path == "device"


def test_trainer_margin_sparse_csr(growers, monkeypatch):
    monkeypatch.setenv("SMXGB_SPARSE", "1")
    X, y = trainer_data()
    mask = np.random.default_rng(2).random(X.shape) < 0.6
    csr = sp.csr_matrix(np.where(mask, X, 0.0).astype(np.float32))
    check_trainer_margins(dict(BASE, objective="binary:logistic"), DMatrix(csr, label=y))
    assert growers[-1].backend.NAME == "hip_sparse"


def test_same_seed_same_model_and_same_trees_on_both_growers(monkeypatch):
    X, y = trainer_data()
    params = dict(BASE, objective="binary:logistic")

    def run():
        return model_json(trainer.train(params, DMatrix(X, label=y), num_boost_round=4,
                                        verbose_eval=False))

    device = run()
    assert run() == device
    monkeypatch.setenv("SMXGB_NO_DEVICE_GROW", "1")
    assert run() == device
