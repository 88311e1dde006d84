"""HIP multiclass gradients and mlogloss / merror (csrc/smxgb_multiclass.hip)
against the rule written out in float64. The bound on the kernels' error is
twice the error of the torch float32 code on the same inputs plus 1e-7 (for
the other summation order over the k classes).

Observed on an MI355X, largest absolute gradient error over the cases of a
class count (kernel / torch float32): see profiles/r21_multiclass_objective.md."""
import numpy as np
import pytest
import torch

from sagemaker_xgboost_container_amd.data.dmatrix import DMatrix
from sagemaker_xgboost_container_amd.models import eval_metrics, trainer
from sagemaker_xgboost_container_amd.models.objectives import Softmax

pytestmark = pytest.mark.gpu

CLASSES = [2, 3, 7, 33, "cap"]


@pytest.fixture
def hip():
    from sagemaker_xgboost_container_amd.ops import hip

    previous = hip.set_softmax_mode("hip")
    yield hip
    hip.set_softmax_mode(previous)


def _inputs(hip, k, n_kind, margins, weighted):
    """k ("cap": the kernels' cap), the n_kind-th of the row counts 1, R - 1,
    R + 1, 3 R + 5 for the tile rows R of that k -> margin, y, weight."""
    k = hip.SOFTMAX_CAP if k == "cap" else k
    R = hip.softmax_tile_rows(k)
    n = [1, R - 1, R + 1, 3 * R + 5][n_kind]
    g = torch.Generator(device="cuda").manual_seed(1000 * k + n)
    draw = lambda *shape: torch.rand(*shape, generator=g, device="cuda")  # noqa: E731
    if margins == "normal":
        m = torch.randn(n, k, generator=g, device="cuda")
    elif margins == "big":  # overflows without the max subtraction
        m = draw(n, k) * 160 - 80
    elif margins == "equal":  # p = 1 / k exactly
        m = torch.full((n, k), 0.25, device="cuda")
    else:  # "ranked": the row's classes in a random order, 160 / k >= 0.5 apart
        m = torch.argsort(draw(n, k), dim=1).float() * (160 / k) - 80
    y = torch.randint(k, (n,), generator=g, device="cuda").float()
    w = (torch.randint(1, 17, (n,), generator=g, device="cuda") / 8).float() if weighted else None
    return m, y, w


def _gradients64(m, y, w):
    p = torch.softmax(m.double(), dim=-1)
    g = p - torch.nn.functional.one_hot(y.long(), m.shape[1])
    gh = torch.stack([g, torch.clamp(2 * p * (1 - p), min=1e-16)], dim=-1)
    return gh if w is None else gh * w.double().reshape(-1, 1, 1)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("margins", ["normal", "big", "equal"])
@pytest.mark.parametrize("k", CLASSES)
def test_gradients_match_float64(hip, k, margins, weighted):
    for n_kind in range(4):
        m, y, w = _inputs(hip, k, n_kind, margins, weighted)
        ref = _gradients64(m, y, w)
        gh = hip.softmax_gradients(m, y, w)
        hip.set_softmax_mode("torch")
        gh_torch = Softmax({"num_class": m.shape[1]}).gradients(m, y, w)
        hip.set_softmax_mode("hip")
        assert not hasattr(gh_torch, "_smxgb_class_absmax")
        err = float((gh.double() - ref).abs().max())
        err_torch = float((gh_torch.double() - ref).abs().max())
        print(f"k={m.shape[1]} n={m.shape[0]} {margins} weighted={weighted}: "
              f"kernel {err:.3e} torch {err_torch:.3e}")
        assert gh.shape == ref.shape and err <= 2 * err_torch + 1e-7
        assert torch.equal(gh._smxgb_class_absmax, gh.abs().amax(0))
        assert all(gh[:, c, :].is_contiguous() for c in range(m.shape[1]))
        assert torch.equal(hip.softmax_gradients(m, y, w), gh)


@pytest.mark.parametrize("kind", ["mlogloss", "merror"])
@pytest.mark.parametrize("k,n_kind,margins,weighted", [
    (2, 0, "normal", False), (3, 1, "big", True), (7, 3, "normal", True),
    (7, 2, "big", False), (33, 3, "big", True), ("cap", 2, "normal", False),
])
def test_metrics_match_float64(hip, kind, k, n_kind, margins, weighted):
    m, y, w = _inputs(hip, k, n_kind, "ranked" if kind == "merror" else margins, weighted)
    k = m.shape[1]
    # row 0: the two top margins equal, the label the lower class: correct
    m[0, 0] = m[0, k - 1] = 81.0
    y[0] = 0.0
    if kind == "mlogloss" and m.shape[0] > 1 and margins == "big":  # p_y = e^-160: the 1e-16 clamp
        m[1] = 80.0
        m[1, 1] = -80.0
        y[1] = 1.0
    p = torch.softmax(m.double(), dim=-1)
    if kind == "mlogloss":
        term = -torch.log(torch.clamp(p.gather(1, y.long()[:, None])[:, 0], min=1e-16))
    else:
        term = (m.argmax(dim=1) != y.long()).double()
        term[0] = 0.0
    wd = torch.ones_like(term) if w is None else w.double()
    ref = float((wd * term).sum() / wd.sum())
    num, den = hip.softmax_metric(kind, m, y, w)
    assert den == float(wd.sum())
    hip.set_softmax_mode("torch")
    torch32 = eval_metrics.evaluate(kind, m, y, w, None)
    hip.set_softmax_mode("hip")
    assert eval_metrics.evaluate(kind, m, y, w, None) == num / den
    print(f"{kind} k={k} n={m.shape[0]}: ref {ref!r} kernel {num / den!r} torch {torch32!r}")
    if kind == "merror":
        assert num / den == ref  # weights in eighths: every sum is exact
    else:
        assert abs(num / den - ref) <= 2 * abs(torch32 - ref) + 1e-7 * abs(ref)


def test_above_the_cap_keeps_torch(hip):
    k = hip.SOFTMAX_CAP + 1
    g = torch.Generator(device="cuda").manual_seed(3)
    m = torch.randn(70, k, generator=g, device="cuda")
    y = torch.randint(k, (70,), generator=g, device="cuda").float()
    assert hip.softmax_tile_rows(k) == 0 and hip.softmax_gradients(m, y, None) is None
    assert hip.softmax_metric("mlogloss", m, y, None) is None
    gh = Softmax({"num_class": k}).gradients(m, y, None)
    hip.set_softmax_mode("torch")
    assert torch.equal(gh, Softmax({"num_class": k}).gradients(m, y, None))
    assert float((gh.double() - _gradients64(m, y, None)).abs().max()) < 1e-6


def test_train_agrees_between_modes(hip, monkeypatch):
    rng = np.random.default_rng(11)
    X = rng.normal(size=(2000, 6)).astype(np.float32)
    y = ((X[:, 0] > 0.3).astype(int) + (X[:, 1] + X[:, 2] > 0)).astype(np.float32)
    Xv, yv = X[:700] + 0.1, y[:700]
    carried = []
    scale = hip.compute_scale
    monkeypatch.setattr(
        hip, "compute_scale",
        lambda gh, comm=None: carried.append(hasattr(gh, "_smxgb_absmax")) or scale(gh, comm=comm))
    out = {}
    for mode in ("hip", "torch"):
        hip.set_softmax_mode(mode)
        del carried[:]
        res = {}
        bst = trainer.train(
            {"objective": "multi:softprob", "num_class": 3, "max_depth": 3, "device": "cuda",
             "eval_metric": ["mlogloss", "merror"]},
            DMatrix(X, label=y), num_boost_round=3, evals=[(DMatrix(Xv, label=yv), "val")],
            evals_result=res, verbose_eval=False)
        out[mode] = res["val"], bst.predict(Xv), bst.predict(Xv, output_margin=True), list(carried)
    assert out["hip"][3] == [True] * 9 and out["torch"][3] == [False] * 9
    # the torch float32 metric's own error on the final margins sets the bound
    mv = torch.as_tensor(out["torch"][2], device="cuda").reshape(len(yv), 3)
    yd = torch.as_tensor(yv, device="cuda")
    for kind in ("mlogloss", "merror"):
        hip.set_softmax_mode("torch")
        v32 = eval_metrics.evaluate(kind, mv, yd, None, None)
        p = torch.softmax(mv.double(), dim=-1)
        v64 = float(-torch.log(p.gather(1, yd.long()[:, None])).mean() if kind == "mlogloss"
                    else (mv.argmax(1) != yd.long()).double().mean())
        for a, b in zip(out["hip"][0][kind], out["torch"][0][kind]):
            print(f"{kind}: hip {a!r} torch {b!r} (torch float32 error {abs(v32 - v64):.3e})")
            assert abs(a - b) <= 2 * abs(v32 - v64) + 1e-7 * abs(b)
    np.testing.assert_allclose(out["hip"][1], out["torch"][1], rtol=0, atol=1e-5)
