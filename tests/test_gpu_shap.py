"""Device TreeSHAP (contributions, interactions) and pred_leaf kernels vs
the host implementations on the same forest.

Kernel tests call hip.tree_shap / hip.tree_shap_interactions /
hip.pred_leaf directly, so a host fallback cannot hide a broken kernel;
booster-level tests make the host functions raise. Comparator: the host
path (fp64 recursion, parallel C++) — both sides compute in fp64 and round
once to float32, so rtol 1e-5 / atol 1e-6 on the float32 outputs (the
tolerance test_cpp_matches_python_fallback uses between two fp64
implementations). The f=4 models are also checked against the brute-force
Shapley definitions at rtol 1e-4 / atol 1e-5.

All tests require an MI355X (pytest tests -m gpu).
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

from sagemaker_xgboost_container_amd.data.dmatrix import DMatrix
from sagemaker_xgboost_container_amd.models import trainer
from sagemaker_xgboost_container_amd.models.booster import Booster
from sagemaker_xgboost_container_amd.ops import torch_ref

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from sagemaker_xgboost_container_amd.ops import hip
else:  # allow collection on CPU boxes
    hip = None

_HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name, filename):
    spec = importlib.util.spec_from_file_location(name, os.path.join(_HERE, filename))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_RTOL, _ATOL = 1e-5, 1e-6


def _train(objective="reg:squarederror", n=400, f=4, depth=3, rounds=3, nan_frac=0.0,
           num_class=None, seed=0, **extra):
    """Small host-trained model whose target depends on every feature, so
    paths hold up to min(depth, f) distinct features."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, f)).astype(np.float32)
    if nan_frac:
        X[rng.random(size=X.shape) < nan_frac] = np.nan
    Xz = np.nan_to_num(X)
    signal = sum((1.0 + 0.3 * j) * Xz[:, j] * (1 if j % 2 == 0 else -1) for j in range(f))
    signal = signal + Xz[:, 0] * Xz[:, f - 1]
    if objective.startswith("multi"):
        y = np.digitize(signal, np.quantile(signal, [1 / 3, 2 / 3])).astype(np.float32)
    elif objective.startswith("binary"):
        y = (signal > 0).astype(np.float32)
    else:
        y = signal.astype(np.float32)
    params = {"objective": objective, "max_depth": depth, "eta": 0.4, "device": "cpu"}
    if num_class:
        params["num_class"] = num_class
    params.update(extra)
    bst = trainer.train(params, DMatrix(X, label=y), num_boost_round=rounds, verbose_eval=False)
    return bst, X


def _flats(bst):
    """(host flat forest, device flat forest with path tables)."""
    return bst._cpu_flat_forest(), bst._device_flat_forest(torch.device("cuda"), with_paths=True)


def _path_len(bst, dev, t_begin=0, t_end=None):
    t_end = dev["n_trees"] if t_end is None else t_end
    return hip.shap_limits(dev["shap_paths"], bst.n_outputs, bst.num_features, t_begin, t_end)[0]


def _check_kernels(bst, X, t_begin=0, t_end=None, interactions=True):
    """Direct kernel calls vs the host path on the same forest."""
    cpu, dev = _flats(bst)
    k = bst.n_outputs
    Xc = torch.as_tensor(X, dtype=torch.float32)
    Xd = Xc.cuda()
    got = hip.tree_shap(dev, Xd, k, t_begin, t_end)
    want = torch_ref.tree_shap(cpu, Xc, k, t_begin, t_end)
    assert got.is_cuda and got.dtype == torch.float64 and got.shape == want.shape
    np.testing.assert_allclose(
        got.to(torch.float32).cpu().numpy(), want.to(torch.float32).numpy(),
        rtol=_RTOL, atol=_ATOL,
    )
    if interactions:
        got_i = hip.tree_shap_interactions(dev, Xd, k, t_begin, t_end)
        want_i = torch_ref.tree_shap_interactions(cpu, Xc, k, t_begin, t_end)
        assert got_i.shape == want_i.shape
        np.testing.assert_allclose(
            got_i.to(torch.float32).cpu().numpy(), want_i.to(torch.float32).numpy(),
            rtol=_RTOL, atol=_ATOL,
        )
    leaves = hip.pred_leaf(dev, Xd, t_begin, t_end)
    assert leaves.is_cuda and leaves.dtype == torch.int32
    np.testing.assert_array_equal(
        leaves.cpu().numpy(), torch_ref.pred_leaf(cpu, Xc, t_begin, t_end).numpy()
    )


@pytest.fixture(scope="module")
def depth3():
    return _train("reg:squarederror", n=400, f=4, depth=3, rounds=3)


@pytest.fixture(scope="module")
def depth5():
    return _train("binary:logistic", n=600, f=8, depth=5, rounds=3, nan_frac=0.2)


class TestKernelsMatchHost:
    def test_depth3_group_exactly_full(self, depth3):
        bst, X = depth3
        assert _path_len(bst, _flats(bst)[1]) == 4  # W = 4, no idle lane
        _check_kernels(bst, X[:67])  # 67: not a multiple of groups per block

    def test_depth5_idle_lanes(self, depth5):
        bst, X = depth5
        assert _path_len(bst, _flats(bst)[1]) == 6  # W = 8, two idle lanes
        _check_kernels(bst, X[:67])

    def test_single_row(self, depth3):
        bst, X = depth3
        _check_kernels(bst, X[:1])

    def test_two_features_depth4_merged_paths(self):
        # every depth-4 path repeats a feature: merging, lo/hi interval,
        # nan_follows conjunction
        bst, X = _train("binary:logistic", n=500, f=2, depth=4, rounds=3, nan_frac=0.2)
        assert max(t.max_depth() for t in bst.trees) == 4
        assert _path_len(bst, _flats(bst)[1]) == 3
        _check_kernels(bst, X[:80])

    def test_stump_forest_bias_only(self):
        bst, X = _train("reg:squarederror", n=200, f=4, depth=3, rounds=3, gamma=1e9)
        assert all(t.num_nodes == 1 for t in bst.trees)
        assert _path_len(bst, _flats(bst)[1]) == 1
        _check_kernels(bst, X[:20])
        out = bst.predict(X[:20], pred_contribs=True)
        assert not out[:, :-1].any()
        np.testing.assert_allclose(out[:, -1], bst.predict(X[:20], output_margin=True),
                                   rtol=1e-5, atol=1e-6)

    def test_many_trees_few_rows_chunked(self):
        bst, X = _train("reg:squarederror", n=300, f=6, depth=3, rounds=40)
        tiles = list(hip._shap_tiles(3, 40, 7 * 8))
        assert len(tiles) == 1 and tiles[0][2] > 1  # n_chunks > 1
        _check_kernels(bst, X[:3])

    def test_many_rows_two_trees_single_chunk(self, monkeypatch):
        bst, X = _train("reg:squarederror", n=300, f=6, depth=3, rounds=2)
        _check_kernels(bst, X[:300])
        monkeypatch.setattr(hip, "_SHAP_TARGET_GROUPS", 1)
        assert list(hip._shap_tiles(300, 2, 7 * 8))[0][2] == 1  # n_chunks == 1
        _check_kernels(bst, X[:300])

    def test_row_tiling_under_partial_cap(self, depth3, monkeypatch):
        bst, X = depth3
        monkeypatch.setattr(hip, "SHAP_PARTIAL_CAP", 25 * 5 * 5 * 8)  # 25 rows of interactions
        assert len(list(hip._shap_tiles(67, 3, 5 * 5 * 8))) == 3
        _check_kernels(bst, X[:67])

    def test_multiclass(self):
        bst, X = _train("multi:softprob", n=300, f=5, depth=3, rounds=3, num_class=3)
        _check_kernels(bst, X[:50])

    def test_dart_weight_drop(self):
        bst, X = _train("reg:squarederror", n=300, f=5, depth=3, rounds=6, booster="dart",
                        rate_drop=0.5, one_drop=1)
        assert any(w != 1.0 for w in bst.weight_drop)
        _check_kernels(bst, X[:40])

    def test_nan_and_infinite_inputs(self, depth5):
        bst, X = depth5
        rows = X[:40].copy()
        rows[0, :] = np.nan
        rows[1, ::2] = np.inf
        rows[1, 1::2] = -np.inf
        rows[2, :] = np.inf
        rows[3, :] = -np.inf
        _check_kernels(bst, rows)

    def test_legacy_saved_booster(self):
        path = os.path.join(_HERE, "golden", "reference_resources", "models", "saved_booster",
                            "xgboost-model")
        b = Booster()
        b.load_model(path)
        X = np.random.default_rng(5).normal(size=(20, 4)).astype(np.float32)
        _check_kernels(b, X)

    def test_tree_range(self):
        bst, X = _train("reg:squarederror", n=300, f=5, depth=3, rounds=5)
        _check_kernels(bst, X[:30], 1, 3)
        got = bst.predict(X[:30], pred_contribs=True, iteration_range=(1, 3))
        bst.set_param("predictor", "cpu_predictor")
        want = bst.predict(X[:30], pred_contribs=True, iteration_range=(1, 3))
        np.testing.assert_allclose(got, want, rtol=_RTOL, atol=_ATOL)


class TestBruteForce:
    """f = 4 models against the definitions (oracles of the host tests)."""

    @pytest.mark.parametrize("objective,nan_frac", [("reg:squarederror", 0.0),
                                                    ("binary:logistic", 0.15)])
    def test_contribs_and_interactions(self, objective, nan_frac, monkeypatch):
        shap_oracle = _load("_treeshap_oracle", "test_treeshap.py")
        inter_oracle = _load("_interactions_oracle", "test_pred_interactions.py")
        bst, X = _train(objective, n=400, f=4, depth=3, rounds=2, nan_frac=nan_frac)
        rows = X[:4]

        def _host(*a, **kw):
            raise AssertionError("host TreeSHAP served a device request")

        monkeypatch.setattr(torch_ref, "tree_shap", _host)
        contribs = bst.predict(rows, pred_contribs=True)
        inter = bst.predict(rows, pred_interactions=True)
        base = bst.objective().base_margin(bst.base_score)
        off = ~np.eye(4, dtype=bool)
        for r in range(4):
            expected = shap_oracle._brute_shap(bst.trees, rows[r], 4)
            expected[-1] += base
            np.testing.assert_allclose(contribs[r], expected, rtol=1e-4, atol=1e-5)
            expected_i = inter_oracle._brute_interactions(bst.trees, rows[r], 4)
            np.testing.assert_allclose(inter[r, :4, :4][off], expected_i[off],
                                       rtol=1e-4, atol=1e-5)


class TestBoosterRouting:
    def test_device_path_serves_predict(self, depth5, monkeypatch):
        bst, X = depth5
        rows = X[:50]
        bst.set_param("predictor", "cpu_predictor")
        want_c = bst.predict(rows, pred_contribs=True)
        want_i = bst.predict(rows, pred_interactions=True)
        want_l = bst.predict(rows, pred_leaf=True)
        bst.set_param("predictor", None)

        def _host(*a, **kw):
            raise AssertionError("host path served a device request")

        monkeypatch.setattr(torch_ref, "tree_shap", _host)
        monkeypatch.setattr(torch_ref, "pred_leaf", _host)
        np.testing.assert_allclose(bst.predict(rows, pred_contribs=True), want_c,
                                   rtol=_RTOL, atol=_ATOL)
        np.testing.assert_allclose(bst.predict(rows, pred_interactions=True), want_i,
                                   rtol=_RTOL, atol=_ATOL)
        np.testing.assert_array_equal(bst.predict(rows, pred_leaf=True), want_l)

    def test_path_length_limit_routes_to_host(self, depth3, monkeypatch):
        bst, X = depth3
        rows = X[:20]
        bst.set_param("predictor", "cpu_predictor")
        want = bst.predict(rows, pred_contribs=True)
        bst.set_param("predictor", None)

        def _device(*a, **kw):
            raise AssertionError("device kernel ran beyond its path-length limit")

        monkeypatch.setattr(hip, "SHAP_MAX_PATH_LEN", 2)
        monkeypatch.setattr(hip, "tree_shap", _device)
        np.testing.assert_array_equal(bst.predict(rows, pred_contribs=True), want)

    def test_narrow_input_raises_before_launch(self, depth3):
        bst, X = depth3
        _, dev = _flats(bst)
        max_f = int(dev["shap_paths"]["tree_max_feature"].max())
        narrow = torch.as_tensor(X[:5, :max_f]).contiguous().cuda()
        with pytest.raises(ValueError):
            hip.tree_shap(dev, narrow, 1)
        with pytest.raises(ValueError):
            hip.tree_shap_interactions(dev, narrow, 1)
        with pytest.raises(ValueError):
            hip.pred_leaf(dev, narrow)
        with pytest.raises(ValueError):  # host tensors never reach a launch
            hip.tree_shap(dev, torch.as_tensor(X[:5]), 1)


class TestDeterminism:
    def test_repeated_calls_bit_identical(self, depth5):
        bst, X = depth5
        _, dev = _flats(bst)
        Xd = torch.as_tensor(X[:64]).cuda()
        c = [hip.tree_shap(dev, Xd, 1).cpu().numpy() for _ in range(3)]
        i = [hip.tree_shap_interactions(dev, Xd, 1).cpu().numpy() for _ in range(3)]
        assert np.array_equal(c[0], c[1]) and np.array_equal(c[0], c[2])
        assert np.array_equal(i[0], i[1]) and np.array_equal(i[0], i[2])
