"""The `xgboost` shim package: reference customer scripts run unmodified.

The reference container satisfies `import xgboost as xgb` with the PyPI
wheel; this container satisfies it with the native framework. Coverage
mirrors what the reference's script-mode examples actually call
(test/resources/boston/single_machine_customer_script.py,
abalone_distributed.py): DMatrix-from-DataFrame, train, Booster
save/load, sklearn wrappers, cv with early stopping, plain pickle of an
upstream Booster, rabit helpers.
"""
import os
import pickle

import numpy as np
import pandas as pd
import pytest

import xgboost as xgb


def _data(n=800, f=5, seed=0, classes=None):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, f)).astype(np.float32)
    if classes:
        y = rng.integers(0, classes, n).astype(np.float32)
    else:
        y = (X[:, 0] * 2 - X[:, 1] + rng.normal(scale=0.3, size=n)).astype(np.float32)
    return X, y


class TestCoreSurface:
    def test_dmatrix_from_dataframe_with_names(self):
        X, y = _data()
        df = pd.DataFrame(X, columns=[f"col{i}" for i in range(5)])
        dm = xgb.DMatrix(data=df, label=pd.Series(y))
        assert dm.num_row() == 800
        assert dm.num_col() == 5
        assert dm.feature_names == ["col0", "col1", "col2", "col3", "col4"]

    def test_train_and_booster_roundtrip(self, tmp_path):
        X, y = _data()
        dtrain = xgb.DMatrix(X, label=y)
        bst = xgb.train({"objective": "reg:squarederror", "max_depth": 3},
                        dtrain, num_boost_round=5)
        path = tmp_path / "model.json"
        bst.save_model(path)
        loaded = xgb.Booster()
        loaded.load_model(path)
        np.testing.assert_allclose(bst.predict(X[:20]), loaded.predict(X[:20]), atol=1e-6)

    def test_version_and_modules_exist(self):
        assert xgb.__version__
        assert xgb.rabit.get_rank() == 0
        assert xgb.rabit.get_world_size() == 1
        xgb.rabit.init()
        xgb.rabit.tracker_print("hello")
        xgb.rabit.finalize()
        assert hasattr(xgb.callback, "TrainingCallback")
        with xgb.collective.CommunicatorContext():
            pass

    def test_plain_pickle_of_upstream_booster(self):
        # with the shim installed, xgboost.core.Booster resolves here and
        # the upstream pickle's handle-bytes state loads via __setstate__
        path = os.path.join(
            os.path.dirname(os.path.abspath(__file__)),
            "golden", "reference_resources", "models", "pickled_model", "xgboost-model",
        )
        with open(path, "rb") as f:
            bst = pickle.load(f)
        assert isinstance(bst, xgb.Booster)
        assert len(bst.trees) == 60
        p = bst.predict(np.zeros((3, 4), dtype=np.float32))
        assert p.shape == (3, 3)


class TestSklearnAPI:
    def test_regressor_boston_script_pattern(self, tmp_path):
        X, y = _data(1000, 6, seed=1)
        df = pd.DataFrame(X)
        reg = xgb.XGBRegressor(
            objective="reg:squarederror", colsample_bytree=0.8, learning_rate=0.1,
            max_depth=5, reg_alpha=10, n_estimators=10,
        )
        reg.fit(df.iloc[:800], y[:800])
        preds = reg.predict(df.iloc[800:])
        assert preds.shape == (200,)
        rmse = float(np.sqrt(np.mean((preds - y[800:]) ** 2)))
        base = float(np.sqrt(np.mean((y[800:] - y[:800].mean()) ** 2)))
        assert rmse < base  # learned something
        reg.get_booster().save_model(tmp_path / "xgb-boston.model")
        fi = reg.feature_importances_
        assert fi.shape == (6,)
        assert abs(float(fi.sum()) - 1.0) < 1e-5

    def test_classifier_binary_and_multiclass(self):
        X, y = _data(600, 4, seed=2)
        yb = (y > 0).astype(int)
        clf = xgb.XGBClassifier(n_estimators=5, max_depth=3)
        clf.fit(X, yb)
        labels = clf.predict(X[:50])
        assert set(np.unique(labels)) <= {0, 1}
        proba = clf.predict_proba(X[:50])
        assert proba.shape == (50, 2)
        np.testing.assert_allclose(proba.sum(axis=1), 1.0, atol=1e-5)
        assert clf.score(X, yb) > 0.6

        Xm, ym = _data(600, 4, seed=3, classes=3)
        clf3 = xgb.XGBClassifier(n_estimators=4, max_depth=3)
        clf3.fit(Xm, ym.astype(int))
        assert clf3.n_classes_ == 3
        assert clf3.predict_proba(Xm[:10]).shape == (10, 3)

    def test_set_get_params(self):
        reg = xgb.XGBRegressor(n_estimators=7, learning_rate=0.2)
        params = reg.get_params()
        assert params["n_estimators"] == 7
        reg.set_params(n_estimators=3, max_depth=2)
        assert reg.n_estimators == 3
        assert reg.kwargs["max_depth"] == 2

    def test_ranker(self):
        rng = np.random.default_rng(4)
        X = rng.normal(size=(300, 4)).astype(np.float32)
        y = rng.integers(0, 3, 300).astype(np.float32)
        qid = np.repeat(np.arange(30), 10)
        rk = xgb.XGBRanker(n_estimators=3, max_depth=3)
        rk.fit(X, y, qid=qid)
        assert rk.predict(X[:10]).shape == (10,)


class TestCV:
    def test_cv_boston_script_pattern(self):
        X, y = _data(1000, 5, seed=5)
        dm = xgb.DMatrix(X, label=y)
        cv_results = xgb.cv(
            dtrain=dm,
            params={"objective": "reg:squarederror", "max_depth": 4,
                    "learning_rate": 0.3, "alpha": 1},
            nfold=5,
            num_boost_round=30,
            early_stopping_rounds=5,
            metrics="rmse",
            as_pandas=True,
            seed=100,
        )
        assert "test-rmse-mean" in cv_results.columns
        assert "train-rmse-std" in cv_results.columns
        # rmse improves over rounds then early stopping bounds the length
        assert len(cv_results) <= 30
        col = cv_results["test-rmse-mean"].to_numpy()
        assert col[min(len(col) - 1, 10)] < col[0]

    def test_cv_dict_output(self):
        X, y = _data(400, 4, seed=6)
        out = xgb.cv({"objective": "reg:squarederror", "max_depth": 3},
                     xgb.DMatrix(X, label=y), num_boost_round=3, nfold=3,
                     as_pandas=False)
        assert isinstance(out, dict) or hasattr(out, "columns")


def test_cv_stratified_preserves_class_balance():
    rng = np.random.default_rng(9)
    X = rng.normal(size=(600, 4)).astype(np.float32)
    y = (rng.random(600) < 0.2).astype(np.float32)  # 20% positives
    out = xgb.cv(
        {"objective": "binary:logistic", "max_depth": 3},
        xgb.DMatrix(X, label=y), num_boost_round=3, nfold=5,
        stratified=True, metrics="logloss", as_pandas=False,
    )
    key = "test-logloss-mean"
    assert len(out[key]) == 3
    # re-derive the folds the same way and check balance
    from xgboost.cv import cv as _  # noqa: F401
    idx = np.arange(600)
    g = np.random.default_rng(0)
    g.shuffle(idx)
    order = idx[np.argsort(y[idx], kind="stable")]
    folds = [order[k::5] for k in range(5)]
    rates = [float(y[f].mean()) for f in folds]
    assert max(rates) - min(rates) < 0.05
