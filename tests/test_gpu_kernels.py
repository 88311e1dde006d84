"""HIP kernel numerics vs the plain-PyTorch fp32/fp64 reference backend.

All tests require an MI355X (run via gpurun: pytest tests -m gpu).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from sagemaker_xgboost_container_amd.ops import hip, torch_ref
    from sagemaker_xgboost_container_amd.ops.quantize import quantize
else:  # allow collection on CPU boxes
    hip = torch_ref = quantize = None


def _random_problem(n=200_000, f=28, max_bin=256, missing=False, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, f)).astype(np.float32)
    if missing:
        X[rng.random(size=X.shape) < 0.05] = np.nan
    Xg = torch.tensor(X, device="cuda")
    qm = quantize(Xg, max_bin=max_bin)
    gh = torch.stack(
        [
            torch.tensor(rng.normal(size=n).astype(np.float32), device="cuda"),
            torch.tensor(rng.random(size=n).astype(np.float32) + 0.01, device="cuda"),
        ],
        dim=1,
    )
    return qm, gh


@pytest.fixture(scope="module")
def problem():
    return _random_problem()


class TestHistogram:
    def test_matches_reference(self, problem):
        qm, gh = problem
        n = qm.num_row
        rowbuf = torch.arange(n, dtype=torch.int32, device="cuda")
        jobs = [(0, n // 2), (n // 2, n)]
        scale = hip.compute_scale(gh)
        acc = hip.build_histograms(qm, gh, rowbuf, jobs, scale)
        hist_hip = hip.hist_to_float(acc, scale)
        hist_ref = torch_ref.hist_to_float(torch_ref.build_histograms(qm, gh, rowbuf, jobs, None))
        torch.cuda.synchronize()
        ref = hist_ref.cpu().numpy()
        got = hist_hip.cpu().numpy()
        denom = np.abs(ref).max()
        np.testing.assert_allclose(got, ref, atol=denom * 1e-5)

    def test_deterministic(self, problem):
        qm, gh = problem
        n = qm.num_row
        rowbuf = torch.arange(n, dtype=torch.int32, device="cuda")
        scale = hip.compute_scale(gh)
        a1 = hip.build_histograms(qm, gh, rowbuf, [(0, n)], scale)
        a2 = hip.build_histograms(qm, gh, rowbuf, [(0, n)], scale)
        torch.cuda.synchronize()
        assert torch.equal(a1, a2), "fixed-point histogram must be bit-deterministic"

    def test_missing_bins(self):
        qm, gh = _random_problem(n=50_000, f=10, missing=True, seed=1)
        assert qm.has_missing
        n = qm.num_row
        rowbuf = torch.arange(n, dtype=torch.int32, device="cuda")
        scale = hip.compute_scale(gh)
        hist_hip = hip.hist_to_float(hip.build_histograms(qm, gh, rowbuf, [(0, n)], scale), scale)
        hist_ref = torch_ref.hist_to_float(torch_ref.build_histograms(qm, gh, rowbuf, [(0, n)], None))
        ref = hist_ref.cpu().numpy()
        np.testing.assert_allclose(hist_hip.cpu().numpy(), ref, atol=np.abs(ref).max() * 1e-5)

    def test_int16_bins(self):
        # >256 slots forces the int16 bin path (max_bin 256 + missing)
        qm, gh = _random_problem(n=50_000, f=8, max_bin=256, missing=True, seed=2)
        if qm.bins.dtype == torch.uint8:
            pytest.skip("stride fits uint8")
        n = qm.num_row
        rowbuf = torch.arange(n, dtype=torch.int32, device="cuda")
        scale = hip.compute_scale(gh)
        hist_hip = hip.hist_to_float(hip.build_histograms(qm, gh, rowbuf, [(0, n)], scale), scale)
        hist_ref = torch_ref.hist_to_float(torch_ref.build_histograms(qm, gh, rowbuf, [(0, n)], None))
        ref = hist_ref.cpu().numpy()
        np.testing.assert_allclose(hist_hip.cpu().numpy(), ref, atol=np.abs(ref).max() * 1e-5)


class TestFindSplits:
    def test_matches_reference(self, problem):
        qm, gh = problem
        n = qm.num_row
        rowbuf = torch.arange(n, dtype=torch.int32, device="cuda")
        jobs = [(0, n // 3), (n // 3, n)]
        scale = hip.compute_scale(gh)
        hist = hip.hist_to_float(hip.build_histograms(qm, gh, rowbuf, jobs, scale), scale)
        parent = torch.stack([hist.reshape(2, qm.num_col, qm.stride, 2)[i].sum(dim=(0, 1)) for i in range(2)])
        s_hip = hip.find_splits(hist, parent, qm, reg_lambda=1.0, min_child_weight=1.0)
        s_ref = torch_ref.find_splits(hist, parent, qm, reg_lambda=1.0, min_child_weight=1.0)
        a = s_hip["packed"].cpu().numpy()
        b = s_ref["packed"].cpu().numpy()
        # same feature/bin/dir chosen; gains equal to fp32 tolerance
        np.testing.assert_array_equal(a[:, 1:4], b[:, 1:4])
        np.testing.assert_allclose(a[:, 0], b[:, 0], rtol=2e-4, atol=1e-5)
        np.testing.assert_allclose(a[:, 4:], b[:, 4:], rtol=2e-4, atol=1e-4)

    def test_missing_and_masks(self):
        qm, gh = _random_problem(n=60_000, f=12, missing=True, seed=7)
        n = qm.num_row
        rowbuf = torch.arange(n, dtype=torch.int32, device="cuda")
        scale = hip.compute_scale(gh)
        hist = hip.hist_to_float(hip.build_histograms(qm, gh, rowbuf, [(0, n)], scale), scale)
        parent = hist.reshape(1, qm.num_col, qm.stride, 2).sum(dim=(1, 2))
        mask = torch.zeros(12, dtype=torch.bool, device="cuda")
        mask[3] = mask[7] = True
        mono = torch.zeros(12, dtype=torch.int8, device="cuda")
        mono[3] = 1
        s_hip = hip.find_splits(hist, parent, qm, feature_mask=mask, monotone=mono)
        s_ref = torch_ref.find_splits(hist, parent, qm, feature_mask=mask, monotone=mono)
        a = s_hip["packed"].cpu().numpy()
        b = s_ref["packed"].cpu().numpy()
        np.testing.assert_array_equal(a[:, 1:4], b[:, 1:4])
        np.testing.assert_allclose(a[:, 0], b[:, 0], rtol=2e-4, atol=1e-5)


class TestPartition:
    def test_matches_reference_sets(self, problem):
        qm, _gh = problem
        n = qm.num_row
        src = torch.arange(n, dtype=torch.int32, device="cuda")
        dst = torch.empty_like(src)
        segs = [(0, n // 3), (n // 3, n)]
        feats = [0, 5]
        sbins = [100, 37]
        dls = [False, True]
        counts = hip.partition_level(qm, src, dst, segs, feats, sbins, dls)

        src_ref = src.clone()
        dst_ref = torch.empty_like(src_ref)
        counts_ref = torch_ref.partition_level(qm, src_ref, dst_ref, segs, feats, sbins, dls)
        assert counts == counts_ref
        for (start, end), lc in zip(segs, counts):
            left_hip = set(dst[start : start + lc].cpu().tolist())
            left_ref = set(dst_ref[start : start + lc].cpu().tolist())
            assert left_hip == left_ref
            right_hip = set(dst[start + lc : end].cpu().tolist())
            right_ref = set(dst_ref[start + lc : end].cpu().tolist())
            assert right_hip == right_ref


class TestLeafUpdate:
    def test_scatter(self):
        n = 10_000
        margin = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
        # contract: the row sets of leaf jobs are disjoint (each training row
        # lives in exactly one leaf), so the scatter is race-free by design
        buf0 = torch.randperm(n, device="cuda").to(torch.int32)
        buf1 = buf0.clone()
        jobs = [(0, 0, n // 2, 0.5), (1, n // 2, n, -0.25)]
        hip.update_margins(margin[:, 1], (buf0, buf1), jobs)
        ref = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
        torch_ref.update_margins(ref[:, 1], (buf0, buf1), jobs)
        torch.cuda.synchronize()
        assert torch.allclose(margin, ref)
        assert margin[:, 0].abs().sum() == 0


class TestPredict:
    def test_forest_matches_reference(self):
        from sagemaker_xgboost_container_amd.data.dmatrix import DMatrix
        from sagemaker_xgboost_container_amd.models import trainer

        rng = np.random.default_rng(3)
        X = rng.normal(size=(5000, 12)).astype(np.float32)
        X[rng.random(size=X.shape) < 0.03] = np.nan
        y = (np.nan_to_num(X[:, 0]) > 0).astype(np.float32)
        bst = trainer.train(
            {"objective": "binary:logistic", "max_depth": 5, "device": "cpu"},
            DMatrix(X, label=y),
            num_boost_round=5,
            verbose_eval=False,
        )
        Xg = torch.tensor(X, device="cuda")
        out_hip = hip.predict_forest(bst.trees, bst.tree_info, Xg, 1)
        ref = torch.zeros((X.shape[0], 1), device="cuda")
        for t in bst.trees:
            ref[:, 0] += torch_ref.predict_tree(t, Xg)
        torch.cuda.synchronize()
        np.testing.assert_allclose(out_hip.cpu().numpy(), ref.cpu().numpy(), rtol=1e-5, atol=1e-6)


class TestEndToEnd:
    def test_gpu_training_learns(self):
        from sagemaker_xgboost_container_amd.data.dmatrix import DMatrix
        from sagemaker_xgboost_container_amd.models import trainer

        rng = np.random.default_rng(4)
        X = rng.normal(size=(100_000, 28)).astype(np.float32)
        logit = X[:, 0] * 2 - X[:, 1] + 0.5 * X[:, 2] * X[:, 3]
        y = (logit + rng.normal(scale=0.5, size=len(X)) > 0).astype(np.float32)
        res = {}
        bst = trainer.train(
            {"objective": "binary:logistic", "max_depth": 6, "eta": 0.3, "tree_method": "gpu_hist"},
            DMatrix(X, label=y),
            num_boost_round=10,
            evals=[(DMatrix(X, label=y), "train")],
            evals_result=res,
            verbose_eval=False,
        )
        assert res["train"]["logloss"][-1] < 0.35
        pred = bst.predict(X[:1000])
        assert ((pred > 0.5) == y[:1000]).mean() > 0.85

    def test_gpu_matches_cpu_model(self):
        """Same small dataset: GPU-grown model close to CPU-grown model."""
        from sagemaker_xgboost_container_amd.data.dmatrix import DMatrix
        from sagemaker_xgboost_container_amd.models import trainer

        rng = np.random.default_rng(5)
        X = rng.normal(size=(20_000, 10)).astype(np.float32)
        y = (X[:, 0] + 0.5 * X[:, 1] > 0).astype(np.float32)
        params = {"objective": "binary:logistic", "max_depth": 4, "eta": 0.5}
        cpu = trainer.train({**params, "device": "cpu"}, DMatrix(X, label=y), 5, verbose_eval=False)
        gpu = trainer.train({**params, "device": "cuda"}, DMatrix(X, label=y), 5, verbose_eval=False)
        p_cpu = cpu.predict(X[:2000])
        p_gpu = gpu.predict(X[:2000])
        # identical cuts + deterministic hist => same trees up to fp noise
        assert np.mean(np.abs(p_cpu - p_gpu)) < 5e-3

    def test_multiclass_gpu(self):
        from sagemaker_xgboost_container_amd.data.dmatrix import DMatrix
        from sagemaker_xgboost_container_amd.models import trainer

        rng = np.random.default_rng(6)
        X = rng.normal(size=(50_000, 54)).astype(np.float32)
        y = ((X[:, 0] > 0.5).astype(int) + (X[:, 1] > 0).astype(int) * 3).astype(np.float32)
        y = np.clip(y, 0, 6)
        res = {}
        trainer.train(
            {"objective": "multi:softprob", "num_class": 7, "max_depth": 6, "tree_method": "gpu_hist"},
            DMatrix(X, label=y),
            num_boost_round=3,
            evals=[(DMatrix(X, label=y), "train")],
            evals_result=res,
            verbose_eval=False,
        )
        assert res["train"]["mlogloss"][-1] < res["train"]["mlogloss"][0]


class TestDeviceGrower:
    def test_matches_per_level_path(self, monkeypatch):
        """The zero-sync device-autonomous grower must produce the same
        ensemble as the per-level path (same kernels, same order)."""
        import json as _json

        from sagemaker_xgboost_container_amd.data.dmatrix import DMatrix
        from sagemaker_xgboost_container_amd.models import trainer

        rng = np.random.default_rng(11)
        X = rng.normal(size=(300_000, 28)).astype(np.float32)
        y = (X[:, 0] * 2 - X[:, 1] + 0.5 * X[:, 2] * X[:, 3] > 0).astype(np.float32)
        params = {"objective": "binary:logistic", "max_depth": 6, "eta": 0.3, "device": "cuda"}

        monkeypatch.setenv("SMXGB_NO_DEVICE_GROW", "1")
        ref = trainer.train(dict(params), DMatrix(X, label=y), 4, verbose_eval=False)
        monkeypatch.delenv("SMXGB_NO_DEVICE_GROW")
        dev = trainer.train(dict(params), DMatrix(X, label=y), 4, verbose_eval=False)

        def sig(b):
            return _json.dumps(
                [
                    {
                        "f": t.feature.tolist(),
                        "b": t.split_bin.tolist(),
                        "l": t.left.tolist(),
                    }
                    for t in b.trees
                ]
            )

        assert sig(ref) == sig(dev), "device grower diverged from per-level path"
        p_ref = ref.predict(X[:2000])
        p_dev = dev.predict(X[:2000])
        np.testing.assert_allclose(p_ref, p_dev, rtol=1e-4, atol=1e-5)

    def test_with_missing_and_subsample(self):
        from sagemaker_xgboost_container_amd.data.dmatrix import DMatrix
        from sagemaker_xgboost_container_amd.models import trainer

        rng = np.random.default_rng(12)
        X = rng.normal(size=(100_000, 12)).astype(np.float32)
        X[rng.random(size=X.shape) < 0.05] = np.nan
        y = (np.nan_to_num(X[:, 0]) > 0).astype(np.float32)
        res = {}
        trainer.train(
            {"objective": "binary:logistic", "max_depth": 5, "subsample": 0.8,
             "colsample_bytree": 0.8, "seed": 3, "device": "cuda"},
            DMatrix(X, label=y),
            6,
            evals=[(DMatrix(X, label=y), "train")],
            evals_result=res,
            verbose_eval=False,
        )
        assert res["train"]["logloss"][-1] < res["train"]["logloss"][0]


class TestFusedGradients:
    """grad_fused_kernel vs the torch objective formulas (same fp32 math)."""

    @pytest.mark.parametrize("name,spw,weighted", [
        ("binary:logistic", 1.0, False),
        ("binary:logistic", 3.5, True),
        ("reg:squarederror", 1.0, True),
        ("reg:logistic", 1.0, False),
    ])
    def test_matches_torch(self, name, spw, weighted):
        from sagemaker_xgboost_container_amd.models import objectives
        from sagemaker_xgboost_container_amd.ops import hip as hip_ops

        torch.manual_seed(3)
        n = 1_000_003
        margin = torch.randn(n, device="cuda") * 3
        y = (torch.rand(n, device="cuda") > 0.5).float() if "logistic" in name \
            else torch.randn(n, device="cuda")
        w = torch.rand(n, device="cuda") + 0.5 if weighted else None

        obj = objectives.create_objective(name, {"scale_pos_weight": spw})
        gh_fused = hip_ops.fused_gradients(name, margin, y, w, getattr(obj, "scale_pos_weight", spw))
        assert gh_fused is not None

        # torch reference path (force it by computing on CPU copies)
        obj_cpu = objectives.create_objective(name, {"scale_pos_weight": spw})
        gh_ref = obj_cpu.gradients(margin.cpu(), y.cpu(), w.cpu() if w is not None else None)

        torch.testing.assert_close(gh_fused.cpu(), gh_ref, rtol=2e-5, atol=2e-6)
        # attached absmax must equal the true column maxima
        expect = gh_ref.abs().amax(dim=0)
        torch.testing.assert_close(gh_fused._smxgb_absmax.cpu(), expect, rtol=2e-5, atol=2e-6)
        # attached root (G, H) must equal the f64 sum of the gh the kernel
        # itself produced (torch's sigmoid differs from expf by ~1e-8 per
        # element, which accumulates to ~1e-2 over 1M rows — comparing sums
        # across the two gradient implementations would test nothing useful)
        expect_sum = gh_fused.to(torch.float64).sum(0)
        torch.testing.assert_close(gh_fused._smxgb_rootsum, expect_sum, rtol=1e-10, atol=1e-8)

    def test_unsupported_objective_falls_back(self):
        from sagemaker_xgboost_container_amd.ops import hip as hip_ops

        m = torch.randn(100, device="cuda")
        assert hip_ops.fused_gradients("binary:hinge", m, m) is None

    # saturation edges of the fp32 sigmoid: expf overflow (|m| >= 89), p
    # rounding to 1 (m >= 17) or to a denormal-sized value, the hessian floor
    _EDGE_MARGINS = [0.0, 1e-8, -1e-8, 16.0, -16.0, 17.0, -17.0, 30.0, -30.0, 87.0, -87.0,
                     89.0, -89.0, 104.0, -104.0, 1e4, -1e4, float("inf"), float("-inf")]
    # 2048 * 256 + 1: the first length past one grid-stride pass of the grid
    _EDGE_LENGTHS = [1, 255, 256, 257, 2048 * 256 + 1]

    @classmethod
    def _edge_inputs(cls, name, n, weighted, seed):
        """Every other element cycles through the edge margins (starting at a
        seed-dependent one, so n = 1 meets several), the rest is N(0, 3)."""
        rng = np.random.default_rng(seed)
        margin = (rng.normal(size=n) * 3).astype(np.float32)
        edges = np.asarray(cls._EDGE_MARGINS, dtype=np.float32)
        at = np.arange(0, n, 2)
        margin[at] = edges[(at // 2 + seed) % edges.size]
        if name == "reg:squarederror":
            y = rng.normal(size=n).astype(np.float32)
        elif name == "reg:logistic":
            y = rng.choice(np.asarray([0.0, 0.25, 0.5, 1.0], dtype=np.float32), size=n)
        else:
            y = rng.integers(0, 2, size=n).astype(np.float32)
        w = (rng.random(size=n) + 0.5).astype(np.float32) if weighted else None
        return margin, y, w

    @staticmethod
    def _oracle(name, margin, y, w, spw):
        """The kernel's contract in float64 numpy on the float32 inputs."""
        m = margin.astype(np.float64)
        y64 = y.astype(np.float64)
        if name == "reg:squarederror":
            g, h = m - y64, np.ones_like(m)
        else:
            with np.errstate(over="ignore"):
                p = 1.0 / (1.0 + np.exp(-m))
            g = p - y64
            h = np.maximum(p * (1.0 - p), 1e-16)
            pos = y == np.float32(1.0)  # scale_pos_weight: exact positives only
            g[pos] *= spw
            h[pos] *= spw
        if w is not None:
            g, h = g * w.astype(np.float64), h * w.astype(np.float64)
        return np.stack([g, h], axis=1)

    @pytest.mark.parametrize("n", _EDGE_LENGTHS)
    @pytest.mark.parametrize("spw,weighted", [(1.0, False), (3.5, True)])
    @pytest.mark.parametrize(
        "name", ["binary:logistic", "reg:logistic", "binary:logitraw", "reg:squarederror"]
    )
    def test_edges_match_float64_oracle(self, name, spw, weighted, n):
        from sagemaker_xgboost_container_amd.ops import hip as hip_ops

        seed = 17 * n + int(weighted)
        margin, y, w = self._edge_inputs(name, n, weighted, seed % 1000)
        dev = lambda a: None if a is None else torch.from_numpy(a).cuda()  # noqa: E731
        gh = hip_ops.fused_gradients(name, dev(margin), dev(y), dev(w), spw)
        assert gh is not None and gh.shape == (n, 2) and gh.dtype == torch.float32
        torch.cuda.synchronize()
        got = gh.cpu().numpy()
        want = self._oracle(name, margin, y, w, spw)
        w32 = np.ones(n, dtype=np.float32) if w is None else w

        if name == "reg:squarederror":
            # one fp32 subtraction and one multiply: bit-equal to numpy. An
            # infinite margin has an infinite gradient; everything else is finite
            g32 = margin - y
            ref = np.stack([g32 * w32 if weighted else g32, w32], axis=1)
            assert np.array_equal(got, ref)
            assert np.isfinite(got[np.isfinite(margin)]).all()
            finite = np.isfinite(margin)
            err = np.abs(got[finite].astype(np.float64) - want[finite])
            print(f"{name} weighted={weighted} n={n}: max |err| vs float64 {err.max(initial=0):.3e}")
        else:
            assert np.isfinite(got).all()
            scale = (w32.astype(np.float64) * max(1.0, spw))[:, None]
            err = np.abs(got.astype(np.float64) - want)
            excess = err - (2e-6 * scale + 2e-5 * np.abs(want))
            worst = int(np.argmax(excess.max(axis=1)))
            print(f"{name} spw={spw} weighted={weighted} n={n}: max |err| g {err[:, 0].max():.3e} "
                  f"h {err[:, 1].max():.3e}; worst row m={margin[worst]!r} y={y[worst]!r}")
            assert (excess <= 0).all(), (
                f"m={margin[worst]!r} y={y[worst]!r} w={w32[worst]!r}: got {got[worst]}, "
                f"oracle {want[worst]}"
            )
            # the hessian floor survives scale_pos_weight and the weight
            factor = np.where(y == np.float32(1.0), np.float32(spw), np.float32(1.0))
            floor = np.float32(1e-16) * factor.astype(np.float32)
            floor = floor * w32 if weighted else floor
            assert (got[:, 1] >= floor).all()
            if spw == 1.0 and not weighted:
                # fp32 saturation: 1 + exp(-17) rounds to 1, exp(89) overflows
                p = got[:, 0] + y
                exact = (y == 0) | (y == 1)
                assert (p[(margin >= 17) & exact] == 1.0).all()
                assert (p[(margin <= -89) & exact] == 0.0).all()
                assert (got[margin <= -89, 1] == np.float32(1e-16)).all()
                assert (got[margin >= 1e4, 1] == np.float32(1e-16)).all()

        # the attached maxima and sums are those of the kernel's own output
        assert torch.equal(gh._smxgb_absmax, gh.abs().amax(dim=0))
        torch.testing.assert_close(
            gh._smxgb_rootsum, gh.to(torch.float64).sum(0), rtol=1e-10, atol=1e-8, equal_nan=True
        )
        if name != "reg:squarederror":
            assert bool(torch.isfinite(gh._smxgb_rootsum).all())

    def test_fractional_labels_get_no_scale_pos_weight(self):
        from sagemaker_xgboost_container_amd.ops import hip as hip_ops

        margin = torch.tensor([0.5, 0.5, 0.5, -2.0], device="cuda")
        y = torch.tensor([1.0, 0.5, 0.25, 0.99999994], device="cuda")
        plain = hip_ops.fused_gradients("reg:logistic", margin, y, None, 1.0).cpu()
        scaled = hip_ops.fused_gradients("reg:logistic", margin, y, None, 3.5).cpu()
        assert torch.equal(scaled[0], plain[0] * 3.5)
        assert torch.equal(scaled[1:], plain[1:])

    def test_launcher_refuses_malformed_arguments(self):
        """Every refusal is a ValueError on the host: a short y or w never
        reaches the kernel."""
        from sagemaker_xgboost_container_amd.ops import hip as hip_ops

        n, grid = 1000, hip_ops._GRAD_GRID
        f32 = dict(dtype=torch.float32, device="cuda")
        good = {
            "margin": torch.zeros(n, **f32), "y": torch.zeros(n, **f32),
            "w": torch.ones(n, **f32), "gh": torch.full((n, 2), -7.0, **f32),
            "pmax": torch.zeros((grid, 2), **f32),
            "psum": torch.zeros((grid, 2), dtype=torch.float64, device="cuda"),
        }

        def launch(mode=0, **swap):
            a = dict(good, **swap)
            hip_ops._K.grad_fused(a["margin"], a["y"], a["w"], a["gh"], a["pmax"], a["psum"],
                                  mode, 1.0)

        bad = {
            "short y": dict(y=good["y"][:-1].contiguous()),
            "long y": dict(y=torch.zeros(n + 1, **f32)),
            "short w": dict(w=good["w"][:-1].contiguous()),
            "gh of another size": dict(gh=torch.zeros((n - 1, 2), **f32)),
            "pmax of another shape": dict(pmax=torch.zeros((grid, 1), **f32)),
            "psum of another size": dict(psum=torch.zeros((grid - 1, 2), dtype=torch.float64,
                                                          device="cuda")),
            "float32 psum": dict(psum=torch.zeros((grid, 2), **f32)),
            "float64 margin": dict(margin=good["margin"].double()),
            "float64 y": dict(y=good["y"].double()),
            "float64 w": dict(w=good["w"].double()),
            "host y": dict(y=good["y"].cpu()),
            "host margin": dict(margin=good["margin"].cpu()),
            "strided margin": dict(margin=torch.zeros(2 * n, **f32)[::2]),
            "strided y": dict(y=torch.zeros(2 * n, **f32)[::2]),
        }
        for what, swap in bad.items():
            with pytest.raises(ValueError):
                launch(**swap)
                pytest.fail(f"{what} was accepted")
        for mode in (-1, 2):
            with pytest.raises(ValueError, match="mode"):
                launch(mode=mode)
        with pytest.raises(ValueError):
            hip_ops.fused_gradients("binary:logistic", good["margin"], good["y"][:10])
        with pytest.raises(ValueError):
            hip_ops.fused_gradients("binary:logistic", good["margin"], good["y"], good["w"][:10])
        torch.cuda.synchronize()
        assert bool((good["gh"] == -7.0).all())  # nothing was launched
        launch()  # the same arguments, unbroken, run
        launch(w=torch.empty(0, **f32))
        torch.cuda.synchronize()
        assert bool((good["gh"][:, 0] == 0.5).all())


class TestMulticlassPipeline:
    """Pipelined multiclass (per-class slots, one drain) must produce the
    same model as the per-level sequential path."""

    def test_parity_with_per_level(self, monkeypatch):
        from sagemaker_xgboost_container_amd.data.dmatrix import DMatrix
        from sagemaker_xgboost_container_amd.models import trainer

        rng = np.random.default_rng(5)
        X = rng.normal(size=(60_000, 10)).astype(np.float32)
        y = (np.abs(X[:, 0]) + X[:, 1] > 1).astype(np.float32) + (X[:, 2] > 1) * 1.0
        params = {"objective": "multi:softprob", "num_class": 3, "max_depth": 5,
                  "eta": 0.4, "device": "cuda"}

        bst_pipe = trainer.train(params, DMatrix(X, label=y), num_boost_round=4,
                                 verbose_eval=False)
        monkeypatch.setenv("SMXGB_NO_DEVICE_GROW", "1")
        bst_seq = trainer.train(params, DMatrix(X, label=y), num_boost_round=4,
                                verbose_eval=False)
        monkeypatch.delenv("SMXGB_NO_DEVICE_GROW")

        p1 = bst_pipe.predict(X[:5000])
        p2 = bst_seq.predict(X[:5000])
        np.testing.assert_allclose(p1, p2, rtol=1e-5, atol=1e-6)


class TestDeterministicHistogramFlag:
    """The flag is accepted (xgboost parity) and training stays
    deterministic either way — the measured float-atomic "fast" path was 3x
    slower than the int64 slab, so both values run the same kernels."""

    def test_flag_accepted_and_identical(self):
        from sagemaker_xgboost_container_amd.data.dmatrix import DMatrix
        from sagemaker_xgboost_container_amd.models import trainer

        rng = np.random.default_rng(9)
        X = rng.normal(size=(100_000, 12)).astype(np.float32)
        y = (X[:, 0] + 0.5 * X[:, 3] > 0).astype(np.float32)
        base = {"objective": "binary:logistic", "max_depth": 5, "eta": 0.3, "device": "cuda"}

        b1 = trainer.train(dict(base, deterministic_histogram="true"), DMatrix(X, label=y),
                           num_boost_round=4, verbose_eval=False)
        b2 = trainer.train(dict(base, deterministic_histogram="false"), DMatrix(X, label=y),
                           num_boost_round=4, verbose_eval=False)
        np.testing.assert_array_equal(b1.predict(X[:2000]), b2.predict(X[:2000]))
