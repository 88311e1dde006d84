"""Booster: the trained GBT model — prediction + xgboost-format persistence.

Serialization writes the XGBoost Booster JSON schema (learner /
gradient_booster / trees with split_indices, split_conditions,
left_children, ...) so models interoperate with the reference container's
checkpoint/model file protocol (reference train.py:475-486,
serve_utils.py:171-197, checkpointing.py:372-378). Files saved by upstream
xgboost in JSON form load here; files saved here load in upstream xgboost.
Pickled boosters (the serving pickle-first path, serve_utils.py:180-182)
are supported via plain-numpy state.
"""
import json
import logging
import os

import numpy as np
import torch

from .. import ops
from .objectives import create_objective, parse_quantile_alpha
from .tree import CAT_WORDS, Tree, cat_bits_from_members, cat_members

MODEL_VERSION = [3, 0, 5]  # schema-compatible xgboost version

# predict() keeps a sparse DMatrix sparse once its dense float32 image would
# exceed this many bytes: the per-launch staging budget the device explainers
# already use (ops/hip.py SHAP_PARTIAL_CAP). The host route densifies at most
# this much at a time.
SPARSE_PREDICT_DENSE_BUDGET = 256 << 20

logger = logging.getLogger(__name__)
_EXPLAIN_ROUTES_LOGGED = set()


def objective_params_from_json(obj_json, params):
    """Restore hyperparameters from a model/config objective block into
    `params` (the inverse of Booster._objective_json). Shared by
    load_json, save_config round-trips and the legacy-binary loader."""
    blocks = {
        "reg_loss_param": (("scale_pos_weight", float),),
        "softmax_multiclass_param": (("num_class", int),),
        "poisson_regression_param": (("max_delta_step", float),),
        "tweedie_regression_param": (("tweedie_variance_power", float),),
        "pseudo_huber_param": (("huber_slope", float),),
        # a JSON-array string ("[0.1, 0.9]"); a bare number is accepted too
        "quantile_loss_param": (("quantile_alpha", parse_quantile_alpha),),
        "aft_loss_param": (
            ("aft_loss_distribution", str),
            ("aft_loss_distribution_scale", float),
        ),
        "lambdarank_param": (
            ("lambdarank_num_pair_per_sample", int),
            ("lambdarank_pair_method", str),
            ("lambdarank_unbiased", int),
        ),
    }
    for block_name, fields in blocks.items():
        block = obj_json.get(block_name)
        if not isinstance(block, dict):
            continue
        for field, conv in fields:
            if field in block:
                try:
                    params[field] = conv(block[field])
                except (TypeError, ValueError):
                    pass
    return params


class Booster:
    def __init__(self, params=None, num_features=0, feature_names=None,
                 cache=None, model_file=None):
        self.params = dict(params or {})
        self.trees = []           # flat list of Tree
        self.tree_info = []       # class id of each tree (0 for single-output)
        self.weight_drop = []     # per-tree scale (dart; 1.0 for gbtree)
        self.linear_model = None  # gblinear state (models.gblinear.LinearModel)
        self.iteration_indptr = [0]
        self.num_features = num_features
        self.feature_names = feature_names
        self.feature_types = None
        self.attributes_map = {}
        self.best_iteration = None
        self.best_score = None
        self._objective = None
        self._predict_cache = None
        if model_file is not None:  # xgb.Booster(model_file=...) parity
            self.load_model(model_file)

    # -- basic accessors ---------------------------------------------------
    @property
    def booster_type(self):
        return self.params.get("booster", "gbtree")

    @property
    def objective_name(self):
        return self.params.get("objective", "reg:squarederror")

    @property
    def num_class(self):
        return int(self.params.get("num_class", 0) or 0)

    @property
    def n_outputs(self):
        if self.objective_name == "reg:quantileerror":
            # one output (and one tree per round) per quantile_alpha
            return len(parse_quantile_alpha(self.params.get("quantile_alpha", 0.5)))
        return max(1, self.num_class)

    @property
    def base_score(self):
        bs = self.params.get("base_score")
        return float(bs) if bs is not None else 0.5

    def objective(self):
        if self._objective is None:
            self._objective = create_objective(self.objective_name, self.params)
        return self._objective

    def set_param(self, key, value=None):
        if isinstance(key, dict):
            self.params.update(key)
        else:
            self.params[key] = value
        self._objective = None

    def num_boosted_rounds(self):
        return len(self.iteration_indptr) - 1

    def attributes(self):
        return dict(self.attributes_map)

    def attr(self, name):
        return self.attributes_map.get(name)

    def set_attr(self, **kwargs):
        for k, v in kwargs.items():
            if v is None:
                self.attributes_map.pop(k, None)
            else:
                self.attributes_map[k] = str(v)

    # -- boosting ----------------------------------------------------------
    def add_iteration(self, trees, tree_info, weight_drop=None):
        """Append one boosting round's trees (n_outputs × num_parallel_tree)."""
        self.trees.extend(trees)
        self.tree_info.extend(tree_info)
        self.weight_drop.extend(weight_drop if weight_drop is not None else [1.0] * len(trees))
        self.iteration_indptr.append(len(self.trees))
        self._predict_cache = None

    # -- prediction ----------------------------------------------------------
    def _start_margin(self, n, device, base_margin):
        """(n, k) float32 starting margin: the per-row base_margin when
        given, else the objective's transform of base_score."""
        k = self.n_outputs
        if base_margin is not None:
            return torch.as_tensor(
                base_margin, dtype=torch.float32, device=device
            ).reshape(n, k).clone()
        base = self.objective().base_margin(self.base_score)
        return torch.full((n, k), float(base), dtype=torch.float32, device=device)

    def _margin(self, X, iteration_range=None, base_margin=None):
        """Raw margin (n,) or (n, k) for dense float32 tensor X.

        `base_margin` (per-row, from the DMatrix) replaces the global
        base_score as the starting margin — xgboost semantics."""
        n = X.shape[0]
        k = self.n_outputs
        device = X.device
        margin = self._start_margin(n, device, base_margin)
        lo, hi = 0, self.num_boosted_rounds()
        if iteration_range is not None and iteration_range != (0, 0):
            lo, hi = iteration_range
            hi = min(hi, self.num_boosted_rounds()) if hi else self.num_boosted_rounds()
        if self.booster_type == "gblinear" and self.linear_model is not None:
            margin += torch.nan_to_num(X, nan=0.0) @ self.linear_model.weights.to(device) \
                + self.linear_model.bias.to(device)
            return margin.squeeze(1) if k == 1 else margin
        if self.trees:
            backend = ops.backend_for(device)
            # cached flat forest: ONE traversal kernel for all trees
            key = str(device)
            cache = self._predict_cache or {}
            if key not in cache:
                wd = self.weight_drop if any(w != 1.0 for w in self.weight_drop) else None
                cache[key] = backend.make_flat_forest(self.trees, self.tree_info, wd, device)
                self._predict_cache = cache
            t_begin = self.iteration_indptr[lo]
            t_end = self.iteration_indptr[hi]
            margin += backend.predict_forest_flat(cache[key], X, k, t_begin, t_end)
        return margin.squeeze(1) if k == 1 else margin

    def predict(
        self,
        data,
        output_margin=False,
        iteration_range=None,
        validate_features=True,
        pred_contribs=False,
        pred_leaf=False,
        approx_contribs=False,
        training=False,
        ntree_limit=None,
        pred_interactions=False,
    ):
        """Predict for a DMatrix / ndarray. Returns numpy array.

        `pred_contribs` / `pred_interactions` / `pred_leaf` are mutually
        exclusive; all three honour `iteration_range` / `ntree_limit`."""
        if int(bool(pred_contribs)) + int(bool(pred_interactions)) + int(bool(pred_leaf)) > 1:
            raise ValueError(
                "only one of pred_contribs, pred_interactions and pred_leaf may be requested"
            )
        if ntree_limit:  # legacy alias: trees -> iterations
            iteration_range = (0, int(ntree_limit) // max(1, self._trees_per_round()))
        if (pred_contribs or pred_interactions) and self.has_categorical_splits():
            raise NotImplementedError(
                "pred_contribs, approx_contribs and pred_interactions are not implemented for "
                "models with categorical splits"
            )
        if pred_contribs and self._sparse_explain_route(
            data, approx_contribs=approx_contribs, iteration_range=iteration_range
        ):
            if validate_features:
                self._validate_features(data)
            return self._pred_contribs_sparse(data, iteration_range)
        if self._sparse_predict_route(data, explain=pred_contribs or pred_interactions):
            if validate_features:
                self._validate_features(data)
            return self._predict_sparse(data, output_margin, iteration_range, pred_leaf)
        X = self._as_tensor(data, validate_features)
        base_margin = getattr(data, "get_base_margin", lambda: None)()
        if pred_contribs:
            return self._pred_contribs(
                X, approx=approx_contribs, iteration_range=iteration_range,
                base_margin=base_margin,
            )
        if pred_interactions:
            return self._pred_interactions(
                X, iteration_range=iteration_range, base_margin=base_margin
            )
        if pred_leaf:
            return self._pred_leaf(X, iteration_range=iteration_range)
        margin = self._margin(X, iteration_range, base_margin=base_margin)
        if output_margin:
            return margin.cpu().numpy()
        out = self.objective().transform(margin)
        return out.cpu().numpy()

    def _trees_per_round(self):
        if self.num_boosted_rounds() == 0:
            return self.n_outputs
        return self.iteration_indptr[1] - self.iteration_indptr[0]

    def _validate_features(self, data):
        """Feature count and names of a DMatrix against the model's (needs
        num_col() and the names only, never the values)."""
        if self.num_features and data.num_col() != self.num_features:
            raise ValueError(
                f"feature_names mismatch: model expects {self.num_features} features, "
                f"got {data.num_col()}"
            )
        if (
            self.feature_names
            and data.feature_names
            and list(data.feature_names) != list(self.feature_names)
        ):
            raise ValueError(
                f"feature_names mismatch: {self.feature_names} vs {data.feature_names}"
            )

    def _predict_device(self):
        """Where predict() runs: the GPU whenever there is one, unless
        predictor=cpu_predictor forces host traversal."""
        use_gpu = torch.cuda.is_available() and self.params.get("predictor") != "cpu_predictor"
        return torch.device("cuda" if use_gpu else "cpu")

    def _sparse_predict_route(self, data, explain=False):
        """Does predict() keep this input sparse?

        Yes for a sparse DMatrix holding a canonical CSR (sorted, no
        duplicate column ids in a row; anything else keeps the densifying
        path, whose last-duplicate-wins rule a search cannot reproduce) on a
        tree booster, unless TreeSHAP output is asked for (n x (f + 1) dense
        anyway). SMXGB_SPARSE_PREDICT=1 forces the route, =0 disables it;
        unset, the rule is memory-driven like training's device rule: wide
        and at most half full (trainer.sparse_auto_engage) AND a dense
        float32 image beyond SPARSE_PREDICT_DENSE_BUDGET. Small payloads
        therefore keep the dense kernel; where the CSR kernel becomes faster
        than densify + dense is not encoded (profiles/r08_sparse_predict.md).
        """
        from ..data.dmatrix import DMatrix

        flag = os.environ.get("SMXGB_SPARSE_PREDICT")
        if flag == "0" or explain:
            return False
        if not isinstance(data, DMatrix) or not data.is_sparse:
            return False
        if self.booster_type not in ("gbtree", "dart"):
            return False
        if self.has_categorical_splits():
            return False  # the CSR kernels know no category sets: densify
        csr = data.csr()
        if flag != "1":
            from .trainer import sparse_auto_engage

            n, f = csr.shape
            if not sparse_auto_engage(n, f, csr.nnz):
                return False
            if n * f * 4 <= SPARSE_PREDICT_DENSE_BUDGET:
                return False
        return bool(csr.has_canonical_format)

    def has_categorical_splits(self):
        """Does any tree hold a categorical (set-valued) node?"""
        cache = self._predict_cache if self._predict_cache is not None else {}
        self._predict_cache = cache
        if "has_cat" not in cache:
            cache["has_cat"] = any(getattr(t, "has_categorical", False) for t in self.trees)
        return cache["has_cat"]

    def _predict_sparse(self, data, output_margin, iteration_range, pred_leaf):
        """predict() for a sparse DMatrix without its n x f image.

        On a ROCm device the CSR arrays are uploaded as they are and the
        forest runs over them (ops/hip_sparse.py predict_forest_csr /
        pred_leaf_csr), equal bit for bit to the dense kernels on the
        NaN-densified rows. Elsewhere rows are densified a budget-bounded
        chunk at a time through the dense path and the chunks concatenated;
        rows are independent, so that equals the full-densify result."""
        from ..data.dmatrix import densify_csr_rows

        csr = data.csr()
        n, f = csr.shape
        k = self.n_outputs
        device = self._predict_device()
        base_margin = data.get_base_margin()
        if base_margin is not None:
            base_margin = np.asarray(base_margin, dtype=np.float32).reshape(n, k)
        t_begin, t_end = self._tree_range(iteration_range)

        if device.type == "cuda" and ops.backend_for(device).NAME == "hip":
            from ..ops import hip_sparse

            dcsr = hip_sparse.DeviceCSR(csr, device)
            flat = self._device_flat_forest(device, with_paths=False) if self.trees else None
            if pred_leaf:
                if flat is None:
                    return np.zeros((n, 0), dtype=np.int32)
                return hip_sparse.pred_leaf_csr(flat, dcsr, t_begin, t_end).cpu().numpy()
            margin = self._start_margin(n, device, base_margin)
            if flat is not None:
                margin += hip_sparse.predict_forest_csr(flat, dcsr, k, t_begin, t_end)
            margin = margin.squeeze(1) if k == 1 else margin
        else:
            step = max(1, SPARSE_PREDICT_DENSE_BUDGET // max(1, f * 4))
            parts = []
            for a in range(0, max(n, 1), step):  # an empty matrix is one empty chunk
                b = min(n, a + step)
                X = torch.as_tensor(densify_csr_rows(csr, a, b), dtype=torch.float32, device=device)
                if pred_leaf:
                    parts.append(self._pred_leaf(X, iteration_range=iteration_range))
                else:
                    bm = base_margin[a:b] if base_margin is not None else None
                    parts.append(self._margin(X, iteration_range, base_margin=bm))
            if pred_leaf:
                return np.concatenate(parts, axis=0)
            margin = torch.cat(parts, dim=0)
        if output_margin:
            return margin.cpu().numpy()
        return self.objective().transform(margin).cpu().numpy()

    def _as_tensor(self, data, validate_features=True):
        from ..data.dmatrix import DMatrix

        if isinstance(data, DMatrix):
            if validate_features:
                self._validate_features(data)
            arr = data.to_dense()
        else:
            arr = np.asarray(data, dtype=np.float32)
            if arr.ndim == 1:
                arr = arr.reshape(1, -1)
            if validate_features and self.num_features and arr.shape[1] != self.num_features:
                raise ValueError(
                    f"feature_names mismatch: model expects {self.num_features} features, "
                    f"got {arr.shape[1]}"
                )
        # with the tree-chunked predict kernel the GPU wins at every batch
        # size (100x500 trees: 0.085 ms GPU vs 0.70 ms CPU —
        # benchmarks/bench_predict_cpu_gpu.py), so GPU is always preferred;
        # predictor=cpu_predictor still forces host traversal
        return torch.as_tensor(arr, dtype=torch.float32, device=self._predict_device())

    def _cpu_flat_forest(self):
        """Flat forest on host for the contrib/leaf paths (cached)."""
        from ..ops import torch_ref

        cache = self._predict_cache or {}
        if "cpu_flat" not in cache:
            wd = self.weight_drop if any(w != 1.0 for w in self.weight_drop) else None
            for t in self.trees:
                t.finalize()
            cache["cpu_flat"] = torch_ref.make_flat_forest(
                self.trees, self.tree_info, wd, torch.device("cpu")
            )
            self._predict_cache = cache
        return cache["cpu_flat"]

    def _tree_range(self, iteration_range):
        """[t_begin, t_end) of `iteration_range`; (0, 0) and None mean all
        rounds, as in _margin."""
        lo, hi = 0, self.num_boosted_rounds()
        if iteration_range is not None and tuple(iteration_range) != (0, 0):
            lo, hi = iteration_range
            hi = min(hi, self.num_boosted_rounds()) if hi else self.num_boosted_rounds()
        return self.iteration_indptr[lo], self.iteration_indptr[hi]

    def _device_flat_forest(self, device, with_paths):
        """hip flat forest on `device`, with the TreeSHAP path tables
        attached when asked for. Forest and tables are cached under their
        own keys, once per device."""
        from ..ops import hip

        cache = self._predict_cache or {}
        self._predict_cache = cache
        wd = self.weight_drop if any(w != 1.0 for w in self.weight_drop) else None
        key = str(device)
        if key not in cache:
            cache[key] = hip.make_flat_forest(self.trees, self.tree_info, wd, device)
        if not with_paths:
            return cache[key]
        pkey = "shap_paths:" + key
        if pkey not in cache:
            cache[pkey] = hip.make_shap_paths(self.trees, self.tree_info, wd, device)
        # compact-kernel plans and slot tables, keyed inside by device, tree
        # range and trees_per_chunk (ops/hip.py)
        slots = cache.setdefault("shap_slots:" + key, {})
        return dict(cache[key], shap_paths=cache[pkey], shap_slot_cache=slots)

    def _explain_on_device(self, X, t_begin, t_end, shap):
        """The hip flat forest when the device kernels serve this request,
        else None (host path). Device when X is on the GPU — so
        predictor=cpu_predictor still forces the host — and, for TreeSHAP,
        the longest path fits a wave and the phi slabs fit LDS. There is no
        small-batch cut-off: the device arm wins at every measured size,
        down to 1k rows (device explanations)."""
        if X.device.type != "cuda" or not self.trees or t_end <= t_begin:
            return None
        hip = ops.backend_for(X.device)
        if hip.NAME != "hip":
            return None
        flat = self._device_flat_forest(X.device, with_paths=shap)
        if shap:
            _, max_f, fits = hip.shap_limits(
                flat["shap_paths"], self.n_outputs, X.shape[1], t_begin, t_end
            )
            if not fits or max_f >= X.shape[1]:
                return None
        return flat

    def _log_explain_route(self, route):
        """Debug-log a contribs route the first time the process takes it."""
        if route not in _EXPLAIN_ROUTES_LOGGED:
            _EXPLAIN_ROUTES_LOGGED.add(route)
            logger.debug("pred_contribs route: %s", route)

    def _compact_explain_flat(self, device, n, f, t_begin, t_end):
        """The hip flat forest when the compact TreeSHAP kernel (chunk-local
        phi slots, ops/hip.py tree_shap_compact) can serve `n` rows of `f`
        columns on `device`, else None: a hip device, a non-empty tree range
        whose splits lie inside the matrix, paths that fit a wave, and slot
        slabs that fit LDS for at least one tree per chunk."""
        if device.type != "cuda" or not self.trees or t_end <= t_begin:
            return None
        hip = ops.backend_for(device)
        if hip.NAME != "hip":
            return None
        flat = self._device_flat_forest(device, with_paths=True)
        L, max_f, _ = hip.shap_limits(flat["shap_paths"], self.n_outputs, f, t_begin, t_end)
        if L > hip.SHAP_MAX_PATH_LEN or max_f >= f:
            return None
        if hip.shap_compact_plan_cached(flat, f, t_begin, t_end, n) is None:
            return None
        return flat

    def _sparse_explain_route(self, data, approx_contribs=False, pred_interactions=False,
                              iteration_range=None):
        """Does predict(pred_contribs=True) keep this input sparse?

        Only exact contributions: approx_contribs and pred_interactions keep
        the densifying path (an interactions result is n * (f + 1)^2, at
        least the dense image). Yes for a sparse DMatrix holding a canonical
        CSR on a tree booster predicting on a hip device, when the compact
        kernel's slot tables fit. SMXGB_SPARSE_EXPLAIN=1 forces the route,
        =0 disables it; unset, the memory rule of _sparse_predict_route
        applies (wide and at most half full, dense float32 image beyond
        SPARSE_PREDICT_DENSE_BUDGET). Independent of SMXGB_SPARSE_PREDICT.
        """
        from ..data.dmatrix import DMatrix

        flag = os.environ.get("SMXGB_SPARSE_EXPLAIN")
        if flag == "0" or approx_contribs or pred_interactions:
            return False
        if not isinstance(data, DMatrix) or not data.is_sparse:
            return False
        if self.booster_type not in ("gbtree", "dart"):
            return False
        device = self._predict_device()
        if device.type != "cuda" or ops.backend_for(device).NAME != "hip":
            return False
        csr = data.csr()
        n, f = csr.shape
        if flag != "1":
            from .trainer import sparse_auto_engage

            if not sparse_auto_engage(n, f, csr.nnz):
                return False
            if n * f * 4 <= SPARSE_PREDICT_DENSE_BUDGET:
                return False
        if not csr.has_canonical_format:
            return False
        t_begin, t_end = self._tree_range(iteration_range)
        return self._compact_explain_flat(device, n, f, t_begin, t_end) is not None

    def _contribs_compact(self, flat, X, n, f, t_begin, t_end, base_margin):
        """pred_contribs through the compact kernel: X is a dense device
        tensor or a DeviceCSR. Each row tile's (rows, U) result is scattered
        into the float32 (n, k, f+1) host array; the device never holds an
        n x (f+1) tensor. Bias column: float32 of expected values + starting
        margin summed in float64, as on the other routes."""
        from ..ops import hip

        k = self.n_outputs
        out = np.zeros((n, k * (f + 1)), dtype=np.float32)
        cols, tiles = hip.tree_shap_compact_tiles(flat, X, k, t_begin, t_end)
        for r0, r1, phi in tiles:
            out[r0:r1, cols] = phi.to(torch.float32).cpu().numpy()
            del phi
        out = out.reshape(n, k, f + 1)
        bias = self._bias_rows(n, base_margin, torch.device("cpu"))
        if t_end > t_begin:
            bias = self._expected_values(t_begin, t_end).to(torch.float64).unsqueeze(0) + bias
        out[:, :, f] = bias.to(torch.float32).numpy()
        return out[:, 0, :] if k == 1 else out

    def _pred_contribs_sparse(self, data, iteration_range):
        """Exact contributions of a sparse DMatrix over its CSR arrays
        (uploaded as they are): equal to the dense kernels on the
        NaN-densified rows, without the n x f image on host or device."""
        from ..ops import hip_sparse

        csr = data.csr()
        n, f = csr.shape
        device = self._predict_device()
        t_begin, t_end = self._tree_range(iteration_range)
        flat = self._device_flat_forest(device, with_paths=True)
        self._log_explain_route("compact kernel over CSR rows")
        dcsr = hip_sparse.DeviceCSR(csr, device)
        return self._contribs_compact(
            flat, dcsr, n, f, t_begin, t_end, data.get_base_margin()
        )

    def _expected_values(self, t_begin, t_end):
        """Per-class TreeSHAP bias of trees [t_begin, t_end) (cached)."""
        from ..ops import torch_ref

        flat = self._cpu_flat_forest()
        cache = self._predict_cache
        key = ("expected_values", t_begin, t_end)
        if key not in cache:
            cache[key] = torch_ref.tree_expected_values(flat, self.n_outputs, t_begin, t_end)
        return cache[key]

    def _bias_rows(self, n, base_margin, device):
        """(n, k) float64 starting margin: the DMatrix base_margin when
        present, else the objective's transform of base_score."""
        k = self.n_outputs
        if base_margin is not None:
            return torch.as_tensor(
                np.asarray(base_margin), dtype=torch.float64, device=device
            ).reshape(n, k)
        base = float(self.objective().base_margin(self.base_score))
        return torch.full((n, k), base, dtype=torch.float64, device=device)

    def _pred_leaf(self, X, iteration_range=None):
        """Leaf indices per (row, tree) — xgboost pred_leaf=True.

        One thread per (row, tree) on the GPU (pred_leaf_kernel) when X is
        there, else ONE parallel C++ traversal over the flat forest."""
        from ..ops import torch_ref

        if self.booster_type == "gblinear":
            raise ValueError("pred_leaf is not defined for the gblinear booster")
        t_begin, t_end = self._tree_range(iteration_range)
        flat = self._explain_on_device(X, t_begin, t_end, shap=False)
        if flat is not None:
            hip = ops.backend_for(X.device)
            return hip.pred_leaf(flat, X, t_begin, t_end).cpu().numpy()
        return torch_ref.pred_leaf(self._cpu_flat_forest(), X.cpu(), t_begin, t_end).numpy()

    def get_score(self, fmap="", importance_type="weight"):
        """Feature importances (weight / gain / total_gain / cover /
        total_cover) keyed like xgboost ('f<idx>' or feature names)."""
        counts = {}
        gains = {}
        covers = {}
        for tree in self.trees:
            for nid in range(tree.num_nodes):
                if tree.left[nid] < 0:
                    continue
                f = int(tree.feature[nid])
                counts[f] = counts.get(f, 0) + 1
                gains[f] = gains.get(f, 0.0) + float(tree.gain[nid])
                covers[f] = covers.get(f, 0.0) + float(tree.sum_hess[nid])

        def name(f):
            if self.feature_names and f < len(self.feature_names):
                return self.feature_names[f]
            return f"f{f}"

        if importance_type == "weight":
            return {name(f): v for f, v in counts.items()}
        if importance_type == "total_gain":
            return {name(f): v for f, v in gains.items()}
        if importance_type == "gain":
            return {name(f): gains[f] / counts[f] for f in counts}
        if importance_type == "total_cover":
            return {name(f): v for f, v in covers.items()}
        if importance_type == "cover":
            return {name(f): covers[f] / counts[f] for f in counts}
        raise ValueError(f"Unknown importance type: {importance_type}")

    def _refuse_categorical_dump(self, what):
        """The dump formats print a node as `feature < threshold`; a
        category set has no such form here."""
        if self.has_categorical_splits():
            raise NotImplementedError(
                f"{what} is not implemented for models with categorical splits"
            )

    def _tree_dump_json(self, tree, with_stats):
        def name(f):
            if self.feature_names and f < len(self.feature_names):
                return self.feature_names[f]
            return f"f{f}"

        def node(nid, depth):
            if tree.left[nid] < 0:
                out = {"nodeid": int(nid), "leaf": float(tree.value[nid])}
                if with_stats:
                    out["cover"] = float(tree.sum_hess[nid])
                return out
            yes, no = int(tree.left[nid]), int(tree.right[nid])
            out = {
                "nodeid": int(nid),
                "depth": depth,
                "split": name(int(tree.feature[nid])),
                "split_condition": float(tree.threshold[nid]),
                "yes": yes,
                "no": no,
                "missing": yes if tree.default_left[nid] else no,
            }
            if with_stats:
                out["gain"] = float(tree.gain[nid])
                out["cover"] = float(tree.sum_hess[nid])
            out["children"] = [node(yes, depth + 1), node(no, depth + 1)]
            return out

        return json.dumps(node(0, 0))

    def trees_to_dataframe(self, fmap=""):
        """Forest as a pandas DataFrame (xgboost column layout)."""
        import pandas as pd

        self._refuse_categorical_dump("trees_to_dataframe")

        rows = []
        for t, tree in enumerate(self.trees):
            for nid in range(tree.num_nodes):
                leaf = tree.left[nid] < 0
                f = int(tree.feature[nid])
                fname = (
                    self.feature_names[f]
                    if self.feature_names and f < len(self.feature_names)
                    else f"f{f}"
                )
                rows.append({
                    "Tree": t,
                    "Node": int(nid),
                    "ID": f"{t}-{nid}",
                    "Feature": "Leaf" if leaf else fname,
                    "Split": None if leaf else float(tree.threshold[nid]),
                    "Yes": None if leaf else f"{t}-{int(tree.left[nid])}",
                    "No": None if leaf else f"{t}-{int(tree.right[nid])}",
                    "Missing": None if leaf else (
                        f"{t}-{int(tree.left[nid]) if tree.default_left[nid] else int(tree.right[nid])}"
                    ),
                    "Gain": float(tree.value[nid]) if leaf else float(tree.gain[nid]),
                    "Cover": float(tree.sum_hess[nid]),
                })
        return pd.DataFrame(rows)

    def get_fscore(self, fmap=""):
        """Alias of get_score(importance_type='weight') — xgboost parity."""
        return self.get_score(fmap=fmap, importance_type="weight")

    def get_dump(self, fmap="", with_stats=False, dump_format="text"):
        """Per-tree dumps in the xgboost text or json format."""
        self._refuse_categorical_dump("get_dump")
        if dump_format == "json":
            return [self._tree_dump_json(t, with_stats) for t in self.trees]
        dumps = []
        for tree in self.trees:
            lines = []

            def walk(nid, depth):
                indent = "\t" * depth
                if tree.left[nid] < 0:
                    stat = f",cover={tree.sum_hess[nid]}" if with_stats else ""
                    lines.append(f"{indent}{nid}:leaf={tree.value[nid]}{stat}")
                else:
                    f = int(tree.feature[nid])
                    fname = (
                        self.feature_names[f]
                        if self.feature_names and f < len(self.feature_names)
                        else f"f{f}"
                    )
                    yes, no = int(tree.left[nid]), int(tree.right[nid])
                    missing = yes if tree.default_left[nid] else no
                    stat = (
                        f",gain={tree.gain[nid]},cover={tree.sum_hess[nid]}" if with_stats else ""
                    )
                    lines.append(
                        f"{indent}{nid}:[{fname}<{tree.threshold[nid]}] "
                        f"yes={yes},no={no},missing={missing}{stat}"
                    )
                    walk(yes, depth + 1)
                    walk(no, depth + 1)

            walk(0, 0)
            dumps.append("\n".join(lines) + "\n")
        return dumps

    def _linear_contribs(self, X, base_margin):
        """gblinear contributions (n, k, f+1) float64: x_j * w_j (missing
        values contribute 0), bias column = linear bias + starting margin."""
        n, f = X.shape
        k = self.n_outputs
        phi = torch.zeros((n, k, f + 1), dtype=torch.float64, device=X.device)
        if self.linear_model is not None:
            w = self.linear_model.weights.to(X.device).to(torch.float64).reshape(f, k)
            b = self.linear_model.bias.to(X.device).to(torch.float64).reshape(k)
            x = torch.nan_to_num(X, nan=0.0).to(torch.float64)
            phi[:, :, :f] = x.unsqueeze(1) * w.t().unsqueeze(0)
            phi[:, :, f] = b.unsqueeze(0)
        phi[:, :, f] += self._bias_rows(n, base_margin, X.device)
        return phi

    def _pred_contribs(self, X, approx=False, iteration_range=None, base_margin=None):
        """Feature contributions of the rounds in `iteration_range`.

        Exact TreeSHAP by default — parity with the reference's native
        pred_contribs path (reference test_abalone.py:65): the path-form
        HIP kernel when X is on the GPU and the forest is within the device
        limits (the compact-slot kernel where the dense phi slab does not
        fit LDS), else Lundberg's recursion in parallel C++ on the host.
        `approx=True` is the Saabas approximation (xgboost's
        approx_contribs=True), vectorized over the flat forest on X's
        device. Returns (n, f+1) for single-output, (n, k, f+1) for
        multiclass; rows sum to the margin (additivity). A DMatrix
        base_margin replaces base_score in the bias column, per row.
        """
        from ..ops import torch_ref

        n = X.shape[0]
        k = self.n_outputs
        if self.booster_type == "gblinear":
            phi = self._linear_contribs(X, base_margin)
            out = phi.to(torch.float32).cpu().numpy()
            return out[:, 0, :] if k == 1 else out
        t_begin, t_end = self._tree_range(iteration_range)
        if approx:
            if X.device.type == "cuda" and ops.backend_for(X.device).NAME == "hip":
                flat = self._device_flat_forest(X.device, with_paths=False)
            else:
                X = X.cpu()
                flat = self._cpu_flat_forest()
            phi = torch_ref.saabas_contribs(flat, X, k, t_begin, t_end)
        else:
            # SMXGB_SHAP_COMPACT: 1 = compact kernel for every device request,
            # 0 = never; unset = only where the dense phi slab does not fit
            # LDS (wide or multiclass models), which used to mean the host
            compact = os.environ.get("SMXGB_SHAP_COMPACT")
            flat = None if compact == "1" else self._explain_on_device(X, t_begin, t_end, shap=True)
            if flat is None and compact != "0":
                cflat = self._compact_explain_flat(X.device, n, X.shape[1], t_begin, t_end)
                if cflat is not None:
                    self._log_explain_route("compact kernel over dense rows")
                    return self._contribs_compact(
                        cflat, X, n, X.shape[1], t_begin, t_end, base_margin
                    )
                if compact == "1":
                    flat = self._explain_on_device(X, t_begin, t_end, shap=True)
            if flat is not None:
                self._log_explain_route("dense-slab kernel")
                phi = ops.backend_for(X.device).tree_shap(flat, X, k, t_begin, t_end)
            else:
                self._log_explain_route("host recursion")
                phi = torch_ref.tree_shap(self._cpu_flat_forest(), X.cpu(), k, t_begin, t_end)
            if t_end > t_begin:
                phi[:, :, -1] += self._expected_values(t_begin, t_end).to(phi.device).unsqueeze(0)
        phi[:, :, -1] += self._bias_rows(n, base_margin, phi.device)
        out = phi.to(torch.float32).cpu().numpy()
        return out[:, 0, :] if k == 1 else out

    def _pred_interactions(self, X, iteration_range=None, base_margin=None):
        """SHAP interaction values: (n, f+1, f+1), or (n, k, f+1, f+1) for
        multiclass, float32. Symmetric; row sums equal pred_contribs; the
        bias sits in cell [f, f] and the rest of the last row and column is
        zero. Same routing as _pred_contribs."""
        from ..ops import torch_ref

        n, f = X.shape
        k = self.n_outputs
        if self.booster_type == "gblinear":
            phi = self._linear_contribs(X, base_margin)
            out = torch.diag_embed(phi)  # a linear model has no interactions
        else:
            t_begin, t_end = self._tree_range(iteration_range)
            flat = self._explain_on_device(X, t_begin, t_end, shap=True)
            if flat is not None:
                out = ops.backend_for(X.device).tree_shap_interactions(
                    flat, X, k, t_begin, t_end
                )
            else:
                out = torch_ref.tree_shap_interactions(
                    self._cpu_flat_forest(), X.cpu(), k, t_begin, t_end
                )
            if t_end > t_begin:
                out[:, :, f, f] += self._expected_values(t_begin, t_end).to(out.device).unsqueeze(0)
            out[:, :, f, f] += self._bias_rows(n, base_margin, out.device)
        out = out.to(torch.float32).cpu().numpy()
        return out[:, 0] if k == 1 else out

    # -- serialization -----------------------------------------------------
    def _tree_to_json(self, tree, tree_id):
        n = tree.num_nodes
        tree.finalize()
        leaf = tree.left < 0
        split_conditions = np.where(leaf, tree.value, tree.threshold).astype(np.float32)
        # upstream's layout of the category sets: the members of every
        # categorical node, flat and ascending, with per-node segments
        categories, cat_nodes, cat_segments, cat_sizes = [], [], [], []
        for nid in np.flatnonzero(np.asarray(tree.split_type)):
            members = cat_members(tree.cat_bits[nid])
            cat_nodes.append(int(nid))
            cat_segments.append(len(categories))
            cat_sizes.append(len(members))
            categories.extend(members)
        return {
            "base_weights": [float(v) for v in tree.value],
            "categories": categories,
            "categories_nodes": cat_nodes,
            "categories_segments": cat_segments,
            "categories_sizes": cat_sizes,
            "default_left": [int(b) for b in tree.default_left],
            "id": tree_id,
            "left_children": [int(v) for v in tree.left],
            "loss_changes": [float(v) for v in tree.gain],
            "parents": [int(v) if v >= 0 else 2147483647 for v in tree.parent],
            "right_children": [int(v) for v in tree.right],
            "split_conditions": [float(v) for v in split_conditions],
            "split_indices": [int(v) for v in tree.feature],
            "split_type": [int(v) for v in tree.split_type],
            "sum_hessian": [float(v) for v in tree.sum_hess],
            "tree_param": {
                "num_deleted": "0",
                "num_feature": str(self.num_features),
                "num_nodes": str(n),
                "size_leaf_vector": "1",
            },
        }

    @staticmethod
    def _tree_from_json(obj):
        left = np.asarray(obj["left_children"], dtype=np.int32)
        cond = np.asarray(obj["split_conditions"], dtype=np.float32)
        leaf = left < 0
        # categorical nodes: split_type 1 and a segment of `categories`, the
        # members of the set that goes right
        split_type = np.asarray(obj.get("split_type") or np.zeros(len(left)), dtype=np.uint8)
        split_type = np.where(leaf, 0, split_type).astype(np.uint8)
        cat_bits = np.zeros((len(left), CAT_WORDS), dtype=np.uint32)
        if split_type.any():
            categories = list(obj.get("categories", []))
            segments = dict(zip(
                (int(v) for v in obj.get("categories_nodes", [])),
                zip(obj.get("categories_segments", []), obj.get("categories_sizes", [])),
            ))
            for nid in np.flatnonzero(split_type):
                if int(nid) not in segments:
                    raise ValueError(f"categorical node {int(nid)} has no entry in categories_nodes")
                start, size = (int(v) for v in segments[int(nid)])
                cat_bits[nid] = cat_bits_from_members(categories[start:start + size])
        tree = Tree.from_arrays(
            {
                "left": left,
                "right": np.asarray(obj["right_children"], dtype=np.int32),
                "parent": [(-1 if p == 2147483647 else p) for p in obj.get("parents", [2147483647] * len(left))],
                "feature": np.asarray(obj["split_indices"], dtype=np.int32),
                "threshold": np.where(leaf, 0.0, cond).astype(np.float32),
                "default_left": np.asarray(obj["default_left"], dtype=bool),
                "value": np.where(leaf, cond, np.asarray(obj.get("base_weights", cond), dtype=np.float32)),
                "gain": obj.get("loss_changes", np.zeros(len(left))),
                "sum_hessian": obj.get("sum_hessian", np.zeros(len(left))),
                "split_type": split_type,
                "cat_bits": cat_bits,
            }
        )
        tree.sum_hess = np.asarray(obj.get("sum_hessian", np.zeros(len(left))), dtype=np.float32)
        return tree

    # objectives whose upstream SaveConfig writes a reg_loss_param block
    _REG_LOSS_OBJECTIVES = (
        "reg:squarederror", "reg:linear", "reg:squaredlogerror", "reg:logistic",
        "binary:logistic", "binary:logitraw",
    )

    def _objective_json(self):
        """Objective block matching what upstream xgboost's SaveConfig
        writes for every objective family — the loader there reads these
        param sub-objects unconditionally, so each family must emit its
        block (advisor round-1 finding)."""
        name = self.objective_name
        obj = {"name": name}
        p = self.params
        if name in self._REG_LOSS_OBJECTIVES:
            obj["reg_loss_param"] = {"scale_pos_weight": str(p.get("scale_pos_weight", 1.0))}
        elif name.startswith("multi:"):
            obj["softmax_multiclass_param"] = {"num_class": str(self.num_class)}
        elif name == "count:poisson":
            obj["poisson_regression_param"] = {"max_delta_step": str(p.get("max_delta_step", 0.7))}
        elif name == "reg:tweedie":
            obj["tweedie_regression_param"] = {
                "tweedie_variance_power": str(p.get("tweedie_variance_power", 1.5))
            }
        elif name == "reg:pseudohubererror":
            obj["pseudo_huber_param"] = {"huber_slope": str(p.get("huber_slope", 1.0))}
        elif name == "reg:quantileerror":
            alphas = parse_quantile_alpha(p.get("quantile_alpha", 0.5))
            obj["quantile_loss_param"] = {"quantile_alpha": json.dumps(alphas)}
        elif name == "survival:aft":
            obj["aft_loss_param"] = {
                "aft_loss_distribution": str(p.get("aft_loss_distribution", "normal")),
                "aft_loss_distribution_scale": str(p.get("aft_loss_distribution_scale", 1.0)),
            }
        elif name.startswith("rank:"):
            obj["lambdarank_param"] = {
                "lambdarank_num_pair_per_sample": str(p.get("lambdarank_num_pair_per_sample", 1)),
                "lambdarank_pair_method": str(p.get("lambdarank_pair_method", "mean")),
                "lambdarank_unbiased": str(p.get("lambdarank_unbiased", 0)),
            }
        return obj

    def _gbtree_model_json(self):
        return {
            "gbtree_model_param": {
                "num_trees": str(len(self.trees)),
                "num_parallel_tree": str(self.params.get("num_parallel_tree", 1)),
            },
            "iteration_indptr": list(self.iteration_indptr),
            "tree_info": list(self.tree_info),
            "trees": [self._tree_to_json(t, i) for i, t in enumerate(self.trees)],
        }

    def _gradient_booster_json(self):
        if self.booster_type == "gblinear":
            flat = self.linear_model.to_flat() if self.linear_model is not None else []
            return {
                "model": {"weights": flat, "boosted_rounds": self.num_boosted_rounds()},
                "name": "gblinear",
            }
        if self.booster_type == "dart":
            return {
                "model": {
                    "gbtree": self._gbtree_model_json(),
                    "weight_drop": [float(w) for w in self.weight_drop],
                },
                "name": "dart",
            }
        return {"model": self._gbtree_model_json(), "name": "gbtree"}

    def save_json(self):
        model = {
            "learner": {
                "attributes": dict(self.attributes_map),
                "feature_names": self.feature_names or [],
                "feature_types": list(self.feature_types or []),
                "gradient_booster": self._gradient_booster_json(),
                "learner_model_param": {
                    "base_score": repr(self.base_score),
                    "boost_from_average": "1",
                    "num_class": str(self.num_class),
                    "num_feature": str(self.num_features),
                    # upstream counts the quantiles of reg:quantileerror as targets
                    "num_target": str(
                        self.n_outputs if self.objective_name == "reg:quantileerror" else 1
                    ),
                },
                "objective": self._objective_json(),
            },
            "version": MODEL_VERSION,
        }
        return model

    def save_model(self, path):
        with open(str(path) + ".tmp", "w") as f:
            json.dump(self.save_json(), f)
        os.replace(str(path) + ".tmp", str(path))

    def load_json(self, model):
        learner = model["learner"]
        booster_name = learner["gradient_booster"].get("name", "gbtree")
        gb = learner["gradient_booster"]["model"]
        lmp = learner["learner_model_param"]
        self.params["objective"] = learner["objective"]["name"]
        # restore objective parameters stored in the model (upstream does;
        # without this, warm-start/predict silently uses defaults)
        objective_params_from_json(learner.get("objective", {}), self.params)
        if int(lmp.get("num_class", "0") or 0) > 0:
            self.params["num_class"] = int(lmp["num_class"])
        self.params["base_score"] = float(lmp.get("base_score", 0.5))
        self.num_features = int(lmp.get("num_feature", 0))
        self.feature_names = learner.get("feature_names") or None
        self.feature_types = list(learner.get("feature_types") or []) or None
        self.attributes_map = dict(learner.get("attributes", {}))
        self.params["booster"] = booster_name

        if booster_name == "gblinear":
            from .gblinear import LinearModel

            flat = gb.get("weights", [])
            self.linear_model = LinearModel.from_flat(flat, self.num_features, self.n_outputs)
            rounds = int(gb.get("boosted_rounds", 1) or 1)
            self.trees = []
            self.tree_info = []
            self.weight_drop = []
            self.iteration_indptr = list(range(rounds + 1))
            self._objective = None
            self._predict_cache = None
            return self

        weight_drop = None
        if booster_name == "dart":
            weight_drop = [float(w) for w in gb.get("weight_drop", [])]
            gb = gb["gbtree"]

        self.trees = [self._tree_from_json(t) for t in gb["trees"]]
        self.tree_info = list(gb.get("tree_info", [0] * len(self.trees)))
        self.weight_drop = weight_drop if weight_drop else [1.0] * len(self.trees)
        indptr = gb.get("iteration_indptr")
        if indptr:
            self.iteration_indptr = list(indptr)
        else:
            per_round = max(1, self.n_outputs)
            self.iteration_indptr = list(range(0, len(self.trees) + 1, per_round))
        self._objective = None
        self._predict_cache = None
        return self

    def load_model(self, path):
        """Load a Booster file: JSON, UBJSON (xgboost >= 1.6 default), or
        the deprecated binary format older reference containers produced
        (reference serve_utils.py:184-186 loads the same three)."""
        with open(path, "rb") as f:
            raw = f.read()
        head = raw[:1]
        if head == b"{" and raw.lstrip()[:1] == b"{":
            try:
                return self.load_json(json.loads(raw))
            except (json.JSONDecodeError, UnicodeDecodeError):
                pass  # '{' is also the UBJSON object marker — fall through
        if head == b"{":
            from ..utils import ubjson

            return self.load_json(ubjson.loads(raw))
        from .legacy_binary import looks_like_legacy_binary, parse_legacy_binary

        if looks_like_legacy_binary(raw):
            return parse_legacy_binary(raw, booster=self)
        raise ValueError(
            f"Unsupported model format in {path} (expected JSON/UBJSON/legacy-binary Booster)"
        )

    def save_model_ubj(self, path):
        from ..utils import ubjson

        with open(str(path) + ".tmp", "wb") as f:
            f.write(ubjson.dumps(self.save_json()))
        os.replace(str(path) + ".tmp", str(path))

    def save_config(self):
        return json.dumps(
            {
                "learner": {
                    "learner_train_param": {"objective": self.objective_name},
                    "objective": self._objective_json(),
                    "learner_model_param": {
                        "num_class": str(self.num_class),
                        "base_score": repr(self.base_score),
                        "num_feature": str(self.num_features),
                    },
                }
            }
        )

    # -- pickling ----------------------------------------------------------
    def __getstate__(self):
        state = dict(self.__dict__)
        state["_objective"] = None
        state["_predict_cache"] = None
        if state.get("linear_model") is not None:
            lm = state["linear_model"]
            lm.weights = lm.weights.cpu()
            lm.bias = lm.bias.cpu()
        return state

    def __setstate__(self, state):
        # pickles of upstream xgboost.core.Booster carry the serialized
        # model as state["handle"] (raw bytes); with the xgboost shim
        # installed this class IS xgboost.core.Booster, so route those
        # through the legacy/JSON byte loader instead of __dict__ update
        raw = state.get("handle")
        if raw is not None and isinstance(raw, (bytes, bytearray)) and "params" not in state:
            from .legacy_binary import load_model_bytes

            self.__init__()
            load_model_bytes(bytes(raw), booster=self)
            fnames = state.get("feature_names")
            if fnames:
                self.feature_names = list(fnames)
            return
        self.__dict__.update(state)

    def copy(self):
        import copy as _copy

        return _copy.deepcopy(self)
