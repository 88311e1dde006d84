"""The boosting loop — this framework's ``xgb.train``.

Replaces the native train loop the reference calls at
algorithm_mode/train.py:367-376,432-442. Signature and callback behavior
follow the xgboost Python API surface the container layers depend on
(callbacks re-entered once per round, evals_result history, early stopping,
xgb_model warm start).

Device strategy (MI355X-first): all round-loop state — quantized bins, row
index buffers, margins, gradients — stays resident on the GPU; one
quantization pass up front; per-round work is the HIP kernel set driven by
the grower. On CPU the same loop runs the torch reference ops (small jobs,
unit tests).
"""
import logging
import math

import numpy as np
import torch

from .booster import Booster
from .callback_api import CallbackContainer, EarlyStopping, EvaluationMonitor
from . import eval_metrics
from .eval_metrics import evaluate as evaluate_metric
from .grower import HistGrower
from .objectives import create_objective
from ..ops import backend_for
from ..ops.quantize import quantize

logger = logging.getLogger(__name__)

_TRAIN_PARAM_KEYS = {
    "eta", "learning_rate", "gamma", "min_split_loss", "max_depth", "min_child_weight",
    "max_delta_step", "subsample", "colsample_bytree", "colsample_bylevel", "colsample_bynode",
    "lambda", "reg_lambda", "alpha", "reg_alpha", "tree_method", "grow_policy", "max_leaves",
    "max_bin", "objective", "num_class", "base_score", "eval_metric", "seed", "nthread",
    "num_parallel_tree", "scale_pos_weight", "tweedie_variance_power", "verbosity",
    "aft_loss_distribution", "aft_loss_distribution_scale", "monotone_constraints",
    "interaction_constraints", "deterministic_histogram", "sampling_method", "booster",
    "predictor", "device", "updater", "refresh_leaf", "process_type", "sketch_eps",
    "one_drop", "skip_drop", "rate_drop", "sample_type", "normalize_type", "lambda_bias",
    "huber_slope", "dsplit", "prob_buffer_row", "quantile_alpha",
    "max_cat_to_onehot", "max_cat_threshold",
}


def sparse_auto_engage(n, f, nnz, free_bytes=None):
    """The automatic (SMXGB_SPARSE unset) sparse-path decision.

    On the host (`free_bytes` None): wide and at most half full. On a ROCm
    device (`free_bytes` = free device memory) the same rule AND the dense
    staging — float32 features plus uint8 bins, n*f*5 bytes — would take
    more than half of the free memory. The device rule is memory-driven
    only, so every job that fits keeps the dense device grower; where the
    sparse path becomes faster than the dense one has not been measured
    and is deliberately not encoded here.
    """
    if not (f >= 64 and nnz <= 0.5 * n * f):
        return False
    if free_bytes is None:
        return True
    return n * f * 5 > free_bytes / 2


def _sparse_path_ok(dtrain, params, device, comm):
    """Engage a CSR training backend (ops/sparse_ref.py on the host,
    ops/hip_sparse.py on a ROCm device)?

    Wide sparse data (libsvm channels, reference data_utils.py:361) never
    densifies; small/narrow data keeps the dense fast path. Forced with
    SMXGB_SPARSE=1 / disabled with SMXGB_SPARSE=0. With a communicator the
    GPU keeps the dense path (distributed device-sparse training is not
    implemented).
    """
    import os as _os

    flag = _os.environ.get("SMXGB_SPARSE")
    if flag == "0":
        return False
    if not getattr(dtrain, "is_sparse", False):
        return False
    if getattr(dtrain, "is_cat", None) is not None:
        return False  # categorical columns train on the dense route
    if device.type not in ("cpu", "cuda"):
        return False
    if device.type == "cuda" and comm is not None:
        return False
    if params.get("booster", "gbtree") != "gbtree":
        return False
    if params.get("process_type") == "update":
        return False
    if flag == "1":
        return True
    n, f = dtrain.num_row(), dtrain.num_col()
    nnz = dtrain.csr().nnz
    if device.type == "cpu":
        return sparse_auto_engage(n, f, nnz)
    if not sparse_auto_engage(n, f, nnz):
        return False  # no device query for jobs the host rule already rejects
    free_bytes, _total = torch.cuda.mem_get_info(device)
    return sparse_auto_engage(n, f, nnz, free_bytes)


def _resolve_device(params):
    device = params.get("device")
    if device:
        return torch.device(device)
    if torch.cuda.is_available():
        return torch.device("cuda")
    return torch.device("cpu")


def _csr_tree_margin_fn(csr, device):
    """tree -> (n,) margin contribution over the rows of a scipy CSR matrix
    that stays sparse: the HIP traversal over an uploaded copy on a ROCm
    device, the chunked host traversal on the CPU."""
    if device.type == "cuda":
        from ..ops import hip_sparse

        dev_csr = hip_sparse.DeviceCSR(csr, device)
        return lambda tree: hip_sparse.predict_tree_csr(tree, dev_csr)
    from ..ops.sparse_ref import predict_tree_csr

    return lambda tree: predict_tree_csr(tree, csr)


class _AdaptiveLeaves:
    """Adaptive tree leaves (reg:absoluteerror, reg:quantileerror): once a
    tree's structure is grown, every leaf value becomes eta times the
    (weighted) alpha quantile of y - margin over the leaf's rows, as
    upstream XGBoost (1.7 and later) defines these objectives. The rule is
    ops/torch_ref.leaf_quantiles; on a ROCm device the segmented radix
    select of csrc/smxgb_quantile.hip computes all leaves at once, and the
    leaf values are the one readback per tree.

    It sits above the growers and only needs the tree, the node id of
    every leaf_jobs entry (grower.leaf_nodes) and the rows the tree grew on
    (grower.tree_rows). Built only for an objective with adaptive_alphas.
    """

    def __init__(self, objective, X, Xcsr, y, weight, device, comm):
        self.alphas = list(objective.adaptive_alphas)
        self.X = X
        self.Xcsr = Xcsr
        self.y = y
        self.weight = weight  # the DMatrix weights, not a sampler's rescaled pairs
        self.device = device
        self.comm = comm if comm is not None and getattr(comm, "world_size", 1) > 1 else None
        self.weight_max = float(weight.max()) if weight is not None and weight.numel() else None
        if self.weight_max is not None and not (
            math.isfinite(self.weight_max) and float(weight.min()) >= 0.0
        ):
            raise ValueError("sample weights must be finite and non-negative")
        self._dev_csr = None

    def _leaf_node_of_rows(self, tree):
        """(n,) node id of the leaf every training row falls into."""
        if self.device.type == "cuda":
            from ..ops import hip, hip_sparse

            flat = hip.make_flat_forest([tree], [0], None, self.device)
            if self.X is not None:
                return hip.pred_leaf(flat, self.X)[:, 0]
            if self._dev_csr is None:
                self._dev_csr = hip_sparse.DeviceCSR(self.Xcsr, self.device)
            return hip_sparse.pred_leaf_csr(flat, self._dev_csr)[:, 0]
        if self.X is not None:
            from ..ops import torch_ref

            return torch_ref.tree_leaf_ids(tree, self.X)
        from ..ops import sparse_ref

        return sparse_ref.tree_leaf_ids_csr(tree, self.Xcsr)

    def update(self, tree, leaf_jobs, grower, margin_col, cls):
        """Replace the leaf values of `tree` (an output-`cls` tree grown from
        the round's margin column `margin_col`) in tree.value and in
        leaf_jobs; returns the new leaf_jobs (same order)."""
        leaf_nodes = grower.leaf_nodes
        n_leaves = len(leaf_nodes)
        slot_of_node = np.full(tree.num_nodes, -1, dtype=np.int32)
        slot_of_node[np.asarray(leaf_nodes, dtype=np.int64)] = np.arange(n_leaves, dtype=np.int32)
        node = self._leaf_node_of_rows(tree).to(self.device)
        pos = torch.from_numpy(slot_of_node).to(self.device)[node.long()]
        rows = grower.tree_rows
        if rows is not None:
            sampled = torch.full_like(pos, -1)
            idx = rows.long()
            sampled[idx] = pos[idx]
            pos = sampled
        resid = (self.y - margin_col).to(torch.float32)
        backend = grower.backend
        if self.device.type == "cuda":
            # pos comes from this tree's own leaves and the weights were
            # checked once: no host check, no synchronization before launch
            q = backend.leaf_quantiles(
                pos, resid, n_leaves, self.alphas[cls], self.weight,
                weight_max=self.weight_max, check=False,
            )
        else:
            q = backend.leaf_quantiles(pos, resid, n_leaves, self.alphas[cls], self.weight)
        q = q.to(torch.float64)
        if self.comm is not None:
            # upstream's rule: the mean of the ranks' local quantiles, over
            # the ranks where the leaf has rows; one fused allreduce per tree
            have = ~torch.isnan(q)
            fused = torch.cat([torch.where(have, q, torch.zeros_like(q)), have.to(torch.float64)])
            self.comm.allreduce_(fused)
            q = fused[:n_leaves] / fused[n_leaves:]  # 0 / 0: NaN, no rank has rows
        q = q.cpu().numpy()  # the tree's one readback
        values = (q * float(grower.p.eta)).astype(np.float32)
        out = []
        for (parity, start, end, value), nid, v in zip(leaf_jobs, leaf_nodes, values):
            if not np.isnan(v):  # a leaf without rows keeps its Newton value
                value = float(v)
                tree.value[nid] = v
            out.append((parity, start, end, value))
        return out


class _EvalSet:
    """Resident eval data: dense features + incrementally updated margins.

    When the eval set IS the training DMatrix (the standard watchlist), it
    aliases the training tensors and margins — no copy, no per-round
    traversal (`is_train`). A wide sparse eval set stays CSR (`self.csr`)
    and is traversed as CSR (on the device by the HIP CSR traversal, on the
    host in bounded-memory chunks) instead of densified.
    """

    def __init__(self, dmatrix, name, device, n_outputs, base_margin_value,
                 train_dmatrix=None, train_X=None, train_y=None, train_w=None,
                 keep_sparse=False):
        self.name = name
        self.csr = None
        self.is_train = dmatrix is train_dmatrix
        if self.is_train:
            self.X = train_X
            self.y = train_y
            self.w = train_w
            self.dmatrix = dmatrix
            self.margin = None  # provided by the trainer each round
            return
        if keep_sparse and getattr(dmatrix, "is_sparse", False):
            self.X = None
            self.csr = dmatrix.csr()
            self._csr_margin = _csr_tree_margin_fn(self.csr, device)
        else:
            self.X = torch.as_tensor(dmatrix.to_dense(), dtype=torch.float32, device=device)
        self.y = torch.as_tensor(dmatrix.get_label(), dtype=torch.float32, device=device)
        w = dmatrix.get_weight()
        self.w = (
            torch.as_tensor(w, dtype=torch.float32, device=device)
            if w is not None and len(w)
            else None
        )
        self.dmatrix = dmatrix
        n_rows = dmatrix.num_row()
        user_margin = dmatrix.get_base_margin()
        if user_margin is not None:
            self.margin = torch.as_tensor(user_margin, dtype=torch.float32, device=device).reshape(
                n_rows, n_outputs
            )
        else:
            self.margin = torch.full(
                (n_rows, n_outputs), float(base_margin_value), dtype=torch.float32, device=device
            )

    def tree_margin(self, backend, tree):
        """One tree's margin contribution over this eval set's rows."""
        if self.X is None:
            return self._csr_margin(tree)
        return backend.predict_tree(tree, self.X)


def train(
    params,
    dtrain,
    num_boost_round=10,
    evals=None,
    obj=None,
    feval=None,
    maximize=None,
    early_stopping_rounds=None,
    evals_result=None,
    verbose_eval=True,
    xgb_model=None,
    callbacks=None,
    custom_metric=None,
    comm=None,
):
    """Train a Booster. API-parity with xgboost.train (reference call sites
    train.py:367-376,432-442; checkpointing.py:74)."""
    if feval is None and custom_metric is not None:
        feval = custom_metric  # xgboost >= 1.6 alias
    params = dict(params or {})
    unknown = set(params) - _TRAIN_PARAM_KEYS
    for key in unknown:
        logger.warning("Ignoring unknown training parameter: %s", key)

    # verbosity 0 silent(ish), 1 default (eval lines are INFO — the
    # CloudWatch scrape contract — so the default keeps INFO), 3 debug
    verbosity = int(params.get("verbosity", 1) or 1)
    logging.getLogger("sagemaker_xgboost_container_amd").setLevel(
        {0: logging.WARNING, 1: logging.INFO, 2: logging.INFO, 3: logging.DEBUG}.get(
            verbosity, logging.INFO
        )
    )

    # tree_method routing: this framework implements ONE updater — the
    # quantized-histogram grower (the reference's hist/gpu_hist). `exact`
    # and `approx` are accepted for configuration compatibility (reference
    # hyperparameter_validation.py:22-25) but deliberately mapped onto
    # hist; with exact cut finding (ops/quantize.py) and max_bin bins the
    # models are near-identical. Warn loudly instead of diverging silently.
    tree_method = params.get("tree_method", "auto")
    if tree_method in ("exact", "approx"):
        logger.warning(
            "tree_method='%s' is not implemented natively; training with the "
            "histogram updater (tree_method=hist) instead. Results are "
            "near-identical for continuous features; increase max_bin "
            "(currently %s) to tighten the approximation.",
            tree_method,
            params.get("max_bin", 256),
        )

    device = _resolve_device(params)
    seed = int(params.get("seed", 0) or 0)
    generator = torch.Generator(device=device)
    generator.manual_seed(seed if seed else 2016)

    objective = create_objective(params.get("objective", "reg:squarederror"), params)
    n_outputs = objective.n_outputs
    num_parallel_tree = int(params.get("num_parallel_tree", 1))

    # -- booster (fresh or warm start) ------------------------------------
    if xgb_model is not None:
        if isinstance(xgb_model, (str, bytes)):
            booster = Booster()
            booster.load_model(xgb_model)
            booster.params.update({k: v for k, v in params.items() if k not in ("objective", "num_class")})
        else:
            booster = xgb_model
            booster.params.update(params)
        start_round = booster.num_boosted_rounds()
    else:
        booster = Booster(params=params, num_features=dtrain.num_col(), feature_names=dtrain.feature_names)
        start_round = 0
    booster.num_features = dtrain.num_col()
    if getattr(dtrain, "feature_types", None):
        booster.feature_types = list(dtrain.feature_types)

    # -- resident training state ------------------------------------------
    sparse_mode = _sparse_path_ok(dtrain, params, device, comm)
    if sparse_mode:
        Xcsr = dtrain.csr()
        X = None
        logger.info(
            "Sparse training path engaged (backend %s): %dx%d CSR, %d nnz (density %.4f) — no densification",
            "hip_sparse" if device.type == "cuda" else "sparse_ref",
            Xcsr.shape[0], Xcsr.shape[1], Xcsr.nnz, Xcsr.nnz / max(1, Xcsr.shape[0] * Xcsr.shape[1]),
        )
    else:
        Xcsr = None
        X = torch.as_tensor(dtrain.to_dense(), dtype=torch.float32, device=device)
    y = torch.as_tensor(dtrain.get_label(), dtype=torch.float32, device=device)
    w_raw = dtrain.get_weight()
    weight = (
        torch.as_tensor(w_raw, dtype=torch.float32, device=device)
        if w_raw is not None and len(w_raw)
        else None
    )
    objective.validate_labels(y)
    objective.set_info(dtrain, device)

    max_bin = int(params.get("max_bin", 256))
    qm = None
    if params.get("booster", "gbtree") != "gblinear":
        if sparse_mode:
            from ..ops.sparse_ref import quantize_sparse

            qm = quantize_sparse(
                Xcsr, max_bin=max_bin,
                sample_weight=weight.cpu().numpy() if weight is not None else None,
                comm=comm,
            )
            if device.type != "cpu":
                # cut finding and binning stay on the host; the CSR arrays
                # (never an n x f matrix) move to the device
                qm = qm.to(device)
        else:
            qm = quantize(
                X, max_bin=max_bin, sample_weight=weight, comm=comm,
                is_cat=getattr(dtrain, "is_cat", None), feature_names=dtrain.feature_names,
            )
    backend = backend_for(device)

    base_margin_value = objective.base_margin(booster.base_score)
    n = dtrain.num_row()
    user_margin = dtrain.get_base_margin()
    if user_margin is not None:
        margin = torch.as_tensor(user_margin, dtype=torch.float32, device=device).reshape(n, n_outputs).clone()
    else:
        margin = torch.full((n, n_outputs), float(base_margin_value), dtype=torch.float32, device=device)
        # warm start: accumulate existing trees' contributions
        train_csr_margin = (
            _csr_tree_margin_fn(Xcsr, device) if sparse_mode and booster.trees else None
        )
        for t_idx, tree in enumerate(booster.trees):
            if sparse_mode:
                margin[:, booster.tree_info[t_idx]] += train_csr_margin(tree)
            else:
                margin[:, booster.tree_info[t_idx]] += backend.predict_tree(tree, X)

    eval_sets = [
        _EvalSet(dm, name, device, n_outputs, base_margin_value,
                 train_dmatrix=dtrain, train_X=X, train_y=y, train_w=weight,
                 keep_sparse=sparse_mode)
        for dm, name in (evals or [])
        if dm is not None
    ]
    # re-play existing trees into eval margins on warm start
    for es in eval_sets:
        if not es.is_train and es.dmatrix.get_base_margin() is None:
            for t_idx, tree in enumerate(booster.trees):
                es.margin[:, booster.tree_info[t_idx]] += es.tree_margin(backend, tree)

    eval_metric = params.get("eval_metric")
    if eval_metric is None:
        metric_names = [objective.default_metric]
    elif isinstance(eval_metric, str):
        metric_names = [eval_metric]
    else:
        metric_names = list(eval_metric)

    # -- callbacks ---------------------------------------------------------
    cbs = list(callbacks or [])
    if verbose_eval and not any(isinstance(c, EvaluationMonitor) for c in cbs):
        rank = comm.rank if comm is not None else 0
        period = 1 if verbose_eval is True else int(verbose_eval)
        cbs.append(EvaluationMonitor(rank=rank, period=period))
    if early_stopping_rounds and not any(isinstance(c, EarlyStopping) for c in cbs):
        cbs.append(EarlyStopping(rounds=early_stopping_rounds, maximize=bool(maximize)))
    container = CallbackContainer(cbs)

    # process_type=update: run refresh/prune updaters over the EXISTING
    # trees instead of growing new ones (xgboost semantics; reference HP
    # surface algorithm_mode/hyperparameter_validation.py updater_validator)
    if params.get("process_type") == "update":
        from .refresh import run_update_process

        booster = container.before_training(booster)
        run_update_process(
            booster, params, X, y, weight, objective, margin, n_outputs,
            num_boost_round, container, eval_sets, metric_names, feval, comm,
        )
        booster = container.after_training(booster)
        if evals_result is not None:
            evals_result.update(container.history)
        return booster

    booster_kind = params.get("booster", "gbtree")
    if booster_kind == "gblinear":
        from .gblinear import LinearModel, LinearUpdater

        linear_updater = LinearUpdater(params)
        if booster.linear_model is None:
            booster.linear_model = LinearModel(dtrain.num_col(), n_outputs, device)
        else:
            booster.linear_model.weights = booster.linear_model.weights.to(device)
            booster.linear_model.bias = booster.linear_model.bias.to(device)
        grower = None
    else:
        grower = HistGrower(qm, params, comm=comm, generator=generator)

    # adaptive tree leaves: only objectives that declare adaptive_alphas
    # ever build (or run a line of) this step
    adaptive = None
    if grower is not None and objective.adaptive_alphas is not None:
        adaptive = _AdaptiveLeaves(objective, X, Xcsr, y, weight, device, comm)

    dart = None
    if booster_kind == "dart":
        dart = {
            "rate_drop": float(params.get("rate_drop", 0.0)),
            "skip_drop": float(params.get("skip_drop", 0.0)),
            "one_drop": int(params.get("one_drop", 0)),
            "sample_type": params.get("sample_type", "uniform"),
            "normalize_type": params.get("normalize_type", "tree"),
            "eta": float(params.get("eta", params.get("learning_rate", 0.3))),
        }

    booster = container.before_training(booster)

    train_tree_margin = [None]  # built on first use: the CSR form uploads a copy

    def add_tree_to_margin(state, tree, leaf_jobs, cls, scale=1.0):
        """Add a new tree (leaf_jobs already carry `scale`) to the training
        margin. The tree's own state knows the rows it grew on and updates
        those; a gradient-sampled tree (`margin_all_rows`) goes to every
        row — by the state's traversal of the bin matrix where it has one,
        else by predicting the tree over the training data."""
        if not getattr(state, "margin_all_rows", False) or getattr(state, "_traverse", None) is not None:
            state.update_margins(margin[:, cls], leaf_jobs)
            return
        if train_tree_margin[0] is None:
            train_tree_margin[0] = (
                _csr_tree_margin_fn(Xcsr, device) if sparse_mode
                else (lambda t: backend.predict_tree(t, X))
            )
        contrib = train_tree_margin[0](tree)
        margin[:, cls] += contrib * scale if scale != 1.0 else contrib

    for epoch in range(start_round, start_round + num_boost_round):
        if container.before_iteration(booster, epoch):
            break

        # -- DART: drop a subset of existing trees before computing gradients
        dropped = []
        drop_contrib = {}
        if dart is not None and booster.trees:
            if float(torch.rand((), generator=generator, device=device)) >= dart["skip_drop"]:
                n_trees = len(booster.trees)
                if dart["sample_type"] == "weighted":
                    wd = torch.tensor(booster.weight_drop, device=device)
                    probs = wd / wd.sum() * (dart["rate_drop"] * n_trees)
                else:
                    probs = torch.full((n_trees,), dart["rate_drop"], device=device)
                mask = torch.rand(n_trees, generator=generator, device=device) < probs
                dropped = mask.nonzero().flatten().tolist()
                if not dropped and dart["one_drop"]:
                    dropped = [int(torch.randint(n_trees, (1,), generator=generator, device=device))]
            for t in dropped:
                contrib = backend.predict_tree(booster.trees[t], X) * booster.weight_drop[t]
                margin[:, booster.tree_info[t]] -= contrib
                drop_contrib[t] = contrib

        gh = objective.gradients(margin.squeeze(1) if n_outputs == 1 else margin, y, weight)

        if booster_kind == "gblinear":
            for cls in range(n_outputs):
                gh_cls = gh if n_outputs == 1 else gh[:, cls, :].contiguous()
                delta = linear_updater.update_round(booster.linear_model, X, gh_cls, cls)
                margin[:, cls] += delta
            booster.add_iteration([], [])
            for es in eval_sets:
                if not es.is_train:
                    es.margin = (
                        torch.nan_to_num(es.X, nan=0.0) @ booster.linear_model.weights
                        + booster.linear_model.bias
                        + float(base_margin_value)
                    )
        else:
            # dart scaling factors for this round's new trees
            k_drop = len(dropped)
            if dart is not None and k_drop > 0:
                lr = dart["eta"]
                if dart["normalize_type"] == "forest":
                    new_tree_scale = 1.0 / (1.0 + lr)
                    dropped_factor = 1.0 / (1.0 + lr)
                else:
                    new_tree_scale = 1.0 / (k_drop + lr)
                    dropped_factor = k_drop / (k_drop + lr)
            else:
                new_tree_scale = 1.0
                dropped_factor = 1.0

            round_trees = []
            round_info = []
            # A round's trees (one per class) all derive from the same margin
            # state, so they are independent: on the device path they are
            # enqueued back-to-back (per-class buffer slots) and drained in
            # order — the GPU never idles while the host builds tree objects.
            pipeline_classes = (
                n_outputs > 1
                and dart is None
                and hasattr(grower, "device_async_ok")
                and grower.device_async_ok()
            )
            if adaptive is not None:
                # every tree of the round takes its residuals from the
                # margin the round began with
                round_margin = margin.clone() if num_parallel_tree > 1 else margin
            for _parallel in range(num_parallel_tree):
                if pipeline_classes:
                    handles = [
                        grower.grow_async(gh[:, cls, :].contiguous(), slot=cls)
                        for cls in range(n_outputs)
                    ]
                    for cls, handle in enumerate(handles):
                        tree, leaf_jobs = grower.grow_finish(handle)
                        if adaptive is not None:
                            leaf_jobs = adaptive.update(tree, leaf_jobs, grower, round_margin[:, cls], cls)
                        add_tree_to_margin(grower.state, tree, leaf_jobs, cls)
                        round_trees.append(tree)
                        round_info.append(cls)
                        for es in eval_sets:
                            if not es.is_train:
                                es.margin[:, cls] += es.tree_margin(backend, tree)
                    continue
                for cls in range(n_outputs):
                    gh_cls = gh if n_outputs == 1 else gh[:, cls, :].contiguous()
                    tree, leaf_jobs = grower.grow(gh_cls)
                    if adaptive is not None:
                        leaf_jobs = adaptive.update(tree, leaf_jobs, grower, round_margin[:, cls], cls)
                    if new_tree_scale != 1.0:
                        leaf_jobs = [(p_, s_, e_, v_ * new_tree_scale) for p_, s_, e_, v_ in leaf_jobs]
                    add_tree_to_margin(grower.state, tree, leaf_jobs, cls, new_tree_scale)
                    round_trees.append(tree)
                    round_info.append(cls)
                    for es in eval_sets:
                        if not es.is_train:
                            es.margin[:, cls] += es.tree_margin(backend, tree) * new_tree_scale
            # rescale dropped trees and restore their (scaled) contribution
            for t in dropped:
                booster.weight_drop[t] *= dropped_factor
                margin[:, booster.tree_info[t]] += drop_contrib[t] * dropped_factor
            booster.add_iteration(round_trees, round_info, weight_drop=[new_tree_scale] * len(round_trees))
            if dropped:
                # dropped-tree rescaling invalidates the incremental eval
                # margins: recompute them from the booster exactly
                for es in eval_sets:
                    if not es.is_train:
                        es.margin = booster._margin(es.X).reshape(es.X.shape[0], -1).clone()

        # -- evaluation ----------------------------------------------------
        # Each rank evaluates its local shard; native metrics are then
        # aggregated to one identical number on every rank (ONE fused
        # allreduce — exact for ratio-of-sums metrics, per-worker weighted
        # average for rank metrics; the reference gets the same property
        # from rabit inside xgboost). Custom feval metrics stay rank-local,
        # exactly as xgboost's feval does in distributed mode; an empty
        # shard contributes (0 value, 0 mass) so it can't NaN the sums.
        results = []
        masses = []
        feval_results = []
        for es in eval_sets:
            es_margin = margin if es.is_train else es.margin
            m = es_margin.squeeze(1) if n_outputs == 1 else es_margin
            empty = es.y.numel() == 0
            for metric_name in metric_names:
                if empty:
                    results.append((es.name, metric_name, 0.0))
                    masses.append(0.0)
                    continue
                value = evaluate_metric(metric_name, m, es.y, es.w, objective)
                results.append((es.name, metric_name, value))
                masses.append(eval_metrics.metric_mass(metric_name, es.y, es.w, objective))
            if feval is not None and not empty:
                m_np = m.cpu().numpy()
                custom = feval(m_np, es.dmatrix)
                if isinstance(custom, tuple):
                    custom = [custom]
                for metric_name, value in custom:
                    feval_results.append((es.name, metric_name, float(value)))

        if comm is not None and comm.world_size > 1 and results:
            vm = torch.tensor(
                [eval_metrics.to_agg_space(nm, v) * mass for (_, nm, v), mass in zip(results, masses)]
                + masses,
                dtype=torch.float64,
                device=device,
            )
            comm.allreduce_(vm)
            k = len(results)
            results = [
                (ds, nm, eval_metrics.from_agg_space(nm, float(vm[i] / vm[k + i]) if float(vm[k + i]) > 0 else 0.0))
                for i, (ds, nm, _) in enumerate(results)
            ]
        results.extend(feval_results)

        if container.after_iteration(booster, epoch, results):
            break

    booster = container.after_training(booster)

    if evals_result is not None:
        evals_result.update(container.history)
    return booster
