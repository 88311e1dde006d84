"""Training objectives: per-row gradient/hessian + prediction transforms.

Replaces the native objective kernels behind ``xgb.train``.
Math is torch (runs on CPU or ROCm device); the hot scalar objectives
(binary:logistic, reg:squarederror) additionally have a one-pass fused HIP
kernel (grad_fused_kernel) that writes the packed gh AND the |g|/|h| maxima
the fixed-point histogram scale needs — torch needs ~5 HBM passes for the
same work (~250 us/round on the 12.5M-row bench vs ~35 us fused).

Error-message substrings for bad labels intentionally match
constants/xgb_constants.CUSTOMER_ERRORS so algorithm_mode/train.py maps them
to UserError (reference train.py:461-467 behavior).
"""
import json
import math
import os

import torch

from ..constants import xgb_constants as xgbc


def _fused_grad(name, margin, y, weight, scale_pos_weight=1.0):
    """HIP fast path for the hot objectives; None -> caller uses torch."""
    if not margin.is_cuda or os.environ.get("SMXGB_FORCE_TORCH_OPS") == "1":
        return None
    from ..ops import hip as _hip  # raises if the extension is missing on GPU

    return _hip.fused_gradients(name, margin, y, weight, scale_pos_weight)


class Objective:
    """Base: scalar-output objective."""

    name = None
    default_metric = "rmse"
    n_outputs = 1
    # adaptive tree: after a tree of output j is grown, each leaf value is
    # replaced by eta times the adaptive_alphas[j] quantile of its rows'
    # residuals (None: the Newton values stay)
    adaptive_alphas = None

    def __init__(self, params=None):
        self.params = params or {}
        self.scale_pos_weight = float(self.params.get("scale_pos_weight", 1.0))
        self.max_delta_step = float(self.params.get("max_delta_step", 0.0))

    def validate_labels(self, y):
        pass

    def set_info(self, dmatrix, device):
        """Pull auxiliary training info (groups, label bounds) off the DMatrix."""

    def base_margin(self, base_score):
        """Transform base_score (prob/mean space) into raw margin space."""
        return float(base_score)

    def transform(self, margin):
        """Raw margin -> user-facing prediction."""
        return margin

    def gradients(self, margin, y, weight=None):
        """Return (n, 2) float32 [grad, hess] (or (n*k, 2) for multiclass)."""
        raise NotImplementedError


class SquaredError(Objective):
    name = "reg:squarederror"
    default_metric = "rmse"

    def gradients(self, margin, y, weight=None):
        fused = _fused_grad(self.name, margin, y, weight)
        if fused is not None:
            return fused
        g = margin - y
        h = torch.ones_like(margin)
        return _pack(g, h, weight)


class SquaredLogError(Objective):
    name = "reg:squaredlogerror"
    default_metric = "rmsle"

    def validate_labels(self, y):
        if bool((y <= -1).any()):
            raise ValueError("label must be greater than -1 for rmsle")

    def gradients(self, margin, y, weight=None):
        p = torch.clamp(margin, min=-1 + 1e-6)
        t = torch.log1p(p) - torch.log1p(y)
        g = t / (p + 1)
        h = torch.clamp((-t + 1) / (p + 1).pow(2), min=1e-6)
        return _pack(g, h, weight)


class Logistic(Objective):
    """binary:logistic — logloss on sigmoid(margin)."""

    name = "binary:logistic"
    default_metric = "logloss"
    prob_output = True

    def validate_labels(self, y):
        if bool(((y < 0) | (y > 1)).any()):
            raise ValueError(xgbc.LOGISTIC_REGRESSION_LABEL_RANGE_ERROR)

    def base_margin(self, base_score):
        if not (0.0 < base_score < 1.0):
            raise ValueError(xgbc.BASE_SCORE_RANGE_ERROR)
        return math.log(base_score / (1.0 - base_score))

    def transform(self, margin):
        return torch.sigmoid(margin)

    def gradients(self, margin, y, weight=None):
        fused = _fused_grad(self.name, margin, y, weight, self.scale_pos_weight)
        if fused is not None:
            return fused
        p = torch.sigmoid(margin)
        g = p - y
        h = torch.clamp(p * (1 - p), min=1e-16)
        if self.scale_pos_weight != 1.0:
            w = torch.where(y == 1.0, torch.full_like(y, self.scale_pos_weight), torch.ones_like(y))
            g = g * w
            h = h * w
        return _pack(g, h, weight)


class RegLogistic(Logistic):
    name = "reg:logistic"
    default_metric = "rmse"

    def validate_labels(self, y):
        pass  # regression on [0,1] targets; no strict label check


class LogitRaw(Logistic):
    name = "binary:logitraw"
    default_metric = "logloss"
    prob_output = False

    def transform(self, margin):
        return margin


class Hinge(Objective):
    name = "binary:hinge"
    default_metric = "error"

    def base_margin(self, base_score):
        return float(base_score)

    def transform(self, margin):
        return (margin > 0).to(margin.dtype)

    def gradients(self, margin, y, weight=None):
        yy = 2.0 * y - 1.0  # {0,1} -> {-1,1}
        active = margin * yy < 1.0
        g = torch.where(active, -yy, torch.zeros_like(margin))
        h = torch.where(active, torch.ones_like(margin), torch.ones_like(margin))
        return _pack(g, h, weight)


class Poisson(Objective):
    name = "count:poisson"
    default_metric = "poisson-nloglik"

    def __init__(self, params=None):
        super().__init__(params)
        if self.max_delta_step == 0.0:
            self.max_delta_step = 0.7

    def validate_labels(self, y):
        if bool((y < 0).any()):
            raise ValueError(xgbc.POISSON_REGRESSION_ERROR)

    def base_margin(self, base_score):
        return math.log(max(base_score, 1e-16))

    def transform(self, margin):
        return torch.exp(margin)

    def gradients(self, margin, y, weight=None):
        mu = torch.exp(margin)
        g = mu - y
        h = mu * math.exp(self.max_delta_step)
        return _pack(g, h, weight)


class Gamma(Objective):
    name = "reg:gamma"
    default_metric = "gamma-nloglik"

    def validate_labels(self, y):
        if bool((y <= 0).any()):
            raise ValueError("label must be positive for gamma regression")

    def base_margin(self, base_score):
        return math.log(max(base_score, 1e-16))

    def transform(self, margin):
        return torch.exp(margin)

    def gradients(self, margin, y, weight=None):
        mu = torch.exp(margin)
        g = 1.0 - y / mu
        h = y / mu
        return _pack(g, h, weight)


class Tweedie(Objective):
    name = "reg:tweedie"
    default_metric = "tweedie-nloglik"

    def __init__(self, params=None):
        super().__init__(params)
        self.rho = float(self.params.get("tweedie_variance_power", 1.5))

    def validate_labels(self, y):
        if bool((y < 0).any()):
            raise ValueError(xgbc.TWEEDIE_REGRESSION_ERROR)

    def base_margin(self, base_score):
        return math.log(max(base_score, 1e-16))

    def transform(self, margin):
        return torch.exp(margin)

    def gradients(self, margin, y, weight=None):
        rho = self.rho
        e1 = torch.exp((1 - rho) * margin)
        e2 = torch.exp((2 - rho) * margin)
        g = -y * e1 + e2
        h = -y * (1 - rho) * e1 + (2 - rho) * e2
        return _pack(g, torch.clamp(h, min=1e-16), weight)


class PseudoHuber(Objective):
    name = "reg:pseudohubererror"
    default_metric = "mphe"

    def __init__(self, params=None):
        super().__init__(params)
        self.slope = float(self.params.get("huber_slope", 1.0))

    def gradients(self, margin, y, weight=None):
        z = margin - y
        d = self.slope
        scale = torch.sqrt(1 + (z / d) ** 2)
        g = z / scale
        h = 1.0 / scale.pow(3)
        return _pack(g, h, weight)


class AbsoluteError(Objective):
    """reg:absoluteerror. The gradients only shape the tree; its leaves are
    then the median residual of their rows (adaptive_alphas)."""

    name = "reg:absoluteerror"
    default_metric = "mae"
    adaptive_alphas = [0.5]

    def gradients(self, margin, y, weight=None):
        g = torch.sign(margin - y)
        h = torch.ones_like(margin)
        return _pack(g, h, weight)


def parse_quantile_alpha(value):
    """quantile_alpha as a list of floats in (0, 1): a number, a list of
    numbers, or the string form of either ("0.5", "[0.1, 0.9]", the JSON
    array string a model file stores)."""
    if isinstance(value, str):
        text = value.strip()
        try:
            value = json.loads(text) if text.startswith("[") else float(text)
        except ValueError:
            raise ValueError(f"quantile_alpha must be a number or a list of numbers, got {value!r}")
    if isinstance(value, (list, tuple)) or (hasattr(value, "tolist") and getattr(value, "ndim", 0) > 0):
        items = list(value)
    else:
        items = [value]
    if not items:
        raise ValueError("quantile_alpha must not be empty")
    alphas = []
    for item in items:
        if isinstance(item, bool) or isinstance(item, str):
            raise ValueError(f"quantile_alpha must hold numbers, got {item!r}")
        try:
            a = float(item)
        except (TypeError, ValueError):
            raise ValueError(f"quantile_alpha must hold numbers, got {item!r}")
        if not (0.0 < a < 1.0):  # also refuses NaN
            raise ValueError(f"quantile_alpha must lie in (0, 1), got {item!r}")
        alphas.append(a)
    return alphas


class QuantileError(Objective):
    """reg:quantileerror — pinball loss, one output per quantile_alpha. The
    leaves of output j are the alpha_j quantile of their rows' residuals
    (adaptive_alphas)."""

    name = "reg:quantileerror"
    default_metric = "quantile"

    def __init__(self, params=None):
        super().__init__(params)
        if "quantile_alpha" not in self.params:
            raise ValueError("reg:quantileerror needs quantile_alpha")
        self.alphas = parse_quantile_alpha(self.params["quantile_alpha"])
        self.adaptive_alphas = self.alphas
        self.n_outputs = len(self.alphas)

    def gradients(self, margin, y, weight=None):
        # margin: (n,) or (n, k); returns (n, 2) or (n, k, 2)
        k = self.n_outputs
        m = margin.reshape(-1, k)
        alpha = torch.tensor(self.alphas, dtype=torch.float32, device=m.device)
        g = torch.where(m >= y.reshape(-1, 1), 1.0 - alpha, -alpha).to(torch.float32)
        h = torch.ones_like(g)
        gh = torch.stack([g, h], dim=-1)
        if weight is not None and weight.numel():
            gh = gh * weight.reshape(-1, 1, 1)
        return gh[:, 0, :].contiguous() if k == 1 else gh


class Softmax(Objective):
    """multi:softprob / multi:softmax — per-class gradients."""

    name = "multi:softprob"
    default_metric = "mlogloss"

    def __init__(self, params=None):
        super().__init__(params)
        self.num_class = int(self.params.get("num_class", 0))
        if self.num_class < 2:
            raise ValueError("num_class must be >= 2 for multi-class objectives")
        self.n_outputs = self.num_class

    def validate_labels(self, y):
        if bool(((y < 0) | (y >= self.num_class)).any()):
            raise ValueError(xgbc.MULTI_CLASS_LABEL_RANGE_ERROR)

    def base_margin(self, base_score):
        return float(base_score)

    def transform(self, margin):
        return torch.softmax(margin, dim=-1)

    def gradients(self, margin, y, weight=None):
        # margin: (n, k); returns (n, k, 2)
        p = torch.softmax(margin, dim=-1)
        onehot = torch.nn.functional.one_hot(y.long(), self.num_class).to(p.dtype)
        g = p - onehot
        h = torch.clamp(2.0 * p * (1.0 - p), min=1e-16)
        gh = torch.stack([g, h], dim=-1)
        if weight is not None and weight.numel():
            gh = gh * weight.reshape(-1, 1, 1)
        return gh


class SoftmaxLabel(Softmax):
    name = "multi:softmax"
    default_metric = "merror"

    def transform(self, margin):
        return margin.argmax(dim=-1).to(torch.float32)


class SquaredErrorLegacy(SquaredError):
    name = "reg:linear"


class _RankObjective(Objective):
    """LambdaMART-style pairwise ranking base.

    Groups come from the DMatrix (qid / set_group); absent group info treats
    the whole dataset as one query (xgboost behavior)."""

    default_metric = "map"

    def __init__(self, params=None):
        super().__init__(params)
        self.group_ptr = None  # (G+1,) int64 boundaries

    def set_info(self, dmatrix, device):
        group = dmatrix.get_group() if hasattr(dmatrix, "get_group") else None
        if group is not None:
            import numpy as np

            ptr = np.concatenate([[0], np.cumsum(group)])
            self.group_ptr = torch.as_tensor(ptr, dtype=torch.long, device=device)
        else:
            self.group_ptr = None

    def _pair_weight(self, y, margin, i, j, g_start, g_end):
        return torch.ones_like(y[i])

    def gradients(self, margin, y, weight=None):
        n = margin.shape[0]
        device = margin.device
        grad = torch.zeros_like(margin)
        hess = torch.zeros_like(margin)
        if self.group_ptr is None:
            bounds = [(0, n)]
        else:
            ptr = self.group_ptr.tolist()
            bounds = list(zip(ptr[:-1], ptr[1:]))
        for g_start, g_end in bounds:
            m = g_end - g_start
            if m < 2:
                continue
            # sample one partner per doc (num_pairsample=1 default)
            perm = torch.randperm(m, device=device) + g_start
            base = torch.arange(g_start, g_end, device=device)
            yi, yj = y[base], y[perm]
            keep = yi != yj
            if not bool(keep.any()):
                continue
            i = torch.where(yi > yj, base, perm)[keep]
            j = torch.where(yi > yj, perm, base)[keep]
            s = margin[i] - margin[j]
            rho = torch.sigmoid(-s)  # 1/(1+e^s)
            w = self._pair_weight(y, margin, i, j, g_start, g_end)
            grad.index_add_(0, i, -rho * w)
            grad.index_add_(0, j, rho * w)
            h = torch.clamp(rho * (1 - rho) * w, min=1e-16)
            hess.index_add_(0, i, h)
            hess.index_add_(0, j, h)
        return _pack(grad, torch.clamp(hess, min=1e-16), weight)


class RankPairwise(_RankObjective):
    name = "rank:pairwise"


class RankNDCG(_RankObjective):
    name = "rank:ndcg"
    default_metric = "ndcg"

    def _pair_weight(self, y, margin, i, j, g_start, g_end):
        # |ΔNDCG| of swapping i and j at current ranking
        seg = slice(g_start, g_end)
        order = torch.argsort(margin[seg], descending=True)
        rank = torch.empty_like(order)
        rank[order] = torch.arange(order.numel(), device=margin.device)
        disc = 1.0 / torch.log2(rank.float() + 2.0)
        gain = torch.pow(2.0, y[seg]) - 1.0
        idcg = (torch.sort(gain, descending=True).values * 1.0 /
                torch.log2(torch.arange(gain.numel(), device=margin.device).float() + 2.0)).sum()
        idcg = torch.clamp(idcg, min=1e-16)
        gi, gj = torch.pow(2.0, y[i]) - 1.0, torch.pow(2.0, y[j]) - 1.0
        di, dj = disc[i - g_start], disc[j - g_start]
        return torch.abs((gi - gj) * (di - dj)) / idcg


class RankMAP(_RankObjective):
    name = "rank:map"
    default_metric = "map"


class SurvivalCox(Objective):
    """Cox proportional hazards (Breslow); label > 0 = event time,
    label < 0 = right-censored at |label|."""

    name = "survival:cox"
    default_metric = "cox-nloglik"

    def base_margin(self, base_score):
        return 0.0

    def transform(self, margin):
        return torch.exp(margin)

    def gradients(self, margin, y, weight=None):
        t = y.abs()
        event = (y > 0).to(margin.dtype)
        order = torch.argsort(t)  # ascending time
        m_s = margin[order].to(torch.float64)
        e_s = event[order].to(torch.float64)
        exp_m = torch.exp(m_s)
        # risk set sum for each i: sum of exp(m_j) with t_j >= t_i
        risk = torch.flip(torch.cumsum(torch.flip(exp_m, [0]), 0), [0])
        risk = torch.clamp(risk, min=1e-16)
        s1 = torch.cumsum(e_s / risk, 0)
        s2 = torch.cumsum(e_s / (risk * risk), 0)
        grad_s = -e_s + exp_m * s1
        hess_s = exp_m * s1 - exp_m * exp_m * s2
        grad = torch.empty_like(grad_s)
        hess = torch.empty_like(hess_s)
        grad[order] = grad_s
        hess[order] = hess_s
        return _pack(grad.to(torch.float32), torch.clamp(hess, min=1e-16).to(torch.float32), weight)


class SurvivalAFT(Objective):
    """Accelerated failure time with interval censoring.

    Label bounds via DMatrix.set_float_info('label_lower_bound'/'label_upper_bound');
    a plain label means uncensored. Gradients/diag-hessians via autograd on
    the exact per-row negative log likelihood.
    """

    name = "survival:aft"
    default_metric = "aft-nloglik"

    def __init__(self, params=None):
        super().__init__(params)
        self.dist = self.params.get("aft_loss_distribution", "normal")
        self.sigma = float(self.params.get("aft_loss_distribution_scale", 1.0))
        self.lower = None
        self.upper = None

    def set_info(self, dmatrix, device):
        lo = dmatrix.get_float_info("label_lower_bound") if hasattr(dmatrix, "get_float_info") else None
        hi = dmatrix.get_float_info("label_upper_bound") if hasattr(dmatrix, "get_float_info") else None
        self.lower = None if lo is None else torch.as_tensor(lo, dtype=torch.float64, device=device)
        self.upper = None if hi is None else torch.as_tensor(hi, dtype=torch.float64, device=device)

    def base_margin(self, base_score):
        import math

        return math.log(max(base_score, 1e-16))

    def transform(self, margin):
        return torch.exp(margin)

    def _log_cdf(self, z):
        if self.dist == "normal":
            return torch.log(torch.clamp(0.5 * (1 + torch.erf(z / 1.4142135623730951)), min=1e-300))
        if self.dist == "logistic":
            return torch.nn.functional.logsigmoid(z)
        # extreme (Gumbel minimum): F(z) = 1 - exp(-exp(z))
        return torch.log(torch.clamp(1.0 - torch.exp(-torch.exp(z)), min=1e-300))

    def _log_pdf(self, z):
        if self.dist == "normal":
            return -0.5 * z * z - 0.9189385332046727
        if self.dist == "logistic":
            return z - 2.0 * torch.nn.functional.softplus(z)
        return z - torch.exp(z)

    def nloglik(self, margin, lower, upper):
        sigma = self.sigma
        uncensored = torch.isfinite(upper) & (lower == upper)
        z_lo = (torch.log(torch.clamp(lower, min=1e-16)) - margin) / sigma
        loss_unc = -(self._log_pdf(z_lo) - torch.log(torch.tensor(sigma, dtype=margin.dtype, device=margin.device)))
        z_hi = torch.where(
            torch.isfinite(upper), (torch.log(torch.clamp(upper, min=1e-16)) - margin) / sigma,
            torch.full_like(margin, 50.0),
        )
        cdf_hi = torch.exp(self._log_cdf(z_hi))
        cdf_lo = torch.where(lower > 0, torch.exp(self._log_cdf(z_lo)), torch.zeros_like(margin))
        loss_cen = -torch.log(torch.clamp(cdf_hi - cdf_lo, min=1e-12))
        return torch.where(uncensored, loss_unc, loss_cen)

    def gradients(self, margin, y, weight=None):
        device = margin.device
        if self.lower is not None:
            lower = self.lower
            upper = self.upper if self.upper is not None else torch.full_like(lower, float("inf"))
        else:
            lower = y.to(torch.float64)
            upper = y.to(torch.float64)
        m = margin.detach().to(torch.float64).requires_grad_(True)
        loss = self.nloglik(m, lower, upper).sum()
        (g,) = torch.autograd.grad(loss, m, create_graph=True)
        (h,) = torch.autograd.grad(g.sum(), m)
        g = g.detach().to(torch.float32)
        h = torch.clamp(h.detach(), min=1e-6).to(torch.float32)
        return _pack(g, h, weight)


OBJECTIVES = {
    cls.name: cls
    for cls in (
        SquaredError,
        SquaredErrorLegacy,
        SquaredLogError,
        Logistic,
        RegLogistic,
        LogitRaw,
        Hinge,
        Poisson,
        Gamma,
        Tweedie,
        PseudoHuber,
        AbsoluteError,
        QuantileError,
        Softmax,
        SoftmaxLabel,
        RankPairwise,
        RankNDCG,
        RankMAP,
        SurvivalCox,
        SurvivalAFT,
    )
}


def _pack(g, h, weight):
    if weight is not None and weight.numel():
        g = g * weight
        h = h * weight
    return torch.stack([g.to(torch.float32), h.to(torch.float32)], dim=-1)


def create_objective(name, params=None):
    name = name or "reg:squarederror"
    if name not in OBJECTIVES:
        raise NotImplementedError(f"Objective '{name}' is not implemented yet")
    return OBJECTIVES[name](params)
