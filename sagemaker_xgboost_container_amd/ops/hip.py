"""CDNA4 HIP ops backend (MI355X compute path).

Wraps the in-tree extension built from csrc/smxgb_kernels.hip. Implements
the same segment-based interface as ops/torch_ref.py. Host code here only
PACKS work descriptors (job tables, block->job maps) — all per-row compute
runs in the HIP kernels.

This module raises ImportError loudly when the extension is missing: on a
GPU box the HIP path must run — there is no silent eager fallback
(set SMXGB_FORCE_TORCH_OPS=1 explicitly for ablation).
"""
import math

import numpy as np
import torch

from . import torch_ref

NAME = "hip"
# models/grower.py: the per-level depthwise loop on this backend uses the
# DeviceGrower's float32 root / node-sum arithmetic
MIRRORS_DEVICE_GROWER = True

try:
    from . import _smxgb_hip as _K  # built in-tree by setup.py build_ext --inplace
except ImportError as _e:  # pragma: no cover - exercised only on GPU boxes
    raise ImportError(
        "smxgb HIP extension is not built. Run `python setup.py build_ext --inplace` "
        f"(hipcc, PYTORCH_ROCM_ARCH=gfx950). Underlying error: {_e}"
    )

# fixed-point scale: values mapped to v * 2^33 / max_abs; sums of up to ~5e8
# rows stay inside int64 with 2^29 headroom.
_FIXED_BITS = 33.0

import os as _os

# LDS histogram slab per feature group (56 KiB -> 2 blocks/CU co-residency).
# Env-tunable for measured sweeps (SMXGB_LDS_KB / SMXGB_ROWS_PER_BLOCK).
_LDS_BYTES = int(_os.environ.get("SMXGB_LDS_KB", "56")) * 1024
# measured sweep (profiles/r01_optimization_log.md): 4096-row blocks with a
# 2048 cap keep every CU fed at the deep levels
_ROWS_PER_BLOCK = int(_os.environ.get("SMXGB_ROWS_PER_BLOCK", "4096"))
_MAX_BLOCKS_PER_JOB = int(_os.environ.get("SMXGB_MAX_BLOCKS", "2048"))


def compute_scale(gh, comm=None):
    """Device-resident (gmax, hmax); kernels derive 2^33/max on device —
    no host synchronization per tree. `fused_gradients` attaches the absmax
    it computed in its single pass; recompute only when absent."""
    m = getattr(gh, "_smxgb_absmax", None)
    if m is None:
        m = gh.abs().amax(dim=0).contiguous()  # (2,)
    if comm is not None:
        comm.allreduce_max_(m)
    return m


_GRAD_GRID = 2048
_FUSED_GRAD_MODES = {
    "binary:logistic": 0,
    "reg:logistic": 0,
    "binary:logitraw": 0,  # same gradient formula; only transform() differs
    "reg:squarederror": 1,
}


def fused_gradients(name, margin, y, weight=None, scale_pos_weight=1.0):
    """One-pass gradient + absmax for the hot objectives (grad_fused_kernel).

    Returns the packed (n, 2) gh tensor with `_smxgb_absmax` attached, or
    None when the objective/layout is unsupported (caller falls back to the
    torch path).
    """
    mode = _FUSED_GRAD_MODES.get(name)
    if mode is None or not margin.is_cuda or margin.dim() != 1:
        return None
    margin = margin.contiguous()
    n = margin.numel()
    gh = torch.empty((n, 2), dtype=torch.float32, device=margin.device)
    pmax = torch.empty((_GRAD_GRID, 2), dtype=torch.float32, device=margin.device)
    psum = torch.empty((_GRAD_GRID, 2), dtype=torch.float64, device=margin.device)
    w = (
        weight.contiguous()
        if (weight is not None and weight.numel())
        else torch.empty(0, dtype=torch.float32, device=margin.device)
    )
    _K.grad_fused(margin, y.contiguous(), w, gh, pmax, psum, mode, float(scale_pos_weight))
    gh._smxgb_absmax = pmax.amax(dim=0).contiguous()
    # deterministic full-data (G, H): fixed per-block partial order + one
    # torch sum over the 2048 partials
    gh._smxgb_rootsum = psum.sum(dim=0)
    return gh


# int64 words of the sampler's scratch: 4 radix passes x 256 buckets x
# (count, significand sum), then 4 words of select state
_MVS_WORK_WORDS = 4 * 256 * 2 + 4
_MVS_APPLY_GRID = 2048


def mvs_threshold(gh, S):
    """Threshold mu of gradient-based sampling for (n, 2) float32 gradients
    and a real sample size S, as a float32 [1] device tensor (no readback):
    the radix select of csrc/smxgb_sampling.hip, bit-deterministic."""
    gh = gh.to(torch.float32).contiguous()
    work = torch.zeros(_MVS_WORK_WORDS, dtype=torch.int64, device=gh.device)
    mu = torch.empty(1, dtype=torch.float32, device=gh.device)
    _K.mvs_threshold(gh, float(S), work, mu)
    return mu


def gradient_sample(gh, subsample, u):
    """Gradient-based row sample (see torch_ref.gradient_sample) on the
    device. The rescaled tensor carries its own `_smxgb_absmax`; the
    unscaled tensor's absmax and root sum do not apply to it."""
    gh = gh.to(torch.float32).contiguous()
    n = gh.shape[0]
    mu = mvs_threshold(gh, float(subsample) * n)
    out = torch.empty_like(gh)
    keep = torch.empty(n, dtype=torch.uint8, device=gh.device)
    blocks = max(1, min((n + 255) // 256, _MVS_APPLY_GRID))
    pmax = torch.empty((blocks, 2), dtype=torch.float32, device=gh.device)
    _K.mvs_apply(gh, u.to(torch.float32).contiguous(), mu, out, keep, pmax)
    out._smxgb_absmax = pmax.amax(dim=0).contiguous()
    rows = keep.nonzero(as_tuple=True)[0].to(torch.int32)
    return rows, out


def leaf_quantile_weight_scale(n, weight_max):
    """Power-of-two fixed-point scale 2^s of the weighted leaf quantile:
    s = 50 - ceil(log2(n)) - e, with weight_max < 2^e. n weights of at most
    weight_max then sum below 2^50, so every int64 sum is also exact as a
    float64."""
    e_n = (max(int(n), 1) - 1).bit_length()
    e_w = math.frexp(float(weight_max))[1] if weight_max > 0 else 0
    return math.ldexp(1.0, 50 - e_n - e_w)


def leaf_quantiles(pos, resid, n_leaves, alpha, weight=None, *, weight_max=None, check=True):
    """Per-leaf (weighted) quantile of `resid` on the device; the rule and
    the float64 reference are torch_ref.leaf_quantiles. Returns (n_leaves,)
    float32, NaN for a leaf without rows (or without weight); nothing is
    read back between the passes of csrc/smxgb_quantile.hip.

    Unweighted results equal the reference bit for bit and do not depend on
    the row order. Weights are summed in int64 fixed point, w -> round(w *
    2^s) with 2^s = leaf_quantile_weight_scale(n, max w): also independent
    of the row order, and exact whenever every w * 2^s is an integer. For
    arbitrary float32 weights a rounded weight is off by at most half a
    unit 2^-s, so the returned value v is a residual of the leaf that
    satisfies the reference's bracket up to slack = n * 2^-s / 2:
        sum(w[resid <= v]) - alpha * W >= -slack  and
        sum(w[resid <  v]) - alpha * W <   slack        (W = the leaf's sum).

    `weight_max` (the largest weight, when the caller knows it) and
    `check=False` (pos and weight already validated) skip the host checks,
    which cost a synchronization before the first launch.
    """
    n_leaves = int(n_leaves)
    alpha = float(alpha)
    if not (0.0 < alpha < 1.0):
        raise ValueError("alpha must be in (0, 1)")
    if n_leaves < 1 or n_leaves >= 1 << 22:
        raise ValueError("n_leaves must be in [1, 2^22)")
    if not pos.is_cuda or pos.dtype != torch.int32 or pos.dim() != 1:
        raise ValueError("pos must be a 1-d int32 ROCm device tensor")
    n = pos.numel()
    if resid.shape != pos.shape or resid.dtype != torch.float32 or resid.device != pos.device:
        raise ValueError("resid must be a float32 tensor of pos's shape on its device")
    weighted = weight is not None and weight.numel() > 0
    if weighted and (weight.shape != pos.shape or weight.device != pos.device):
        raise ValueError("weight must match pos")
    dev = pos.device
    out = torch.full((n_leaves,), float("nan"), dtype=torch.float32, device=dev)
    if n == 0:
        return out
    pos = pos.contiguous()
    resid = resid.contiguous()
    w = weight.to(torch.float32).contiguous() if weighted else torch.empty(0, dtype=torch.float32, device=dev)
    if check or (weighted and weight_max is None):
        lim = [pos.max().to(torch.float64), pos.min().to(torch.float64)]
        if weighted:
            lim += [w.max().to(torch.float64), w.min().to(torch.float64)]
        lim = torch.stack(lim).tolist()  # the one synchronization, before any launch
        if lim[0] >= n_leaves or lim[1] < -1:
            raise ValueError(f"pos must lie in [-1, {n_leaves}): found [{int(lim[1])}, {int(lim[0])}]")
        if weighted:
            if not (math.isfinite(lim[2]) and lim[3] >= 0.0):
                raise ValueError("weights must be finite and non-negative")
            weight_max = lim[2]
    scale = leaf_quantile_weight_scale(n, weight_max) if weighted else 1.0
    i64 = dict(dtype=torch.int64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    none64 = torch.empty(0, **i64)
    cnt = torch.zeros(n_leaves, **i32)
    wtot = torch.zeros(n_leaves, **i64) if weighted else none64
    _K.leaf_quantile_count(pos, w, scale, cnt, wtot)
    off = torch.cumsum(cnt, 0, dtype=torch.int64) - cnt  # exclusive scan, on the device
    cursor = torch.zeros(n_leaves, **i32)
    keys = torch.empty(n, **i32)
    seg = torch.empty(n, **i32)
    wq = torch.empty(n, **i64) if weighted else none64
    _K.leaf_quantile_scatter(pos, resid, w, scale, off, cursor, keys, seg, wq)
    table = torch.zeros(n_leaves * 256, **i64)
    state32 = torch.empty(3 * n_leaves, **i32)
    target = torch.empty(n_leaves, **i64)
    frac = torch.empty(n_leaves, dtype=torch.float64, device=dev)
    _K.leaf_quantile_select(keys, seg, wq, off, cnt, wtot, alpha, table, state32, target, frac, out)
    return out


def _padded_words(pairs):
    """LDS u64 words for `pairs` histogram slots incl. bank-skew padding."""
    return (pairs + (pairs >> 3) + 1) * 2


def _feature_groups(nfeat, stride):
    # 18 bytes per slot effective (16 + 1/8 padding)
    per_group = max(1, min(nfeat, (_LDS_BYTES // 18) // max(stride, 1)))
    groups = []
    f = 0
    while f < nfeat:
        groups.append((f, min(f + per_group, nfeat)))
        f += per_group
    return groups


def _device_hist_plan(nfeat, stride):
    """Pick the device-grower hist configuration: (groups, lds_words, block).

    A single full-feature slab at 512 threads (1 block/CU = the same 8
    waves as two 256-thread blocks on 56 KB slabs) streams bins/gh ONCE per
    row instead of once per feature group; used whenever the padded slab
    fits the 160 KB LDS. SMXGB_LDS_KB forces the grouped layout for sweeps.
    """
    if not _os.environ.get("SMXGB_LDS_KB"):
        words = _padded_words(nfeat * stride)
        if words * 8 <= 158 * 1024:
            return [(0, nfeat)], words, 512
    groups = _feature_groups(nfeat, stride)
    return groups, _padded_words(max(fe - fs for fs, fe in groups) * stride), 256


def _pack_jobs(fields_list):
    """fields_list: list of tuples of int32 words -> (jobs_dev, width)."""
    arr = np.asarray(fields_list, dtype=np.int32)
    return torch.from_numpy(arr).cuda(non_blocking=True)


def _block_map(blocks_per_job):
    total = int(sum(blocks_per_job))
    bj = np.empty(total, dtype=np.int32)
    ofs = 0
    for j, nb in enumerate(blocks_per_job):
        bj[ofs : ofs + nb] = j
        ofs += nb
    return torch.from_numpy(bj).cuda(non_blocking=True)


def _pack_jobs_and_map(fields_list, blocks_per_job):
    """One fused H2D upload: [job table | block->job map]."""
    width = len(fields_list[0])
    total_blocks = int(sum(blocks_per_job))
    arr = np.empty(len(fields_list) * width + total_blocks, dtype=np.int32)
    jobs_flat = np.asarray(fields_list, dtype=np.int32).reshape(-1)
    arr[: jobs_flat.size] = jobs_flat
    ofs = jobs_flat.size
    for j, nb in enumerate(blocks_per_job):
        arr[ofs : ofs + nb] = j
        ofs += nb
    dev = torch.from_numpy(arr).cuda(non_blocking=True)
    return dev[: jobs_flat.size], dev[jobs_flat.size :]


def build_histograms(qm, gh, rowbuf, jobs, scale):
    f = qm.num_col
    stride = qm.stride
    groups = _feature_groups(f, stride)
    acc = torch.zeros((len(jobs), f * stride, 2), dtype=torch.int64, device=qm.bins.device)

    job_rows = []
    first_block = 0
    packed = []
    blocks_per = []
    for hist_idx, (start, end) in enumerate(jobs):
        rows = end - start
        nb = int(max(1, min((rows + _ROWS_PER_BLOCK - 1) // _ROWS_PER_BLOCK, _MAX_BLOCKS_PER_JOB)))
        for fg_start, fg_end in groups:
            packed.append((start, end, hist_idx, fg_start, fg_end, first_block, nb))
            blocks_per.append(nb)
            first_block += nb
        job_rows.append(rows)

    jobs_dev = _pack_jobs(packed)
    block_job = _block_map(blocks_per)
    lds_words = _padded_words(max((fe - fs) for fs, fe in groups) * stride)
    if isinstance(scale, torch.Tensor):  # device-resident (gmax, hmax)
        gmax, hmax = (float(v) for v in scale.cpu())
        scale = (2.0**_FIXED_BITS / max(gmax, 1e-30), 2.0**_FIXED_BITS / max(hmax, 1e-30))
    _K.hist_build(
        qm.bins, gh.contiguous(), rowbuf, jobs_dev, block_job, acc,
        f, stride, scale[0], scale[1], lds_words,
    )
    return acc


def hist_to_float(acc, scale):
    out = torch.empty(acc.shape, dtype=torch.float32, device=acc.device)
    if isinstance(scale, torch.Tensor):
        _K.hist_convert_dev(acc, out, scale)
    else:
        _K.hist_convert(acc, out, 1.0 / scale[0], 1.0 / scale[1])
    return out


def find_splits(
    hist,
    parent_sum,
    qm,
    reg_lambda=1.0,
    reg_alpha=0.0,
    gamma=0.0,
    min_child_weight=1.0,
    feature_mask=None,
    monotone=None,
    max_cat_to_onehot=4,
    max_cat_threshold=64,
):
    """Fused HIP split scan: 2 kernel launches per level, zero host syncs.

    A matrix with categorical columns (qm.is_cat) adds two launches: the
    category-set scan of those features between the numeric scan and the
    reduce, and the gather of the winners' sets into "cat_bits" [k, 8]
    int32 (torch_ref.find_splits states the rule). Without such a column
    nothing else is launched and only "packed" is returned.

    Falls back to the torch reference when a feature has > 256 real bins
    (max_bin > 256 configurations)."""
    k = hist.shape[0]
    f = qm.num_col
    stride = qm.stride
    if not hasattr(qm, "_nbins_i32"):
        qm._nbins_i32 = qm.nbins.to(torch.int32).contiguous()
    if int(qm._nbins_i32.max()) > 256:
        return torch_ref.find_splits(
            hist, parent_sum, qm, reg_lambda=reg_lambda, reg_alpha=reg_alpha, gamma=gamma,
            min_child_weight=min_child_weight, feature_mask=feature_mask, monotone=monotone,
            max_cat_to_onehot=max_cat_to_onehot, max_cat_threshold=max_cat_threshold,
        )
    if getattr(qm, "is_cat", None) is not None:
        return _find_splits_cat(
            hist, parent_sum, qm, reg_lambda, reg_alpha, gamma, min_child_weight,
            feature_mask, monotone, max_cat_to_onehot, max_cat_threshold,
        )
    device = hist.device
    if feature_mask is None:
        mask = torch.empty(0, dtype=torch.uint8, device=device)
        per_node = 0
    else:
        mask = feature_mask.to(torch.uint8).contiguous()
        per_node = 1 if feature_mask.dim() == 2 else 0
    mono = (
        monotone.to(torch.int8).contiguous()
        if monotone is not None
        else torch.empty(0, dtype=torch.int8, device=device)
    )
    cands = torch.empty((k, f, 5), dtype=torch.float32, device=device)
    out = torch.empty((k, 6), dtype=torch.float32, device=device)
    _K.find_splits(
        hist.contiguous(), parent_sum.contiguous(), qm._nbins_i32, mask, mono, cands, out,
        k, f, stride, 1 if qm.has_missing else 0, per_node,
        reg_lambda, reg_alpha, gamma, min_child_weight,
    )
    return {"packed": out}


def _cat_tables(qm):
    """Per-matrix device tables of the categorical columns: is_cat as uint8
    [f], its complement, and the int32 indices of the set entries."""
    tables = getattr(qm, "_cat_tables", None)
    if tables is None:
        is_cat = qm.is_cat.to(torch.bool)
        tables = (
            is_cat.to(torch.uint8).contiguous(),
            (~is_cat).to(torch.uint8).contiguous(),
            is_cat.nonzero().flatten().to(torch.int32).contiguous(),
        )
        qm._cat_tables = tables
    return tables


def _find_splits_cat(hist, parent_sum, qm, reg_lambda, reg_alpha, gamma, min_child_weight,
                     feature_mask, monotone, max_cat_to_onehot, max_cat_threshold):
    k = hist.shape[0]
    f = qm.num_col
    device = hist.device
    is_cat_u8, not_cat_u8, cat_feats = _cat_tables(qm)
    if feature_mask is None:
        cat_mask = torch.empty(0, dtype=torch.uint8, device=device)
        num_mask = not_cat_u8
        per_node = 0
    else:
        cat_mask = feature_mask.to(torch.uint8).contiguous()
        num_mask = (cat_mask & not_cat_u8).contiguous()  # broadcasts over nodes
        per_node = 1 if feature_mask.dim() == 2 else 0
    mono = (
        monotone.to(torch.int8).contiguous()
        if monotone is not None
        else torch.empty(0, dtype=torch.int8, device=device)
    )
    cands = torch.empty((k, f, 5), dtype=torch.float32, device=device)
    out = torch.empty((k, 6), dtype=torch.float32, device=device)
    cand_bits = torch.empty((k, f, 8), dtype=torch.int32, device=device)
    cat_bits = torch.empty((k, 8), dtype=torch.int32, device=device)
    _K.find_splits_cat(
        hist.contiguous(), parent_sum.contiguous(), qm._nbins_i32, num_mask, per_node,
        cat_mask, per_node, mono, cands, out, is_cat_u8, cat_feats, cand_bits, cat_bits,
        k, f, qm.stride, 1 if qm.has_missing else 0,
        reg_lambda, reg_alpha, gamma, min_child_weight,
        int(max_cat_to_onehot), int(max_cat_threshold),
    )
    return {"packed": out, "cat_bits": cat_bits}


def partition_level(qm, src, dst, segs, feats, split_bins, default_lefts, cat_bits=None):
    """cat_bits: (J, 8) int32 category sets on the device, read for the jobs
    whose split feature is categorical (qm.is_cat)."""
    J = len(segs)
    packed = []
    blocks_per = []
    first_block = 0
    for (start, end), feature, sbin, dl in zip(segs, feats, split_bins, default_lefts):
        rows = end - start
        nb = int(max(1, min((rows + _ROWS_PER_BLOCK - 1) // _ROWS_PER_BLOCK, _MAX_BLOCKS_PER_JOB)))
        packed.append((start, end, int(feature), int(sbin), int(bool(dl)), first_block, nb))
        blocks_per.append(nb)
        first_block += nb
    jobs_dev = _pack_jobs(packed)
    block_job = _block_map(blocks_per)
    counters = torch.zeros((J, 2), dtype=torch.int32, device=src.device)
    missing_bin = qm.stride - 1 if qm.has_missing else -1
    if cat_bits is not None and getattr(qm, "is_cat", None) is not None:
        if tuple(cat_bits.shape) != (J, 8):
            raise ValueError("cat_bits must hold one (8,) category set per job")
        _K.partition_cat(
            qm.bins, src, dst, jobs_dev, block_job, counters, qm.num_col, missing_bin,
            _cat_tables(qm)[0], cat_bits.to(torch.int32).contiguous(),
        )
    else:
        _K.partition(qm.bins, src, dst, jobs_dev, block_job, counters, qm.num_col, missing_bin)
    return counters[:, 0].cpu().tolist()  # the level's single device sync


def update_margins(margin_col, bufs, leaf_jobs):
    if not leaf_jobs:
        return
    packed = []
    blocks_per = []
    first_block = 0
    for parity, start, end, value in leaf_jobs:
        rows = end - start
        nb = int(max(1, min((rows + _ROWS_PER_BLOCK - 1) // _ROWS_PER_BLOCK, _MAX_BLOCKS_PER_JOB)))
        vbits = int(np.float32(value).view(np.int32))
        packed.append((start, end, int(parity), vbits, first_block, nb))
        blocks_per.append(nb)
        first_block += nb
    jobs_dev = _pack_jobs(packed)
    block_job = _block_map(blocks_per)
    _K.leaf_update(bufs[0], bufs[1], margin_col, jobs_dev, block_job, margin_col.stride(0))


class _FlatForest:
    """Trees flattened into device arrays with global node ids."""

    def __init__(self, trees, tree_info, device):
        import numpy as np

        offsets = np.cumsum([0] + [t.num_nodes for t in trees]).astype(np.int32)
        left = np.concatenate([t.left + (t.left >= 0) * offsets[i] for i, t in enumerate(trees)])
        right = np.concatenate([t.right + (t.right >= 0) * offsets[i] for i, t in enumerate(trees)])
        self.left = torch.from_numpy(left.astype(np.int32)).to(device)
        self.right = torch.from_numpy(right.astype(np.int32)).to(device)
        self.feat = torch.from_numpy(np.concatenate([t.feature for t in trees]).astype(np.int32)).to(device)
        self.thresh = torch.from_numpy(np.concatenate([t.threshold for t in trees]).astype(np.float32)).to(device)
        self.defl = torch.from_numpy(
            np.concatenate([t.default_left for t in trees]).astype(np.uint8)
        ).to(device)
        self.value = torch.from_numpy(np.concatenate([t.value for t in trees]).astype(np.float32)).to(device)
        self.tree_root = torch.from_numpy(offsets[:-1]).to(device)
        self.tree_cls = torch.from_numpy(np.asarray(tree_info, dtype=np.int32)).to(device)
        self.tree_max_feature = torch_ref.tree_max_feature(trees)
        self.tree_cls_max = int(max(tree_info, default=0))
        self.n_trees = len(trees)
        self.cat = _flat_cat(trees, device)  # {} for a forest without categorical nodes


def _flat_cat(trees, device):
    """The categorical entries of a flat forest dict: has_cat, cat_slot
    (int32 per node, -1 at a numeric node), cat_table ([n_cat_nodes, 8]
    int32 bit patterns) and cat_max_slot; empty without categorical nodes."""
    has_cat, slot, table = torch_ref.flat_cat_arrays(trees)
    if not has_cat:
        return {}
    return {
        "has_cat": True,
        "cat_slot": torch.from_numpy(slot).to(device),
        "cat_table": torch.from_numpy(table.view(np.int32)).to(device),
        "cat_max_slot": int(slot.max()),
    }


def _predict_chunking(n, T):
    """(n_chunks, trees_per_chunk): split the tree axis so small batches
    still produce >=128k work items (a 1k-row, 500-tree request fills 4
    blocks otherwise — measured 1.36 ms vs the chip's ~0.1 ms)."""
    target = 131072
    n_chunks = int(min(T, max(1, (target + n - 1) // max(n, 1))))
    trees_per_chunk = (T + n_chunks - 1) // n_chunks
    n_chunks = (T + trees_per_chunk - 1) // trees_per_chunk
    return n_chunks, trees_per_chunk


def _run_predict(X, fl, k, t_begin, t_end):
    """Check the arguments on the host (torch_ref.check_predict_args: tree
    range, class ids, width of X), then launch; nothing is launched for a
    refused or an empty request."""
    max_f = torch_ref.check_predict_args(fl, X, k, t_begin, t_end)
    if not X.is_cuda:
        raise ValueError("X must be a 2-d float32 ROCm device tensor")
    n = X.shape[0]
    T = t_end - t_begin
    if T == 0 or n == 0:
        return torch.zeros((n, k), dtype=torch.float32, device=X.device)
    n_chunks, tpc = _predict_chunking(n, T)
    if n_chunks == 1:
        tpc = T
    out = torch.zeros((n_chunks, n, k), dtype=torch.float32, device=X.device)
    args = (
        X.contiguous(), fl["left"], fl["right"], fl["feature"], fl["threshold"],
        fl["default_left"], fl["value"], fl["tree_root"], fl["tree_cls"],
        t_begin, t_end, max_f, int(fl["tree_cls_max"]), out, k, n_chunks, tpc,
    )
    if fl.get("has_cat"):
        _K.predict_forest_cat(*args, fl["cat_slot"], fl["cat_table"], fl["cat_max_slot"])
    else:
        _K.predict_forest(*args)
    # fixed-order reduce over the chunk axis: deterministic
    return out.sum(0) if n_chunks > 1 else out[0]


def predict_forest(trees, tree_info, X, k, t_begin=0, t_end=None, out=None):
    """Summed margin contributions of trees[t_begin:t_end] -> (n, k)."""
    forest = _FlatForest(trees, tree_info, X.device)
    if t_end is None:
        t_end = forest.n_trees
    fl = {
        "left": forest.left, "right": forest.right, "feature": forest.feat,
        "threshold": forest.thresh, "default_left": forest.defl, "value": forest.value,
        "tree_root": forest.tree_root, "tree_cls": forest.tree_cls,
        "tree_max_feature": forest.tree_max_feature, "tree_cls_max": forest.tree_cls_max,
        "n_trees": forest.n_trees, **forest.cat,
    }
    res = _run_predict(X, fl, k, t_begin, t_end)
    if out is not None:
        out += res
        return out
    return res


def predict_tree(tree, X):
    out = predict_forest([tree], [0], X, 1)
    return out[:, 0]


def make_flat_forest(trees, tree_info, weight_drop, device):
    """Flatten trees for the HIP forest kernel (int32 ids, u8 default-left)."""
    offsets = np.cumsum([0] + [t.num_nodes for t in trees]).astype(np.int32)
    left = np.concatenate([t.left + (t.left >= 0) * offsets[i] for i, t in enumerate(trees)])
    right = np.concatenate([t.right + (t.right >= 0) * offsets[i] for i, t in enumerate(trees)])
    value = np.concatenate(
        [t.value * (weight_drop[i] if weight_drop else 1.0) for i, t in enumerate(trees)]
    ).astype(np.float32)
    return {
        "left": torch.from_numpy(left.astype(np.int32)).to(device),
        "right": torch.from_numpy(right.astype(np.int32)).to(device),
        "feature": torch.from_numpy(np.concatenate([t.feature for t in trees]).astype(np.int32)).to(device),
        "threshold": torch.from_numpy(np.concatenate([t.threshold for t in trees]).astype(np.float32)).to(device),
        "default_left": torch.from_numpy(
            np.concatenate([t.default_left for t in trees]).astype(np.uint8)
        ).to(device),
        "value": torch.from_numpy(value).to(device),
        "tree_root": torch.from_numpy(offsets[:-1]).to(device),
        "tree_cls": torch.from_numpy(np.asarray(tree_info, dtype=np.int32)).to(device),
        "cover": torch.from_numpy(
            np.concatenate([np.asarray(t.sum_hess, dtype=np.float32) for t in trees])
        ).to(device),
        # largest split feature per tree (-1 for a stump): lets the forest
        # launchers reject a too-narrow X without a device round trip
        "tree_max_feature": torch_ref.tree_max_feature(trees),
        # largest class id: the CSR forest launcher checks it against k
        "tree_cls_max": int(max(tree_info, default=0)),
        "n_trees": len(trees),
        **_flat_cat(trees, device),
    }


def predict_forest_flat(flat, X, k, t_begin=0, t_end=None):
    """(n, k) float32 summed margins of trees [t_begin, t_end) of a
    make_flat_forest dict over the dense float32 device matrix X."""
    if t_end is None:
        t_end = flat["n_trees"]
    return _run_predict(X, flat, k, t_begin, t_end)


# ---------------------------------------------------------------------------
# Device explanations: path-form exact TreeSHAP (contributions and
# interaction values) and leaf indices. Same signatures as the torch_ref
# host functions; the flat forest must carry the path tables under
# flat["shap_paths"] (make_shap_paths below).
# ---------------------------------------------------------------------------

# device limits (the booster routes to the host path beyond them)
SHAP_MAX_PATH_LEN = 64            # one lane per path element, one wave at most
SHAP_LDS_BUDGET = 48 * 1024       # phi slabs of all lane groups of a block
SHAP_PARTIAL_CAP = 256 << 20      # bytes of per-chunk fp64 partials per launch
_SHAP_BLOCK = 256                 # SHAP_BLOCK in the kernel source
_SHAP_TARGET_GROUPS = 32768       # (row, tree-chunk) items wanted per launch


def make_shap_paths(trees, tree_info, weight_drop, device):
    """Path tables (ops/shap_paths.py) uploaded to `device`; the per-tree
    limits stay on the host."""
    from . import shap_paths as _sp

    host = _sp.make_shap_paths(trees, tree_info, weight_drop)
    dev = {
        name: torch.from_numpy(host[name]).to(device)
        for name in (
            "elem_feature", "elem_lo", "elem_hi", "elem_flags", "elem_zero_fraction",
            "path_offset", "path_value", "path_cls", "tree_path_ptr",
        )
    }
    dev["tree_max_len"] = host["tree_max_len"]
    dev["tree_max_feature"] = host["tree_max_feature"]
    dev["n_trees"] = len(trees)
    # the numpy tables: make_shap_slots (compact kernel) is built from them
    dev["host"] = host
    return dev


def shap_group_width(L):
    """Lane-group width: smallest power of two >= the longest path."""
    W = 1
    while W < L:
        W *= 2
    return W


def shap_limits(paths, k, nfeat, t_begin, t_end):
    """(L, max_feature, fits): path-length / feature limits of the tree
    range and whether the contribution kernel's LDS slabs fit."""
    from . import shap_paths as _sp

    L, max_f = _sp.range_limits(paths, t_begin, t_end)
    fits = L <= SHAP_MAX_PATH_LEN
    if fits:
        groups = _SHAP_BLOCK // shap_group_width(L)
        fits = groups * k * (nfeat + 1) * 8 <= SHAP_LDS_BUDGET
    return L, max_f, fits


def _shap_prepare(flat, X, k, t_begin, t_end):
    torch_ref.refuse_categorical(flat, "device TreeSHAP")
    paths = flat.get("shap_paths")
    if paths is None:
        raise ValueError("flat forest carries no path tables (flat['shap_paths'])")
    if t_end is None:
        t_end = paths["n_trees"]
    if not (0 <= t_begin <= t_end <= paths["n_trees"]):
        raise ValueError(f"tree range [{t_begin}, {t_end}) out of bounds")
    if not X.is_cuda or X.dim() != 2 or X.dtype != torch.float32:
        raise ValueError("X must be a 2-d float32 ROCm device tensor")
    X = X.contiguous()
    L, max_f, _ = shap_limits(paths, k, X.shape[1], t_begin, t_end)
    if max_f >= X.shape[1]:
        raise ValueError(
            f"X has {X.shape[1]} columns but the forest splits on feature {max_f}"
        )
    if L > SHAP_MAX_PATH_LEN:
        raise ValueError(f"path length {L} exceeds the device limit {SHAP_MAX_PATH_LEN}")
    return paths, X, t_end, L, max_f


def _shap_tiles(n, T, cell_bytes):
    """Yield (row_start, row_end, n_chunks, trees_per_chunk) so that each
    launch's partial buffer (n_chunks * rows * cell_bytes) stays under
    SHAP_PARTIAL_CAP and small batches still split the tree axis."""
    rows_per_tile = max(1, min(n, SHAP_PARTIAL_CAP // max(cell_bytes, 1)))
    for r0 in range(0, n, rows_per_tile):
        r1 = min(n, r0 + rows_per_tile)
        rows = r1 - r0
        want = max(1, (_SHAP_TARGET_GROUPS + rows - 1) // rows)
        cap = max(1, SHAP_PARTIAL_CAP // (rows * cell_bytes))
        n_chunks = int(min(T, want, cap))
        tpc = (T + n_chunks - 1) // n_chunks
        n_chunks = (T + tpc - 1) // tpc
        yield r0, r1, n_chunks, tpc


def _launch_shap(kernel, paths, X, k, t_begin, t_end, L, max_f, cells):
    n = X.shape[0]
    out = torch.empty((n, cells), dtype=torch.float64, device=X.device)
    W = shap_group_width(L)
    for r0, r1, n_chunks, tpc in _shap_tiles(n, t_end - t_begin, cells * 8):
        Xt = X[r0:r1]
        part = torch.zeros((n_chunks, r1 - r0, cells), dtype=torch.float64, device=X.device)
        kernel(
            Xt, paths["elem_feature"], paths["elem_lo"], paths["elem_hi"],
            paths["elem_flags"], paths["elem_zero_fraction"], paths["path_offset"],
            paths["path_value"], paths["path_cls"], paths["tree_path_ptr"],
            t_begin, t_end, part, k, n_chunks, tpc, W, L, max_f,
        )
        out[r0:r1] = part.sum(0)  # fixed-order reduce: deterministic
    return out


def tree_shap(flat, X, k, t_begin=0, t_end=None):
    """Exact TreeSHAP contributions on the device: (n, k, f+1) float64, bias
    column NOT filled (same contract as torch_ref.tree_shap)."""
    paths, X, t_end, L, max_f = _shap_prepare(flat, X, k, t_begin, t_end)
    n, f = X.shape
    if n == 0 or t_end <= t_begin:
        return torch.zeros((n, k, f + 1), dtype=torch.float64, device=X.device)
    if (_SHAP_BLOCK // shap_group_width(L)) * k * (f + 1) * 8 > SHAP_LDS_BUDGET:
        raise ValueError("phi slab does not fit the LDS budget")
    out = _launch_shap(_K.tree_shap_paths, paths, X, k, t_begin, t_end, L, max_f, k * (f + 1))
    return out.reshape(n, k, f + 1)


def tree_shap_interactions(flat, X, k, t_begin=0, t_end=None):
    """Exact TreeSHAP interaction values on the device: (n, k, f+1, f+1)
    float64. Off-diagonals come from shap_interactions_kernel; the diagonal
    is phi_i - sum_{j != i} phi_int[i, j] from a contributions pass. The
    bias row/column stay zero (the booster fills cell [f, f])."""
    paths, X, t_end, L, max_f = _shap_prepare(flat, X, k, t_begin, t_end)
    n, f = X.shape
    c = f + 1
    if n == 0 or t_end <= t_begin:
        return torch.zeros((n, k, c, c), dtype=torch.float64, device=X.device)
    phi = tree_shap(flat, X, k, t_begin, t_end)
    out = _launch_shap(
        _K.tree_shap_interactions_paths, paths, X, k, t_begin, t_end, L, max_f, k * c * c
    ).reshape(n, k, c, c)
    diag = phi - out.sum(dim=3)
    out.diagonal(dim1=2, dim2=3).copy_(diag)
    return out


# -- compact TreeSHAP: chunk-local phi slots, dense or CSR rows ----------------
# shap_paths_compact_kernel keeps max_c S_c doubles per lane group in LDS
# (S_c = distinct (class, feature) cells of chunk c), so neither f nor k
# bounds it; see csrc/smxgb_shap_compact.hip and shap_paths.make_shap_slots.

def _shap_want_tpc(n, T):
    """trees_per_chunk _shap_tiles would pick for occupancy alone."""
    want = max(1, (_SHAP_TARGET_GROUPS + max(n, 1) - 1) // max(n, 1))
    n_chunks = int(min(T, want))
    return (T + n_chunks - 1) // n_chunks


def shap_compact_plan(paths, f, t_begin, t_end, n):
    """(trees_per_chunk, block) for the compact kernel over `n` rows, or
    None when the range does not fit: the largest uniform trees_per_chunk,
    no larger than what occupancy wants, whose largest chunk keeps
    groups_per_block * max_slots * 8 within SHAP_LDS_BUDGET. When a single
    tree does not fit a 256-thread block the block drops to one wave
    (64 / W groups). `paths` are the host path tables (or the device dict
    that carries them)."""
    from . import shap_paths as _sp

    host = paths.get("host", paths)
    T = t_end - t_begin
    if T <= 0:
        return None
    L, _ = _sp.range_limits(host, t_begin, t_end)
    if L > SHAP_MAX_PATH_LEN:
        return None
    W = shap_group_width(L)
    pairs = _sp.range_pairs(host, f, t_begin, t_end)
    one_tree = _sp.max_chunk_slots(pairs, 1)
    want = _shap_want_tpc(n, T)
    for block in (_SHAP_BLOCK, 64):
        cap = SHAP_LDS_BUDGET // (8 * (block // W))
        if one_tree > cap:
            continue
        for tpc in range(want, 1, -1):
            if _sp.max_chunk_slots(pairs, tpc) <= cap:
                return tpc, block
        return 1, block
    return None


def shap_compact_plan_cached(flat, f, t_begin, t_end, n):
    """shap_compact_plan of flat['shap_paths'], remembered in
    flat['shap_slot_cache'] (the Booster's predict cache) when present."""
    cache = flat.get("shap_slot_cache")
    key = ("plan", f, t_begin, t_end, _shap_want_tpc(n, t_end - t_begin), SHAP_LDS_BUDGET)
    if cache is not None and key in cache:
        return cache[key]
    plan = shap_compact_plan(flat["shap_paths"], f, t_begin, t_end, n)
    if cache is not None:
        cache[key] = plan
    return plan


def _shap_slot_tables(flat, f, t_begin, t_end, tpc, device):
    """Slot tables of (range, trees_per_chunk) on `device`; cached in
    flat['shap_slot_cache'] (the Booster's predict cache) when present."""
    from . import shap_paths as _sp

    cache = flat.get("shap_slot_cache")
    key = ("slots", str(device), f, t_begin, t_end, tpc)
    if cache is not None and key in cache:
        return cache[key]
    host = _sp.make_shap_slots(flat["shap_paths"]["host"], f, t_begin, t_end, tpc)
    # content checks the launcher relies on (it sees only sizes)
    S = int(host["slot_col"].shape[0])
    ptr = host["chunk_slot_ptr"]
    if (
        ptr[0] != 0 or ptr[-1] != S or (np.diff(ptr) < 0).any()
        or (host["elem_slot"] < 0).any()
        or (host["elem_slot"].size and host["elem_slot"].max() >= max(host["max_slots"], 1))
        or (host["col_slots"].size and (host["col_slots"].min() < 0 or host["col_slots"].max() >= S))
        or host["col_ptr"][-1] != S
    ):
        raise ValueError("inconsistent TreeSHAP slot tables")
    tabs = dict(host)
    for name in ("elem_slot", "chunk_slot_ptr", "col_ptr", "col_slots"):
        tabs[name] = torch.from_numpy(host[name]).to(device)
    tabs["cols_dev"] = torch.from_numpy(host["cols"]).to(device)
    tabs["S"] = S
    if cache is not None:
        cache[key] = tabs
    return tabs


def _shap_compact_prepare(flat, X, k, t_begin, t_end):
    """Host-side validation of a compact TreeSHAP request; raises ValueError
    before anything is launched. Returns (paths, t_end, n, f, csr, L, max_f)."""
    from . import hip_sparse as _hs
    from . import shap_paths as _sp

    torch_ref.refuse_categorical(flat, "device TreeSHAP")
    paths = flat.get("shap_paths")
    if paths is None or "host" not in paths:
        raise ValueError("flat forest carries no path tables (flat['shap_paths'])")
    if t_end is None:
        t_end = paths["n_trees"]
    if not (0 <= t_begin <= t_end <= paths["n_trees"]):
        raise ValueError(f"tree range [{t_begin}, {t_end}) out of bounds")
    csr = isinstance(X, _hs.DeviceCSR)
    if csr:
        for name, t, dt in (
            ("indptr", X.indptr, torch.int64), ("indices", X.indices, torch.int32),
            ("data", X.data, torch.float32),
        ):
            if (
                not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dt
                or not t.is_contiguous() or t.dim() != 1
            ):
                raise ValueError(f"device CSR {name} must be a contiguous 1-d {dt} ROCm tensor")
        n, f = int(X.shape[0]), int(X.shape[1])
        nnz = X.indices.numel()
        if X.indptr.numel() != n + 1 or X.data.numel() != nnz:
            raise ValueError("device CSR arrays do not match the matrix shape")
        # offsets against the buffers: a slice's offsets need not start at 0
        lo, hi = (int(v) for v in X.indptr[[0, -1]].tolist())
        if not (0 <= lo <= hi <= nnz) or bool((X.indptr[1:] < X.indptr[:-1]).any()):
            raise ValueError("device CSR offsets leave the index buffer")
        device = X.data.device
    else:
        if (
            not isinstance(X, torch.Tensor) or not X.is_cuda or X.dim() != 2
            or X.dtype != torch.float32
        ):
            raise ValueError("X must be a 2-d float32 ROCm device tensor or a DeviceCSR")
        n, f = X.shape
        device = X.device
    if paths["elem_feature"].device != device:
        raise ValueError("the path tables live on another device than the matrix")
    k = int(k)
    host = paths["host"]
    p0, p1 = int(host["tree_path_ptr"][t_begin]), int(host["tree_path_ptr"][t_end])
    if k < 1 or (p1 > p0 and int(host["path_cls"][p0:p1].max()) >= k):
        raise ValueError(f"k = {k} outputs do not cover the forest's class ids")
    L, max_f = _sp.range_limits(host, t_begin, t_end)
    if max_f >= f:
        raise ValueError(f"the matrix has {f} columns but the forest splits on feature {max_f}")
    if L > SHAP_MAX_PATH_LEN:
        raise ValueError(f"path length {L} exceeds the device limit {SHAP_MAX_PATH_LEN}")
    return paths, t_end, n, f, csr, L, max_f


def tree_shap_compact_tiles(flat, X, k, t_begin=0, t_end=None):
    """Exact TreeSHAP contributions over a dense (n, f) float32 device
    tensor or a hip_sparse.DeviceCSR, one row tile at a time.

    Returns (cols, tiles): `cols` (U,) int64 host array of the dense output
    columns cls * (f + 1) + feature the range touches, sorted; `tiles` a
    generator of (r0, r1, phi) with phi (r1 - r0, U) float64 on the device,
    valid until the next tile is drawn. Rows are tiled so that the slot
    partials rows * S * 8 stay under SHAP_PARTIAL_CAP. The bias column is
    never produced. Everything is validated before the first launch."""
    paths, t_end, n, f, csr, L, max_f = _shap_compact_prepare(flat, X, k, t_begin, t_end)
    empty = np.zeros(0, dtype=np.int64)
    if n == 0 or t_end <= t_begin or max_f < 0:
        return empty, iter(())
    plan = shap_compact_plan_cached(flat, f, t_begin, t_end, n)
    if plan is None:
        raise ValueError("slot slabs do not fit the LDS budget")
    tpc, block = plan
    device = X.data.device if csr else X.device
    tabs = _shap_slot_tables(flat, f, t_begin, t_end, tpc, device)
    S, U = tabs["S"], int(tabs["cols"].shape[0])
    W = shap_group_width(L)
    if not csr:
        X = X.contiguous()
    rows_per_tile = max(1, min(n, SHAP_PARTIAL_CAP // (S * 8)))
    none64 = torch.empty(0, dtype=torch.int64, device=device)
    none32 = torch.empty(0, dtype=torch.int32, device=device)

    def tiles():
        part = torch.empty((rows_per_tile, S), dtype=torch.float64, device=device)
        for r0 in range(0, n, rows_per_tile):
            r1 = min(n, r0 + rows_per_tile)
            rows = r1 - r0
            if csr:
                args = (X.data, X.indptr[r0:r1 + 1], X.indices)
            else:
                args = (X[r0:r1], none64, none32)
            _K.tree_shap_compact(
                *args, rows, f, csr,
                paths["elem_feature"], paths["elem_lo"], paths["elem_hi"],
                paths["elem_flags"], paths["elem_zero_fraction"], paths["path_offset"],
                paths["path_value"], paths["tree_path_ptr"], t_begin, t_end,
                tabs["elem_slot"], tabs["elem_base"], tabs["chunk_slot_ptr"],
                part[:rows], S, tabs["n_chunks"], tpc, W, L, max_f, tabs["max_slots"], block,
            )
            phi = torch.empty((rows, U), dtype=torch.float64, device=device)
            _K.shap_slot_reduce(part[:rows], tabs["col_ptr"], tabs["col_slots"], phi)
            yield r0, r1, phi

    return tabs["cols"], tiles()


def tree_shap_compact(flat, X, k, t_begin=0, t_end=None):
    """Exact TreeSHAP contributions in compact form: (phi, cols) with phi
    (n, U) float64 on the device and cols (U,) int64 the dense output columns
    cls * (f + 1) + feature, sorted. Columns the tree range never splits on
    are absent (their contribution is zero); the bias column is NOT filled
    (same contract as tree_shap). X is a dense float32 device tensor or a
    hip_sparse.DeviceCSR, where an absent entry is a missing value."""
    cols, tiles = tree_shap_compact_tiles(flat, X, k, t_begin, t_end)
    csr = not isinstance(X, torch.Tensor)
    device = X.data.device if csr else X.device
    n = int(X.shape[0])
    phi = torch.empty((n, cols.shape[0]), dtype=torch.float64, device=device)
    for r0, r1, tile in tiles:
        phi[r0:r1] = tile
    return phi, torch.from_numpy(cols).to(device)


def pred_leaf(flat, X, t_begin=0, t_end=None):
    """(n, T) int32 tree-local leaf indices on the device."""
    if t_end is None:
        t_end = flat["n_trees"]
    if not (0 <= t_begin <= t_end <= flat["n_trees"]):
        raise ValueError(f"tree range [{t_begin}, {t_end}) out of bounds")
    if not X.is_cuda or X.dim() != 2 or X.dtype != torch.float32:
        raise ValueError("X must be a 2-d float32 ROCm device tensor")
    X = X.contiguous()
    T = t_end - t_begin
    max_f = int(flat["tree_max_feature"][t_begin:t_end].max()) if T > 0 else -1
    if max_f >= X.shape[1]:
        raise ValueError(
            f"X has {X.shape[1]} columns but the forest splits on feature {max_f}"
        )
    out = torch.zeros((X.shape[0], T), dtype=torch.int32, device=X.device)
    if T > 0 and X.shape[0] > 0:
        args = (
            X, flat["left"], flat["right"], flat["feature"], flat["threshold"],
            flat["default_left"], flat["tree_root"], t_begin, t_end, max_f, out,
        )
        if flat.get("has_cat"):
            _K.pred_leaf_cat(*args, flat["cat_slot"], flat["cat_table"], flat["cat_max_slot"])
        else:
            _K.pred_leaf(*args)
    return out


class TreeState:
    """Per-tree compact-layout state (v2 pipeline).

    Rows live in node-contiguous compact SoA buffers (bins bytes, float2
    gradient pairs, original row ids) that the compacting partition kernel
    ping-pongs between; histogram builds stream them with perfectly
    coalesced loads — no kernel gathers by row id after the root level.
    Level 0 streams the original bin matrix directly (no setup copy) unless
    the tree is row-subsampled.
    """

    def __init__(self, qm, gh, sample_rows=None, slot=0):
        self.qm = qm
        device = qm.bins.device
        n = qm.num_row
        if sample_rows is None:
            cap = n
            rid = getattr(qm, "_arange_cache", None)
            if rid is None or rid.numel() != n:
                rid = torch.arange(n, dtype=torch.int32, device=device)
                qm._arange_cache = rid
            self._rows_init = rid
            self._bins_init = qm.bins
            self._gh_init = gh.contiguous()
        else:
            cap = sample_rows.numel()
            self._rows_init = sample_rows.to(torch.int32)
            idx = sample_rows.long()
            self._bins_init = qm.bins.index_select(0, idx).contiguous()
            self._gh_init = gh.index_select(0, idx).contiguous()
        self.cap = cap
        # `slot` keys independent buffer sets so several trees of one round
        # (multiclass / bagging) can be in flight on the GPU at once
        caches = getattr(qm, "_compact_cache", None)
        if caches is None:
            caches = {}
            qm._compact_cache = caches
        cache = caches.get(slot)
        if cache is None or cache[0].shape[0] < cap:
            cache = (
                torch.empty((cap, qm.num_col), dtype=qm.bins.dtype, device=device),
                torch.empty((cap, qm.num_col), dtype=qm.bins.dtype, device=device),
                torch.empty((cap, 2), dtype=torch.float32, device=device),
                torch.empty((cap, 2), dtype=torch.float32, device=device),
                torch.empty(cap, dtype=torch.int32, device=device),
                torch.empty(cap, dtype=torch.int32, device=device),
            )
            caches[slot] = cache
        self._bins = [cache[0], cache[1]]
        self._gh = [cache[2], cache[3]]
        self._rows = [cache[4], cache[5]]
        self._level0 = True  # parity-0 source is still the original matrix
        # (split heap, depth, leaf heap indices) of a device-grown tree whose
        # margins are updated by traversal; None selects the leaf scatter
        self._traverse = None
        # set by the grower for a gradient-sampled tree: its leaf values go
        # to every training row's margin, not only to the sampled rows'
        self.margin_all_rows = False

    def traverse_ok(self):
        """Margins of this tree can be updated by streaming the original
        bin matrix through the finished tree: a full-data state, or a
        gradient-sampled one (`margin_all_rows`). A uniformly subsampled
        tree must leave the rows it did not see untouched.
        SMXGB_LEAF_UPDATE=scatter keeps the row-id scatter for A/B runs."""
        mode = _os.environ.get("SMXGB_LEAF_UPDATE", "traverse")
        if mode not in ("traverse", "scatter"):
            raise ValueError(f"SMXGB_LEAF_UPDATE must be 'traverse' or 'scatter', got {mode!r}")
        return mode == "traverse" and (self._bins_init is self.qm.bins or self.margin_all_rows)

    def _src(self, parity):
        if parity == 0 and self._level0:
            return self._bins_init, self._gh_init, self._rows_init
        return self._bins[parity], self._gh[parity], self._rows[parity]

    def build_histograms(self, jobs, parity, scale):
        qm = self.qm
        f = qm.num_col
        stride = qm.stride
        bins_c, gh_c, _ = self._src(parity)
        groups = _feature_groups(f, stride)
        acc = torch.zeros((len(jobs), f * stride, 2), dtype=torch.int64, device=bins_c.device)
        packed = []
        blocks_per = []
        first_block = 0
        for hist_idx, (start, end) in enumerate(jobs):
            rows = end - start
            nb = int(max(1, min((rows + _ROWS_PER_BLOCK - 1) // _ROWS_PER_BLOCK, _MAX_BLOCKS_PER_JOB)))
            for fg_start, fg_end in groups:
                packed.append((start, end, hist_idx, fg_start, fg_end, first_block, nb))
                blocks_per.append(nb)
                first_block += nb
        jobs_dev, block_job = _pack_jobs_and_map(packed, blocks_per)
        lds_words = _padded_words(max((fe - fs) for fs, fe in groups) * stride)
        _K.hist_build_compact(
            bins_c, gh_c, jobs_dev, block_job, acc, f, stride, scale, lds_words
        )
        return acc

    def partition_level(self, segs, node_rows, split_packed, src_parity, cat_bits=None):
        """Partition every segment whose on-device split has gain > 0.

        node_rows[i] = row of segs[i] in split_packed ([k, 6] float32 from
        find_splits, still on device — no host round-trip). Returns the
        DEVICE counters tensor [J, 2]; the caller reads it back together
        with the packed splits in one drain. cat_bits ([k, 8] int32, the
        category sets find_splits returned with split_packed) is passed
        for a matrix with categorical columns."""
        qm = self.qm
        src_bins, src_gh, src_rows = self._src(src_parity)
        dst = 1 - src_parity
        packed = []
        blocks_per = []
        first_block = 0
        for (start, end), node_row in zip(segs, node_rows):
            rows = end - start
            nb = int(max(1, min((rows + _ROWS_PER_BLOCK - 1) // _ROWS_PER_BLOCK, _MAX_BLOCKS_PER_JOB)))
            packed.append((start, end, int(node_row), 0, 0, first_block, nb))
            blocks_per.append(nb)
            first_block += nb
        jobs_dev, block_job = _pack_jobs_and_map(packed, blocks_per)
        counters = torch.zeros((len(segs), 2), dtype=torch.int32, device=src_bins.device)
        missing_bin = qm.stride - 1 if qm.has_missing else -1
        args = (
            src_bins, src_gh, src_rows, self._bins[dst], self._gh[dst], self._rows[dst],
            jobs_dev, block_job, split_packed.contiguous(), counters, qm.num_col, missing_bin,
        )
        if cat_bits is not None and getattr(qm, "is_cat", None) is not None:
            if tuple(cat_bits.shape) != (split_packed.shape[0], 8):
                raise ValueError("cat_bits must hold one (8,) category set per split row")
            _K.partition_compact_cat(
                *args, _cat_tables(qm)[0], cat_bits.to(torch.int32).contiguous()
            )
        else:
            _K.partition_compact(*args)
        if src_parity == 0:
            self._level0 = False
        return counters

    def update_margins(self, margin_col, leaf_jobs):
        if not leaf_jobs:
            return
        if self._traverse is not None:
            # the value table is built HERE, from the values the caller
            # passes: DART rescales them after the tree was grown. Leaf i of
            # leaf_jobs sits at heap index leaf_heap[i]; its row range is a
            # placeholder (the deepest level was never partitioned). A root
            # that did not split is just the depth-0 leaf.
            splits, depth, leaf_heap = self._traverse
            assert len(leaf_heap) == len(leaf_jobs)
            table = np.zeros((2 << depth) - 1, dtype=np.float32)
            table[leaf_heap] = np.asarray([job[3] for job in leaf_jobs], dtype=np.float32)
            values = torch.from_numpy(table).to(margin_col.device, non_blocking=True)
            qm = self.qm
            missing_bin = qm.stride - 1 if qm.has_missing else -1
            _K.leaf_update_traverse(
                qm.bins, splits, values, margin_col, depth, missing_bin, margin_col.stride(0)
            )
            return
        # partition_level clears _level0 at the root level without knowing
        # (no host sync) whether the root split. When it did not, the tree is
        # one parity-0 leaf over rows that were never copied into _rows[0]:
        # read the original row ids, not that unwritten buffer.
        root_leaf = len(leaf_jobs) == 1 and tuple(leaf_jobs[0][:3]) == (0, 0, self.cap)
        rows0 = self._rows_init if (self._level0 or root_leaf) else self._rows[0]
        packed = []
        blocks_per = []
        first_block = 0
        for parity, start, end, value in leaf_jobs:
            rows = end - start
            nb = int(max(1, min((rows + _ROWS_PER_BLOCK - 1) // _ROWS_PER_BLOCK, _MAX_BLOCKS_PER_JOB)))
            vbits = int(np.float32(value).view(np.int32))
            packed.append((start, end, int(parity), vbits, first_block, nb))
            blocks_per.append(nb)
            first_block += nb
        jobs_dev = _pack_jobs(packed)
        block_job = _block_map(blocks_per)
        _K.leaf_update_compact(
            rows0, self._rows[1], margin_col, jobs_dev, block_job, margin_col.stride(0)
        )


class _V1TreeState:
    """Gather-based (v1) pipeline kept for measured A/B comparisons
    (SMXGB_PIPELINE=v1)."""

    def __init__(self, qm, gh, sample_rows=None):
        self.qm = qm
        self.gh = gh.contiguous()
        device = qm.bins.device
        rows = (
            sample_rows.to(torch.int32)
            if sample_rows is not None
            else torch.arange(qm.num_row, dtype=torch.int32, device=device)
        )
        self.cap = rows.numel()
        self._bufs = (rows.clone(), torch.empty_like(rows))

    def build_histograms(self, jobs, parity, scale):
        return build_histograms(self.qm, self.gh, self._bufs[parity], jobs, scale)

    def partition_level(self, segs, node_rows, split_packed, src_parity, cat_bits=None):
        sp = split_packed.cpu().numpy()
        counters = torch.zeros((len(segs), 2), dtype=torch.int32)
        do_segs, do_feats, do_bins, do_dls, rows_of = [], [], [], [], []
        for j, ((start, end), node_row) in enumerate(zip(segs, node_rows)):
            if sp[node_row, 0] <= 0.0:
                continue
            do_segs.append((start, end))
            do_feats.append(int(sp[node_row, 1]))
            do_bins.append(int(sp[node_row, 2]))
            do_dls.append(bool(sp[node_row, 3] > 0.5))
            rows_of.append(j)
        if do_segs:
            job_bits = None
            if cat_bits is not None:
                job_bits = cat_bits[
                    torch.as_tensor([node_rows[j] for j in rows_of], dtype=torch.long,
                                    device=cat_bits.device)
                ]
            counts = partition_level(
                self.qm, self._bufs[src_parity], self._bufs[1 - src_parity],
                do_segs, do_feats, do_bins, do_dls, job_bits,
            )
            for j, c, (start, end) in zip(rows_of, counts, do_segs):
                counters[j, 0] = c
                counters[j, 1] = (end - start) - c
        return counters

    def update_margins(self, margin_col, leaf_jobs):
        update_margins(margin_col, self._bufs, leaf_jobs)



_GROW_HIST_GRID = int(_os.environ.get("SMXGB_GROW_HIST_GRID", "1536"))
_GROW_PART_GRID = int(_os.environ.get("SMXGB_GROW_PART_GRID", "4096"))
# How a tree whose margins are updated by traversal builds its deepest
# level's histograms: "filter" streams the ranges of the level above and
# keeps each build child's rows by the parent's split (that level is then not
# partitioned either); "partition" keeps the partition for A/B runs.
# "filter-predicate" is "filter" held to plain predication where the kernel
# would compact the kept rows per wave (A/B of the two forms).
_DEEPEST_HIST = _os.environ.get("SMXGB_DEEPEST_HIST", "filter")
_DEEPEST_HIST_MODES = {"partition": 0, "filter": 1, "filter-predicate": 2}
if _DEEPEST_HIST not in _DEEPEST_HIST_MODES:
    raise ValueError(
        f"SMXGB_DEEPEST_HIST must be one of {sorted(_DEEPEST_HIST_MODES)}, got {_DEEPEST_HIST!r}"
    )
# Which kernel partitions a level's rows: "staged" reads every source row
# once (the tile is held in registers between classification and the copy)
# wherever it applies: u8 bins, a width that is a multiple of 4 up to 32, and
# the payload is copied; everything else runs the classic kernel. "classic"
# keeps the two-read kernel everywhere for A/B runs; "staged-512",
# "staged-1024" and "staged-2048" pick the rows per tile ("staged" is the
# 2048-row geometry, the fastest measured). Read once at import like
# SMXGB_DEEPEST_HIST; set_partition_mode() switches it within a process.
_PARTITION = _os.environ.get("SMXGB_PARTITION", "staged")
_PARTITION_MODES = {
    "classic": 0, "staged": 1, "staged-512": 512, "staged-1024": 1024, "staged-2048": 2048,
}


def set_partition_mode(mode):
    """Select the partition kernel ("classic", "staged", "staged-<tile>") for
    every tree grown from now on; returns the mode that was set before."""
    global _PARTITION
    if mode not in _PARTITION_MODES:
        raise ValueError(
            f"SMXGB_PARTITION must be one of {sorted(_PARTITION_MODES)}, got {mode!r}"
        )
    previous = _PARTITION
    _K.set_partition_mode(_PARTITION_MODES[mode])
    _PARTITION = mode
    return previous


set_partition_mode(_PARTITION)


def interaction_union_bitsets(interaction_sets, f):
    """[f, ceil(f/32)] uint32 table: row j has bit i set when feature i may
    follow a split on j, i.e. i == j or some constraint set holds both."""
    W = (f + 31) // 32
    table = np.zeros((f, W), dtype=np.uint32)
    for j in range(f):
        members = {j}
        for group in interaction_sets:
            if j in group:
                members.update(int(i) for i in group if 0 <= int(i) < f)
        for i in members:
            table[j, i >> 5] |= np.uint32(1 << (i & 31))
    return table


class DeviceGrower:
    """v3: the whole depthwise tree enqueued with ZERO host syncs; one
    readback (splits + counts heaps) per tree.

    Level tables, block-assignment prefixes and the sibling-subtraction
    choice are computed on device by `make_level`; hist/partition kernels
    walk virtual-block work lists via binary search. Python time between
    enqueues overlaps GPU execution.

    Constraint tables (single-process enqueue only): `mono` is the [f] int8
    monotone vector the split scan checks directions against; `mask` is
    empty, a tree-wide [f] mask or a [D, f] table whose row d is level d's
    mask; `inter_union` (with the `allowed` bitset heap and the `node_mask`
    level buffer) carries interaction constraints. The latter two exist
    only when a constraint is set.
    """

    def __init__(self, state, max_depth, feature_mask=None, monotone=None,
                 interaction_sets=None):
        assert 1 <= max_depth <= 10, "device grower supports max_depth 1..10"
        self.state = state
        self.qm = state.qm
        self.D = max_depth
        # set per tree by the grower (TreeState.traverse_ok()): margins are
        # updated by traversal, so the deepest level is not partitioned. Off
        # for direct users, whose leaf scatter needs that level's row ids.
        self.traverse = False
        # virtual-block granularity adapts to the tree's row count: small
        # trees (multiclass class-trees, small data) need more blocks in
        # flight to fill 256 CUs — measured 141 -> 178 r/s on Covertype-
        # shape at 2048 vs 4096 (profiles/r02_optimization_log.md); the
        # 12.5M-row flagship keeps 4096 (267 vs 257 at 2048).
        if _os.environ.get("SMXGB_ROWS_PER_BLOCK"):
            self.rows_per_block = _ROWS_PER_BLOCK
        else:
            self.rows_per_block = 4096 if state.cap >= (1 << 22) else 2048
        qm = state.qm
        device = qm.bins.device
        f = qm.num_col
        stride = qm.stride
        self.slots2 = f * stride * 2
        H = (1 << max_depth) - 1           # nodes in levels 0..D-1
        max_k = 1 << (max_depth - 1)
        self.H = H
        self.nodes = torch.empty((H, 3), dtype=torch.int32, device=device)
        self.node_gh = torch.zeros((H, 2), dtype=torch.float32, device=device)
        self.splits = torch.empty((H, 6), dtype=torch.float32, device=device)
        self.counts = torch.zeros((H, 2), dtype=torch.int32, device=device)
        self.hist_f32 = torch.empty((H, self.slots2), dtype=torch.float32, device=device)
        self.acc = torch.empty((max_k, self.slots2), dtype=torch.int64, device=device)
        self.cands = torch.empty((max_k, f, 5), dtype=torch.float32, device=device)
        self.hp = [torch.empty((1 << d) + 1, dtype=torch.int32, device=device) for d in range(max_depth)]
        self.pp = [torch.empty((1 << d) + 1, dtype=torch.int32, device=device) for d in range(max_depth)]
        self.work = torch.empty((max_depth, 2), dtype=torch.int32, device=device)
        groups, self.lds_words, self.hist_block = _device_hist_plan(f, stride)
        self.n_groups = len(groups)
        self.feats_per_group = groups[0][1] - groups[0][0]
        if feature_mask is None:
            self.mask = torch.empty(0, dtype=torch.uint8, device=device)
        else:
            self.mask = feature_mask.to(torch.uint8).contiguous()
        if monotone is None:
            self.mono = torch.empty(0, dtype=torch.int8, device=device)
        else:
            self.mono = monotone.to(device=device, dtype=torch.int8).contiguous()
        empty_i32 = torch.empty(0, dtype=torch.int32, device=device)
        self.inter_union = empty_i32
        self.allowed = empty_i32
        self.node_mask = torch.empty(0, dtype=torch.uint8, device=device)
        if interaction_sets:
            W = (f + 31) // 32
            self.inter_union = torch.from_numpy(
                interaction_union_bitsets(interaction_sets, f).view(np.int32)
            ).to(device)
            # heap-indexed like `nodes`; the root may use every feature
            self.allowed = torch.empty((H, W), dtype=torch.int32, device=device)
            self.allowed[0].fill_(-1)
            self.node_mask = torch.empty((max_k, f), dtype=torch.uint8, device=device)
        if not hasattr(qm, "_nbins_i32"):
            qm._nbins_i32 = qm.nbins.to(torch.int32).contiguous()

    def _enqueue_body(self, gh_init, scale, split_params, rootsum=None, alloc_free=False):
        """The tree's full kernel sequence + pinned readback. Pointer-stable
        given (gh_init, scale) tensors — hipGraph-capturable.

        alloc_free=True (the captured variant) requires `rootsum` staged by
        the caller and performs ZERO allocator calls: capture-time
        allocations route through the graph's private pool, and on this
        ROCm stack later eager allocations between replays corrupt replayed
        output (measured: gpurun_out/graph_il2.log — replay #2 returns
        wrong splits once the host allocates between replays).
        """
        st = self.state
        qm = self.qm
        f = qm.num_col
        stride = qm.stride
        missing_bin = stride - 1 if qm.has_missing else -1
        reg_lambda, reg_alpha, gamma, mcw = split_params

        self.counts.zero_()
        if alloc_free:
            # f64 -> f32 conversion happens inside copy_ — no temporaries
            self.node_gh[0].copy_(rootsum)
        else:
            # full-data (G, H): the fused gradient kernel attaches its
            # one-pass partial-sum result; recompute only for
            # subsampled/torch-path gh
            root_gh = rootsum.clone() if rootsum is not None else gh_init.to(torch.float64).sum(0)
            self.node_gh[0] = root_gh.to(torch.float32)

        # whole tree enqueued from ONE extension call
        _K.grow_tree_enqueue(
            st._bins_init, gh_init, st._rows_init,
            st._bins[0], st._gh[0], st._rows[0],
            st._bins[1], st._gh[1], st._rows[1],
            self.nodes, self.node_gh, self.splits, self.counts,
            self.hist_f32, self.acc, self.cands, self.hp, self.pp, self.work,
            qm._nbins_i32, self.mask, self.mono,
            self.inter_union, self.allowed, self.node_mask, scale,
            self.D, st.cap, f, stride, self.n_groups, self.feats_per_group,
            self.lds_words, 1 if qm.has_missing else 0, missing_bin,
            self.rows_per_block, _MAX_BLOCKS_PER_JOB, _GROW_HIST_GRID, _GROW_PART_GRID,
            reg_lambda, reg_alpha, gamma, mcw, self.hist_block,
            1 if self.traverse else 0,
            _DEEPEST_HIST_MODES[_DEEPEST_HIST],
        )
        if not hasattr(self, "_pinned"):
            self._pinned = (
                torch.empty_like(self.splits, device="cpu", pin_memory=True),
                torch.empty_like(self.counts, device="cpu", pin_memory=True),
                torch.empty((2,), dtype=torch.float32, device="cpu", pin_memory=True),
            )
        self._pinned[0].copy_(self.splits, non_blocking=True)
        self._pinned[1].copy_(self.counts, non_blocking=True)
        self._pinned[2].copy_(self.node_gh[0], non_blocking=True)

    def _graph_eligible(self):
        """hipGraph replay needs stable pointers: full-data state (bins/rows
        alias the matrix; only gh changes round to round — staged) and no
        per-tree feature mask (its contents change every tree) or
        constraint table."""
        st = self.state
        # default OFF: capture/replay of this sequence currently memory-
        # faults on gfx950 (gpurun_out/graph_triage.log); opt in with
        # SMXGB_HIPGRAPH=1 once the faulting node is resolved
        return (
            _os.environ.get("SMXGB_HIPGRAPH", "0") == "1"
            and st._bins_init is self.qm.bins
            and self.mask.numel() == 0
            and self.mono.numel() == 0
            and self.inter_union.numel() == 0
        )

    def grow_enqueue(self, scale, split_params):
        """Enqueue the full tree plus the non-blocking heap readback into
        pinned host buffers; returns a torch.cuda.Event to wait on. Lets the
        caller enqueue several independent trees (multiclass / bagging
        rounds) back-to-back so the GPU never idles between them.

        When eligible, the ~45-kernel sequence is captured ONCE into a
        hipGraph and replayed as a single launch per tree (the per-launch
        submission gaps bounded the round at ~4%, ROADMAP r01); per-round
        inputs (gradients, fixed-point scale) are staged into persistent
        buffers the captured kernels read.
        """
        st = self.state
        rootsum = getattr(st._gh_init, "_smxgb_rootsum", None)
        if self._graph_eligible():
            # root (G, H) must stay BIT-identical with the non-graphed
            # paths: the fused-gradient partial sum (when present) is
            # staged; otherwise the same f64 sum runs EAGERLY here (the
            # captured body must be allocation-free — see _enqueue_body)
            if rootsum is None:
                rootsum = st._gh_init.to(torch.float64).sum(0)
            key = (st.cap, split_params, self.traverse, _DEEPEST_HIST, _PARTITION)
            dbg = _os.environ.get("SMXGB_GRAPH_DEBUG") == "1"

            def _d(msg):
                if dbg:
                    import sys as _sys

                    print(f"[graphdbg] {msg}", file=_sys.stderr, flush=True)
                    torch.cuda.synchronize()

            if getattr(self, "_graph_key", None) != key:
                try:
                    _d(f"build start cap={st.cap}")
                    self._gh_stage = torch.empty(
                        (st.cap, 2), dtype=torch.float32, device=self.nodes.device
                    )
                    self._scale_stage = torch.empty_like(scale)
                    self._root_stage = torch.empty(
                        2, dtype=torch.float64, device=self.nodes.device
                    )
                    # warmup on a side stream (allocator settles), then capture
                    side = torch.cuda.Stream(device=self.nodes.device)
                    side.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(side):
                        self._enqueue_body(self._gh_stage, self._scale_stage, split_params,
                                           rootsum=self._root_stage, alloc_free=True)
                    torch.cuda.current_stream().wait_stream(side)
                    torch.cuda.synchronize()
                    _d("warmup done")
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph):
                        self._enqueue_body(self._gh_stage, self._scale_stage, split_params,
                                           rootsum=self._root_stage, alloc_free=True)
                    _d("capture done")
                    self._graph = graph
                    self._graph_key = key
                except Exception as e:  # capture unsupported -> plain enqueue
                    import logging

                    logging.getLogger(__name__).warning(
                        "hipGraph capture unavailable (%s); using per-kernel launches", e
                    )
                    _os.environ["SMXGB_HIPGRAPH"] = "0"
                    self._enqueue_body(st._gh_init, scale, split_params, rootsum=rootsum)
                    ev = torch.cuda.Event()
                    ev.record()
                    return ev
            self._gh_stage.copy_(st._gh_init, non_blocking=True)
            self._scale_stage.copy_(scale, non_blocking=True)
            self._root_stage.copy_(rootsum, non_blocking=True)
            self._graph.replay()
            if _os.environ.get("SMXGB_GRAPH_DEBUG") == "1":
                import sys as _sys

                torch.cuda.synchronize()
                print("[graphdbg] replay ok", file=_sys.stderr, flush=True)
        else:
            self._enqueue_body(st._gh_init, scale, split_params, rootsum=rootsum)
        ev = torch.cuda.Event()
        ev.record()
        return ev

    def grow_wait(self, ev):
        """Wait for a grow_enqueue readback; returns (splits, counts, root)
        numpy views of this grower's pinned buffers (valid until the next
        grow_enqueue on the same instance)."""
        ev.synchronize()
        return (
            self._pinned[0].numpy(),
            self._pinned[1].numpy(),
            self._pinned[2].numpy(),
        )

    def grow(self, scale, split_params, comm=None):
        """Enqueue the full tree; returns (splits_np [H,6], counts_np [H,2],
        root_gh_np [2])."""
        if comm is None:
            return self.grow_wait(self.grow_enqueue(scale, split_params))

        # the distributed loop knows neither per-level masks nor
        # interaction constraints: constrained trees with a communicator
        # stay on the per-level path
        assert self.mask.dim() <= 1 and self.inter_union.numel() == 0 and self.mono.numel() == 0
        st = self.state
        qm = self.qm
        f = qm.num_col
        stride = qm.stride
        missing_bin = stride - 1 if qm.has_missing else -1
        reg_lambda, reg_alpha, gamma, mcw = split_params

        self.counts.zero_()
        root_gh = getattr(st._gh_init, "_smxgb_rootsum", None)
        root_gh = root_gh.clone() if root_gh is not None else st._gh_init.to(torch.float64).sum(0)
        comm.allreduce_(root_gh)
        self.node_gh[0] = root_gh.to(torch.float32)

        # traversal needs no row ids; with the filtered deepest histogram
        # level D-2 is not partitioned either (see grow_tree_enqueue)
        filter_mode = _DEEPEST_HIST_MODES[_DEEPEST_HIST]
        filter_last = self.traverse and filter_mode != 0 and self.D >= 2
        predicate_only = 1 if filter_mode == 2 else 0
        copy_rows = 0 if self.traverse else 1
        no_splits = torch.empty(0, dtype=torch.float32, device=self.splits.device)

        for d in range(self.D):
            k = 1 << d
            base = k - 1
            nodes_d = self.nodes[base : base + k]
            gh_d = self.node_gh[base : base + k]
            splits_d = self.splits[base : base + k]
            counts_d = self.counts[base : base + k]
            filtered = filter_last and d == self.D - 1
            par_splits = self.splits[(k >> 1) - 1 : k - 1] if filtered else no_splits

            if d == 0:
                _K.grow_make_root(nodes_d, self.hp[0], self.pp[0], self.work[0],
                                  st.cap, self.rows_per_block, _MAX_BLOCKS_PER_JOB)
            else:
                pk = k >> 1
                pbase = pk - 1
                _K.grow_make_level(
                    self.nodes[pbase : pbase + pk], self.splits[pbase : pbase + pk],
                    self.counts[pbase : pbase + pk], self.node_gh[pbase : pbase + pk],
                    nodes_d, gh_d, self.hp[d], self.pp[d], self.work[d],
                    pk, self.rows_per_block, _MAX_BLOCKS_PER_JOB,
                    1 if filtered else 0,
                )

            # a filtered level reads what the level above it read
            sd = d - 1 if filtered else d
            src_bins, src_gh, src_rows = (
                (st._bins_init, st._gh_init, st._rows_init) if sd == 0
                else (st._bins[sd % 2], st._gh[sd % 2], st._rows[sd % 2])
            )
            acc_d = self.acc[:k]
            acc_d.zero_()
            # Default ON for real multi-rank groups (the driver's scaling
            # run): correctness is proven bit-identical under gloo 2-rank
            # and nccl async handles (tests/test_distributed_gpu.py,
            # tests/test_rccl_rehearsal.py). SMXGB_COMM_OVERLAP=0 disables,
            # =1 forces even at world 1 (rehearsal).
            _ov_env = _os.environ.get("SMXGB_COMM_OVERLAP")
            overlap = (
                comm is not None
                and k >= 4
                and hasattr(comm, "allreduce_async_")
                and (_ov_env == "1" or (_ov_env != "0" and getattr(comm, "world_size", 1) > 1))
            )
            if overlap:
                # Chunked hist/allreduce pipelining: the collective for the
                # first half of the level's slots runs on the comm stream
                # WHILE the compute stream builds the second half's
                # histograms (the nccl stream only waits on the tensors it
                # reduces). Fold-compaction per half as below.
                mid = k >> 1  # even: pairs stay within a half
                _K.grow_hist_level(
                    src_bins, src_gh, nodes_d, self.hp[d], self.work[d], acc_d,
                    k, f, stride, self.n_groups, self.feats_per_group, scale,
                    self.rows_per_block, _GROW_HIST_GRID, self.lds_words, self.hist_block,
                    0, mid, par_splits, missing_bin, predicate_only,
                )
                c1 = acc_d[0:mid:2] + acc_d[1:mid:2]
                w1 = comm.allreduce_async_(c1)
                _K.grow_hist_level(
                    src_bins, src_gh, nodes_d, self.hp[d], self.work[d], acc_d,
                    k, f, stride, self.n_groups, self.feats_per_group, scale,
                    self.rows_per_block, _GROW_HIST_GRID, self.lds_words, self.hist_block,
                    mid, k, par_splits, missing_bin, predicate_only,
                )
                c2 = acc_d[mid::2] + acc_d[mid + 1 :: 2]
                w2 = comm.allreduce_async_(c2)
                w1.wait()
                acc_d[0:mid:2] = c1
                acc_d[1:mid:2] = c1
                w2.wait()
                acc_d[mid::2] = c2
                acc_d[mid + 1 :: 2] = c2
            else:
                _K.grow_hist_level(
                    src_bins, src_gh, nodes_d, self.hp[d], self.work[d], acc_d,
                    k, f, stride, self.n_groups, self.feats_per_group, scale,
                    self.rows_per_block, _GROW_HIST_GRID, self.lds_words, self.hist_block,
                    0, 1 << 30, par_splits, missing_bin, predicate_only,
                )
                if comm is not None:
                    if k == 1:
                        comm.allreduce_(acc_d)
                    else:
                        # Compacted allreduce: of each sibling pair exactly
                        # one slot was built from rows (the other is all
                        # zeros — make_level's subtraction trick), so
                        # folding pairs halves the message without a gather
                        # kernel. The sum lands back in BOTH child slots;
                        # convert_level only reads the built one. int64
                        # adds wrap mod 2^64, matching the kernel's
                        # unsigned fixed-point.
                        compact = acc_d[0::2] + acc_d[1::2]
                        comm.allreduce_(compact)
                        acc_d[0::2] = compact
                        acc_d[1::2] = compact
            hist_d = self.hist_f32[base : base + k]
            _K.grow_convert_level(acc_d, hist_d, nodes_d, k, self.slots2, scale)
            if d > 0:
                pbase = (k >> 1) - 1
                _K.grow_derive_level(hist_d, self.hist_f32[pbase : pbase + (k >> 1)],
                                     nodes_d, k, self.slots2)

            _K.find_splits(
                hist_d, gh_d, qm._nbins_i32, self.mask, self.mono,
                self.cands[:k], splits_d, k, f, stride,
                1 if qm.has_missing else 0, 0, reg_lambda, reg_alpha, gamma, mcw,
            )

            if self.traverse and d == self.D - 1:
                # margins updated by traversal: nothing reads the deepest
                # level's row ids or counts
                continue
            if filter_last and d == self.D - 2:
                continue
            dst = 1 - d % 2
            _K.grow_partition_level(
                src_bins, src_gh, src_rows, st._bins[dst], st._gh[dst], st._rows[dst],
                nodes_d, self.pp[d], self.work[d], splits_d, counts_d,
                k, f, missing_bin, _GROW_PART_GRID,
                1 if d < self.D - 1 else 0,  # last level feeds leaf_update only
                copy_rows,
            )
        # (the grower decides _level0 from whether the root split)

        # the tree's single host drain
        splits_np = self.splits.cpu().numpy()
        counts_np = self.counts.cpu().numpy()
        root_np = self.node_gh[0].cpu().numpy()
        return splits_np, counts_np, root_np


def make_tree_state(qm, gh, sample_rows=None, slot=0):
    if _os.environ.get("SMXGB_PIPELINE") == "v1":
        return _V1TreeState(qm, gh, sample_rows)
    return TreeState(qm, gh, sample_rows, slot=slot)
