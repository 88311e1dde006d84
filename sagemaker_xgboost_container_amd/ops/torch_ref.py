"""Reference ops backend: pure PyTorch, any device.

This is (a) the CPU execution path for small jobs/tests and (b) the numerics
reference the CDNA4 HIP kernels are validated against (fp64 histogram
accumulation). The function contracts here define the backend interface the
HIP module (ops/hip.py + csrc/) implements.

Interface (segment-based, one device sync per tree level):
  compute_scale(gh)                     -> backend-specific scale (None here)
  build_histograms(qm, gh, rowbuf, jobs, scale) -> accumulator [J, slots, 2]
  hist_to_float(acc, scale)             -> float32 view of the accumulator
  find_splits(hist, parent_sum, qm, **) -> best split per node
  partition_level(qm, src, dst, segs, feats, bins, dls) -> left counts (host)
  update_margins(margin_col, bufs, leaf_jobs)
  predict_tree(tree, X)                 -> (n,) margin contribution
  gradient_sample(gh, subsample, u)     -> (rows, rescaled gh) of
                                           sampling_method=gradient_based
"""
import math

import torch

NAME = "torch_ref"


def compute_scale(gh, comm=None):
    """torch_ref accumulates in fp64 — no fixed-point scale needed."""
    return None


def build_histograms(qm, gh, rowbuf, jobs, scale=None):
    """Accumulate (grad, hess) histograms for a batch of row segments.

    jobs: list of (start, end) into rowbuf. Returns (J, f*stride, 2) fp64.
    """
    f = qm.num_col
    stride = qm.stride
    device = qm.bins.device
    offsets = torch.arange(f, device=device, dtype=torch.long) * stride
    acc = torch.zeros((len(jobs), f * stride, 2), dtype=torch.float64, device=device)
    for i, (start, end) in enumerate(jobs):
        rows = rowbuf[start:end].long()
        bins = qm.bins[rows].long()  # (m, f)
        slots = (bins + offsets).reshape(-1)
        weights = gh[rows].to(torch.float64).repeat_interleave(f, dim=0)
        acc[i].index_add_(0, slots, weights)
    return acc


def hist_to_float(acc, scale=None):
    return acc.to(torch.float32)


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
    """Best split per node from per-node histograms.

    hist: (k, f * stride, 2) float32; parent_sum: (k, 2) float32.
    feature_mask: (f,) or (k, f) bool — allowed features (colsample and
    interaction constraints). monotone: (f,) int8 in {-1, 0, 1} — splits
    violating the implied child-weight ordering are masked out.
    Returns dict of tensors (all shape (k,)):
      feature, bin, gain, default_left, left_g, left_h
    A node with no valid split has gain <= 0.

    Categorical features (qm.is_cat; bin = category code). A candidate is a
    set R of categories that go right; the others go left, missing goes
    either way. A category whose (g, h) is (0, 0) is empty and never in R;
    with fewer than two non-empty categories there is no candidate.
      one-hot (nbins < max_cat_to_onehot): candidate c is R = {c}.
      partition: non-empty categories sorted ascending by
        (g / (h + reg_lambda), category); candidate p - 1, p = 1..m-1, cuts
        the sorted list after p entries, kept when min(p, m - p) <=
        max_cat_threshold; R is the shorter side (the prefix when equal).
    The left sums come from the histogram (everything not in R, plus
    missing when it goes left), the right sums from parent_sum, as for a
    numeric feature. Ties go to the lowest candidate, missing-right first.
    With a categorical column the result also holds "cat_bits": (k, 8) int32,
    the winner's R (bit c & 31 of word c >> 5), zero for a numeric winner or
    gain <= 0; column 2 of "packed" is 0 for a categorical winner.
    As the numerics reference it then also returns "gain64": the winners'
    gains as float64, before the float32 store (-inf: no candidate). The
    device backends compute in float32 and have no such value to return.
    """
    k = hist.shape[0]
    f = qm.num_col
    stride = qm.stride
    device = hist.device
    h = hist.reshape(k, f, stride, 2).to(torch.float64)

    nbins = qm.nbins.to(device)  # (f,)
    bin_ar = torch.arange(stride, device=device)
    # split after bin j is valid iff j <= nbins_f - 2 (right side non-empty)
    valid_bin = bin_ar.unsqueeze(0) < (nbins.unsqueeze(1) - 1)  # (f, stride)

    if qm.has_missing:
        missing = h[:, :, stride - 1, :]  # (k, f, 2)
        real = h[:, :, : stride - 1, :]
        real_valid = valid_bin[:, : stride - 1]
    else:
        missing = torch.zeros((k, f, 2), dtype=torch.float64, device=device)
        real = h
        real_valid = valid_bin

    scan = torch.cumsum(real, dim=2)  # (k, f, b, 2) left sums (missing excluded)
    parent = parent_sum.to(torch.float64).reshape(k, 1, 1, 2)

    lam = reg_lambda
    alpha = reg_alpha

    def score(g, hs):
        ag = torch.clamp(g.abs() - alpha, min=0.0)
        return ag * ag / (hs + lam)

    parent_score = score(parent[..., 0], parent[..., 1])

    def weight(g, hs):
        ag = torch.clamp(g.abs() - alpha, min=0.0)
        return -torch.sign(g) * ag / (hs + lam)

    mono = None
    if monotone is not None and bool((monotone != 0).any()):
        mono = monotone.to(device).reshape(1, f, 1)

    # categorical features: their rows of the left-sum and validity tables
    # are indexed by candidate instead of by bin
    is_cat = getattr(qm, "is_cat", None)
    cat_feats = is_cat.nonzero().flatten().tolist() if is_cat is not None else []
    cat_info = {}
    valid = real_valid.unsqueeze(0)
    if cat_feats:
        width = real.shape[2]
        scan = scan.clone()
        valid = valid.expand(k, f, width).clone()
        for j in cat_feats:
            nbj = min(int(nbins[j]), width)
            onehot = int(nbins[j]) < int(max_cat_to_onehot)
            lg, lh, ok, order, nonempty, m = _cat_candidates(
                real[:, j, :nbj, 0], real[:, j, :nbj, 1], onehot, lam, int(max_cat_threshold)
            )
            scan[:, j] = 0.0
            scan[:, j, :nbj, 0] = lg
            scan[:, j, :nbj, 1] = lh
            valid[:, j] = False
            valid[:, j, :nbj] = ok
            cat_info[j] = (onehot, order, nonempty, m)

    results = []
    for default_left in (False, True):
        gl = scan[..., 0] + (missing[..., 0].unsqueeze(2) if default_left else 0.0)
        hl = scan[..., 1] + (missing[..., 1].unsqueeze(2) if default_left else 0.0)
        gr = parent[..., 0] - gl
        hr = parent[..., 1] - hl
        gain = 0.5 * (score(gl, hl) + score(gr, hr) - parent_score) - gamma
        invalid = (hl < min_child_weight) | (hr < min_child_weight) | ~valid
        if mono is not None:
            wl = weight(gl, hl)
            wr = weight(gr, hr)
            invalid = invalid | ((mono > 0) & (wl > wr)) | ((mono < 0) & (wl < wr))
        gain = torch.where(invalid, torch.full_like(gain, -float("inf")), gain)
        results.append((gain, gl, hl))

    gain_r, gl_r, hl_r = results[0]
    gain_l, gl_l, hl_l = results[1]
    use_left = gain_l > gain_r
    gain = torch.where(use_left, gain_l, gain_r)  # (k, f, b)
    gl = torch.where(use_left, gl_l, gl_r)
    hl = torch.where(use_left, hl_l, hl_r)

    if feature_mask is not None:
        if feature_mask.dim() == 1:
            mask = feature_mask.reshape(1, f, 1)
        else:
            mask = feature_mask.reshape(k, f, 1)
        gain = torch.where(mask, gain, torch.full_like(gain, -float("inf")))

    flat_gain = gain.reshape(k, -1)
    best = flat_gain.argmax(dim=1)  # (k,)
    best_gain = flat_gain.gather(1, best.unsqueeze(1)).squeeze(1)
    nb = gain.shape[2]
    best_feat = best // nb
    best_bin = best % nb
    idx = (best_feat * nb + best_bin).unsqueeze(1)
    out_default_left = use_left.reshape(k, -1).gather(1, idx).squeeze(1)
    out_gl = gl.reshape(k, -1).gather(1, idx).squeeze(1)
    out_hl = hl.reshape(k, -1).gather(1, idx).squeeze(1)

    gain_out = torch.where(torch.isinf(best_gain), torch.full_like(best_gain, -1.0), best_gain).to(torch.float32)
    cat_bits = None
    if cat_feats:
        cat_bits = torch.zeros((k, 8), dtype=torch.int32, device=device)
        for j, (onehot, order, nonempty, m) in cat_info.items():
            rows = ((best_feat == j) & (gain_out > 0)).nonzero().flatten()
            if rows.numel():
                cat_bits[rows] = _cat_winner_bits(
                    best_bin[rows], onehot,
                    None if order is None else order[rows], nonempty[rows], m[rows],
                )
            best_bin = torch.where(best_feat == j, torch.zeros_like(best_bin), best_bin)
    packed = torch.stack(
        [
            gain_out,
            best_feat.to(torch.float32),
            best_bin.to(torch.float32),
            out_default_left.to(torch.float32),
            out_gl.to(torch.float32),
            out_hl.to(torch.float32),
        ],
        dim=1,
    )
    out = {
        "feature": best_feat.to(torch.int32),
        "bin": best_bin.to(torch.int32),
        "gain": gain_out,
        "default_left": out_default_left,
        "left_g": out_gl.to(torch.float32),
        "left_h": out_hl.to(torch.float32),
        "packed": packed,
    }
    if cat_bits is not None:
        out["cat_bits"] = cat_bits
        # the winners' gains before the float32 store (-inf: no candidate),
        # for comparisons at float64 precision
        out["gain64"] = best_gain
    return out


def _cat_candidates(G, H, onehot, lam, max_cat_threshold):
    """Candidate table of one categorical feature over k nodes (find_splits
    states the rule). G, H: (k, nb) float64 per-category sums. Returns
    (left_g, left_h, valid, order, nonempty, m): the left child's sums
    without missing and the validity of candidate i, (k, nb) each; the
    sorted category order (None in one-hot mode); the non-empty mask and
    its count m (k,)."""
    k, nb = G.shape
    nonempty = ~((G == 0) & (H == 0))
    m = nonempty.sum(1)
    tot_g = G.sum(1, keepdim=True)
    tot_h = H.sum(1, keepdim=True)
    if onehot:
        return tot_g - G, tot_h - H, nonempty & (m >= 2).unsqueeze(1), None, nonempty, m
    key = G / (H + lam)
    key = torch.where(torch.isnan(key), torch.full_like(key, float("inf")), key)
    # ascending by (empty, key, category): two stable passes
    order = torch.sort(key, dim=1, stable=True).indices
    empty_sorted = (~nonempty).gather(1, order).to(torch.uint8)
    order = order.gather(1, torch.sort(empty_sorted, dim=1, stable=True).indices)
    Gs = G.gather(1, order).cumsum(1)  # column p - 1: the first p sorted
    Hs = H.gather(1, order).cumsum(1)
    p = torch.arange(1, nb + 1, device=G.device).unsqueeze(0)
    mm = m.unsqueeze(1)
    valid = (p <= mm - 1) & (torch.minimum(p, mm - p) <= max_cat_threshold)
    prefix_right = p <= mm - p
    left_g = torch.where(prefix_right, tot_g - Gs, Gs)
    left_h = torch.where(prefix_right, tot_h - Hs, Hs)
    return left_g, left_h, valid, order, nonempty, m


def _cat_winner_bits(cand, onehot, order, nonempty, m):
    """(r, 8) int32 category sets R of candidates `cand` (r,) of one
    categorical feature; order / nonempty / m as _cat_candidates returns."""
    r, nb = nonempty.shape
    cats = torch.arange(nb, device=nonempty.device).unsqueeze(0)
    if onehot:
        member = cats == cand.unsqueeze(1)
    else:
        rank = torch.argsort(order, dim=1)  # position of each category
        p = (cand + 1).unsqueeze(1)
        mm = m.unsqueeze(1)
        member = nonempty & torch.where(p <= mm - p, rank < p, (rank >= p) & (rank < mm))
    return pack_cat_bits(member)


def pack_cat_bits(member):
    """(r, nb <= 256) bool membership -> (r, 8) int32 bitset words."""
    r, nb = member.shape
    full = torch.zeros((r, 256), dtype=torch.int64, device=member.device)
    full[:, :nb] = member.to(torch.int64)
    weights = torch.ones(32, dtype=torch.int64, device=member.device) << torch.arange(
        32, device=member.device
    )
    words = (full.reshape(r, 8, 32) * weights).sum(2)
    words = torch.where(words >= 2**31, words - 2**32, words)  # uint32 pattern as int32
    return words.to(torch.int32)


def cat_bit_of(bits, b):
    """Is category b (m,) int64 in [0, 256) set in the rows of bits (m, 8)
    (int32 or wider, the uint32 words' bit patterns)?"""
    word = bits.to(torch.int64).gather(1, (b >> 5).unsqueeze(1)).squeeze(1)
    return ((word >> (b & 31)) & 1).to(torch.bool)


def cat_goes_left(fv, bits):
    """Decision at categorical nodes for non-missing values fv (m,) against
    the sets bits (m, 8): outside [0, 256) left; else the truncated value is
    the category and members go right (models/tree.py cat_goes_left)."""
    inside = (fv >= 0) & (fv < 256)
    c = torch.where(inside, fv, torch.zeros_like(fv)).to(torch.int64)
    return ~(inside & cat_bit_of(bits, c))


def tree_cat_tensors(tree, device):
    """(slot, table) of a tree for goes_left: slot (num_nodes,) int64, -1 at
    numeric nodes; table (n_cat_nodes, 8) int64. None without categorical
    nodes."""
    import numpy as np

    split_type = np.asarray(getattr(tree, "split_type", ()))
    if not split_type.any():
        return None
    nodes = np.flatnonzero(split_type)
    slot = np.full(len(split_type), -1, dtype=np.int64)
    slot[nodes] = np.arange(len(nodes))
    table = np.stack([np.asarray(tree.cat_bits[i], dtype=np.uint32) for i in nodes])
    return (
        torch.from_numpy(slot).to(device),
        torch.from_numpy(table.astype(np.int64)).to(device),
    )


def flat_cat_tensors(flat):
    """(slot, table) of a flat forest for goes_left, None when numeric."""
    if not flat.get("has_cat"):
        return None
    return flat["cat_slot"], flat["cat_table"]


def goes_left(fv, thresh, cat, cur):
    """Left/right of non-missing values fv (m,) at nodes cur (m,): the one
    decision every host traversal uses. cat: None or (slot, table)."""
    num = fv < thresh[cur]
    if cat is None:
        return num
    slot, table = cat
    s = slot[cur].long()
    at_cat = s >= 0
    return torch.where(at_cat, cat_goes_left(fv, table[s.clamp(min=0)]), num)


def refuse_categorical(flat, what):
    """Explanations are not defined here for set-valued nodes."""
    if flat.get("has_cat"):
        raise NotImplementedError(f"{what} is not implemented for models with categorical splits")


def _go_left_mask(qm, bins, split_bin, default_left, cat_set=None):
    """cat_set: (8,) bitset of the bins that go right (categorical split
    feature), None for a numeric feature's `bin <= split_bin`."""
    if cat_set is None:
        real = bins <= int(split_bin)
    else:
        inside = bins < 256
        b = torch.where(inside, bins, torch.zeros_like(bins))
        real = ~(inside & cat_bit_of(cat_set.reshape(1, 8).expand(bins.numel(), 8), b))
    if qm.has_missing:
        is_missing = bins == (qm.stride - 1)
        return torch.where(is_missing, torch.full_like(is_missing, bool(default_left)), real)
    return real


def partition_level(qm, src, dst, segs, feats, split_bins, default_lefts, cat_bits=None):
    """Partition each (start, end) segment of src into dst (left block then
    right block in the same index range). Returns list of left counts.
    cat_bits: (J, 8) category sets, read for the jobs whose split feature is
    categorical (qm.is_cat)."""
    counts = []
    is_cat = getattr(qm, "is_cat", None)
    for j, ((start, end), feature, sbin, dl) in enumerate(zip(segs, feats, split_bins, default_lefts)):
        rows = src[start:end]
        bins = qm.bins[rows.long(), int(feature)].long()
        cat_set = None
        if cat_bits is not None and is_cat is not None and bool(is_cat[int(feature)]):
            cat_set = cat_bits[j]
        go_left = _go_left_mask(qm, bins, sbin, dl, cat_set)
        left = rows[go_left]
        right = rows[~go_left]
        dst[start : start + left.numel()] = left
        dst[start + left.numel() : end] = right
        counts.append(int(left.numel()))
    return counts


def update_margins(margin_col, bufs, leaf_jobs):
    """margin_col[rows] += value for each (parity, start, end, value) job."""
    for parity, start, end, value in leaf_jobs:
        rows = bufs[parity][start:end].long()
        margin_col[rows] += value


def _mvs_norm(gh):
    g = gh[:, 0].to(torch.float32)
    h = gh[:, 1].to(torch.float32)
    return torch.sqrt(g * g + h * h)


def mvs_threshold(gh, S):
    """Threshold mu of gradient-based sampling (Minimal Variance Sampling)
    as a float32 scalar tensor on gh's device: the solution of
    sum_i min(1, r_i / mu) = S with r_i = sqrt(g_i^2 + h_i^2), or 0 when no
    more than S rows have r_i > 0 (all of them are then kept).

    Reference form: sort, float64 cumulative sum, closed form. With the k
    largest rows certain (p = 1), mu_k = sum(rest) / (S - k); the solution
    is the smallest k whose largest uncertain row is <= mu_k.
    """
    S = float(S)
    r = _mvs_norm(gh).to(torch.float64)
    r = torch.sort(r[r > 0]).values
    m = r.numel()
    if m <= S:
        return torch.zeros((), dtype=torch.float32, device=gh.device)
    csum = torch.cumsum(r, 0)
    # k < S keeps the denominator positive; m > S leaves a row uncertain
    k = torch.arange(0, min(m, math.ceil(S)), device=gh.device)
    top = m - 1 - k  # largest uncertain row when k rows are certain
    mu_k = csum[top] / (S - k.to(torch.float64))
    first = int((r[top] <= mu_k).nonzero()[0])
    return mu_k[first].to(torch.float32)


def gradient_sample(gh, subsample, u):
    """Gradient-based row sample of one tree's (n, 2) float32 gradients.

    Row i is kept when u_i < p_i = min(1, r_i / mu) (mu = 0: p_i = 1 where
    r_i > 0) and its pair is multiplied by 1 / p_i; dropped rows get a zero
    pair. Returns (ascending int32 row list, rescaled (n, 2) tensor)."""
    n = gh.shape[0]
    mu = mvs_threshold(gh, float(subsample) * n)
    r = _mvs_norm(gh)
    if float(mu) > 0.0:
        p = torch.clamp(r / mu, max=1.0)
    else:
        p = (r > 0).to(torch.float32)
    keep = u < p
    inv = torch.where(keep, 1.0 / p, torch.zeros_like(p))
    out = gh.to(torch.float32) * inv.unsqueeze(1)
    out = torch.where(keep.unsqueeze(1), out, torch.zeros_like(out))
    rows = keep.nonzero(as_tuple=True)[0].to(torch.int32)
    return rows, out


def leaf_quantiles(pos, resid, n_leaves, alpha, weight=None):
    """Per-leaf (weighted) quantile of the residuals: the values adaptive
    trees (reg:absoluteerror, reg:quantileerror) put into their leaves.

    pos: int32 (n,) leaf slot in [0, n_leaves), or -1 for a row that takes
    no part; resid: finite float32 (n,). Returns (n_leaves,) float32.

    For a leaf with m rows and sorted residuals v_0 <= ... <= v_{m-1}:
      m == 0 (or total weight 0)            -> NaN
      unweighted: alpha <= 1/(m+1)          -> v_0
                  alpha >= m/(m+1)          -> v_{m-1}
                  else x = alpha*(m+1), k = floor(x) - 1, d = x - 1 - k,
                       q = v_k + d * (v_{k+1} - v_k)
                  (float64 from the float32 values, rounded to float32 once)
      weighted:   q = v_i for the smallest i with sum_{j<=i} w_j >=
                  alpha * sum w, clamped to m - 1; no interpolation.

    This float64 sort-based function IS the definition of the rule here. It
    follows the published description of upstream XGBoost's common::Quantile
    and WeightedQuantile, but no copy of upstream is available to compare
    against, so agreement with it in the last bit is not claimed.
    """
    import numpy as np

    n_leaves = int(n_leaves)
    alpha = float(alpha)
    if not (0.0 < alpha < 1.0):
        raise ValueError("alpha must be in (0, 1)")
    p = pos.detach().cpu().numpy().astype(np.int64)
    r = resid.detach().cpu().numpy().astype(np.float32)
    if p.shape != r.shape or p.ndim != 1:
        raise ValueError("pos and resid must be 1-d and of one shape")
    if p.size and (p.max() >= n_leaves or p.min() < -1):
        raise ValueError(f"pos must lie in [-1, {n_leaves})")
    w = None
    if weight is not None and weight.numel():
        w = weight.detach().cpu().numpy().astype(np.float32)
        if w.shape != p.shape:
            raise ValueError("weight must match pos")
    order = np.lexsort((r, p))
    ps, vs = p[order], r[order].astype(np.float64)
    ws = w[order].astype(np.float64) if w is not None else None
    lo = np.searchsorted(ps, np.arange(n_leaves), side="left")
    hi = np.searchsorted(ps, np.arange(n_leaves), side="right")
    out = np.full(n_leaves, np.nan, dtype=np.float32)
    for leaf in range(n_leaves):
        m = int(hi[leaf] - lo[leaf])
        if m == 0:
            continue
        v = vs[lo[leaf]:hi[leaf]]
        if ws is not None:
            cs = np.cumsum(ws[lo[leaf]:hi[leaf]])
            if not cs[-1] > 0.0:
                continue
            i = min(int(np.searchsorted(cs, alpha * cs[-1], side="left")), m - 1)
            out[leaf] = v[i]
        elif alpha <= 1.0 / (m + 1.0):
            out[leaf] = v[0]
        elif alpha >= m / (m + 1.0):
            out[leaf] = v[m - 1]
        else:
            x = alpha * (m + 1.0)
            k = min(max(int(math.floor(x)) - 1, 0), m - 1)
            d = (x - 1.0) - k
            k1 = min(k + 1, m - 1)
            out[leaf] = np.float32(v[k] + d * (v[k1] - v[k]))
    return torch.from_numpy(out).to(resid.device)


def predict_tree(tree, X):
    """Margin contribution of one tree for dense X (n, f) float32 (NaN missing).

    tree: models.tree.Tree (host arrays). Vectorized level-by-level traversal.
    """
    device = X.device
    n = X.shape[0]
    node = torch.zeros(n, dtype=torch.long, device=device)
    left = torch.as_tensor(tree.left, device=device, dtype=torch.long)
    right = torch.as_tensor(tree.right, device=device, dtype=torch.long)
    feat = torch.as_tensor(tree.feature, device=device, dtype=torch.long)
    thresh = torch.as_tensor(tree.threshold, device=device, dtype=torch.float32)
    default_left = torch.as_tensor(tree.default_left, device=device, dtype=torch.bool)
    is_leaf = left < 0
    value = torch.as_tensor(tree.value, device=device, dtype=torch.float32)
    cat = tree_cat_tensors(tree, device)

    active = ~is_leaf[node]
    while bool(active.any()):
        cur = node[active]
        fv = X[active.nonzero(as_tuple=True)[0], feat[cur]]
        missing = torch.isnan(fv)
        go_left = torch.where(missing, default_left[cur], goes_left(fv, thresh, cat, cur))
        node[active] = torch.where(go_left, left[cur], right[cur])
        active = ~is_leaf[node]
    return value[node]


def tree_leaf_ids(tree, X):
    """(n,) int32 node id of the leaf each row of dense X (NaN missing)
    falls into: predict_tree's traversal, stopping short of the value."""
    device = X.device
    node = torch.zeros(X.shape[0], dtype=torch.long, device=device)
    left = torch.as_tensor(tree.left, device=device, dtype=torch.long)
    right = torch.as_tensor(tree.right, device=device, dtype=torch.long)
    feat = torch.as_tensor(tree.feature, device=device, dtype=torch.long)
    thresh = torch.as_tensor(tree.threshold, device=device, dtype=torch.float32)
    default_left = torch.as_tensor(tree.default_left, device=device, dtype=torch.bool)
    is_leaf = left < 0
    cat = tree_cat_tensors(tree, device)
    active = ~is_leaf[node]
    while bool(active.any()):
        cur = node[active]
        fv = X[active.nonzero(as_tuple=True)[0], feat[cur]]
        go_left = torch.where(torch.isnan(fv), default_left[cur], goes_left(fv, thresh, cat, cur))
        node[active] = torch.where(go_left, left[cur], right[cur])
        active = ~is_leaf[node]
    return node.to(torch.int32)


def tree_max_feature(trees):
    """Largest split feature per tree (-1 for a stump), on the host: lets an
    entry point reject a too-narrow X before any row is read."""
    import numpy as np

    out = []
    for t in trees:
        internal = np.asarray(t.left) >= 0
        out.append(int(np.asarray(t.feature)[internal].max()) if internal.any() else -1)
    return np.asarray(out, dtype=np.int64)


def check_predict_args(flat, X, k, t_begin, t_end, classes=True):
    """Refuse, before any row is read, a tree range outside the forest, a
    class id beyond k and a matrix narrower than the widest split feature of
    the range. Returns that feature (-1: the range holds no split).
    `classes=False` for outputs without a class axis (leaf ids)."""
    if not (0 <= t_begin <= t_end <= flat["n_trees"]):
        raise ValueError(f"tree range [{t_begin}, {t_end}) out of bounds")
    if X.dim() != 2 or X.dtype != torch.float32:
        raise ValueError("X must be a 2-d float32 tensor")
    if classes and (k < 1 or (t_end > t_begin and int(flat["tree_cls_max"]) >= k)):
        raise ValueError(f"the forest holds class id {flat['tree_cls_max']} but k is {k}")
    max_f = int(flat["tree_max_feature"][t_begin:t_end].max()) if t_end > t_begin else -1
    if max_f >= X.shape[1]:
        raise ValueError(
            f"X has {X.shape[1]} columns but the forest splits on feature {max_f}"
        )
    return max_f


def flat_cat_arrays(trees):
    """Categorical part of a flat forest, on the host: (has_cat, slot,
    table). slot: int32 per global node, the node's row of table or -1 at a
    numeric node; table: (n_cat_nodes, 8) uint32 category sets. A forest
    without categorical nodes gets (False, None, None)."""
    import numpy as np

    types = [np.asarray(getattr(t, "split_type", ()), dtype=np.uint8) for t in trees]
    if not any(ty.any() for ty in types):
        return False, None, None
    split_type = np.concatenate(
        [ty if ty.size else np.zeros(t.num_nodes, np.uint8) for ty, t in zip(types, trees)]
    )
    nodes = np.flatnonzero(split_type)
    slot = np.full(split_type.size, -1, dtype=np.int32)
    slot[nodes] = np.arange(nodes.size, dtype=np.int32)
    bits = np.concatenate(
        [
            np.asarray(t.cat_bits, dtype=np.uint32).reshape(-1, 8)
            if ty.any()
            else np.zeros((t.num_nodes, 8), np.uint32)
            for ty, t in zip(types, trees)
        ]
    )
    return True, slot, np.ascontiguousarray(bits[nodes])


def make_flat_forest(trees, tree_info, weight_drop, device):
    """Flatten trees into device arrays with global node ids; leaf values
    pre-scaled by weight_drop (dart). A forest with categorical nodes also
    carries has_cat / cat_slot / cat_table (flat_cat_arrays)."""
    import numpy as np

    has_cat, cat_slot, cat_table = flat_cat_arrays(trees)
    cat = {}
    if has_cat:
        cat = {
            "has_cat": True,
            "cat_slot": torch.from_numpy(cat_slot.astype(np.int64)).to(device),
            "cat_table": torch.from_numpy(cat_table.astype(np.int64)).to(device),
        }
    offsets = np.cumsum([0] + [t.num_nodes for t in trees]).astype(np.int64)
    left = np.concatenate([t.left + (t.left >= 0) * offsets[i] for i, t in enumerate(trees)])
    right = np.concatenate([t.right + (t.right >= 0) * offsets[i] for i, t in enumerate(trees)])
    value = np.concatenate(
        [t.value * (weight_drop[i] if weight_drop else 1.0) for i, t in enumerate(trees)]
    ).astype(np.float32)
    return {
        "left": torch.from_numpy(left.astype(np.int64)).to(device),
        "right": torch.from_numpy(right.astype(np.int64)).to(device),
        "feature": torch.from_numpy(np.concatenate([t.feature for t in trees]).astype(np.int64)).to(device),
        "threshold": torch.from_numpy(np.concatenate([t.threshold for t in trees]).astype(np.float32)).to(device),
        "default_left": torch.from_numpy(np.concatenate([t.default_left for t in trees])).to(device),
        "value": torch.from_numpy(value).to(device),
        "cover": torch.from_numpy(
            np.concatenate([np.asarray(t.sum_hess, dtype=np.float32) for t in trees])
        ).to(device),
        "tree_root": torch.from_numpy(offsets[:-1].astype(np.int64)).to(device),
        "tree_cls": torch.from_numpy(np.asarray(tree_info, dtype=np.int64)).to(device),
        # host-side limits, checked before a traversal reads any row
        "tree_max_feature": tree_max_feature(trees),
        "tree_cls_max": int(max(tree_info, default=0)),
        "max_depth": max((t.max_depth() for t in trees), default=0),
        "n_trees": len(trees),
        **cat,
    }


def _native_predict(flat, X, k, t_begin, t_end, max_f):
    """Parallel C++ traversal (serving hot path on CPU hosts)."""
    from . import _smxgb_hip as K

    f = _flat_i32(flat)
    out = torch.zeros((X.shape[0], k), dtype=torch.float32)
    args = (
        X.contiguous(), f["left"], f["right"], f["feature"],
        flat["threshold"].contiguous(), f["default_left"], flat["value"].contiguous(),
        f["tree_root"], f["tree_cls"], t_begin, t_end, max_f, int(flat["tree_cls_max"]),
        out, k,
    )
    if flat.get("has_cat"):
        K.predict_forest_cat_cpu(*args, f["cat_slot"], f["cat_table"])
    else:
        K.predict_forest_cpu(*args)
    return out


def predict_forest_flat(flat, X, k, t_begin=0, t_end=None):
    """(n, k) margin contributions of trees [t_begin, t_end) — native C++
    traversal when the extension is built, else vectorized torch."""
    if t_end is None:
        t_end = flat["n_trees"]
    max_f = check_predict_args(flat, X, k, t_begin, t_end)
    n = X.shape[0]
    T = t_end - t_begin
    out = torch.zeros((n, k), dtype=torch.float32, device=X.device)
    if T <= 0:
        return out
    if X.device.type == "cpu":
        try:
            return _native_predict(flat, X, k, t_begin, t_end, max_f)
        except ImportError:
            pass
    node = flat["tree_root"][t_begin:t_end].unsqueeze(0).expand(n, T).contiguous()
    left = flat["left"]
    right = flat["right"]
    feat = flat["feature"]
    thresh = flat["threshold"]
    defl = flat["default_left"]
    cat = flat_cat_tensors(flat)
    active = left[node] >= 0
    while bool(active.any()):
        cur = node[active]
        fidx = feat[cur]
        rows = active.nonzero(as_tuple=True)[0]
        fv = X[rows, fidx]
        missing = torch.isnan(fv)
        go_left = torch.where(missing, defl[cur], goes_left(fv, thresh, cat, cur))
        node[active] = torch.where(go_left, left[cur], right[cur])
        active = left[node] >= 0
    out.index_add_(1, flat["tree_cls"][t_begin:t_end], flat["value"][node])
    return out


class TreeState:
    """Reference tree state: row-index ping-pong buffers (same contract as
    the HIP compact-layout state)."""

    def __init__(self, qm, gh, sample_rows=None):
        self.qm = qm
        self.gh = gh
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
        """Same contract as the HIP state: consume the packed split tensor
        (and, with categorical columns, the [k, 8] category sets of the same
        rows), skip gain <= 0 jobs, return a [J, 2] counters tensor."""
        sp = split_packed.detach().cpu().numpy()
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
        job_bits = None
        if cat_bits is not None and rows_of:
            job_bits = cat_bits[
                torch.as_tensor([node_rows[j] for j in rows_of], dtype=torch.long, device=cat_bits.device)
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


def make_tree_state(qm, gh, sample_rows=None, slot=0):
    return TreeState(qm, gh, sample_rows)  # CPU reference: slot unused


# ---------------------------------------------------------------------------
# Exact TreeSHAP + pred_leaf (host). C++ fast path (tree_shap_cpu /
# pred_leaf_cpu in text_parsers.cpp); pure-Python recursion as the
# no-extension fallback. Replaces the reference's native pred_contribs
# (booster.predict(pred_contribs=True), reference test_abalone.py:65).
# ---------------------------------------------------------------------------
def _flat_i32(flat):
    if "_i32" not in flat:
        flat["_i32"] = {
            "left": flat["left"].to(torch.int32).contiguous(),
            "right": flat["right"].to(torch.int32).contiguous(),
            "feature": flat["feature"].to(torch.int32).contiguous(),
            "default_left": flat["default_left"].to(torch.uint8).contiguous(),
            "tree_root": flat["tree_root"].to(torch.int32).contiguous(),
            "tree_cls": flat["tree_cls"].to(torch.int32).contiguous(),
        }
        if flat.get("has_cat"):
            table = flat["cat_table"]
            table = torch.where(table >= 2**31, table - 2**32, table)  # uint32 pattern as int32
            flat["_i32"]["cat_slot"] = flat["cat_slot"].to(torch.int32).contiguous()
            flat["_i32"]["cat_table"] = table.to(torch.int32).contiguous()
    return flat["_i32"]


def _py_tree_shap_one(flat, xr, phi, root):
    """Pure-Python exact TreeSHAP for one (row, tree) — fallback/oracle."""
    import math

    left = flat["left"].numpy()
    right = flat["right"].numpy()
    feat = flat["feature"].numpy()
    thresh = flat["threshold"].numpy()
    defl = flat["default_left"].numpy()
    value = flat["value"].numpy()
    cover = flat["cover"].numpy()

    def extend(path, zf, of, fi):
        # deep-copy elements: both recursion branches extend the same
        # parent path and must not share mutable state
        path = [list(p) for p in path] + [[fi, zf, of, 1.0 if not path else 0.0]]
        d = len(path) - 1
        for i in range(d - 1, -1, -1):
            path[i + 1][3] += of * path[i][3] * (i + 1) / (d + 1)
            path[i][3] = zf * path[i][3] * (d - i) / (d + 1)
        return path

    def unwind(path, i):
        d = len(path) - 1
        of, zf = path[i][2], path[i][1]
        out = [list(p) for p in path[:d]]
        nxt = path[d][3]
        for j in range(d - 1, -1, -1):
            if of != 0:
                tmp = out[j][3]
                out[j][3] = nxt * (d + 1) / ((j + 1) * of)
                nxt = tmp - out[j][3] * zf * (d - j) / (d + 1)
            else:
                out[j][3] = out[j][3] * (d + 1) / (zf * (d - j))
        for j in range(i, d):
            out[j][:3] = path[j + 1][:3]
        return out

    def unwound_sum(path, i):
        d = len(path) - 1
        of, zf = path[i][2], path[i][1]
        nxt = path[d][3]
        total = 0.0
        for j in range(d - 1, -1, -1):
            if of != 0:
                tmp = nxt * (d + 1) / ((j + 1) * of)
                total += tmp
                nxt = path[j][3] - tmp * zf * (d - j) / (d + 1)
            elif zf != 0:
                total += (path[j][3] / zf) * (d + 1) / (d - j)
        return total

    def rec(node, path, pzf, pof, pfi):
        path = extend(path, pzf, pof, pfi)
        l = left[node]
        if l < 0:
            for i in range(1, len(path)):
                w = unwound_sum(path, i)
                phi[path[i][0]] += w * (path[i][2] - path[i][1]) * value[node]
            return
        r = right[node]
        split = int(feat[node])
        fv = xr[split]
        hot = (l if defl[node] else r) if math.isnan(float(fv)) else (l if fv < thresh[node] else r)
        cold = r if hot == l else l
        c = cover[node] if cover[node] > 0 else 1.0
        izf, iof = 1.0, 1.0
        idx = next((i for i, p in enumerate(path) if p[0] == split), None)
        if idx is not None:
            izf, iof = path[idx][1], path[idx][2]
            path = unwind(path, idx)
        rec(hot, path, cover[hot] / c * izf, iof, split)
        rec(cold, path, cover[cold] / c * izf, 0.0, split)

    rec(root, [], 1.0, 1.0, -1)


def _py_tree_shap_cond_one(flat, xr, phi, root, condition, condition_feature):
    """Pure-Python conditional TreeSHAP for one (row, tree): Lundberg's
    form with `condition_feature` fixed on (condition=+1) or off (-1). The
    conditioned feature never enters the path; it scales the leaf value
    through the condition fraction. Fallback/oracle for interactions."""
    import math

    left = flat["left"].numpy()
    right = flat["right"].numpy()
    feat = flat["feature"].numpy()
    thresh = flat["threshold"].numpy()
    defl = flat["default_left"].numpy()
    value = flat["value"].numpy()
    cover = flat["cover"].numpy()

    def leaf_weights(elems):
        """Unwound sums of a finished path: elems = [(feature, z, o)],
        duplicate-free. Returns one permutation-weight sum per element."""
        path = [[-1, 1.0, 1.0, 1.0]]
        for fi, zf, of in elems:
            path.append([fi, zf, of, 0.0])
            d = len(path) - 1
            for i in range(d - 1, -1, -1):
                path[i + 1][3] += of * path[i][3] * (i + 1) / (d + 1)
                path[i][3] = zf * path[i][3] * (d - i) / (d + 1)
        d = len(path) - 1
        sums = []
        for i in range(1, d + 1):
            of, zf = path[i][2], path[i][1]
            nxt = path[d][3]
            total = 0.0
            for j in range(d - 1, -1, -1):
                if of != 0:
                    tmp = nxt * (d + 1) / ((j + 1) * of)
                    total += tmp
                    nxt = path[j][3] - tmp * zf * (d - j) / (d + 1)
                elif zf != 0:
                    total += (path[j][3] / zf) * (d + 1) / (d - j)
            sums.append(total)
        return sums

    def rec(node, elems, cond_fraction):
        if cond_fraction == 0.0:
            return
        l = left[node]
        if l < 0:
            for (fi, zf, of), w in zip(elems, leaf_weights(elems)):
                phi[fi] += w * (of - zf) * value[node] * cond_fraction
            return
        r = right[node]
        split = int(feat[node])
        fv = xr[split]
        hot = (l if defl[node] else r) if math.isnan(float(fv)) else (l if fv < thresh[node] else r)
        cold = r if hot == l else l
        c = float(cover[node]) if cover[node] > 0 else 1.0
        hz, cz = float(cover[hot]) / c, float(cover[cold]) / c
        if split == condition_feature:
            if condition > 0:
                rec(hot, elems, cond_fraction)
            else:
                rec(hot, elems, cond_fraction * hz)
                rec(cold, elems, cond_fraction * cz)
            return
        izf, iof = 1.0, 1.0
        rest = elems
        for idx, (fi, zf, of) in enumerate(elems):
            if fi == split:  # merge with the earlier split on this feature
                izf, iof = zf, of
                rest = elems[:idx] + elems[idx + 1:]
                break
        rec(hot, rest + [(split, hz * izf, iof)], cond_fraction)
        rec(cold, rest + [(split, cz * izf, 0.0)], cond_fraction)

    rec(root, [], 1.0)


def tree_shap(flat, X, k, t_begin=0, t_end=None, condition=0, condition_feature=-1):
    """Exact TreeSHAP contributions: (n, k, f+1) float64 (bias column NOT
    filled — the booster adds expected values + base margin).

    `condition` = +1 / -1 computes Lundberg's conditional contributions
    with `condition_feature` fixed on / off (the building block of the
    interaction values); the default 0 is plain TreeSHAP."""
    refuse_categorical(flat, "TreeSHAP")
    if t_end is None:
        t_end = flat["n_trees"]
    X = X.cpu().contiguous()
    n, f = X.shape
    phi = torch.zeros((n, k, f + 1), dtype=torch.float64)
    if t_end <= t_begin:
        return phi
    try:
        from . import _smxgb_hip as K

        i32 = _flat_i32(flat)
        args = (
            X, i32["left"], i32["right"], i32["feature"],
            flat["threshold"].contiguous(), i32["default_left"],
            flat["value"].contiguous(), flat["cover"].contiguous(),
            i32["tree_root"], i32["tree_cls"], t_begin, t_end, phi, k,
            int(flat.get("max_depth", 32)),
        )
        if condition:
            K.tree_shap_cpu(*args, int(condition), int(condition_feature))
        else:
            K.tree_shap_cpu(*args)
        return phi
    except ImportError:
        pass
    Xn = X.numpy()
    roots = flat["tree_root"].numpy()
    cls = flat["tree_cls"].numpy()
    phi_np = phi.numpy()
    for row in range(n):
        for t in range(t_begin, t_end):
            if condition:
                _py_tree_shap_cond_one(
                    flat, Xn[row], phi_np[row, cls[t]], int(roots[t]),
                    condition, condition_feature,
                )
            else:
                _py_tree_shap_one(flat, Xn[row], phi_np[row, cls[t]], int(roots[t]))
    return phi


def split_features(flat, t_begin=0, t_end=None):
    """Sorted feature indices that trees [t_begin, t_end) split on."""
    if t_end is None:
        t_end = flat["n_trees"]
    if t_end <= t_begin:
        return []
    roots = flat["tree_root"]
    s = int(roots[t_begin])
    e = int(roots[t_end]) if t_end < flat["n_trees"] else flat["left"].shape[0]
    internal = flat["left"][s:e] >= 0
    return sorted(int(v) for v in torch.unique(flat["feature"][s:e][internal]))


def tree_shap_interactions(flat, X, k, t_begin=0, t_end=None):
    """Exact TreeSHAP interaction values: (n, k, f+1, f+1) float64.

    For every feature j the forest splits on, off-diagonal column j is half
    the difference of the contributions conditioned on j being on and off;
    features the forest never splits on interact with nothing. The diagonal
    is phi_i - sum_{j != i} phi_int[i, j]; the bias row/column stay zero
    (the booster fills cell [f, f])."""
    refuse_categorical(flat, "TreeSHAP interactions")
    if t_end is None:
        t_end = flat["n_trees"]
    n, f = X.shape
    out = torch.zeros((n, k, f + 1, f + 1), dtype=torch.float64)
    if t_end <= t_begin or n == 0:
        return out
    phi = tree_shap(flat, X, k, t_begin, t_end)
    for j in split_features(flat, t_begin, t_end):
        on = tree_shap(flat, X, k, t_begin, t_end, condition=1, condition_feature=j)
        off = tree_shap(flat, X, k, t_begin, t_end, condition=-1, condition_feature=j)
        out[:, :, :, j] = (on - off) / 2
        out[:, :, j, j] = 0.0
    diag = phi - out.sum(dim=3)
    out.diagonal(dim1=2, dim2=3).copy_(diag)
    return out


def saabas_contribs(flat, X, k, t_begin=0, t_end=None):
    """Saabas path attribution (xgboost approx_contribs=True) over the flat
    forest, vectorized on whatever device X and the flat forest live on:
    (n, k, f+1) float64. Walking each (row, tree) root -> leaf, the change
    of the node expectation value[next] - value[cur] is credited to the
    split feature; the bias column collects the root values."""
    refuse_categorical(flat, "Saabas attribution")
    if t_end is None:
        t_end = flat["n_trees"]
    n, f = X.shape
    T = t_end - t_begin
    phi = torch.zeros((n, k, f + 1), dtype=torch.float64, device=X.device)
    if T <= 0 or n == 0:
        return phi
    left = flat["left"].long()
    right = flat["right"].long()
    feat = flat["feature"].long()
    thresh = flat["threshold"]
    defl = flat["default_left"].to(torch.bool)
    value = flat["value"].to(torch.float64)
    roots = flat["tree_root"][t_begin:t_end].long()
    cls = flat["tree_cls"][t_begin:t_end].long()
    phi[:, :, f].index_add_(1, cls, value[roots].unsqueeze(0).expand(n, T).contiguous())
    node = roots.unsqueeze(0).expand(n, T).contiguous()
    cls_nt = cls.unsqueeze(0).expand(n, T)
    flat_phi = phi.view(-1)
    active = left[node] >= 0
    while bool(active.any()):
        cur = node[active]
        rows = active.nonzero(as_tuple=True)[0]
        fidx = feat[cur]
        fv = X[rows, fidx]
        go_left = torch.where(torch.isnan(fv), defl[cur], fv < thresh[cur])
        nxt = torch.where(go_left, left[cur], right[cur])
        flat_phi.index_add_(
            0, (rows * k + cls_nt[active]) * (f + 1) + fidx, value[nxt] - value[cur]
        )
        node[active] = nxt
        active = left[node] >= 0
    return phi


def tree_expected_values(flat, k, t_begin=0, t_end=None):
    """Per-class expected margin of trees [t_begin, t_end): sum over trees
    of the cover-weighted leaf mean (the TreeSHAP bias term)."""
    if t_end is None:
        t_end = flat["n_trees"]
    left = flat["left"]
    value = flat["value"].to(torch.float64)
    cover = flat["cover"].to(torch.float64)
    roots = flat["tree_root"]
    cls = flat["tree_cls"]
    n_nodes = left.shape[0]
    bounds = torch.cat([roots, torch.tensor([n_nodes], dtype=roots.dtype)])
    ev = torch.zeros(k, dtype=torch.float64)
    leaf = left < 0
    for t in range(t_begin, t_end):
        s, e = int(bounds[t]), int(bounds[t + 1])
        lmask = leaf[s:e]
        croot = float(cover[s])
        if croot <= 0:
            continue
        ev[cls[t]] += float((value[s:e][lmask] * cover[s:e][lmask]).sum()) / croot
    return ev


def pred_leaf(flat, X, t_begin=0, t_end=None):
    """(n, T) int32 tree-local leaf indices (xgboost pred_leaf=True)."""
    if t_end is None:
        t_end = flat["n_trees"]
    X = X.cpu().contiguous()
    max_f = check_predict_args(flat, X, 1, t_begin, t_end, classes=False)
    n = X.shape[0]
    T = t_end - t_begin
    out = torch.zeros((n, T), dtype=torch.int32)
    if T <= 0:
        return out
    try:
        from . import _smxgb_hip as K

        i32 = _flat_i32(flat)
        args = (
            X, i32["left"], i32["right"], i32["feature"],
            flat["threshold"].contiguous(), i32["default_left"],
            i32["tree_root"], t_begin, t_end, max_f, out,
        )
        if flat.get("has_cat"):
            K.pred_leaf_cat_cpu(*args, i32["cat_slot"], i32["cat_table"])
        else:
            K.pred_leaf_cpu(*args)
        return out
    except ImportError:
        pass
    # vectorized torch fallback: iterate depth levels for all (row, tree)
    left = flat["left"]
    right = flat["right"]
    feat = flat["feature"]
    thresh = flat["threshold"]
    defl = flat["default_left"]
    roots = flat["tree_root"][t_begin:t_end]
    cat = flat_cat_tensors(flat)
    node = roots.unsqueeze(0).expand(n, T).contiguous()
    active = left[node] >= 0
    while bool(active.any()):
        nid = node[active]
        fv = X[active.any(dim=1).nonzero(as_tuple=True)[0], :] if False else None  # noqa
        rows = active.nonzero(as_tuple=True)[0]
        fvals = X[rows, feat[nid]]
        goleft = torch.where(
            torch.isnan(fvals), defl[nid].to(torch.bool), goes_left(fvals, thresh, cat, nid)
        )
        node[active] = torch.where(goleft, left[nid], right[nid]).to(node.dtype)
        active = left[node] >= 0
    return (node - roots.unsqueeze(0)).to(torch.int32)
