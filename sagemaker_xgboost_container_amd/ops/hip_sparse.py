"""CDNA4 HIP backend for CSR data (MI355X sparse training and prediction).

The device twin of ops/sparse_ref.py: a SparseQuantizedMatrix that lives on
the GPU (`quantize_csr`, or `SparseQuantizedMatrix.to(device)`) trains
without ever becoming an n x f bin matrix. Same backend interface as sparse_ref / hip
(make_tree_state, compute_scale, hist_to_float, find_splits,
predict_tree_csr), so models/grower.py runs its per-level and lossguide
loops unchanged. Kernels: csrc/smxgb_sparse.hip.

* histograms: `hist_sparse` adds the fixed-point (g, h) of every stored
  entry with global u64 atomics (f * stride slots do not fit LDS for wide
  data) and sums each segment's rows once; `hist_sparse_close` writes each
  feature's missing slot as segment total - present bins. In int64 that is
  exact: the accumulator equals hip.build_histograms on the dense bin matrix
  of the same data bit for bit.
* partition: `partition_sparse` finds the split feature in a row's sorted
  column ids by binary search (absent = default direction); every split
  node of a level goes in one launch, counters are read back once per level
  by the grower.
* margins of eval sets and warm-start replay: `predict_tree_csr` over the
  raw CSR values, equal to hip.predict_tree on the NaN-densified rows.
* Booster.predict on a sparse DMatrix: `predict_forest_csr` (margins) and
  `pred_leaf_csr` (leaf ids) run a whole hip.make_flat_forest dict over a
  DeviceCSR in one launch. A block owns R consecutive rows and every tree
  chunk (or tree) of them, stages the rows' entries in LDS when they fit
  PREDICT_CSR_TILE and binary-searches there at every split node; longer
  groups search global memory. The (row, tree-chunk) items, the tree order
  inside a chunk and the fixed-order chunk reduce are the dense kernel's, so
  the results equal hip.predict_forest_flat / hip.pred_leaf on the
  NaN-densified rows bit for bit.
* exact TreeSHAP contributions over a DeviceCSR: hip.tree_shap_compact (the
  compact-slot kernel of csrc/smxgb_shap_compact.hip with a binary-search
  row accessor), bit-equal to its dense accessor on the NaN-densified rows.
  Interaction values over CSR are not implemented.

* quantization: `quantize_csr` finds the cuts and bins the stored entries
  of an unweighted scipy CSR matrix on the device (csrc/smxgb_quantize_csr.hip)
  and returns the device matrix directly; weighted and distributed data are
  quantized by sparse_ref.quantize_sparse on the host and moved with `.to`.

There is no DeviceGrower for this layout: HistGrower.grow_path stays
"per_level", which mirrors the device grower's float32 node arithmetic
(MIRRORS_DEVICE_GROWER) so the trees equal the dense device path's.
"""
import numpy as np
import torch

from . import hip
from .hip import _K, _MAX_BLOCKS_PER_JOB, _pack_jobs_and_map

NAME = "hip_sparse"
MIRRORS_DEVICE_GROWER = True

# layout-agnostic pieces of the dense device backend
compute_scale = hip.compute_scale
hist_to_float = hip.hist_to_float
find_splits = hip.find_splits
# gradient-based row sampling reads the dense (n, 2) gradients only
mvs_threshold = hip.mvs_threshold
gradient_sample = hip.gradient_sample
# so does the per-leaf quantile of adaptive tree leaves: (pos, resid, weight)
leaf_quantiles = hip.leaf_quantiles

# rows of a segment per block. A row costs its stored entries (tens for the
# wide data this path is for, against f for a dense row), so blocks take
# fewer rows than the dense kernels' 4096 to keep every CU issuing atomics.
_HIST_ROWS_PER_BLOCK = 1024
_PART_ROWS_PER_BLOCK = 4096  # one SPART_TILE


# -- quantization ---------------------------------------------------------------
# Longest feature segment (stored entries of one column) that quantize_csr
# sorts in LDS; longer ones go through the radix select of hip.make_cuts.
QUANTIZE_CSR_SORT_CAP = int(_K.quantize_csr_sort_cap())
_QUANTIZE_CSR_WAVE_CAP = int(_K.quantize_csr_wave_cap())


def _long_segment_cuts(keys, csc_ptr, heavy, m, max_bin, ranks, ridx, cuts_pad, ncut):
    """Cuts of the features `heavy` (host ids, segments longer than the sort
    cap) by hip.make_cuts' three radix passes over their key segments, in
    chunks of features whose counters fit hip.QUANTIZE_COUNTER_BYTES."""
    dev = keys.device
    A, T = max_bin, max_bin - 1
    Tp = max(T, 1)
    i32 = dict(dtype=torch.int32, device=dev)
    none = torch.empty(0, **i32)
    per_feature = A * hip._QZ_DIGITS
    chunk = max(1, min(hip.QUANTIZE_COUNTER_BYTES // (4 * per_feature),
                       ((1 << 31) - 1) // per_feature, 65535, heavy.size))
    counts = torch.empty(chunk * per_feature, **i32)
    for c0 in range(0, heavy.size, chunk):
        ids = heavy[c0:c0 + chunk]
        fc = ids.size
        ids32 = torch.from_numpy(ids.astype(np.int32)).to(dev)
        ids64 = ids32.long()
        mc = torch.from_numpy(m[ids].astype(np.int32)).to(dev)
        rc = ridx[ids64].contiguous()
        max_len = int(m[ids].max())
        act = [torch.empty(fc * A, **i32) for _ in range(2)]
        nact = [torch.empty(fc, **i32) for _ in range(2)]
        state = torch.empty(3 * fc * Tp, **i32)
        flag = torch.empty(fc, **i32)
        counts1 = torch.zeros(fc * hip._QZ_DIGITS, **i32)
        cnt = counts[: fc * per_feature]

        def refine(p, table, src, dst):
            _K.quantize_refine(p, table, act[src], nact[src], act[dst], nact[dst], A, max_bin,
                               mc, ranks, rc, T, state, flag)

        _K.quantize_csr_hist(keys, csc_ptr, ids32, max_len, 1, none, none, A, counts1)
        refine(1, counts1, 1, 0)
        cnt.zero_()
        _K.quantize_csr_hist(keys, csc_ptr, ids32, max_len, 2, act[0], nact[0], A, cnt)
        refine(2, cnt, 0, 1)
        cnt.zero_()
        _K.quantize_csr_hist(keys, csc_ptr, ids32, max_len, 3, act[1], nact[1], A, cnt)
        refine(3, cnt, 1, 0)
        pad = torch.empty((fc, Tp), dtype=torch.float32, device=dev)
        nc = torch.empty(fc, **i32)
        _K.quantize_final(act[0], nact[0], A, mc, flag, pad, Tp, nc)
        cuts_pad[ids64] = pad
        ncut[ids64] = nc


def quantize_csr(csr, max_bin=256, device="cuda"):
    """The SparseQuantizedMatrix of an unweighted scipy CSR matrix, built on
    the ROCm device: what sparse_ref.quantize_sparse(csr, max_bin).to(device)
    returns, array for array and bit for bit, without its per-feature host
    loop (kernels: csrc/smxgb_quantize_csr.hip).

    The stored entries are counted per column and their keys scattered to a
    CSC image; a feature of at most QUANTIZE_CSR_SORT_CAP entries is sorted in
    LDS and cut there, a longer one goes through the radix select of
    hip.make_cuts; one more kernel bins the entries in CSR order. The counts
    are read back once: they size the job lists, and the target ranks come
    from the reference's own linspace expression, once per distinct count.
    Peak device memory is the CSR arrays, 4 bytes a stored entry for the
    keys, the bins, f * max(max_bin - 1, 1) floats of padded cuts and at most
    hip.QUANTIZE_COUNTER_BYTES; nothing of n x f size exists.

    `csr` is not modified (unsorted column ids are sorted in a copy). A
    stored NaN, or an empty matrix, returns the host result."""
    from .sparse_ref import SparseQuantizedMatrix, quantize_sparse

    max_bin = int(max_bin)
    if not 1 <= max_bin <= hip.MAX_HIST_STRIDE:
        raise ValueError(f"max_bin must be in [1, {hip.MAX_HIST_STRIDE}]")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError("quantize_csr needs a ROCm device")
    csr = csr.tocsr()
    n, f = csr.shape
    nnz = int(csr.indptr[-1]) if n else 0
    if nnz >= 1 << 31:
        raise ValueError("quantize_csr takes fewer than 2^31 stored entries")
    if n == 0 or f == 0 or nnz == 0:
        return quantize_sparse(csr, max_bin).to(dev)
    if not csr.has_sorted_indices:
        csr = csr.sorted_indices()
    indptr = np.asarray(csr.indptr, dtype=np.int64)
    if indptr.shape[0] != n + 1 or indptr[0] != 0 or csr.indices.shape[0] != nnz \
            or csr.data.shape[0] != nnz or (np.diff(indptr) < 0).any():
        raise ValueError("malformed CSR offsets")
    i32 = dict(dtype=torch.int32, device=dev)
    indices = torch.from_numpy(np.asarray(csr.indices, dtype=np.int32)).to(dev)
    values = torch.from_numpy(np.asarray(csr.data, dtype=np.float32)).to(dev)

    counts = torch.zeros(f + 1, **i32)
    _K.quantize_csr_count(indices, values, counts)
    counts_host = counts.cpu().numpy()  # the one readback the job lists need
    if counts_host[f] & 2:
        raise ValueError("CSR column ids out of range")
    if counts_host[f] & 1:  # the host code owns the rule for a stored NaN
        return quantize_sparse(csr, max_bin).to(dev)
    m = counts_host[:f].astype(np.int64)
    csc_ptr = torch.zeros(f + 1, **i32)
    csc_ptr[1:] = torch.cumsum(counts[:f], 0, dtype=torch.int32)
    keys = torch.empty(nnz, **i32)
    _K.quantize_csr_scatter(indices, values, csc_ptr[:f].clone(), keys)

    T = max_bin - 1
    Tp = max(T, 1)
    sizes = np.unique(m[m > max_bin])
    if T > 0 and sizes.size:
        ranks = torch.stack([
            # ops/quantize._feature_cuts_sorted's positions, to the letter
            torch.linspace(0, int(v) - 1, max_bin + 1)[1:-1].round().long() for v in sizes
        ]).to(torch.int32).to(dev)
        ridx = np.minimum(np.searchsorted(sizes, m), sizes.size - 1)
    else:
        ranks = torch.zeros((1, Tp), **i32)
        ridx = np.zeros(f, dtype=np.int64)
    ridx = torch.from_numpy(ridx.astype(np.int32)).to(dev)

    cuts_pad = torch.empty((f, Tp), dtype=torch.float32, device=dev)
    ncut = torch.zeros(f, **i32)  # a feature with fewer than two entries has no cut
    below, P = 1, _QUANTIZE_CSR_WAVE_CAP
    while P <= QUANTIZE_CSR_SORT_CAP:  # one job list per size class
        jobs = np.flatnonzero((m > below) & (m <= P))
        if jobs.size:
            _K.quantize_csr_sort(keys, csc_ptr, torch.from_numpy(jobs.astype(np.int32)).to(dev),
                                 P, max_bin, ranks, ridx, cuts_pad, Tp, ncut)
        below, P = P, 2 * P
    heavy = np.flatnonzero(m > QUANTIZE_CSR_SORT_CAP)
    if heavy.size:
        _long_segment_cuts(keys, csc_ptr, heavy, m, max_bin, ranks, ridx, cuts_pad, ncut)
    del keys

    cut_ptr = torch.zeros(f + 1, dtype=torch.int64, device=dev)
    cut_ptr[1:] = torch.cumsum(ncut, 0, dtype=torch.int64)
    total, widest = torch.stack([cut_ptr[-1], ncut.max().long()]).tolist()  # the sizes
    cuts = torch.empty(total, dtype=torch.float32, device=dev)
    if total:
        _K.quantize_compact(cuts_pad, Tp, ncut, cut_ptr, cuts)
    del cuts_pad
    stride = widest + 2  # the widest feature's bins and the missing slot
    bins = torch.empty(nnz, dtype=torch.uint8 if stride <= 256 else torch.int16, device=dev)
    _K.quantize_csr_bin(indices, values, cuts, cut_ptr, bins)
    return SparseQuantizedMatrix(
        csr_bins=(torch.from_numpy(indptr).to(dev), indices, bins),
        csc=(None, None, None),
        cuts=cuts, cut_ptr=cut_ptr, nbins=ncut.to(torch.int64) + 1,
        stride=stride, num_row=n, num_col=f,
    )


def _blocks(rows, per_block):
    return int(max(1, min((rows + per_block - 1) // per_block, _MAX_BLOCKS_PER_JOB)))


def _check_qm(qm):
    if not qm.bin_data.is_cuda:
        raise ValueError("hip_sparse needs a SparseQuantizedMatrix on a ROCm device (qm.to(device))")
    if qm.indices.dtype != torch.int32 or qm.indptr.dtype != torch.int64:
        raise ValueError("device CSR needs int64 offsets and int32 column ids (qm.to(device))")


def _check_segments(segs, cap):
    for start, end in segs:
        if not (0 <= start <= end <= cap):
            raise ValueError(f"segment [{start}, {end}) outside the row buffer of {cap} rows")


def build_histograms(qm, gh, rowbuf, jobs, scale):
    """(J, f*stride, 2) int64 fixed-point histograms over row segments of a
    device sparse qm; `scale` is the device (gmax, hmax) tensor."""
    _check_qm(qm)
    _check_segments(jobs, rowbuf.numel())
    if not isinstance(scale, torch.Tensor):
        raise ValueError("hip_sparse derives the fixed-point scale on device: pass compute_scale()'s tensor")
    f = qm.num_col
    stride = qm.stride
    device = qm.bin_data.device
    acc = torch.zeros((len(jobs), f * stride, 2), dtype=torch.int64, device=device)
    if not jobs:
        return acc
    totals = torch.zeros((len(jobs), 2), dtype=torch.int64, device=device)
    packed = []
    blocks_per = []
    first_block = 0
    for hist_idx, (start, end) in enumerate(jobs):
        nb = _blocks(end - start, _HIST_ROWS_PER_BLOCK)
        packed.append((start, end, hist_idx, 0, f, first_block, nb))
        blocks_per.append(nb)
        first_block += nb
    jobs_dev, block_job = _pack_jobs_and_map(packed, blocks_per)
    _K.hist_sparse(
        qm.indptr, qm.indices, qm.bin_data, gh.contiguous(), rowbuf, jobs_dev, block_job,
        acc, totals, f, stride, scale.to(torch.float32).contiguous(),
    )
    _K.hist_sparse_close(acc, totals, f, stride)
    return acc


def partition_level(qm, src, dst, segs, node_rows, split_packed):
    """Partition every segment whose row of the on-device packed split
    tensor has gain > 0; returns the DEVICE counters tensor [J, 2]."""
    _check_qm(qm)
    _check_segments(segs, src.numel())
    counters = torch.zeros((len(segs), 2), dtype=torch.int32, device=src.device)
    if not segs:
        return counters
    k = split_packed.shape[0]
    packed = []
    blocks_per = []
    first_block = 0
    for (start, end), node_row in zip(segs, node_rows):
        if not (0 <= int(node_row) < k):
            raise ValueError(f"split row {node_row} outside the packed split tensor of {k} rows")
        nb = _blocks(end - start, _PART_ROWS_PER_BLOCK)
        packed.append((start, end, int(node_row), 0, 0, first_block, nb))
        blocks_per.append(nb)
        first_block += nb
    jobs_dev, block_job = _pack_jobs_and_map(packed, blocks_per)
    _K.partition_sparse(
        qm.indptr, qm.indices, qm.bin_data, src, dst, jobs_dev, block_job,
        split_packed.to(torch.float32).contiguous(), counters,
    )
    return counters


class TreeState:
    """Row-id ping-pong buffers (int32) over a device SparseQuantizedMatrix."""

    def __init__(self, qm, gh, sample_rows=None):
        _check_qm(qm)
        self.qm = qm
        self.gh = gh.contiguous()
        device = qm.bin_data.device
        rows = (
            sample_rows.to(device=device, dtype=torch.int32)
            if sample_rows is not None
            else torch.arange(qm.num_row, dtype=torch.int32, device=device)
        )
        self.cap = rows.numel()
        self._bufs = (rows.clone(), torch.empty_like(rows))

    def build_histograms(self, jobs, parity, scale):
        return build_histograms(self.qm, self.gh, self._bufs[parity], jobs, scale)

    def partition_level(self, segs, node_rows, split_packed, src_parity):
        return partition_level(
            self.qm, self._bufs[src_parity], self._bufs[1 - src_parity],
            segs, node_rows, split_packed,
        )

    def update_margins(self, margin_col, leaf_jobs):
        hip.update_margins(margin_col, self._bufs, leaf_jobs)


def make_tree_state(qm, gh, sample_rows=None, slot=0):
    return TreeState(qm, gh, sample_rows)


# -- sparse prediction ---------------------------------------------------------
class DeviceCSR:
    """Raw CSR values on the device (int64 offsets, sorted int32 column ids,
    float32 data) for predict_tree_csr; upload once, traverse every round."""

    def __init__(self, csr, device):
        csr = csr.tocsr()
        if not csr.has_sorted_indices:
            csr = csr.sorted_indices()
        n, f = csr.shape
        indptr = np.asarray(csr.indptr, dtype=np.int64)
        indices = np.asarray(csr.indices, dtype=np.int32)
        if indptr[0] != 0 or indptr[-1] != indices.shape[0] or (np.diff(indptr) < 0).any():
            raise ValueError("malformed CSR offsets")
        if indices.size and (indices.min() < 0 or indices.max() >= f):
            raise ValueError("CSR column ids out of range")
        self.shape = (n, f)
        self.indptr = torch.from_numpy(indptr).to(device)
        self.indices = torch.from_numpy(indices).to(device)
        self.data = torch.from_numpy(np.asarray(csr.data, dtype=np.float32)).to(device)


def predict_tree_csr(tree, csr, device=None):
    """(n,) device margin contribution of one tree over CSR rows. `csr` is a
    DeviceCSR, or a scipy matrix uploaded to `device` for this call."""
    if not isinstance(csr, DeviceCSR):
        csr = DeviceCSR(csr, device if device is not None else torch.device("cuda"))
    dev = csr.data.device
    if getattr(tree, "has_categorical", False):
        raise NotImplementedError("CSR traversal is not implemented for categorical splits")
    split = tree.left >= 0
    if split.any() and int(tree.feature[split].max()) >= csr.shape[1]:
        raise ValueError("tree splits on a feature the matrix does not have")
    flat = hip._FlatForest([tree], [0], dev)
    out = torch.empty(csr.shape[0], dtype=torch.float32, device=dev)
    _K.predict_tree_csr(
        csr.indptr, csr.indices, csr.data,
        flat.left, flat.right, flat.feat, flat.thresh, flat.defl, flat.value, out,
    )
    return out


# -- whole-forest prediction over CSR rows ---------------------------------------
# Knobs of predict_forest_csr_kernel / pred_leaf_csr_kernel (values and the
# sweep behind them: profiles/r08_sparse_predict.md). A block owns R
# consecutive rows and every tree chunk (or tree) of them, R ~ block items /
# chunks; a group of at most PREDICT_CSR_TILE stored entries is searched in
# LDS, a longer one in global memory.
PREDICT_CSR_TILE = 8192          # entries; 8 bytes each of dynamic LDS (64 KiB)
PREDICT_CSR_BLOCK_ITEMS = 256    # (row, chunk) items a block is sized for
_PREDICT_CSR_MAX_TILE = 8192     # PCSR_MAX_TILE in the kernel source

_FLAT_DTYPES = (
    ("left", torch.int32), ("right", torch.int32), ("feature", torch.int32),
    ("threshold", torch.float32), ("default_left", torch.uint8), ("value", torch.float32),
    ("tree_root", torch.int32), ("tree_cls", torch.int32),
)


def _rows_per_group(n_inner):
    return max(1, PREDICT_CSR_BLOCK_ITEMS // max(1, n_inner))


def _check_forest_csr(flat, dcsr, t_begin, t_end):
    """Host-side validation shared by the two forest launchers; returns the
    resolved t_end. Raises ValueError before anything is launched."""
    if not isinstance(dcsr, DeviceCSR):
        raise ValueError("expected a hip_sparse.DeviceCSR (upload the matrix once, predict many times)")
    if flat.get("has_cat"):
        raise NotImplementedError("CSR forest traversal is not implemented for categorical splits")
    if t_end is None:
        t_end = flat["n_trees"]
    if not (0 <= t_begin <= t_end <= flat["n_trees"]):
        raise ValueError(f"tree range [{t_begin}, {t_end}) out of bounds")
    for name, t, dt in (
        ("indptr", dcsr.indptr, torch.int64), ("indices", dcsr.indices, torch.int32),
        ("data", dcsr.data, torch.float32),
    ):
        if not t.is_cuda or t.dtype != dt or not t.is_contiguous() or t.dim() != 1:
            raise ValueError(f"device CSR {name} must be a contiguous 1-d {dt} ROCm tensor")
    n = dcsr.shape[0]
    if dcsr.indptr.numel() != n + 1 or dcsr.data.numel() != dcsr.indices.numel():
        raise ValueError("device CSR arrays do not match the matrix shape")
    for name, dt in _FLAT_DTYPES:
        t = flat[name]
        if not t.is_cuda or t.dtype != dt or not t.is_contiguous() or t.device != dcsr.data.device:
            raise ValueError(f"flat forest '{name}' must be a contiguous {dt} tensor on the matrix's device")
    if not (0 <= PREDICT_CSR_TILE <= _PREDICT_CSR_MAX_TILE):
        raise ValueError(f"PREDICT_CSR_TILE must be within [0, {_PREDICT_CSR_MAX_TILE}] entries")
    if t_end > t_begin:
        max_f = int(flat["tree_max_feature"][t_begin:t_end].max())
        if max_f >= dcsr.shape[1]:
            raise ValueError(
                f"the matrix has {dcsr.shape[1]} columns but the forest splits on feature {max_f}"
            )
    return t_end


def predict_forest_csr(flat, dcsr, k, t_begin=0, t_end=None):
    """(n, k) float32 summed margin contributions of trees [t_begin, t_end)
    of a hip.make_flat_forest dict over a DeviceCSR. Equal, bit for bit, to
    hip.predict_forest_flat on the NaN-densified rows: same (row, tree-chunk)
    items, same tree order inside a chunk, same fixed-order chunk reduce."""
    t_end = _check_forest_csr(flat, dcsr, t_begin, t_end)
    k = int(k)
    if k < 1 or (t_end > t_begin and int(flat["tree_cls_max"]) >= k):
        raise ValueError(f"k = {k} outputs do not cover the forest's class ids")
    n = dcsr.shape[0]
    dev = dcsr.data.device
    T = t_end - t_begin
    if n == 0 or T == 0:
        return torch.zeros((n, k), dtype=torch.float32, device=dev)
    n_chunks, tpc = hip._predict_chunking(n, T)
    part = torch.zeros((n_chunks, n, k), dtype=torch.float32, device=dev)
    _K.predict_forest_csr(
        dcsr.indptr, dcsr.indices, dcsr.data,
        flat["left"], flat["right"], flat["feature"], flat["threshold"],
        flat["default_left"], flat["value"], flat["tree_root"], flat["tree_cls"],
        t_begin, t_end, part, k, n_chunks, tpc, _rows_per_group(n_chunks), PREDICT_CSR_TILE,
    )
    return part.sum(0) if n_chunks > 1 else part[0]


def pred_leaf_csr(flat, dcsr, t_begin=0, t_end=None):
    """(n, T) int32 tree-local leaf indices of trees [t_begin, t_end) over a
    DeviceCSR; equal to hip.pred_leaf on the NaN-densified rows."""
    t_end = _check_forest_csr(flat, dcsr, t_begin, t_end)
    n = dcsr.shape[0]
    T = t_end - t_begin
    out = torch.zeros((n, T), dtype=torch.int32, device=dcsr.data.device)
    if n == 0 or T == 0:
        return out
    _K.pred_leaf_csr(
        dcsr.indptr, dcsr.indices, dcsr.data,
        flat["left"], flat["right"], flat["feature"], flat["threshold"],
        flat["default_left"], flat["value"], flat["tree_root"], flat["tree_cls"],
        t_begin, t_end, out, _rows_per_group(T), PREDICT_CSR_TILE,
    )
    return out
