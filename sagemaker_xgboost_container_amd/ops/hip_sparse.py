"""CDNA4 HIP backend for CSR data (MI355X sparse training and prediction).

The device twin of ops/sparse_ref.py: a SparseQuantizedMatrix that lives on
the GPU (`SparseQuantizedMatrix.to(device)`) trains without ever becoming an
n x f bin matrix. Same backend interface as sparse_ref / hip
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
