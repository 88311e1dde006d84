"""CDNA4 HIP backend for quantized CSR data (MI355X sparse training path).

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
