"""Device CSR kernels (ops/hip_sparse.py, csrc/smxgb_sparse.hip) against the
dense HIP kernels on the SAME bins: every comparison is exact.

The dense twin of a SparseQuantizedMatrix is built by scattering its bin ids
into an n x f matrix pre-filled with the missing slot (stride - 1), with the
sparse matrix's own cuts, so cut finding cannot differ between the two.

All tests require an MI355X (pytest tests -m gpu).
"""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from sagemaker_xgboost_container_amd.models.tree import Tree
    from sagemaker_xgboost_container_amd.ops import backend_for_qm, hip, hip_sparse
    from sagemaker_xgboost_container_amd.ops.quantize import QuantizedMatrix
    from sagemaker_xgboost_container_amd.ops.sparse_ref import quantize_sparse
else:  # allow collection on CPU boxes
    Tree = backend_for_qm = hip = hip_sparse = QuantizedMatrix = quantize_sparse = None


def _blank_rows(n):
    """A run of rows that store nothing (none for tiny n)."""
    if n < 10:
        return 0, 0
    return n // 3, n // 3 + max(1, n // 10)


def _rand_csr(n, f, density, seed, eighths):
    """Random CSR with a run of empty rows and (f >= 2) an empty last column.
    `eighths` rounds values to multiples of 1/8 (few distinct values per
    feature: uint8 bins); otherwise they are continuous."""
    rng = np.random.default_rng(seed)
    mask = rng.random((n, f)) < density
    b0, b1 = _blank_rows(n)
    mask[b0:b1] = False
    if f >= 2:
        mask[:, f - 1] = False
    vals = rng.normal(size=(n, f)).astype(np.float32)
    if eighths:
        vals = np.round(vals * 8) / 8
    rows, cols = np.nonzero(mask)
    # explicit (rows, cols, data): stored zeros stay stored entries
    return sp.csr_matrix((vals[rows, cols], (rows, cols)), shape=(n, f), dtype=np.float32)


class _Problem:
    def __init__(self, n, f, density, max_bin, seed=0):
        self.n, self.f = n, f
        self.csr = _rand_csr(n, f, density, seed, eighths=(max_bin == 256))
        host = quantize_sparse(self.csr, max_bin=max_bin)
        self.sqm = host.to("cuda")
        # dense twin from the same bins
        bins = torch.full((n, f), host.stride - 1, dtype=host.bin_data.dtype)
        counts = np.diff(host.indptr.numpy())
        row_of = torch.from_numpy(np.repeat(np.arange(n), counts))
        bins[row_of, host.indices.long()] = host.bin_data
        self.twin = QuantizedMatrix(
            bins.cuda(), host.cuts.cuda(), host.cut_ptr.cuda(), host.nbins.cuda(),
            host.stride, True, n, f,
        )
        rng = np.random.default_rng(seed + 1)
        self.gh = torch.stack(
            [
                torch.tensor(rng.normal(size=n).astype(np.float32)),
                torch.tensor(rng.random(size=n).astype(np.float32) + 0.01),
            ],
            dim=1,
        ).cuda()
        self.scale = hip.compute_scale(self.gh)
        self.identity = torch.arange(n, dtype=torch.int32, device="cuda")
        self.permuted = torch.from_numpy(rng.permutation(n).astype(np.int32)).cuda()


_SHAPES = [(1, 3), (257, 70), (5000, 300)]
_CASES = [(n, f, d, 256) for (n, f) in _SHAPES for d in (0.05, 0.5)] + [(5000, 300, 0.5, 512)]
_problems = {}


@pytest.fixture(params=_CASES, ids=lambda c: "n%d-f%d-d%s-mb%d" % c)
def problem(request):
    key = request.param
    if key not in _problems:  # built once, shared, never modified
        _problems[key] = _Problem(*key)
    return _problems[key]


def _both(p, rowbuf, jobs):
    got = hip_sparse.build_histograms(p.sqm, p.gh, rowbuf, jobs, p.scale)
    want = hip.build_histograms(p.twin, p.gh, rowbuf, jobs, p.scale)
    torch.cuda.synchronize()
    return got, want


class TestHistSparse:
    def test_backend_and_bin_type(self, problem):
        assert backend_for_qm(problem.sqm) is hip_sparse
        assert problem.sqm.indices.dtype == torch.int32 and problem.sqm.indptr.dtype == torch.int64
        assert problem.sqm.csc_ptr is None  # no CSC mirror on the device
        if problem.sqm.stride > 256:
            # a feature with more than 256 distinct values at max_bin=512
            assert problem.sqm.bin_data.dtype == torch.int16
            assert int(problem.sqm.nbins.max()) > 256
        else:
            assert problem.sqm.bin_data.dtype == torch.uint8
        assert problem.sqm.bin_data.dtype == problem.twin.bins.dtype

    def test_full_range(self, problem):
        got, want = _both(problem, problem.identity, [(0, problem.n)])
        assert got.dtype == torch.int64 and got.shape == want.shape
        assert torch.equal(got, want)

    def test_one_row_segment(self, problem):
        k = problem.n // 2
        got, want = _both(problem, problem.identity, [(k, k + 1)])
        assert torch.equal(got, want)

    def test_segment_of_empty_rows(self, problem):
        b0, b1 = _blank_rows(problem.n)
        if b1 == b0:  # n == 1: no run of blank rows, the row itself
            b0, b1 = 0, problem.n
        got, want = _both(problem, problem.identity, [(b0, b1)])
        assert torch.equal(got, want)
        indptr = problem.sqm.indptr.cpu()
        if int(indptr[b1] - indptr[b0]) == 0:
            # only missing slots hold anything
            view = got.reshape(1, problem.f, problem.sqm.stride, 2)
            assert not view[:, :, :-1, :].any()
        else:
            assert problem.n == 1

    def test_several_jobs_one_launch(self, problem):
        n = problem.n
        # includes an empty segment and the segment with the empty rows
        jobs = [(0, n // 4), (n // 4, n // 2), (n // 2, n // 2), (n // 2, n)]
        got, want = _both(problem, problem.identity, jobs)
        assert torch.equal(got, want)

    def test_permuted_row_buffer(self, problem):
        n = problem.n
        jobs = [(0, n)] if n < 4 else [(0, n // 3), (n // 3, n)]
        got, want = _both(problem, problem.permuted, jobs)
        assert torch.equal(got, want)


def _split_choices(p):
    """(feature, bin, default_left) per segment pair: both default
    directions, and the empty last column (no row stores it)."""
    f = p.f
    mid_bin = max(0, int(p.sqm.nbins[0]) // 2 - 1)
    choices = [((0, mid_bin, True), (min(1, f - 1), 0, False))]
    choices.append(((0, mid_bin, False), (min(1, f - 1), 0, True)))
    if f >= 2:
        choices.append(((f - 1, 0, True), (f - 1, 0, False)))
    return choices


class TestPartitionSparse:
    def test_counts_and_row_sets(self, problem):
        p = problem
        n = p.n
        segs = [(0, n // 2), (n // 2, n)]
        src = p.permuted
        for pair in _split_choices(p):
            feats = [c[0] for c in pair]
            sbins = [c[1] for c in pair]
            dls = [c[2] for c in pair]
            dst_dense = torch.full_like(src, -1)
            want_left = hip.partition_level(p.twin, src, dst_dense, segs, feats, sbins, dls)
            packed = torch.tensor(
                [[1.0, ft, sb, float(dl), 0.0, 0.0] for ft, sb, dl in pair],
                dtype=torch.float32, device="cuda",
            )
            dst_sparse = torch.full_like(src, -1)
            counters = hip_sparse.partition_level(p.sqm, src, dst_sparse, segs, [0, 1], packed)
            torch.cuda.synchronize()
            counters = counters.cpu().numpy()
            want = np.asarray(
                [[lc, (e - s) - lc] for lc, (s, e) in zip(want_left, segs)], dtype=np.int32
            )
            assert np.array_equal(counters, want)
            for (s, e), lc in zip(segs, want_left):
                # the order within a side is free
                assert torch.equal(
                    torch.sort(dst_sparse[s : s + lc]).values, torch.sort(dst_dense[s : s + lc]).values
                )
                assert torch.equal(
                    torch.sort(dst_sparse[s + lc : e]).values, torch.sort(dst_dense[s + lc : e]).values
                )

    def test_absent_feature_follows_default(self, problem):
        p = problem
        n = p.n
        assert int(p.sqm.nbins[p.f - 1]) == 1  # the empty last column
        for dl in (True, False):
            packed = torch.tensor([[1.0, p.f - 1, 0, float(dl), 0, 0]], dtype=torch.float32, device="cuda")
            dst = torch.full_like(p.identity, -1)
            counters = hip_sparse.partition_level(p.sqm, p.identity, dst, [(0, n)], [0], packed)
            assert counters.cpu().tolist() == ([[n, 0]] if dl else [[0, n]])
            assert torch.equal(torch.sort(dst).values, p.identity)

    def test_non_positive_gain_is_skipped(self, problem):
        p = problem
        packed = torch.tensor([[0.0, 0, 0, 1, 0, 0]], dtype=torch.float32, device="cuda")
        dst = torch.full_like(p.identity, -1)
        counters = hip_sparse.partition_level(p.sqm, p.identity, dst, [(0, p.n)], [0], packed)
        assert counters.cpu().tolist() == [[0, 0]]
        assert bool((dst == -1).all())


def _full_tree(depth, f, seed):
    rng = np.random.default_rng(seed)
    tree = Tree()
    frontier = [tree.add_node(value=0.0)]
    for _ in range(depth):
        nxt = []
        for nid in frontier:
            lid, rid = tree.apply_split(
                nid, int(rng.integers(0, f)), float(np.round(rng.normal() * 8) / 8), 0,
                bool(rng.integers(0, 2)), 1.0,
                left_value=float(rng.normal()), right_value=float(rng.normal()),
                left_hess=1.0, right_hess=1.0,
            )
            nxt += [lid, rid]
        frontier = nxt
    return tree.finalize()


class TestPredictTreeCsr:
    @pytest.mark.parametrize("n,f,density", [(1, 3, 0.5), (257, 70, 0.5), (5000, 300, 0.05)])
    def test_equals_dense_traversal(self, n, f, density):
        # values in eighths hit the thresholds (also eighths) exactly at times;
        # the blank rows store nothing at all
        csr = _rand_csr(n, f, density, seed=7, eighths=True)
        if csr.nnz:
            csr.data[0] = 0.0  # an explicit stored zero is a value, not missing
        dense = np.full((n, f), np.nan, dtype=np.float32)
        rr = np.repeat(np.arange(n), np.diff(csr.indptr))
        dense[rr, csr.indices] = csr.data
        tree = _full_tree(6, f, seed=3)
        got = hip_sparse.predict_tree_csr(tree, csr, torch.device("cuda"))
        want = hip.predict_tree(tree, torch.from_numpy(dense).cuda())
        torch.cuda.synchronize()
        assert got.shape == want.shape and torch.equal(got, want)
        # uploaded once, reused
        dev = hip_sparse.DeviceCSR(csr, torch.device("cuda"))
        assert torch.equal(hip_sparse.predict_tree_csr(tree, dev), want)

    def test_unsorted_rows_are_sorted_on_upload(self):
        csr = _rand_csr(257, 70, 0.5, seed=9, eighths=True)
        shuffled = csr.copy()
        rng = np.random.default_rng(0)
        for r in range(csr.shape[0]):
            s, e = shuffled.indptr[r], shuffled.indptr[r + 1]
            perm = rng.permutation(e - s)
            shuffled.indices[s:e] = shuffled.indices[s:e][perm]
            shuffled.data[s:e] = shuffled.data[s:e][perm]
        shuffled.has_sorted_indices = False
        tree = _full_tree(6, 70, seed=4)
        a = hip_sparse.predict_tree_csr(tree, csr, torch.device("cuda"))
        b = hip_sparse.predict_tree_csr(tree, shuffled, torch.device("cuda"))
        assert torch.equal(a, b)
