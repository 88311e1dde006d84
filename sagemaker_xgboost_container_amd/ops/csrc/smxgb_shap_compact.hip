// MI355X (gfx950 / CDNA4) path-form TreeSHAP with chunk-local phi slots.
//
// shap_paths_kernel (smxgb_kernels.hip) keeps a dense k * (f + 1) phi slab
// per lane group in LDS, which bounds k * (f + 1). A chunk of a few trees
// touches at most as many distinct (class, feature) cells as it has split
// nodes, so the host (ops/shap_paths.py make_shap_slots) numbers those cells
// 0 .. S_c-1 per chunk and gives every path element its slot. The slab of a
// group is then max_c S_c doubles, whatever f and k are, and the row
// accessor is the only difference between dense and CSR input.
//
// Work decomposition, lane mapping, fp64 arithmetic and the no-atomics rule
// are shap_paths_kernel's: a W-wide lane group owns one (row, chunk) item,
// one lane per path element, items chunk-major. A group flushes its slab to
// part[row, chunk_slot_ptr[c] ..) of the ragged slot axis (length S, the sum
// of the S_c); shap_slot_reduce_kernel then sums, per output column, that
// column's slots in ascending chunk order. Both steps have a fixed order, so
// results are bit-identical from call to call.

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <algorithm>
#include <cmath>

#include "smxgb_jobs.h"
#include "smxgb_shap.h"

#define CHECK_DEV(x, dt)                                                       \
  TORCH_CHECK_VALUE(x.is_cuda() && x.is_contiguous() && x.scalar_type() == dt, \
                    #x " must be a contiguous ROCm device tensor of the expected dtype")

static hipStream_t compact_stream() { return at::hip::getCurrentHIPStream().stream(); }

// values: X (n, nfeat) row-major when !CSR, else the CSR data array with
// int64 row offsets `indptr` and sorted int32 column ids `indices`; an
// absent entry is NaN, a stored value (NaN, zero, +-inf included) is itself.
// elem_slot is indexed by (element id - elem_base): the tables cover the
// tree range only. blockDim.x is SHAP_BLOCK or one wave.
template <bool CSR>
__global__ __launch_bounds__(SHAP_BLOCK) void shap_paths_compact_kernel(
    const float* __restrict__ values, const long long* __restrict__ indptr,
    const int* __restrict__ indices, long long n, int nfeat,
    const int* __restrict__ elem_feat, const float* __restrict__ elem_lo,
    const float* __restrict__ elem_hi, const unsigned char* __restrict__ elem_flags,
    const double* __restrict__ elem_z, const int* __restrict__ path_off,
    const float* __restrict__ path_value, const int* __restrict__ tree_path_ptr,
    int t_begin, int t_end, const int* __restrict__ elem_slot, int elem_base,
    const int* __restrict__ chunk_slot_ptr, double* __restrict__ part, long long S,
    int n_chunks, int trees_per_chunk, int W, int lmax, int max_slots) {
  extern __shared__ double shap_compact_slab[];
  const int gpb = blockDim.x / W;
  const int g = threadIdx.x / W;
  const int gl = threadIdx.x - g * W;
  double* slab = shap_compact_slab + (long long)g * max_slots;
  for (int i = gl; i < max_slots; i += W) slab[i] = 0.0;

  const long long total = n * (long long)n_chunks;
  const long long ngroups = (long long)gridDim.x * gpb;
  for (long long item = (long long)blockIdx.x * gpb + g; item < total; item += ngroups) {
    // chunk-major items: neighbouring groups share a chunk, so a wave walks
    // one path list in lock-step and the table loads broadcast
    const long long c = item / n;
    const long long row = item - c * n;
    const int ts = t_begin + (int)c * trees_per_chunk;
    const int te = min(t_end, ts + trees_per_chunk);
    const int p0 = tree_path_ptr[ts];
    const int p1 = tree_path_ptr[te];
    const int s0 = chunk_slot_ptr[c];
    const int sc = chunk_slot_ptr[c + 1] - s0;
    long long rlo = 0, rhi = 0;
    if (CSR) {
      rlo = indptr[row];
      rhi = indptr[row + 1];
    }
    for (int p = p0; p < p1; ++p) {
      const int off = path_off[p];
      const int len = path_off[p + 1] - off + 1;  // + dummy root element
      const bool mine = gl > 0 && gl < len;
      double z = 1.0, o = 1.0;
      int slot = 0;
      if (mine) {
        const int e = off + gl - 1;
        const int fidx = elem_feat[e];
        slot = elem_slot[e - elem_base];
        z = elem_z[e];
        float x;
        if (CSR) {
          // global-memory search; lanes of a wave may take different trip
          // counts, no cross-lane op is inside this branch
          const long long pos = csr_find(indices, rlo, rhi, fidx);
          x = pos >= 0 ? values[pos] : __builtin_nanf("");
        } else {
          x = values[row * nfeat + fidx];
        }
        o = shap_one_fraction(x, elem_lo[e], elem_hi[e], elem_flags[e]);
      }
      const double s = shap_unwound_sum(z, o, gl, len, lmax, W);
      // Plain LDS read-modify-write, as in shap_paths_kernel: merged paths
      // hold a feature once and a tree has one class, so no two lanes of a
      // path share a slot; groups own disjoint slabs. Across paths a slot
      // may be written by one lane and read by another lane of the SAME
      // wave: a wave's DS instructions execute in issue order, and the
      // wavefront fence + wave barrier keep the compiler from moving them.
      if (mine) slab[slot] += s * (o - z) * (double)path_value[p];
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
    double* prow = part + row * S + s0;
    for (int i = gl; i < sc; i += W) {
      prow[i] = slab[i];
      slab[i] = 0.0;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

// compact[row, j] = sum of part[row, col_slots[col_ptr[j] .. col_ptr[j+1])]
// in that stored order (ascending chunk). One thread per (row, j).
__global__ __launch_bounds__(HIST_BLOCK) void shap_slot_reduce_kernel(
    const double* __restrict__ part, long long n, long long S,
    const int* __restrict__ col_ptr, const int* __restrict__ col_slots, int U,
    double* __restrict__ compact) {
  const long long total = n * (long long)U;
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += step) {
    const long long row = idx / U;
    const int j = (int)(idx - row * U);
    const double* prow = part + row * S;
    double acc = 0.0;
    const int q1 = col_ptr[j + 1];
    for (int q = col_ptr[j]; q < q1; ++q) acc += prow[col_slots[q]];
    compact[idx] = acc;
  }
}

// values/indptr/indices: a dense (n, f) float32 matrix with two empty index
// tensors, or the three CSR arrays with `n` and `nfeat` given explicitly.
// The slot tables' CONTENT (slot ids below max_slots, offsets inside S) is
// validated on the host by ops/hip.py from the numpy arrays they were
// uploaded from; here every size and scalar is checked against the buffers.
void tree_shap_compact(torch::Tensor values, torch::Tensor indptr, torch::Tensor indices,
                       int64_t n, int64_t nfeat, bool csr, torch::Tensor elem_feat,
                       torch::Tensor elem_lo, torch::Tensor elem_hi, torch::Tensor elem_flags,
                       torch::Tensor elem_z, torch::Tensor path_off, torch::Tensor path_value,
                       torch::Tensor tree_path_ptr, int64_t t_begin, int64_t t_end,
                       torch::Tensor elem_slot, int64_t elem_base, torch::Tensor chunk_slot_ptr,
                       torch::Tensor part, int64_t S, int64_t n_chunks,
                       int64_t trees_per_chunk, int64_t W, int64_t lmax, int64_t max_feature,
                       int64_t max_slots, int64_t block) {
  CHECK_DEV(values, torch::kFloat32);
  CHECK_DEV(elem_feat, torch::kInt32);
  CHECK_DEV(elem_lo, torch::kFloat32);
  CHECK_DEV(elem_hi, torch::kFloat32);
  CHECK_DEV(elem_flags, torch::kUInt8);
  CHECK_DEV(elem_z, torch::kFloat64);
  CHECK_DEV(path_off, torch::kInt32);
  CHECK_DEV(path_value, torch::kFloat32);
  CHECK_DEV(tree_path_ptr, torch::kInt32);
  CHECK_DEV(elem_slot, torch::kInt32);
  CHECK_DEV(chunk_slot_ptr, torch::kInt32);
  CHECK_DEV(part, torch::kFloat64);
  TORCH_CHECK_VALUE(n >= 0 && nfeat >= 0, "negative matrix shape");
  if (csr) {
    CHECK_DEV(indptr, torch::kInt64);
    CHECK_DEV(indices, torch::kInt32);
    TORCH_CHECK_VALUE(values.dim() == 1 && indptr.dim() == 1 && indices.dim() == 1 &&
                          indptr.numel() == n + 1 && indices.numel() == values.numel(),
                      "CSR arrays do not match the matrix shape");
  } else {
    TORCH_CHECK_VALUE(values.dim() == 2 && values.size(0) == n && values.size(1) == nfeat,
                      "X must be (n, f)");
  }
  TORCH_CHECK_VALUE(max_feature < nfeat, "the matrix has ", nfeat,
                    " columns but the forest splits on feature ", max_feature);
  TORCH_CHECK_VALUE(lmax >= 1 && lmax <= WAVE, "path length ", lmax, " exceeds the wave width");
  TORCH_CHECK_VALUE(W >= lmax && W <= WAVE && (W & (W - 1)) == 0,
                    "lane-group width must be a power of two in [lmax, 64]");
  TORCH_CHECK_VALUE(block == SHAP_BLOCK || block == WAVE, "block must be 256 or one wave");
  TORCH_CHECK_VALUE(0 <= t_begin && t_begin <= t_end && t_end < tree_path_ptr.numel(),
                    "tree range out of bounds");
  TORCH_CHECK_VALUE(n_chunks >= 1 && trees_per_chunk >= 1 &&
                        n_chunks * trees_per_chunk >= t_end - t_begin &&
                        (n_chunks - 1) * trees_per_chunk <= t_end - t_begin,
                    "bad tree chunking");
  const int64_t n_paths = path_off.numel() - 1;
  TORCH_CHECK_VALUE(n_paths >= 0 && path_value.numel() == n_paths, "path tables disagree");
  const int64_t n_elem = elem_feat.numel();
  TORCH_CHECK_VALUE(elem_lo.numel() == n_elem && elem_hi.numel() == n_elem &&
                        elem_flags.numel() == n_elem && elem_z.numel() == n_elem,
                    "element tables disagree");
  TORCH_CHECK_VALUE(elem_base >= 0 && elem_base + elem_slot.numel() <= n_elem,
                    "slot table does not lie inside the element tables");
  TORCH_CHECK_VALUE(chunk_slot_ptr.numel() == n_chunks + 1, "chunk_slot_ptr must be (C+1,)");
  TORCH_CHECK_VALUE(S >= 0 && S < (1ll << 31) && part.numel() == n * S,
                    "partial buffer has the wrong size");
  TORCH_CHECK_VALUE(max_slots >= 0 && max_slots <= S, "max_slots outside the slot axis");
  const long long gpb = block / W;
  const size_t lds_bytes = (size_t)gpb * max_slots * sizeof(double);
  TORCH_CHECK_VALUE(lds_bytes <= 64 * 1024, "slot slabs do not fit the LDS budget");
  if (n == 0 || t_end == t_begin || S == 0) return;
  const long long total = (long long)n * n_chunks;
  const long long grid_cap = 8192ll * (SHAP_BLOCK / block);
  const int grid =
      (int)std::max<long long>(1, std::min<long long>((total + gpb - 1) / gpb, grid_cap));
  auto kernel = csr ? shap_paths_compact_kernel<true> : shap_paths_compact_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3((int)block), lds_bytes, compact_stream(),
                     values.data_ptr<float>(),
                     csr ? (const long long*)indptr.data_ptr<int64_t>() : nullptr,
                     csr ? indices.data_ptr<int>() : nullptr, (long long)n, (int)nfeat,
                     elem_feat.data_ptr<int>(), elem_lo.data_ptr<float>(),
                     elem_hi.data_ptr<float>(), elem_flags.data_ptr<unsigned char>(),
                     elem_z.data_ptr<double>(), path_off.data_ptr<int>(),
                     path_value.data_ptr<float>(), tree_path_ptr.data_ptr<int>(), (int)t_begin,
                     (int)t_end, elem_slot.data_ptr<int>(), (int)elem_base,
                     chunk_slot_ptr.data_ptr<int>(), part.data_ptr<double>(), (long long)S,
                     (int)n_chunks, (int)trees_per_chunk, (int)W, (int)lmax, (int)max_slots);
}

void shap_slot_reduce(torch::Tensor part, torch::Tensor col_ptr, torch::Tensor col_slots,
                      torch::Tensor compact) {
  CHECK_DEV(part, torch::kFloat64);
  CHECK_DEV(col_ptr, torch::kInt32);
  CHECK_DEV(col_slots, torch::kInt32);
  CHECK_DEV(compact, torch::kFloat64);
  TORCH_CHECK_VALUE(part.dim() == 2 && compact.dim() == 2 && part.size(0) == compact.size(0),
                    "part must be (n, S) and compact (n, U)");
  const int64_t n = part.size(0), S = part.size(1), U = compact.size(1);
  TORCH_CHECK_VALUE(col_ptr.numel() == U + 1 && col_slots.numel() == S && U < (1ll << 31),
                    "column tables do not match the buffers");
  if (n == 0 || U == 0) return;
  const long long total = (long long)n * U;
  const int grid = (int)std::min<long long>((total + HIST_BLOCK - 1) / HIST_BLOCK, 16384);
  hipLaunchKernelGGL(shap_slot_reduce_kernel, dim3(grid), dim3(HIST_BLOCK), 0, compact_stream(),
                     part.data_ptr<double>(), (long long)n, (long long)S, col_ptr.data_ptr<int>(),
                     col_slots.data_ptr<int>(), (int)U, compact.data_ptr<double>());
}

void init_shap_compact_kernels(pybind11::module_& m) {
  m.def("tree_shap_compact", &tree_shap_compact,
        "path-form exact TreeSHAP into chunk-local slots, dense or CSR rows");
  m.def("shap_slot_reduce", &shap_slot_reduce, "fixed-order sum of a column's slots");
}
