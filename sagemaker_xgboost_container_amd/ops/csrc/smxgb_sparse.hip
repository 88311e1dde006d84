// MI355X (gfx950 / CDNA4) kernels for training on quantized CSR data.
//
// The dense kernels index an n x f bin matrix; these walk a quantized CSR
// matrix (int64 row offsets, int32 sorted column ids, one local bin id per
// stored entry) so wide sparse data never densifies. They keep the dense
// path's contracts: int64 fixed-point histograms (value * 2^33 / max_abs,
// scale derived on device), host-packed job tables with a block -> job map,
// row ids in ping-pong int32 buffers, splits read from the on-device packed
// split tensor.
//
// An absent entry is a missing value. Histograms accumulate stored entries
// only; hist_sparse_close_kernel then writes every feature's missing slot
// as (segment total - sum of present bins) in integers, which makes the
// accumulator equal, bit for bit, to the dense build over the same bins.

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <algorithm>

#include "smxgb_jobs.h"
#include "smxgb_shap.h"

typedef unsigned long long u64;

#define CHECK_DEV(x, dt)                                                       \
  TORCH_CHECK_VALUE(x.is_cuda() && x.is_contiguous() && x.scalar_type() == dt, \
                    #x " must be a contiguous ROCm device tensor of the expected dtype")

static hipStream_t sparse_stream() { return at::hip::getCurrentHIPStream().stream(); }

// ---------------------------------------------------------------------------
// histogram build over CSR entries
// ---------------------------------------------------------------------------

// Lane mapping: a wave takes 64 consecutive rows of the segment (one row
// per lane for the row id, offsets and gradient pair), then walks the
// FLATTENED entry range of those 64 rows, 64 entries per step. The owner
// of entry e is found by a 6-step binary search over the wave's exclusive
// prefix of row lengths (LDS). A row of any length is thereby spread over
// all lanes, and where the rows are consecutive in the matrix (the root
// level) the column / bin loads of a step are contiguous.
//
// f * stride slots do not fit LDS for wide data, so entries go straight to
// the global accumulator with u64 atomics: scattered and low-contention
// for sparse data. Each row's pair is also summed once into the job total
// (registers -> block reduction -> one atomic pair per block).
template <typename BinT>
__global__ __launch_bounds__(HIST_BLOCK) void hist_sparse_kernel(
    const long long* __restrict__ indptr, const int* __restrict__ indices,
    const BinT* __restrict__ bin_data, const float2* __restrict__ gh,
    const int* __restrict__ rowbuf, const HistJob* __restrict__ jobs,
    const int* __restrict__ block_job, u64* __restrict__ out, u64* __restrict__ totals,
    int nfeat, int stride, const float* __restrict__ gh_max) {
  __shared__ int s_pre[HIST_BLOCK];          // exclusive prefix of row lengths, per wave
  __shared__ long long s_start[HIST_BLOCK];  // first entry of the lane's row
  __shared__ u64 s_g[HIST_BLOCK];
  __shared__ u64 s_h[HIST_BLOCK];

  const float scale_g = 8589934592.0f / fmaxf(gh_max[0], 1e-30f);
  const float scale_h = 8589934592.0f / fmaxf(gh_max[1], 1e-30f);
  const HistJob job = jobs[block_job[blockIdx.x]];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wbase = threadIdx.x - lane;  // first LDS slot of this wave
  u64* gout = out + (long long)job.hist_idx * nfeat * (long long)stride * 2;

  u64 tot_g = 0ull, tot_h = 0ull;
  const int chunk = blockIdx.x - job.first_block;
  const long long tile_step = (long long)job.num_blocks * HIST_BLOCK;
  // the tile loop is uniform over the block: every thread reaches the
  // barriers and the wave scan with all lanes active
  for (long long tile = job.start + (long long)chunk * HIST_BLOCK; tile < job.end;
       tile += tile_step) {
    const long long r = tile + threadIdx.x;
    int cnt = 0;
    long long first = 0;
    u64 gfix = 0ull, hfix = 0ull;
    if (r < job.end) {
      const int row = rowbuf[r];
      first = indptr[row];
      cnt = (int)(indptr[row + 1] - first);
      const float2 gp = gh[row];
      gfix = (u64)(long long)llrintf(gp.x * scale_g);
      hfix = (u64)(long long)llrintf(gp.y * scale_h);
      tot_g += gfix;
      tot_h += hfix;
    }
    int incl = cnt;
    #pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
      const int up = __shfl_up(incl, d, WAVE);
      if (lane >= d) incl += up;
    }
    const int wave_entries = __shfl(incl, WAVE - 1, WAVE);
    s_pre[threadIdx.x] = incl - cnt;
    s_start[threadIdx.x] = first;
    s_g[threadIdx.x] = gfix;
    s_h[threadIdx.x] = hfix;
    __syncthreads();
    for (int e = lane; e < wave_entries; e += WAVE) {
      // last row of the wave whose prefix is <= e: it is non-empty and owns e
      int lo = 0;
      #pragma unroll
      for (int step = WAVE >> 1; step > 0; step >>= 1) {
        if (s_pre[wbase + lo + step] <= e) lo += step;
      }
      const long long pos = s_start[wbase + lo] + (e - s_pre[wbase + lo]);
      const int col = indices[pos];
      const int b = (int)bin_data[pos];
      u64* dst = gout + ((long long)col * stride + b) * 2;
      atomicAdd(dst, s_g[wbase + lo]);
      atomicAdd(dst + 1, s_h[wbase + lo]);
    }
    __syncthreads();
  }

  // job total: block reduction (the LDS arrays are free again), one atomic
  // pair per block
  s_g[threadIdx.x] = tot_g;
  s_h[threadIdx.x] = tot_h;
  __syncthreads();
  for (int w = HIST_BLOCK >> 1; w > 0; w >>= 1) {
    if (threadIdx.x < w) {
      s_g[threadIdx.x] += s_g[threadIdx.x + w];
      s_h[threadIdx.x] += s_h[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (s_g[0]) atomicAdd(&totals[job.hist_idx * 2], s_g[0]);
    if (s_h[0]) atomicAdd(&totals[job.hist_idx * 2 + 1], s_h[0]);
  }
}

// missing slot of every (histogram, feature): total - sum of present bins.
// One wave per (histogram, feature); lanes stride over the feature's bins so
// the reads coalesce. Integer arithmetic mod 2^64, as the accumulator's.
__global__ __launch_bounds__(HIST_BLOCK) void hist_sparse_close_kernel(
    u64* __restrict__ out, const u64* __restrict__ totals, long long n_pairs /* J * nfeat */,
    int nfeat, int stride) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long long wave0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  const long long wave_step = (long long)gridDim.x * blockDim.x / WAVE;
  for (long long p = wave0; p < n_pairs; p += wave_step) {
    u64* slots = out + p * stride * 2;
    u64 sg = 0ull, sh = 0ull;
    for (int b = lane; b < stride - 1; b += WAVE) {
      sg += slots[b * 2];
      sh += slots[b * 2 + 1];
    }
    #pragma unroll
    for (int d = WAVE >> 1; d > 0; d >>= 1) {
      sg += __shfl_down(sg, d, WAVE);
      sh += __shfl_down(sh, d, WAVE);
    }
    if (lane == 0) {
      const long long j = p / nfeat;
      slots[(stride - 1) * 2] = totals[j * 2] - sg;
      slots[(stride - 1) * 2 + 1] = totals[j * 2 + 1] - sh;
    }
  }
}

// ---------------------------------------------------------------------------
// row partition
// ---------------------------------------------------------------------------

// csr_find (binary search of a row's sorted column ids): smxgb_shap.h

#define SPART_TILE 4096

// Two-ended LDS tile compaction (one global atomic per side per tile), all
// split nodes of a level in one launch. job.feature is the node's row in
// the on-device packed split tensor; gain <= 0 jobs are skipped. A row that
// does not store the split feature goes to the default direction.
template <typename BinT>
__global__ __launch_bounds__(HIST_BLOCK) void partition_sparse_kernel(
    const long long* __restrict__ indptr, const int* __restrict__ indices,
    const BinT* __restrict__ bin_data, const int* __restrict__ src, int* __restrict__ dst,
    const PartJob* __restrict__ jobs, const int* __restrict__ block_job,
    const float* __restrict__ split_packed, int* __restrict__ counters) {
  __shared__ int lbuf[SPART_TILE];
  __shared__ int rbuf[SPART_TILE];
  __shared__ int lcnt, rcnt, lbase, rbase;

  const int j = block_job[blockIdx.x];
  const PartJob job = jobs[j];
  const float* sp6 = split_packed + (long long)job.feature * 6;
  if (sp6[0] <= 0.0f) return;  // no split for this node (uniform over the block)
  const int feature = (int)sp6[1];
  const int split_bin = (int)sp6[2];
  const bool default_left = sp6[3] > 0.5f;

  const int chunk = blockIdx.x - job.first_block;
  const long long tile_step = (long long)job.num_blocks * SPART_TILE;
  for (long long tile = job.start + (long long)chunk * SPART_TILE; tile < job.end;
       tile += tile_step) {
    if (threadIdx.x == 0) {
      lcnt = 0;
      rcnt = 0;
    }
    __syncthreads();
    const int tile_n = (int)min((long long)SPART_TILE, job.end - tile);
    for (int i = threadIdx.x; i < tile_n; i += blockDim.x) {
      const int row = src[tile + i];
      const long long pos = csr_find(indices, indptr[row], indptr[row + 1], feature);
      const bool left = pos < 0 ? default_left : ((int)bin_data[pos] <= split_bin);
      if (left) {
        lbuf[atomicAdd(&lcnt, 1)] = row;
      } else {
        rbuf[atomicAdd(&rcnt, 1)] = row;
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      lbase = atomicAdd(&counters[j * 2], lcnt);
      rbase = atomicAdd(&counters[j * 2 + 1], rcnt);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < lcnt; i += blockDim.x) dst[job.start + lbase + i] = lbuf[i];
    for (int i = threadIdx.x; i < rcnt; i += blockDim.x) dst[job.end - 1 - rbase - i] = rbuf[i];
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// one tree over raw CSR rows (eval-set margins, warm-start replay)
// ---------------------------------------------------------------------------

// One thread per row. The dense kernel's rule on the NaN-densified row: an
// absent entry (or a stored NaN) takes the default direction.
__global__ __launch_bounds__(HIST_BLOCK) void predict_tree_csr_kernel(
    const long long* __restrict__ indptr, const int* __restrict__ indices,
    const float* __restrict__ data, long long n, const int* __restrict__ left,
    const int* __restrict__ right, const int* __restrict__ feat,
    const float* __restrict__ thresh, const unsigned char* __restrict__ defl,
    const float* __restrict__ value, float* __restrict__ out) {
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x; row < n; row += step) {
    const long long lo = indptr[row];
    const long long hi = indptr[row + 1];
    int nid = 0;
    int l;
    while ((l = left[nid]) >= 0) {
      const long long pos = csr_find(indices, lo, hi, feat[nid]);
      bool goleft = defl[nid] != 0;
      if (pos >= 0) {
        const float fv = data[pos];
        if (!isnan(fv)) goleft = fv < thresh[nid];
      }
      nid = goleft ? l : right[nid];
    }
    out[row] = value[nid];
  }
}

// ---------------------------------------------------------------------------
// whole forest over raw CSR rows (Booster.predict on sparse data)
// ---------------------------------------------------------------------------

// most entries of one row group the launcher lets a block stage in LDS:
// 8192 x (int, float) = 64 KiB of dynamic LDS
#define PCSR_MAX_TILE 8192

// csr_find over an LDS slice (int offsets into the tile)
__device__ inline int tile_find(const int* cols, int lo, int hi, int feature) {
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    const int c = cols[mid];
    if (c < feature) {
      lo = mid + 1;
    } else if (c > feature) {
      hi = mid;
    } else {
      return mid;
    }
  }
  return -1;
}

// The CSR twin of predict_kernel (LEAF = false) and pred_leaf_kernel
// (LEAF = true), same work decomposition so the results are equal bit for
// bit on the NaN-densified rows: an item is (row, c) with c < n_inner, where
// c is a tree chunk (trees [t_begin + c * trees_per_chunk, ...) visited in
// ascending order, each adding into out[c, row, tree_cls[t]]) or, for LEAF,
// one tree (trees_per_chunk == 1, out[row, c] = tree-local leaf id).
//
// A block owns R consecutive rows and all n_inner items of each; blocks
// grid-stride over such groups. The group's entries are contiguous in the
// matrix: when they fit the tile (`tile` entries of dynamic LDS, column ids
// then values) they are copied to LDS once (coalesced) and
// every split node's binary search runs there; a longer group (one very
// long row, say) searches global memory as predict_tree_csr_kernel does.
// The choice is uniform over the block. The split rule is
// predict_tree_csr_kernel's.
template <bool LEAF>
__device__ __forceinline__ void forest_csr_body(
    const long long* __restrict__ indptr, const int* __restrict__ indices,
    const float* __restrict__ data, long long n, int rows_per_group,
    const int* __restrict__ left, const int* __restrict__ right,
    const int* __restrict__ feat, const float* __restrict__ thresh,
    const unsigned char* __restrict__ defl, const float* __restrict__ value,
    const int* __restrict__ tree_root, const int* __restrict__ tree_cls, int t_begin,
    int t_end, void* __restrict__ out_raw, int k, int n_inner, int trees_per_chunk,
    int tile) {
  extern __shared__ int s_tile[];
  int* s_col = s_tile;
  float* s_val = (float*)(s_tile + tile);

  const long long n_groups = (n + rows_per_group - 1) / rows_per_group;
  for (long long g = blockIdx.x; g < n_groups; g += gridDim.x) {
    const long long r0 = g * rows_per_group;
    const int rows = (int)min((long long)rows_per_group, n - r0);
    const long long e0 = indptr[r0];
    const long long e1 = indptr[r0 + rows];
    const bool staged = e1 - e0 <= tile;
    __syncthreads();  // the previous group's searches are done with the tile
    if (staged) {
      const int cnt = (int)(e1 - e0);
      for (int i = threadIdx.x; i < cnt; i += blockDim.x) {
        s_col[i] = indices[e0 + i];
        s_val[i] = data[e0 + i];
      }
    }
    __syncthreads();

    const long long items = (long long)rows * n_inner;
    for (long long it = threadIdx.x; it < items; it += blockDim.x) {
      const int lr = (int)(it / n_inner);
      const int c = (int)(it - (long long)lr * n_inner);
      const long long row = r0 + lr;
      const long long lo = indptr[row];
      const long long hi = indptr[row + 1];
      const int tlo = (int)(lo - e0);  // used when staged only
      const int thi = (int)(hi - e0);
      const int ts = t_begin + c * trees_per_chunk;
      const int te = min(t_end, ts + trees_per_chunk);
      for (int t = ts; t < te; ++t) {
        const int root = tree_root[t];
        int nid = root;
        int l;
        while ((l = left[nid]) >= 0) {
          const int f = feat[nid];
          bool goleft = defl[nid] != 0;
          if (staged) {
            const int pos = tile_find(s_col, tlo, thi, f);
            if (pos >= 0) {
              const float fv = s_val[pos];
              if (!isnan(fv)) goleft = fv < thresh[nid];
            }
          } else {
            const long long pos = csr_find(indices, lo, hi, f);
            if (pos >= 0) {
              const float fv = data[pos];
              if (!isnan(fv)) goleft = fv < thresh[nid];
            }
          }
          nid = goleft ? l : right[nid];
        }
        if (LEAF) {
          ((int*)out_raw)[row * n_inner + c] = nid - root;
        } else {
          ((float*)out_raw)[((long long)c * n + row) * k + tree_cls[t]] += value[nid];
        }
      }
    }
  }
}

#define FOREST_CSR_PARAMS                                                                 \
  const long long *__restrict__ indptr, const int *__restrict__ indices,                  \
      const float *__restrict__ data, long long n, int rows_per_group,                    \
      const int *__restrict__ left, const int *__restrict__ right,                        \
      const int *__restrict__ feat, const float *__restrict__ thresh,                     \
      const unsigned char *__restrict__ defl, const float *__restrict__ value,            \
      const int *__restrict__ tree_root, const int *__restrict__ tree_cls, int t_begin,   \
      int t_end, void *__restrict__ out, int k, int n_inner, int trees_per_chunk, int tile
#define FOREST_CSR_ARGS                                                                    \
  indptr, indices, data, n, rows_per_group, left, right, feat, thresh, defl, value,        \
      tree_root, tree_cls, t_begin, t_end, out, k, n_inner, trees_per_chunk, tile

__global__ __launch_bounds__(HIST_BLOCK) void predict_forest_csr_kernel(FOREST_CSR_PARAMS) {
  forest_csr_body<false>(FOREST_CSR_ARGS);
}

__global__ __launch_bounds__(HIST_BLOCK) void pred_leaf_csr_kernel(FOREST_CSR_PARAMS) {
  forest_csr_body<true>(FOREST_CSR_ARGS);
}

// ---------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------

static void check_csr(const torch::Tensor& indptr, const torch::Tensor& indices) {
  CHECK_DEV(indptr, torch::kInt64);
  CHECK_DEV(indices, torch::kInt32);
  TORCH_CHECK_VALUE(indptr.dim() == 1 && indptr.size(0) >= 1, "indptr must hold n + 1 offsets");
}

void hist_sparse(torch::Tensor indptr, torch::Tensor indices, torch::Tensor bin_data,
                 torch::Tensor gh, torch::Tensor rowbuf, torch::Tensor jobs,
                 torch::Tensor block_job, torch::Tensor out, torch::Tensor totals,
                 int64_t nfeat, int64_t stride, torch::Tensor gh_max) {
  check_csr(indptr, indices);
  CHECK_DEV(gh, torch::kFloat32);
  CHECK_DEV(rowbuf, torch::kInt32);
  CHECK_DEV(jobs, torch::kInt32);
  CHECK_DEV(block_job, torch::kInt32);
  CHECK_DEV(out, torch::kInt64);
  CHECK_DEV(totals, torch::kInt64);
  CHECK_DEV(gh_max, torch::kFloat32);
  TORCH_CHECK_VALUE(bin_data.is_cuda() && bin_data.is_contiguous() &&
                        bin_data.numel() == indices.numel(),
                    "bin_data must be a device tensor with one bin per stored entry");
  TORCH_CHECK_VALUE(gh.numel() == 2 * (indptr.size(0) - 1), "gh must be (n, 2)");
  TORCH_CHECK_VALUE(gh_max.numel() == 2, "gh_max must hold (gmax, hmax)");
  // the wave prefix of 64 row lengths is an int
  TORCH_CHECK_VALUE(nfeat > 0 && stride > 1 && nfeat < (1ll << 31) / WAVE,
                    "feature count out of range for the sparse histogram kernel");
  const long long n_hist = totals.numel() / 2;
  TORCH_CHECK_VALUE(out.numel() == n_hist * nfeat * stride * 2,
                    "out must be (J, nfeat * stride, 2) for (J, 2) totals");
  const int grid = (int)block_job.size(0);
  if (grid == 0) return;
  auto stream = sparse_stream();
#define LAUNCH_HIST_SPARSE(T, PTR)                                                          \
  hipLaunchKernelGGL(hist_sparse_kernel<T>, dim3(grid), dim3(HIST_BLOCK), 0, stream,        \
                     (const long long*)indptr.data_ptr<int64_t>(), indices.data_ptr<int>(), \
                     PTR, (const float2*)gh.data_ptr<float>(), rowbuf.data_ptr<int>(),      \
                     (const HistJob*)jobs.data_ptr<int>(), block_job.data_ptr<int>(),       \
                     (u64*)out.data_ptr<int64_t>(), (u64*)totals.data_ptr<int64_t>(),       \
                     (int)nfeat, (int)stride, gh_max.data_ptr<float>())
  if (bin_data.scalar_type() == torch::kUInt8) {
    LAUNCH_HIST_SPARSE(unsigned char, bin_data.data_ptr<unsigned char>());
  } else {
    TORCH_CHECK_VALUE(bin_data.scalar_type() == torch::kInt16, "bin_data must be uint8 or int16");
    LAUNCH_HIST_SPARSE(short, bin_data.data_ptr<short>());
  }
#undef LAUNCH_HIST_SPARSE
}

void hist_sparse_close(torch::Tensor out, torch::Tensor totals, int64_t nfeat, int64_t stride) {
  CHECK_DEV(out, torch::kInt64);
  CHECK_DEV(totals, torch::kInt64);
  const long long n_hist = totals.numel() / 2;
  TORCH_CHECK_VALUE(nfeat > 0 && stride > 1 && out.numel() == n_hist * nfeat * stride * 2,
                    "out must be (J, nfeat * stride, 2) for (J, 2) totals");
  const long long n_pairs = n_hist * nfeat;
  if (n_pairs == 0) return;
  const int waves_per_block = HIST_BLOCK / WAVE;
  const int grid =
      (int)std::min<long long>((n_pairs + waves_per_block - 1) / waves_per_block, 8192);
  hipLaunchKernelGGL(hist_sparse_close_kernel, dim3(grid), dim3(HIST_BLOCK), 0, sparse_stream(),
                     (u64*)out.data_ptr<int64_t>(), (const u64*)totals.data_ptr<int64_t>(),
                     n_pairs, (int)nfeat, (int)stride);
}

void partition_sparse(torch::Tensor indptr, torch::Tensor indices, torch::Tensor bin_data,
                      torch::Tensor src, torch::Tensor dst, torch::Tensor jobs,
                      torch::Tensor block_job, torch::Tensor split_packed,
                      torch::Tensor counters) {
  check_csr(indptr, indices);
  CHECK_DEV(src, torch::kInt32);
  CHECK_DEV(dst, torch::kInt32);
  CHECK_DEV(jobs, torch::kInt32);
  CHECK_DEV(block_job, torch::kInt32);
  CHECK_DEV(split_packed, torch::kFloat32);
  CHECK_DEV(counters, torch::kInt32);
  TORCH_CHECK_VALUE(bin_data.is_cuda() && bin_data.is_contiguous() &&
                        bin_data.numel() == indices.numel(),
                    "bin_data must be a device tensor with one bin per stored entry");
  TORCH_CHECK_VALUE(src.numel() == dst.numel(), "src and dst row buffers differ in size");
  const int grid = (int)block_job.size(0);
  if (grid == 0) return;
  auto stream = sparse_stream();
#define LAUNCH_PART_SPARSE(T, PTR)                                                            \
  hipLaunchKernelGGL(partition_sparse_kernel<T>, dim3(grid), dim3(HIST_BLOCK), 0, stream,     \
                     (const long long*)indptr.data_ptr<int64_t>(), indices.data_ptr<int>(),   \
                     PTR, src.data_ptr<int>(), dst.data_ptr<int>(),                           \
                     (const PartJob*)jobs.data_ptr<int>(), block_job.data_ptr<int>(),         \
                     split_packed.data_ptr<float>(), counters.data_ptr<int>())
  if (bin_data.scalar_type() == torch::kUInt8) {
    LAUNCH_PART_SPARSE(unsigned char, bin_data.data_ptr<unsigned char>());
  } else {
    TORCH_CHECK_VALUE(bin_data.scalar_type() == torch::kInt16, "bin_data must be uint8 or int16");
    LAUNCH_PART_SPARSE(short, bin_data.data_ptr<short>());
  }
#undef LAUNCH_PART_SPARSE
}

void predict_tree_csr(torch::Tensor indptr, torch::Tensor indices, torch::Tensor data,
                      torch::Tensor left, torch::Tensor right, torch::Tensor feat,
                      torch::Tensor thresh, torch::Tensor defl, torch::Tensor value,
                      torch::Tensor out) {
  check_csr(indptr, indices);
  CHECK_DEV(data, torch::kFloat32);
  CHECK_DEV(left, torch::kInt32);
  CHECK_DEV(right, torch::kInt32);
  CHECK_DEV(feat, torch::kInt32);
  CHECK_DEV(thresh, torch::kFloat32);
  CHECK_DEV(defl, torch::kUInt8);
  CHECK_DEV(value, torch::kFloat32);
  CHECK_DEV(out, torch::kFloat32);
  const long long n = indptr.size(0) - 1;
  TORCH_CHECK_VALUE(data.numel() == indices.numel(), "data and indices differ in size");
  TORCH_CHECK_VALUE(out.numel() == n, "out must hold one value per row");
  TORCH_CHECK_VALUE(left.numel() >= 1, "empty tree");
  if (n == 0) return;
  const int grid = (int)std::min<long long>((n + HIST_BLOCK - 1) / HIST_BLOCK, 4096);
  hipLaunchKernelGGL(predict_tree_csr_kernel, dim3(grid), dim3(HIST_BLOCK), 0, sparse_stream(),
                     (const long long*)indptr.data_ptr<int64_t>(), indices.data_ptr<int>(),
                     data.data_ptr<float>(), n, left.data_ptr<int>(), right.data_ptr<int>(),
                     feat.data_ptr<int>(), thresh.data_ptr<float>(),
                     defl.data_ptr<unsigned char>(), value.data_ptr<float>(),
                     out.data_ptr<float>());
}

// Shared validation and launch of the forest-over-CSR kernel. `n_inner` is
// the chunk count (margins, out = (n_inner, n, k) float32) or the tree count
// (leaves, out = (n, n_inner) int32). Everything is checked on the host
// before the launch; the offsets and column ids themselves are checked when
// the matrix is uploaded (hip_sparse.DeviceCSR).
template <bool LEAF>
static void launch_forest_csr(torch::Tensor indptr, torch::Tensor indices, torch::Tensor data,
                              torch::Tensor left, torch::Tensor right, torch::Tensor feat,
                              torch::Tensor thresh, torch::Tensor defl, torch::Tensor value,
                              torch::Tensor tree_root, torch::Tensor tree_cls, int64_t t_begin,
                              int64_t t_end, torch::Tensor out, int64_t k, int64_t n_inner,
                              int64_t trees_per_chunk, int64_t rows_per_group, int64_t tile) {
  check_csr(indptr, indices);
  CHECK_DEV(data, torch::kFloat32);
  CHECK_DEV(left, torch::kInt32);
  CHECK_DEV(right, torch::kInt32);
  CHECK_DEV(feat, torch::kInt32);
  CHECK_DEV(thresh, torch::kFloat32);
  CHECK_DEV(defl, torch::kUInt8);
  CHECK_DEV(value, torch::kFloat32);
  CHECK_DEV(tree_root, torch::kInt32);
  CHECK_DEV(tree_cls, torch::kInt32);
  const auto out_dtype = LEAF ? torch::kInt32 : torch::kFloat32;
  CHECK_DEV(out, out_dtype);
  const long long n = indptr.size(0) - 1;
  const long long nodes = left.numel();
  TORCH_CHECK_VALUE(data.numel() == indices.numel(), "data and indices differ in size");
  TORCH_CHECK_VALUE(right.numel() == nodes && feat.numel() == nodes && thresh.numel() == nodes &&
                        defl.numel() == nodes && value.numel() == nodes,
                    "forest node arrays differ in size");
  TORCH_CHECK_VALUE(tree_cls.numel() == tree_root.numel(), "tree_root and tree_cls differ in size");
  TORCH_CHECK_VALUE(0 <= t_begin && t_begin <= t_end && t_end <= tree_root.numel(),
                    "tree range out of bounds");
  TORCH_CHECK_VALUE(k >= 1 && n_inner >= 1 && trees_per_chunk >= 1 &&
                        n_inner * trees_per_chunk >= t_end - t_begin &&
                        n_inner * trees_per_chunk <= (1ll << 30) && t_end <= (1ll << 30),
                    "tree chunking does not cover the tree range");
  TORCH_CHECK_VALUE(rows_per_group >= 1 && rows_per_group <= (1 << 20),
                    "rows_per_group out of range");
  TORCH_CHECK_VALUE(tile >= 0 && tile <= PCSR_MAX_TILE, "LDS tile of ", tile,
                    " entries exceeds ", PCSR_MAX_TILE);
  TORCH_CHECK_VALUE(out.numel() == (LEAF ? n * n_inner : n_inner * n * k),
                    LEAF ? "out must be (n, T) for n + 1 offsets"
                         : "out must be (n_chunks, n, k) for n + 1 offsets");
  if (n == 0 || t_end == t_begin) return;
  const long long n_groups = (n + rows_per_group - 1) / rows_per_group;
  const int grid = (int)std::min<long long>(n_groups, 4096);
  const size_t lds = (size_t)tile * (sizeof(int) + sizeof(float));
  hipLaunchKernelGGL(LEAF ? pred_leaf_csr_kernel : predict_forest_csr_kernel, dim3(grid), dim3(HIST_BLOCK), lds,
                     sparse_stream(), (const long long*)indptr.data_ptr<int64_t>(),
                     indices.data_ptr<int>(), data.data_ptr<float>(), n, (int)rows_per_group,
                     left.data_ptr<int>(), right.data_ptr<int>(), feat.data_ptr<int>(),
                     thresh.data_ptr<float>(), defl.data_ptr<unsigned char>(),
                     value.data_ptr<float>(), tree_root.data_ptr<int>(),
                     tree_cls.data_ptr<int>(), (int)t_begin, (int)t_end, out.data_ptr(), (int)k,
                     (int)n_inner, (int)trees_per_chunk, (int)tile);
  const hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, "forest-over-CSR kernel launch failed: ", hipGetErrorString(err));
}

void predict_forest_csr(torch::Tensor indptr, torch::Tensor indices, torch::Tensor data,
                        torch::Tensor left, torch::Tensor right, torch::Tensor feat,
                        torch::Tensor thresh, torch::Tensor defl, torch::Tensor value,
                        torch::Tensor tree_root, torch::Tensor tree_cls, int64_t t_begin,
                        int64_t t_end, torch::Tensor out, int64_t k, int64_t n_chunks,
                        int64_t trees_per_chunk, int64_t rows_per_group, int64_t tile) {
  launch_forest_csr<false>(indptr, indices, data, left, right, feat, thresh, defl, value,
                           tree_root, tree_cls, t_begin, t_end, out, k, n_chunks,
                           trees_per_chunk, rows_per_group, tile);
}

void pred_leaf_csr(torch::Tensor indptr, torch::Tensor indices, torch::Tensor data,
                   torch::Tensor left, torch::Tensor right, torch::Tensor feat,
                   torch::Tensor thresh, torch::Tensor defl, torch::Tensor value,
                   torch::Tensor tree_root, torch::Tensor tree_cls, int64_t t_begin,
                   int64_t t_end, torch::Tensor out, int64_t rows_per_group, int64_t tile) {
  launch_forest_csr<true>(indptr, indices, data, left, right, feat, thresh, defl, value,
                          tree_root, tree_cls, t_begin, t_end, out, 1, t_end - t_begin, 1,
                          rows_per_group, tile);
}

void init_sparse_kernels(pybind11::module_& m) {
  m.def("predict_forest_csr", &predict_forest_csr,
        "summed margins of a flat forest over raw CSR rows, per tree chunk");
  m.def("pred_leaf_csr", &pred_leaf_csr, "leaf index per (row, tree) over raw CSR rows");
  m.def("hist_sparse", &hist_sparse, "fixed-point histogram of stored CSR entries + job totals");
  m.def("hist_sparse_close", &hist_sparse_close, "missing slot = job total - present bins");
  m.def("partition_sparse", &partition_sparse, "batched two-ended row partition over CSR rows");
  m.def("predict_tree_csr", &predict_tree_csr, "one tree over raw CSR rows");
}
