// MI355X (gfx950 / CDNA4) kernels that quantize a CSR float32 matrix: cuts
// per feature over its stored values, and the bin of every stored entry. The
// rule is ops/sparse_ref.quantize_sparse's, bit for bit.
//
// A feature's stored values are not contiguous in CSR, and wide data has tens
// of thousands of features with a few hundred entries each, so the dense
// radix select (2 MiB of counters a feature) does not fit. Instead:
//
//   count    entries per column (and: is a NaN stored, is a column id out of
//            range), one atomic per entry
//   scatter  qz_key(value) to a per-column cursor: the CSC *key image*. Only
//            keys move, no row ids; the order inside a segment is arbitrary
//            and does not matter, every segment is sorted or counted next
//   sort     a segment of at most QC_SORT_CAP keys is sorted in LDS (bitonic,
//            padded to a power of two) and its cuts come out of the same
//            kernel: distinct values by head flags and a scan, then either
//            the float32 midpoints of neighbours (at most max_bin distinct
//            values) or the values at the feature's target ranks without
//            repeats. One workgroup per segment; segments of at most
//            QC_WAVE_CAP keys take one wave each, four to a block, without a
//            block barrier
//   hist     a longer segment goes through the radix select of
//            smxgb_quantize.hip: this file only adds the histogram pass that
//            reads a slice of the contiguous keys (no tile to turn), with
//            the same counter layouts, so that quantize_refine and
//            quantize_final serve it unchanged
//   bin      one thread per stored entry, in CSR order: binary search of the
//            value in its feature's cuts
//
// Both tiers write cuts_pad[feature][:] and ncut[feature], which
// quantize_compact flattens.

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <algorithm>

// Built without packed float32 instructions, as ops/csrc/smxgb_rank.hip is
// (and says why).
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

// the midpoint (a + b) * 0.5 rounds like the reference's two operations
#pragma clang fp contract(off)

#include "smxgb_quantize.h"

#define CHECK_DEV(x, dt)                                                       \
  TORCH_CHECK_VALUE(x.is_cuda() && x.is_contiguous() && x.scalar_type() == dt, \
                    #x " must be a contiguous ROCm device tensor of the expected dtype")

#define QC_SORT_CAP 8192   // keys of the longest segment sorted in LDS (32 KiB)
#define QC_WAVE_CAP 256    // keys of the longest segment sorted by one wave
#define QC_PAD_KEY 0xffffffffu
#define QC_FLAG_NAN 1
#define QC_FLAG_RANGE 2

static hipStream_t quantize_csr_stream() { return at::hip::getCurrentHIPStream().stream(); }

// counts[col] += 1 for every stored entry; counts[f] collects the flags.
__global__ __launch_bounds__(QZ_BLOCK) void qc_count_kernel(
    const int* __restrict__ indices, const unsigned* __restrict__ values, long long nnz, int f,
    int* __restrict__ counts) {
  const long long i = (long long)blockIdx.x * QZ_BLOCK + threadIdx.x;
  if (i >= nnz) return;
  const int col = indices[i];
  int flags = qz_is_nan(values[i]) ? QC_FLAG_NAN : 0;
  if (col < 0 || col >= f) flags |= QC_FLAG_RANGE;
  else atomicAdd(&counts[col], 1);
  if (flags) atomicOr(&counts[f], flags);
}

// keys[cursor[col]++] = qz_key(value). cursor starts as the columns' first
// positions (the exclusive scan of the counts).
__global__ __launch_bounds__(QZ_BLOCK) void qc_scatter_kernel(
    const int* __restrict__ indices, const unsigned* __restrict__ values, long long nnz, int f,
    int* __restrict__ cursor, unsigned* __restrict__ keys) {
  const long long i = (long long)blockIdx.x * QZ_BLOCK + threadIdx.x;
  if (i >= nnz) return;
  const int col = indices[i];
  if (col < 0 || col >= f) return;
  const int at = atomicAdd(&cursor[col], 1);
  if (at >= 0 && at < nnz) keys[at] = qz_key(values[i]);
}

// The threads that share a segment: a wave (no block barrier: the LDS
// accesses of one wave complete in program order, the fence keeps the
// compiler from moving them) or the block.
template <bool WAVE>
__device__ __forceinline__ void qc_sync() {
  if constexpr (WAVE) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  } else {
    __syncthreads();
  }
}

template <bool WAVE>
__device__ __forceinline__ int qc_scan(int v, int* s_w, int& total) {
  if constexpr (WAVE) return qz_wave_scan(v, total);
  else return qz_block_scan(v, s_w, total);
}

// Sorts the m keys of a segment in s[0, P) (P a power of two, 2 <= m <= P)
// and writes the feature's cuts to out[0, Tpad) and their number to *nc_out.
// rk: the T = max_bin - 1 target ranks of a segment of this length (read only
// when the segment has more than max_bin distinct values). Called by all NT
// threads of the wave (tid = lane) or the block (tid = threadIdx.x).
template <bool WAVE>
__device__ __forceinline__ void qc_segment_cuts(
    unsigned* s, const unsigned* __restrict__ keys, int m, int P, int tid, int* s_w, int max_bin,
    const int* __restrict__ rk, int T, float* __restrict__ out, int Tpad, int* __restrict__ nc_out) {
  constexpr int NT = WAVE ? QZ_WAVE : QZ_BLOCK;
  for (int i = tid; i < P; i += NT) s[i] = i < m ? keys[i] : QC_PAD_KEY;
  qc_sync<WAVE>();

  // bitonic network: pair (a, a | j) of the i-th of P / 2 comparators
  for (int size = 2; size <= P; size <<= 1) {
    for (int j = size >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < (P >> 1); i += NT) {
        const int a = ((i & ~(j - 1)) << 1) | (i & (j - 1));
        const int b = a | j;
        const unsigned ka = s[a];
        const unsigned kb = s[b];
        const bool up = (a & size) == 0;
        if ((ka > kb) == up) {
          s[a] = kb;
          s[b] = ka;
        }
      }
      qc_sync<WAVE>();
    }
  }

  // distinct values: heads of runs of equal keys
  int heads = 0;
  for (int i = tid; i < m; i += NT) heads += (i == 0 || s[i] != s[i - 1]) ? 1 : 0;
  int d;
  qc_scan<WAVE>(heads, s_w, d);

  int nc = 0;
  if (d <= max_bin) {  // uniform
    // the distinct keys to s[0, d), in place: a head moves to the number of
    // heads before it, never past itself. A tile's reads come before its
    // writes, and the element before a tile is only ever rewritten by itself
    int run = 0;
    for (int base = 0; base < m; base += NT) {
      const int i = base + tid;
      unsigned k = 0u;
      int h = 0;
      if (i < m) {
        k = s[i];
        h = (i == 0 || k != s[i - 1]) ? 1 : 0;
      }
      qc_sync<WAVE>();
      int tot;
      const int pos = run + qc_scan<WAVE>(h, s_w, tot);
      if (h) s[pos] = k;
      run += tot;
      qc_sync<WAVE>();
    }
    nc = d - 1 < Tpad ? d - 1 : Tpad;
    for (int i = tid; i < nc; i += NT) out[i] = (qz_value(s[i]) + qz_value(s[i + 1])) * 0.5f;
  } else {
    // the values at the target ranks; a rank's value equal to the one before
    // it is dropped (the ranks rise, so equal values are neighbours)
    int run = 0;
    for (int t0 = 0; t0 < T; t0 += NT) {
      const int t = t0 + tid;
      unsigned k = 0u;
      int first = 0;
      if (t < T) {
        int p = rk[t];
        p = p < 0 ? 0 : (p >= m ? m - 1 : p);
        k = s[p];
        first = 1;
        if (t > 0) {
          int q = rk[t - 1];
          q = q < 0 ? 0 : (q >= m ? m - 1 : q);
          first = s[q] != k ? 1 : 0;
        }
      }
      int tot;
      const int pos = run + qc_scan<WAVE>(first, s_w, tot);
      if (first && pos < Tpad) out[pos] = qz_value(k);
      run += tot;
    }
    nc = run < Tpad ? run : Tpad;
  }
  if (tid == 0) *nc_out = nc;
}

// Segment of job `job`: its feature, first key and length; false when the job
// table or the offsets do not describe a segment of 2 .. cap keys.
__device__ __forceinline__ bool qc_job_segment(
    const int* __restrict__ jobs, int job, const int* __restrict__ csc_ptr, int f, long long nnz,
    int cap, int& feat, int& first, int& m) {
  feat = jobs[job];
  if (feat < 0 || feat >= f) return false;
  first = csc_ptr[feat];
  m = csc_ptr[feat + 1] - first;
  return first >= 0 && m >= 2 && m <= cap && (long long)first + m <= nnz;
}

__device__ __forceinline__ const int* qc_rank_row(
    const int* __restrict__ ranks, const int* __restrict__ ridx, int feat, int n_rank_rows, int T) {
  int rr = ridx[feat];
  rr = rr < 0 ? 0 : (rr >= n_rank_rows ? n_rank_rows - 1 : rr);
  return ranks + (long long)rr * T;
}

// One workgroup per job: a segment of at most P keys, P * 4 bytes of dynamic
// LDS. jobs: feature ids; ranks: [n_rank_rows][T], ridx: [f].
__global__ __launch_bounds__(QZ_BLOCK) void qc_sort_block_kernel(
    const unsigned* __restrict__ keys, long long nnz, const int* __restrict__ csc_ptr, int f,
    const int* __restrict__ jobs, int P, int max_bin, const int* __restrict__ ranks,
    const int* __restrict__ ridx, int n_rank_rows, int T, float* __restrict__ cuts_pad, int Tpad,
    int* __restrict__ ncut) {
  extern __shared__ unsigned qc_lds[];
  __shared__ int s_w[QZ_WAVES];
  int feat, first, m;
  if (!qc_job_segment(jobs, blockIdx.x, csc_ptr, f, nnz, P, feat, first, m)) return;  // uniform
  qc_segment_cuts<false>(qc_lds, keys + first, m, P, threadIdx.x, s_w, max_bin,
                         qc_rank_row(ranks, ridx, feat, n_rank_rows, T), T,
                         cuts_pad + (long long)feat * Tpad, Tpad, ncut + feat);
}

// One wave per job, QZ_WAVES jobs a block, segments of at most QC_WAVE_CAP
// keys: the waves of a block never wait for each other.
__global__ __launch_bounds__(QZ_BLOCK) void qc_sort_wave_kernel(
    const unsigned* __restrict__ keys, long long nnz, const int* __restrict__ csc_ptr, int f,
    const int* __restrict__ jobs, int njobs, int max_bin, const int* __restrict__ ranks,
    const int* __restrict__ ridx, int n_rank_rows, int T, float* __restrict__ cuts_pad, int Tpad,
    int* __restrict__ ncut) {
  __shared__ unsigned s_keys[QZ_WAVES * QC_WAVE_CAP];
  const int wave = threadIdx.x / QZ_WAVE;
  const int job = blockIdx.x * QZ_WAVES + wave;
  if (job >= njobs) return;  // uniform over the wave
  int feat, first, m;
  if (!qc_job_segment(jobs, job, csc_ptr, f, nnz, QC_WAVE_CAP, feat, first, m)) return;
  int P = 2;
  while (P < m) P <<= 1;
  qc_segment_cuts<true>(s_keys + wave * QC_WAVE_CAP, keys + first, m, P,
                        threadIdx.x & (QZ_WAVE - 1), nullptr, max_bin,
                        qc_rank_row(ranks, ridx, feat, n_rank_rows, T), T,
                        cuts_pad + (long long)feat * Tpad, Tpad, ncut + feat);
}

// A radix pass over the key segments of the long features heavy[0, fcount).
// Block (x, y): the x-th slice of `slice` keys of feature heavy[y]. counts,
// active and nactive are indexed by y, with qz_hist_kernel's layouts:
//   PASS 1: counts[y][2048]
//   PASS 2, 3: counts[y][A][2048], active[y][A] sorted, nactive[y] <= A
// Dynamic LDS: 2048 counters (pass 1, flushed once) or A prefixes.
template <int PASS>
__global__ __launch_bounds__(QZ_BLOCK) void qc_seg_hist_kernel(
    const unsigned* __restrict__ keys, long long nnz, const int* __restrict__ csc_ptr, int f,
    const int* __restrict__ heavy, int slice, const unsigned* __restrict__ active,
    const int* __restrict__ nactive, int A, int* __restrict__ counts) {
  extern __shared__ unsigned qc_lds[];
  const int y = blockIdx.y;
  const int feat = heavy[y];
  if (feat < 0 || feat >= f) return;  // uniform
  const long long seg_lo = csc_ptr[feat];
  const long long seg_hi = csc_ptr[feat + 1];
  const long long lo = seg_lo + (long long)blockIdx.x * slice;
  const long long hi = lo + slice < seg_hi ? lo + slice : seg_hi;
  if (seg_lo < 0 || seg_hi > nnz || lo >= hi) return;  // uniform

  int na = 0;
  if (PASS == 1) {
    for (int i = threadIdx.x; i < QZ_DIGITS; i += QZ_BLOCK) qc_lds[i] = 0u;
  } else {
    na = nactive[y];
    na = na < 0 ? 0 : (na > A ? A : na);
    for (int i = threadIdx.x; i < na; i += QZ_BLOCK) qc_lds[i] = active[(long long)y * A + i];
  }
  __syncthreads();

  for (long long base = lo; base < hi; base += QZ_BLOCK) {  // uniform: every lane adds
    const long long i = base + threadIdx.x;
    int addr = -1;
    if (i < hi) {
      const unsigned key = keys[i];
      if (PASS == 1) {
        addr = (int)(key >> 21);
      } else {
        const unsigned pre = PASS == 2 ? key >> 21 : key >> 10;
        const int dig = PASS == 2 ? (int)((key >> 10) & 2047u) : (int)(key & 1023u);
        int l = 0, h = na;
        while (l < h) {
          const int mid = (l + h) >> 1;
          if (qc_lds[mid] < pre) l = mid + 1; else h = mid;
        }
        if (l < na && qc_lds[l] == pre) addr = (y * A + l) * QZ_DIGITS + dig;
      }
    }
    qz_wave_add(PASS == 1 ? (int*)qc_lds : counts, addr, 1, addr >= 0);
  }

  if (PASS == 1) {
    __syncthreads();
    for (int i = threadIdx.x; i < QZ_DIGITS; i += QZ_BLOCK) {
      const int v = (int)qc_lds[i];
      if (v != 0) atomicAdd(&counts[(long long)y * QZ_DIGITS + i], v);
    }
  }
}

// bins[i] = #{cuts of entry i's feature that are <= its value}. The cuts of
// wide data (f * (max_bin - 1) floats) do not fit LDS and entries of a row
// touch another feature each, so the search reads global memory (L2).
template <typename OutT>
__global__ __launch_bounds__(QZ_BLOCK) void qc_bin_kernel(
    const int* __restrict__ indices, const float* __restrict__ values, long long nnz, int f,
    const float* __restrict__ cuts, const long long* __restrict__ cut_ptr, long long ncuts,
    OutT* __restrict__ bins) {
  const long long i = (long long)blockIdx.x * QZ_BLOCK + threadIdx.x;
  if (i >= nnz) return;
  const int col = indices[i];
  int b = 0;
  if (col >= 0 && col < f) {
    const float v = values[i];
    long long lo = cut_ptr[col], hi = cut_ptr[col + 1];
    if (lo >= 0 && hi <= ncuts) {
      const long long first = lo;
      while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (cuts[mid] <= v) lo = mid + 1; else hi = mid;
      }
      b = (int)(lo - first);
    }
  }
  bins[i] = (OutT)b;
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

static void qc_check_launch(const char* what) {
  const hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, what, " launch failed: ", hipGetErrorString(err));
}

static long long qc_entries(const torch::Tensor& indices, const torch::Tensor& values) {
  CHECK_DEV(indices, torch::kInt32);
  CHECK_DEV(values, torch::kFloat32);
  const long long nnz = indices.numel();
  TORCH_CHECK_VALUE(nnz >= 1 && nnz < (1ll << 31) && values.numel() == nnz,
                    "need 1 <= nnz < 2^31 column ids and as many values");
  return nnz;
}

int64_t quantize_csr_sort_cap() { return QC_SORT_CAP; }
int64_t quantize_csr_wave_cap() { return QC_WAVE_CAP; }

// counts: int32 [f + 1], zeroed by the caller. counts[:f] gets the entries per
// column, counts[f] the flags: 1 a NaN is stored, 2 a column id is outside [0, f).
void quantize_csr_count(torch::Tensor indices, torch::Tensor values, torch::Tensor counts) {
  const long long nnz = qc_entries(indices, values);
  CHECK_DEV(counts, torch::kInt32);
  const long long f = counts.numel() - 1;
  TORCH_CHECK_VALUE(f >= 1 && f < (1ll << 31) - 1, "counts must be [f + 1]");
  hipLaunchKernelGGL(qc_count_kernel, dim3((unsigned)((nnz + QZ_BLOCK - 1) / QZ_BLOCK)),
                     dim3(QZ_BLOCK), 0, quantize_csr_stream(), indices.data_ptr<int>(),
                     (const unsigned*)values.data_ptr<float>(), nnz, (int)f, counts.data_ptr<int>());
  qc_check_launch("qc_count_kernel");
}

// cursor: int32 [f], every column's first position in keys (advanced to its
// end here); keys: int32 [nnz], written.
void quantize_csr_scatter(torch::Tensor indices, torch::Tensor values, torch::Tensor cursor,
                          torch::Tensor keys) {
  const long long nnz = qc_entries(indices, values);
  CHECK_DEV(cursor, torch::kInt32);
  CHECK_DEV(keys, torch::kInt32);
  const long long f = cursor.numel();
  TORCH_CHECK_VALUE(f >= 1 && f < (1ll << 31) - 1 && keys.numel() == nnz,
                    "cursor must be [f] and keys [nnz]");
  hipLaunchKernelGGL(qc_scatter_kernel, dim3((unsigned)((nnz + QZ_BLOCK - 1) / QZ_BLOCK)),
                     dim3(QZ_BLOCK), 0, quantize_csr_stream(), indices.data_ptr<int>(),
                     (const unsigned*)values.data_ptr<float>(), nnz, (int)f, cursor.data_ptr<int>(),
                     (unsigned*)keys.data_ptr<int>());
  qc_check_launch("qc_scatter_kernel");
}

// Cuts of the features jobs[:] (int32 ids), whose segments keys[csc_ptr[j] :
// csc_ptr[j + 1]] hold 2 .. P keys each. P: a power of two up to the sort
// cap; P == quantize_csr_wave_cap() sorts one segment per wave. ranks: int32
// [rows][T] with T = max_bin - 1 (any one row when T == 0), ridx: int32 [f].
// Writes cuts_pad[j][:] (float32 [f][Tpad]) and ncut[j] (int32 [f]).
void quantize_csr_sort(torch::Tensor keys, torch::Tensor csc_ptr, torch::Tensor jobs, int64_t P,
                       int64_t max_bin, torch::Tensor ranks, torch::Tensor ridx,
                       torch::Tensor cuts_pad, int64_t Tpad, torch::Tensor ncut) {
  CHECK_DEV(keys, torch::kInt32);
  CHECK_DEV(csc_ptr, torch::kInt32);
  CHECK_DEV(jobs, torch::kInt32);
  CHECK_DEV(ranks, torch::kInt32);
  CHECK_DEV(ridx, torch::kInt32);
  CHECK_DEV(cuts_pad, torch::kFloat32);
  CHECK_DEV(ncut, torch::kInt32);
  const long long nnz = keys.numel();
  const long long f = csc_ptr.numel() - 1;
  const long long njobs = jobs.numel();
  const long long T = max_bin - 1;
  TORCH_CHECK_VALUE(nnz >= 1 && nnz < (1ll << 31) && f >= 1 && njobs >= 1 && njobs < (1ll << 31),
                    "empty launch");
  TORCH_CHECK_VALUE(P >= QC_WAVE_CAP && P <= QC_SORT_CAP && (P & (P - 1)) == 0,
                    "P must be a power of two between the wave cap and the sort cap");
  TORCH_CHECK_VALUE(max_bin >= 1 && Tpad >= 1 && Tpad >= T, "need Tpad >= max(max_bin - 1, 1)");
  TORCH_CHECK_VALUE(ridx.numel() == f && ncut.numel() == f && cuts_pad.numel() == f * Tpad,
                    "per-feature buffers do not match the feature count");
  const long long nrr = T > 0 ? ranks.numel() / T : 1;
  TORCH_CHECK_VALUE(ranks.numel() >= 1 && (T == 0 || (nrr >= 1 && ranks.numel() == nrr * T)),
                    "ranks must be [rows][max_bin - 1]");
  const unsigned* kp = (const unsigned*)keys.data_ptr<int>();
  if (P == QC_WAVE_CAP)
    hipLaunchKernelGGL(qc_sort_wave_kernel, dim3((unsigned)((njobs + QZ_WAVES - 1) / QZ_WAVES)),
                       dim3(QZ_BLOCK), 0, quantize_csr_stream(), kp, nnz, csc_ptr.data_ptr<int>(),
                       (int)f, jobs.data_ptr<int>(), (int)njobs, (int)max_bin, ranks.data_ptr<int>(),
                       ridx.data_ptr<int>(), (int)nrr, (int)T, cuts_pad.data_ptr<float>(), (int)Tpad,
                       ncut.data_ptr<int>());
  else
    hipLaunchKernelGGL(qc_sort_block_kernel, dim3((unsigned)njobs), dim3(QZ_BLOCK), (size_t)P * 4,
                       quantize_csr_stream(), kp, nnz, csc_ptr.data_ptr<int>(), (int)f,
                       jobs.data_ptr<int>(), (int)P, (int)max_bin, ranks.data_ptr<int>(),
                       ridx.data_ptr<int>(), (int)nrr, (int)T, cuts_pad.data_ptr<float>(), (int)Tpad,
                       ncut.data_ptr<int>());
  qc_check_launch("qc_sort_kernel");
}

// quantize_hist for the long features heavy[:] (int32 ids) of the key image;
// max_len: the longest of their segments. counts, active, nactive as there,
// indexed by the position in heavy.
void quantize_csr_hist(torch::Tensor keys, torch::Tensor csc_ptr, torch::Tensor heavy,
                       int64_t max_len, int64_t pass, torch::Tensor active, torch::Tensor nactive,
                       int64_t A, torch::Tensor counts) {
  CHECK_DEV(keys, torch::kInt32);
  CHECK_DEV(csc_ptr, torch::kInt32);
  CHECK_DEV(heavy, torch::kInt32);
  CHECK_DEV(active, torch::kInt32);
  CHECK_DEV(nactive, torch::kInt32);
  CHECK_DEV(counts, torch::kInt32);
  const long long nnz = keys.numel();
  const long long f = csc_ptr.numel() - 1;
  const long long fc = heavy.numel();
  TORCH_CHECK_VALUE(nnz >= 1 && nnz < (1ll << 31) && f >= 1 && fc >= 1 && fc <= 65535,
                    "need 1 .. 65535 features a launch");
  TORCH_CHECK_VALUE(max_len >= 1 && max_len <= nnz, "max_len out of range");
  TORCH_CHECK_VALUE(pass >= 1 && pass <= 3, "pass must be 1, 2 or 3");
  TORCH_CHECK_VALUE(A >= 1 && A * 4 <= 48 * 1024, "the active list does not fit the LDS");
  if (pass == 1) {
    TORCH_CHECK_VALUE(counts.numel() == fc * QZ_DIGITS, "counts must be [fcount][2048]");
  } else {
    TORCH_CHECK_VALUE(fc * A * QZ_DIGITS < (1ll << 31) && counts.numel() == fc * A * QZ_DIGITS,
                      "counts must be [fcount][A][2048] with fewer than 2^31 counters");
    TORCH_CHECK_VALUE(active.numel() == fc * A && nactive.numel() == fc,
                      "active must be [fcount][A] and nactive [fcount]");
  }
  // about 2048 blocks if every segment were the longest; at least 16 steps each
  long long slice = (max_len * fc + 2047) / 2048;
  slice = std::max<long long>(16 * QZ_BLOCK, (slice + QZ_BLOCK - 1) / QZ_BLOCK * QZ_BLOCK);
  const long long gx = (max_len + slice - 1) / slice;
  TORCH_CHECK_VALUE(slice < (1ll << 31) && gx < (1ll << 31), "grid out of range");
  const dim3 grid((unsigned)gx, (unsigned)fc);
  const size_t lds = pass == 1 ? (size_t)QZ_DIGITS * 4 : (size_t)A * 4;
  const unsigned* kp = (const unsigned*)keys.data_ptr<int>();
  const unsigned* act = (const unsigned*)active.data_ptr<int>();
  hipStream_t stream = quantize_csr_stream();
  if (pass == 1)
    hipLaunchKernelGGL(qc_seg_hist_kernel<1>, grid, dim3(QZ_BLOCK), lds, stream, kp, nnz,
                       csc_ptr.data_ptr<int>(), (int)f, heavy.data_ptr<int>(), (int)slice, act,
                       nactive.data_ptr<int>(), (int)A, counts.data_ptr<int>());
  else if (pass == 2)
    hipLaunchKernelGGL(qc_seg_hist_kernel<2>, grid, dim3(QZ_BLOCK), lds, stream, kp, nnz,
                       csc_ptr.data_ptr<int>(), (int)f, heavy.data_ptr<int>(), (int)slice, act,
                       nactive.data_ptr<int>(), (int)A, counts.data_ptr<int>());
  else
    hipLaunchKernelGGL(qc_seg_hist_kernel<3>, grid, dim3(QZ_BLOCK), lds, stream, kp, nnz,
                       csc_ptr.data_ptr<int>(), (int)f, heavy.data_ptr<int>(), (int)slice, act,
                       nactive.data_ptr<int>(), (int)A, counts.data_ptr<int>());
  qc_check_launch("qc_seg_hist_kernel");
}

// bins (uint8 or int16, [nnz]) of the stored entries in CSR order; cut_ptr:
// int64 [f + 1] on the device.
void quantize_csr_bin(torch::Tensor indices, torch::Tensor values, torch::Tensor cuts,
                      torch::Tensor cut_ptr, torch::Tensor bins) {
  const long long nnz = qc_entries(indices, values);
  CHECK_DEV(cuts, torch::kFloat32);
  CHECK_DEV(cut_ptr, torch::kInt64);
  TORCH_CHECK_VALUE(bins.is_cuda() && bins.is_contiguous() && bins.numel() == nnz,
                    "bins must be a contiguous device tensor with one element per entry");
  const long long f = cut_ptr.numel() - 1;
  TORCH_CHECK_VALUE(f >= 1 && f < (1ll << 31) - 1, "cut_ptr must be [f + 1]");
  const bool wide = bins.scalar_type() == torch::kInt16;
  TORCH_CHECK_VALUE(wide || bins.scalar_type() == torch::kUInt8, "bins must be uint8 or int16");
  const dim3 grid((unsigned)((nnz + QZ_BLOCK - 1) / QZ_BLOCK));
  hipStream_t stream = quantize_csr_stream();
  if (wide)
    hipLaunchKernelGGL(qc_bin_kernel<short>, grid, dim3(QZ_BLOCK), 0, stream,
                       indices.data_ptr<int>(), values.data_ptr<float>(), nnz, (int)f,
                       cuts.data_ptr<float>(), (const long long*)cut_ptr.data_ptr<int64_t>(),
                       (long long)cuts.numel(), (short*)bins.data_ptr<int16_t>());
  else
    hipLaunchKernelGGL(qc_bin_kernel<unsigned char>, grid, dim3(QZ_BLOCK), 0, stream,
                       indices.data_ptr<int>(), values.data_ptr<float>(), nnz, (int)f,
                       cuts.data_ptr<float>(), (const long long*)cut_ptr.data_ptr<int64_t>(),
                       (long long)cuts.numel(), bins.data_ptr<unsigned char>());
  qc_check_launch("qc_bin_kernel");
}

void init_quantize_csr_kernels(pybind11::module_& m) {
  m.def("quantize_csr_sort_cap", &quantize_csr_sort_cap, "longest segment sorted in LDS");
  m.def("quantize_csr_wave_cap", &quantize_csr_wave_cap, "longest segment sorted by one wave");
  m.def("quantize_csr_count", &quantize_csr_count, "entries per column, NaN and range flags");
  m.def("quantize_csr_scatter", &quantize_csr_scatter, "the CSC key image of a CSR matrix");
  m.def("quantize_csr_sort", &quantize_csr_sort, "cuts of short features by an LDS sort");
  m.def("quantize_csr_hist", &quantize_csr_hist, "one radix pass over long key segments");
  m.def("quantize_csr_bin", &quantize_csr_bin, "bins of the stored entries of a CSR matrix");
}
