// MI355X (gfx950 / CDNA4) kernels for adaptive tree leaves
// (reg:absoluteerror, reg:quantileerror): one (weighted) quantile of the
// residuals per leaf, for every leaf of a tree at once.
//
// pos[i] is row i's leaf slot in [0, L) or negative for a row that takes no
// part. The passes, none of which is followed by a host readback:
//
//   count    rows (and fixed-point weight) per leaf
//   (torch)  exclusive scan of the counts -> segment offsets
//   scatter  each leaf's residuals, as orderable u32 keys, into its segment,
//            with the leaf slot of every element and its fixed-point weight
//   init     per leaf: the rank k (unweighted) or the weight threshold
//   4 x (hist, select)  segmented radix select over the key, 8 bits a pass
//   next     unweighted only: the smallest key above v_k where v_{k+1} is
//            not v_k itself
//   final    interpolation in float64, one rounding to float32
//
// The key of a float32 pattern b is b ^ (sign ? ~0u : 0x80000000u): unsigned
// order of the keys is the order of the values (-0 sorts below +0, which the
// result does not see: both have the value 0).
//
// Work distribution. The segmented passes cut the scattered array into
// chunks of LQ_CHUNK elements, one block each, whatever the leaf sizes: one
// huge leaf spans many blocks and a thousand tiny leaves share a few. The
// sizes are known on the device only, so a host-packed (leaf, chunk) job
// table would cost a readback. A chunk that lies inside one leaf (every
// chunk but two of a large leaf) builds its 256-bucket table in LDS, with
// LQ_REP replicas since the residuals of one objective crowd into a few
// buckets, and adds it to the leaf's global table; a chunk that holds a
// boundary adds each element to its leaf's global table directly.
//
// Every sum is an integer sum (row counts, or weights in int64 fixed point
// with a power-of-two scale chosen by the host so that no sum passes 2^50),
// and the minimum of `next` is exact: the result does not depend on the
// order of the rows or of the atomics, bit for bit.

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <algorithm>
#include <cmath>

typedef unsigned long long u64;

// The float64 arithmetic below has to round like the reference's, operation
// by operation: no fused multiply-add.
#pragma clang fp contract(off)

#define CHECK_DEV(x, dt)                                                       \
  TORCH_CHECK_VALUE(x.is_cuda() && x.is_contiguous() && x.scalar_type() == dt, \
                    #x " must be a contiguous ROCm device tensor of the expected dtype")

static hipStream_t quantile_stream() { return at::hip::getCurrentHIPStream().stream(); }

#define LQ_BLOCK 256
#define LQ_WAVE 64
#define LQ_BUCKETS 256
#define LQ_PASSES 4
#define LQ_REP 8           // LDS replicas of a chunk's bucket table (lane % 8)
#define LQ_CHUNK 4096      // scattered elements per block of a segmented pass
#define LQ_ITEMS 8         // rows per thread of the scatter kernel
#define LQ_LDS_LEAVES 2048 // count/scatter aggregate per block in LDS up to here
// per-leaf flag bits
#define LQ_EMPTY 1         // no rows (or no weight): the result is NaN
#define LQ_NEED_NEXT 2     // v_{k+1} is still to be found

__device__ __forceinline__ unsigned lq_key(float v) {
  const unsigned b = __float_as_uint(v);
  return b ^ ((b & 0x80000000u) ? 0xffffffffu : 0x80000000u);
}

__device__ __forceinline__ float lq_value(unsigned key) {
  return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}

__device__ __forceinline__ u64 lq_fixed(float w, double scale) {
  return (u64)llrint((double)w * scale);  // w >= 0 and finite (host-checked)
}

// cnt: int32 [L], wtot: int64 [L] (weighted only), both zeroed.
__global__ __launch_bounds__(LQ_BLOCK) void lq_count_kernel(
    const int* __restrict__ pos, const float* __restrict__ w, long long n, int L, double scale,
    int* __restrict__ cnt, u64* __restrict__ wtot) {
  __shared__ unsigned s_cnt[LQ_LDS_LEAVES];
  __shared__ u64 s_w[LQ_LDS_LEAVES];
  const bool lds = L <= LQ_LDS_LEAVES;  // uniform
  const bool weighted = w != nullptr;
  if (lds) {
    for (int s = threadIdx.x; s < L; s += LQ_BLOCK) {
      s_cnt[s] = 0u;
      s_w[s] = 0ull;
    }
    __syncthreads();
  }
  const long long step = (long long)gridDim.x * LQ_BLOCK;
  for (long long i = (long long)blockIdx.x * LQ_BLOCK + threadIdx.x; i < n; i += step) {
    const int p = pos[i];
    if (p < 0 || p >= L) continue;
    if (lds) {
      atomicAdd(&s_cnt[p], 1u);
      if (weighted) atomicAdd(&s_w[p], lq_fixed(w[i], scale));
    } else {
      atomicAdd(&cnt[p], 1);
      if (weighted) atomicAdd(&wtot[p], lq_fixed(w[i], scale));
    }
  }
  if (lds) {
    __syncthreads();
    for (int s = threadIdx.x; s < L; s += LQ_BLOCK) {
      const unsigned c = s_cnt[s];
      if (c != 0u) {
        atomicAdd(&cnt[s], (int)c);
        if (weighted) atomicAdd(&wtot[s], s_w[s]);
      }
    }
  }
}

// off: int64 [L] exclusive scan of cnt; cursor: int32 [L], zeroed. A block
// owns LQ_BLOCK * LQ_ITEMS rows. Up to LQ_LDS_LEAVES leaves it ranks its
// rows per leaf in LDS and reserves one run per leaf with a single global
// atomic; beyond that every row takes its slot from the global cursor.
__global__ __launch_bounds__(LQ_BLOCK) void lq_scatter_kernel(
    const int* __restrict__ pos, const float* __restrict__ resid, const float* __restrict__ w,
    long long n, int L, double scale, const long long* __restrict__ off, int* __restrict__ cursor,
    unsigned* __restrict__ keys, int* __restrict__ seg, u64* __restrict__ wq) {
  __shared__ unsigned s_cnt[LQ_LDS_LEAVES];
  const bool lds = L <= LQ_LDS_LEAVES;  // uniform
  const bool weighted = w != nullptr;
  if (lds) {
    for (int s = threadIdx.x; s < L; s += LQ_BLOCK) s_cnt[s] = 0u;
    __syncthreads();
  }
  const long long base = (long long)blockIdx.x * (LQ_BLOCK * LQ_ITEMS);
  int leaf[LQ_ITEMS];
  unsigned rank[LQ_ITEMS];
  #pragma unroll
  for (int j = 0; j < LQ_ITEMS; ++j) {
    const long long i = base + (long long)j * LQ_BLOCK + threadIdx.x;
    int p = -1;
    if (i < n) {
      p = pos[i];
      if (p < 0 || p >= L) p = -1;
    }
    leaf[j] = p;
    rank[j] = 0u;
    if (p >= 0) rank[j] = lds ? atomicAdd(&s_cnt[p], 1u) : (unsigned)atomicAdd(&cursor[p], 1);
  }
  if (lds) {
    __syncthreads();
    // s_cnt[s] becomes the start of this block's run inside leaf s
    for (int s = threadIdx.x; s < L; s += LQ_BLOCK) {
      const unsigned c = s_cnt[s];
      if (c != 0u) s_cnt[s] = (unsigned)atomicAdd(&cursor[s], (int)c);
    }
    __syncthreads();
  }
  #pragma unroll
  for (int j = 0; j < LQ_ITEMS; ++j) {
    const int p = leaf[j];
    if (p < 0) continue;
    const long long i = base + (long long)j * LQ_BLOCK + threadIdx.x;
    const long long dst = off[p] + (long long)(lds ? s_cnt[p] + rank[j] : rank[j]);
    if (dst < 0 || dst >= n) continue;  // cannot happen with cnt/off of the same pos
    keys[dst] = lq_key(resid[i]);
    seg[dst] = p;
    if (weighted) wq[dst] = lq_fixed(w[i], scale);
  }
}

// One thread per leaf. target: the select looks for the first bucket at
// which the running sum (of rows, or of fixed-point weight) reaches it.
__global__ __launch_bounds__(LQ_BLOCK) void lq_init_kernel(
    const int* __restrict__ cnt, const u64* __restrict__ wtot, int L, double alpha, int weighted,
    unsigned* __restrict__ prefix, long long* __restrict__ target, double* __restrict__ frac,
    unsigned* __restrict__ next, int* __restrict__ flag) {
  const int l = blockIdx.x * LQ_BLOCK + threadIdx.x;
  if (l >= L) return;
  const long long m = cnt[l];
  prefix[l] = 0u;
  next[l] = 0xffffffffu;
  long long t = 1;
  double d = 0.0;
  int f = 0;
  if (m == 0) {
    f = LQ_EMPTY;
  } else if (weighted) {
    const u64 W = wtot[l];
    if (W == 0ull) {
      f = LQ_EMPTY;
    } else {
      // W < 2^50: exact in float64, and so is the comparison of an integer
      // running sum with the product through its ceiling
      t = (long long)ceil(alpha * (double)W);
      t = t < 1 ? 1 : (t > (long long)W ? (long long)W : t);
    }
  } else {
    const double md = (double)m;
    long long k;
    if (alpha <= 1.0 / (md + 1.0)) {
      k = 0;
    } else if (alpha >= md / (md + 1.0)) {
      k = m - 1;
    } else {
      const double x = alpha * (md + 1.0);
      k = (long long)floor(x) - 1;
      k = k < 0 ? 0 : (k > m - 1 ? m - 1 : k);
      d = (x - 1.0) - (double)k;
      if (k >= m - 1) d = 0.0;  // no v_{k+1}
    }
    t = k + 1;
    if (d != 0.0) f = LQ_NEED_NEXT;
  }
  target[l] = t;
  frac[l] = d;
  flag[l] = f;
}

// total: rows that take part = off[L - 1] + cnt[L - 1]
__device__ __forceinline__ long long lq_total(const long long* __restrict__ off,
                                              const int* __restrict__ cnt, int L) {
  return off[L - 1] + (long long)cnt[L - 1];
}

// table: u64 [L][LQ_BUCKETS], zero on entry (the select kernel clears what
// it has read). An element takes part when the key bits above this pass's
// field equal its leaf's prefix.
__global__ __launch_bounds__(LQ_BLOCK) void lq_hist_kernel(
    const unsigned* __restrict__ keys, const int* __restrict__ seg, const u64* __restrict__ wq,
    const long long* __restrict__ off, const int* __restrict__ cnt, int L, long long n,
    const unsigned* __restrict__ prefix, u64* __restrict__ table, int shift, int first) {
  __shared__ u64 s_tab[LQ_BUCKETS * LQ_REP];
  long long total = lq_total(off, cnt, L);
  if (total > n) total = n;
  const long long cs = (long long)blockIdx.x * LQ_CHUNK;
  if (cs >= total) return;  // uniform
  const long long ce = cs + LQ_CHUNK < total ? cs + LQ_CHUNK : total;
  const bool weighted = wq != nullptr;
  const int l0 = seg[cs];
  const int l1 = seg[ce - 1];
  if (l0 < 0 || l0 >= L || l1 < 0 || l1 >= L) return;  // uniform; seg is this file's own output
  if (l0 == l1) {  // uniform
    for (int s = threadIdx.x; s < LQ_BUCKETS * LQ_REP; s += LQ_BLOCK) s_tab[s] = 0ull;
    __syncthreads();
    const unsigned pre = prefix[l0];
    const int rep = threadIdx.x & (LQ_REP - 1);
    for (long long i = cs + threadIdx.x; i < ce; i += LQ_BLOCK) {
      const unsigned key = keys[i];
      if (!first && (key >> (shift + 8)) != pre) continue;
      const int slot = (int)((key >> shift) & 255u) * LQ_REP + rep;  // < LQ_BUCKETS * LQ_REP
      atomicAdd(&s_tab[slot], weighted ? wq[i] : 1ull);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < LQ_BUCKETS; b += LQ_BLOCK) {
      u64 s = 0ull;
      #pragma unroll
      for (int k = 0; k < LQ_REP; ++k) s += s_tab[b * LQ_REP + k];
      if (s != 0ull) atomicAdd(&table[(long long)l0 * LQ_BUCKETS + b], s);
    }
  } else {
    for (long long i = cs + threadIdx.x; i < ce; i += LQ_BLOCK) {
      const int l = seg[i];
      if (l < 0 || l >= L) continue;
      const unsigned key = keys[i];
      if (!first && (key >> (shift + 8)) != prefix[l]) continue;
      const u64 v = weighted ? wq[i] : 1ull;
      if (v != 0ull) atomicAdd(&table[(long long)l * LQ_BUCKETS + (int)((key >> shift) & 255u)], v);
    }
  }
}

// One wave per leaf, four buckets per lane: the first bucket at which the
// running sum reaches the leaf's target is appended to its prefix, and the
// target becomes the rank inside that bucket. The table row is cleared for
// the next pass.
__global__ __launch_bounds__(LQ_BLOCK) void lq_select_kernel(
    u64* __restrict__ table, int L, unsigned* __restrict__ prefix, long long* __restrict__ target,
    unsigned* __restrict__ next, int* __restrict__ flag, int first, int last) {
  const int lane = threadIdx.x & (LQ_WAVE - 1);
  const int l = blockIdx.x * (LQ_BLOCK / LQ_WAVE) + threadIdx.x / LQ_WAVE;
  if (l >= L) return;  // uniform over the wave; the kernel has no barrier
  const int f = flag[l];
  if (f & LQ_EMPTY) return;
  u64* row = table + (long long)l * LQ_BUCKETS + lane * 4;
  long long v[4];
  long long s = 0;
  #pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[j] = (long long)row[j];
    row[j] = 0ull;
    s += v[j];
  }
  long long incl = s;
  #pragma unroll
  for (int d = 1; d < LQ_WAVE; d <<= 1) {
    const long long o = __shfl_up(incl, d, LQ_WAVE);
    if (lane >= d) incl += o;
  }
  const long long t = target[l];
  const unsigned pre = first ? 0u : prefix[l];
  const u64 hits = __ballot(incl >= t);
  // the target never exceeds the sum of the row (init clamps it and every
  // pass keeps it inside the chosen bucket); should it, take the last lane
  const int owner = hits != 0ull ? __ffsll((long long)hits) - 1 : LQ_WAVE - 1;
  if (lane != owner) return;
  long long before = incl - s;
  int b = 3;
  #pragma unroll
  for (int j = 0; j < 3; ++j) {
    if (before + v[j] >= t) {
      b = j;
      break;
    }
    before += v[j];
  }
  long long c = v[b];
  long long r = t - before;
  r = r < 1 ? 1 : (r > c && c > 0 ? c : r);
  const unsigned key = (pre << 8) | (unsigned)(lane * 4 + b);
  prefix[l] = key;
  target[l] = r;
  if (last && (f & LQ_NEED_NEXT) && r < c) {
    // the bucket is one value and holds more rows than the rank needs
    next[l] = key;
    flag[l] = f & ~LQ_NEED_NEXT;
  }
}

// The smallest key above v_k (prefix holds the finished key) for the leaves
// that still need v_{k+1}.
__global__ __launch_bounds__(LQ_BLOCK) void lq_next_kernel(
    const unsigned* __restrict__ keys, const int* __restrict__ seg,
    const long long* __restrict__ off, const int* __restrict__ cnt, int L, long long n,
    const unsigned* __restrict__ prefix, const int* __restrict__ flag,
    unsigned* __restrict__ next) {
  long long total = lq_total(off, cnt, L);
  if (total > n) total = n;
  const long long cs = (long long)blockIdx.x * LQ_CHUNK;
  if (cs >= total) return;
  const long long ce = cs + LQ_CHUNK < total ? cs + LQ_CHUNK : total;
  const int l0 = seg[cs];
  const int l1 = seg[ce - 1];
  if (l0 < 0 || l0 >= L || l1 < 0 || l1 >= L) return;
  if (l0 == l1) {  // uniform
    if (!(flag[l0] & LQ_NEED_NEXT)) return;
    const unsigned vk = prefix[l0];
    unsigned mn = 0xffffffffu;
    for (long long i = cs + threadIdx.x; i < ce; i += LQ_BLOCK) {
      const unsigned key = keys[i];
      if (key > vk && key < mn) mn = key;
    }
    #pragma unroll
    for (int d = LQ_WAVE >> 1; d > 0; d >>= 1) {
      const unsigned o = (unsigned)__shfl_xor((int)mn, d, LQ_WAVE);
      mn = o < mn ? o : mn;
    }
    if ((threadIdx.x & (LQ_WAVE - 1)) == 0 && mn != 0xffffffffu) atomicMin(&next[l0], mn);
  } else {
    for (long long i = cs + threadIdx.x; i < ce; i += LQ_BLOCK) {
      const int l = seg[i];
      if (l < 0 || l >= L || !(flag[l] & LQ_NEED_NEXT)) continue;
      const unsigned key = keys[i];
      // next[l] only falls: a stale read costs an atomic, never a result
      if (key > prefix[l] && key < next[l]) atomicMin(&next[l], key);
    }
  }
}

__global__ __launch_bounds__(LQ_BLOCK) void lq_final_kernel(
    int L, const unsigned* __restrict__ prefix, const unsigned* __restrict__ next,
    const double* __restrict__ frac, const int* __restrict__ flag, float* __restrict__ out) {
  const int l = blockIdx.x * LQ_BLOCK + threadIdx.x;
  if (l >= L) return;
  if (flag[l] & LQ_EMPTY) {
    out[l] = __uint_as_float(0x7fc00000u);
    return;
  }
  const float a = lq_value(prefix[l]);
  const double d = frac[l];
  const unsigned nk = next[l];
  if (d == 0.0 || nk == 0xffffffffu) {
    out[l] = a;
    return;
  }
  const double lo = (double)a;
  const double hi = (double)lq_value(nk);
  const double step = d * (hi - lo);
  out[l] = (float)(lo + step);
}

static void check_launch(const char* what) {
  const hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, what, " launch failed: ", hipGetErrorString(err));
}

static int grid_for(long long items, long long per_block) {
  return (int)std::max<long long>(1, (items + per_block - 1) / per_block);
}

// The row count that the chunked launches are sized for: 2^31 rows would
// overflow the int32 counts.
static void check_rows(long long n) {
  TORCH_CHECK_VALUE(n >= 1 && n < (1ll << 31), "row count must be in [1, 2^31)");
}

// weight may be empty (unweighted); scale is the fixed-point scale.
void leaf_quantile_count(torch::Tensor pos, torch::Tensor weight, double scale, torch::Tensor cnt,
                         torch::Tensor wtot) {
  CHECK_DEV(pos, torch::kInt32);
  CHECK_DEV(weight, torch::kFloat32);
  CHECK_DEV(cnt, torch::kInt32);
  CHECK_DEV(wtot, torch::kInt64);
  const long long n = pos.numel();
  const long long L = cnt.numel();
  check_rows(n);
  TORCH_CHECK_VALUE(L >= 1 && L < (1ll << 22), "n_leaves must be in [1, 2^22)");
  const bool weighted = weight.numel() != 0;
  TORCH_CHECK_VALUE(!weighted || (weight.numel() == n && wtot.numel() == L),
                    "weight must match pos, and wtot the leaves");
  const int grid = (int)std::min<long long>(grid_for(n, 8 * LQ_BLOCK), 2048);
  hipLaunchKernelGGL(lq_count_kernel, dim3(grid), dim3(LQ_BLOCK), 0, quantile_stream(),
                     pos.data_ptr<int>(), weighted ? weight.data_ptr<float>() : nullptr, n, (int)L,
                     scale, cnt.data_ptr<int>(),
                     weighted ? (u64*)wtot.data_ptr<int64_t>() : nullptr);
  check_launch("lq_count_kernel");
}

void leaf_quantile_scatter(torch::Tensor pos, torch::Tensor resid, torch::Tensor weight,
                           double scale, torch::Tensor off, torch::Tensor cursor,
                           torch::Tensor keys, torch::Tensor seg, torch::Tensor wq) {
  CHECK_DEV(pos, torch::kInt32);
  CHECK_DEV(resid, torch::kFloat32);
  CHECK_DEV(weight, torch::kFloat32);
  CHECK_DEV(off, torch::kInt64);
  CHECK_DEV(cursor, torch::kInt32);
  CHECK_DEV(keys, torch::kInt32);
  CHECK_DEV(seg, torch::kInt32);
  CHECK_DEV(wq, torch::kInt64);
  const long long n = pos.numel();
  const long long L = off.numel();
  check_rows(n);
  TORCH_CHECK_VALUE(L >= 1 && L < (1ll << 22) && cursor.numel() == L,
                    "off and cursor must have one entry per leaf");
  TORCH_CHECK_VALUE(resid.numel() == n && keys.numel() == n && seg.numel() == n,
                    "resid, keys and seg must match pos");
  const bool weighted = weight.numel() != 0;
  TORCH_CHECK_VALUE(!weighted || (weight.numel() == n && wq.numel() == n),
                    "weight and wq must match pos");
  hipLaunchKernelGGL(lq_scatter_kernel, dim3(grid_for(n, LQ_BLOCK * LQ_ITEMS)), dim3(LQ_BLOCK), 0,
                     quantile_stream(), pos.data_ptr<int>(), resid.data_ptr<float>(),
                     weighted ? weight.data_ptr<float>() : nullptr, n, (int)L, scale,
                     (const long long*)off.data_ptr<int64_t>(), cursor.data_ptr<int>(),
                     (unsigned*)keys.data_ptr<int>(), seg.data_ptr<int>(),
                     weighted ? (u64*)wq.data_ptr<int64_t>() : nullptr);
  check_launch("lq_scatter_kernel");
}

// table: zeroed int64 [L * 256]; state32: int32 [3 * L] (prefix, next,
// flag); target: int64 [L]; frac: float64 [L]; out: float32 [L], written.
void leaf_quantile_select(torch::Tensor keys, torch::Tensor seg, torch::Tensor wq,
                          torch::Tensor off, torch::Tensor cnt, torch::Tensor wtot, double alpha,
                          torch::Tensor table, torch::Tensor state32, torch::Tensor target,
                          torch::Tensor frac, torch::Tensor out) {
  CHECK_DEV(keys, torch::kInt32);
  CHECK_DEV(seg, torch::kInt32);
  CHECK_DEV(wq, torch::kInt64);
  CHECK_DEV(off, torch::kInt64);
  CHECK_DEV(cnt, torch::kInt32);
  CHECK_DEV(wtot, torch::kInt64);
  CHECK_DEV(table, torch::kInt64);
  CHECK_DEV(state32, torch::kInt32);
  CHECK_DEV(target, torch::kInt64);
  CHECK_DEV(frac, torch::kFloat64);
  CHECK_DEV(out, torch::kFloat32);
  const long long n = keys.numel();
  const long long L = cnt.numel();
  check_rows(n);
  TORCH_CHECK_VALUE(L >= 1 && L < (1ll << 22), "n_leaves must be in [1, 2^22)");
  TORCH_CHECK_VALUE(seg.numel() == n, "seg must match keys");
  const bool weighted = wq.numel() != 0;
  TORCH_CHECK_VALUE(!weighted || (wq.numel() == n && wtot.numel() == L),
                    "wq must match keys, and wtot the leaves");
  TORCH_CHECK_VALUE(off.numel() == L && table.numel() == L * LQ_BUCKETS &&
                        state32.numel() == 3 * L && target.numel() == L && frac.numel() == L &&
                        out.numel() == L,
                    "per-leaf buffers must have one entry (table: 256) per leaf");
  TORCH_CHECK_VALUE(alpha > 0.0 && alpha < 1.0, "alpha must be in (0, 1)");
  const unsigned* keys_p = (const unsigned*)keys.data_ptr<int>();
  const int* seg_p = seg.data_ptr<int>();
  const u64* wq_p = weighted ? (const u64*)wq.data_ptr<int64_t>() : nullptr;
  const long long* off_p = (const long long*)off.data_ptr<int64_t>();
  const int* cnt_p = cnt.data_ptr<int>();
  u64* table_p = (u64*)table.data_ptr<int64_t>();
  unsigned* prefix = (unsigned*)state32.data_ptr<int>();
  unsigned* next = prefix + L;
  int* flag = state32.data_ptr<int>() + 2 * L;
  long long* target_p = (long long*)target.data_ptr<int64_t>();
  hipStream_t stream = quantile_stream();
  const int leaf_grid = grid_for(L, LQ_BLOCK);
  const int chunk_grid = grid_for(n, LQ_CHUNK);
  hipLaunchKernelGGL(lq_init_kernel, dim3(leaf_grid), dim3(LQ_BLOCK), 0, stream, cnt_p,
                     weighted ? (const u64*)wtot.data_ptr<int64_t>() : nullptr, (int)L, alpha,
                     weighted ? 1 : 0, prefix, target_p, frac.data_ptr<double>(), next, flag);
  check_launch("lq_init_kernel");
  for (int p = 0; p < LQ_PASSES; ++p) {
    const int shift = 24 - 8 * p;
    hipLaunchKernelGGL(lq_hist_kernel, dim3(chunk_grid), dim3(LQ_BLOCK), 0, stream, keys_p, seg_p,
                       wq_p, off_p, cnt_p, (int)L, n, (const unsigned*)prefix, table_p, shift,
                       p == 0 ? 1 : 0);
    check_launch("lq_hist_kernel");
    hipLaunchKernelGGL(lq_select_kernel, dim3(grid_for(L, LQ_BLOCK / LQ_WAVE)), dim3(LQ_BLOCK), 0,
                       stream, table_p, (int)L, prefix, target_p, next, flag, p == 0 ? 1 : 0,
                       p == LQ_PASSES - 1 ? 1 : 0);
    check_launch("lq_select_kernel");
  }
  if (!weighted) {
    hipLaunchKernelGGL(lq_next_kernel, dim3(chunk_grid), dim3(LQ_BLOCK), 0, stream, keys_p, seg_p,
                       off_p, cnt_p, (int)L, n, (const unsigned*)prefix, (const int*)flag, next);
    check_launch("lq_next_kernel");
  }
  hipLaunchKernelGGL(lq_final_kernel, dim3(leaf_grid), dim3(LQ_BLOCK), 0, stream, (int)L,
                     (const unsigned*)prefix, (const unsigned*)next,
                     (const double*)frac.data_ptr<double>(), (const int*)flag,
                     out.data_ptr<float>());
  check_launch("lq_final_kernel");
}

void init_quantile_kernels(pybind11::module_& m) {
  m.def("leaf_quantile_count", &leaf_quantile_count,
        "rows and fixed-point weight per leaf slot");
  m.def("leaf_quantile_scatter", &leaf_quantile_scatter,
        "scatter residual keys, leaf slots and fixed-point weights into per-leaf segments");
  m.def("leaf_quantile_select", &leaf_quantile_select,
        "segmented radix select of one (weighted) quantile per leaf");
}
