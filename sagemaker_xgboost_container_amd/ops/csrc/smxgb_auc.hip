// MI355X (gfx950 / CDNA4) kernels for the binary ROC AUC eval metric. The
// rule and its float64 reference are ops/torch_ref.binary_auc:
//   AUC = sum_i p_i * (N_<(s_i) + N_<=(s_i)) / (2 * P * N)
// with p_i = w_i * y_i, n_i = w_i * (1 - y_i), N_<(s) / N_<=(s) the sums of
// n_j over the rows with s_j < s / s_j <= s, P = sum p_i, N = sum n_i.
//
// Everything up to the last division is integer arithmetic. Weights are
// int64 fixed point, w -> round(w * 2^s) (1 without weights), with 2^s chosen
// so that P and N stay below 2^50; the numerator, up to about 2^101, is kept
// in a (hi, lo) pair of 64-bit words. Integer sums are exact in any order, so
// the value depends neither on the row order nor on how equal scores are
// ordered by the sort, and its bits do not change from call to call.
//
// Plan, once per data set (labels and weights do not change between rounds):
//   auc_plan_stats_kernel  checks labels and weights, finds the largest weight
//   auc_plan_pack_kernel   derives s from it on the device, writes one int64
//                          per row, fixed-point weight << 1 | label, and adds
//                          up P and N (integer atomics)
// The host reads the six words of plan state once, after both.
//
// Per call:
//   auc_keys_kernel        key = signed-orderable(margin) << 32 | row. The
//                          high word is qz_key's pattern with the top bit
//                          flipped, so that a signed int64 sort (torch.sort,
//                          the only step that is not in this file) orders the
//                          keys as float32 values, -0.0 equal to +0.0.
//   auc_gather_kernel      one workgroup per chunk of AUC_CHUNK sorted
//                          positions: packed weights by row id, written back
//                          in sorted order (the one random read of the call),
//                          and the chunk's negative weight.
//   auc_chunk_scan_kernel  one workgroup: exclusive scan of the chunk totals.
//   auc_prefix_kernel      per chunk, scan of the negative weights in LDS;
//                          prefix[q] = negative weight at sorted positions
//                          below q, for q in [0, n].
//   auc_sum_kernel         per chunk, key high words in LDS; a head flag where
//                          a word differs from its left neighbour, then a
//                          forward max scan and a backward min scan over the
//                          flags give every position the first position of
//                          its tie run and the first one after it. A run that
//                          leaves the chunk is found by one binary search of
//                          the sorted keys per side and workgroup. N_< is
//                          prefix[run start], N_<= is prefix[run end]; the
//                          128-bit terms p * (N_< + N_<=) meet in a wave
//                          shuffle tree, then in LDS.
//   auc_finish_kernel      one workgroup adds the chunks' (hi, lo) partials,
//                          converts numerator and 2 * P * N to float64 with
//                          one rounding each, and divides. A NaN margin makes
//                          the value NaN.
// No kernel waits for another workgroup; the prefix array carries the one
// grid-wide dependency from one launch to the next.

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <algorithm>

typedef unsigned long long u64;
typedef long long i64;

// Built without packed float32 instructions, as ops/csrc/smxgb_rank.hip is
// (and says why).
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#include "smxgb_quantize.h"

#define AUC_BLOCK 256
#define AUC_WAVE 64
#define AUC_WAVES (AUC_BLOCK / AUC_WAVE)
#define AUC_PER 8                        // consecutive positions per thread
#define AUC_CHUNK (AUC_BLOCK * AUC_PER)  // sorted positions per workgroup
#define AUC_GRID 2048                    // grid-stride kernels
#define AUC_WEIGHT_BITS 50               // P, N <= 2^50
#define AUC_NONE AUC_CHUNK               // no run head: head positions are below the chunk size

// plan state words
enum { AUC_ST_FLAGS = 0, AUC_ST_WMAX = 1, AUC_ST_P = 2, AUC_ST_N = 3, AUC_ST_S = 4, AUC_ST_NPOS = 5,
       AUC_ST_WORDS = 6 };
enum { AUC_BAD_LABEL = 1, AUC_BAD_WEIGHT = 2, AUC_HAS_POS = 4, AUC_HAS_NEG = 8 };

#define CHECK_DEV(x, dt)                                                       \
  TORCH_CHECK_VALUE(x.is_cuda() && x.is_contiguous() && x.scalar_type() == dt, \
                    #x " must be a contiguous ROCm device tensor of the expected dtype")

struct auc_u128 {
  u64 lo, hi;
};

__device__ __forceinline__ void auc_add(auc_u128& a, u64 lo, u64 hi) {
  a.lo += lo;
  a.hi += hi + (a.lo < lo ? 1ull : 0ull);
}

// Correctly rounded float64 of a 128-bit unsigned integer: the leading 64
// bits, with a sticky bit for what is shifted out, far below the 53 kept.
__device__ __forceinline__ double auc_to_double(auc_u128 a) {
  if (a.hi == 0ull) return (double)a.lo;
  const int lz = __clzll((i64)a.hi);
  u64 top = a.hi, rest = a.lo;
  if (lz > 0) {
    top = (a.hi << lz) | (a.lo >> (64 - lz));
    rest = a.lo << lz;
  }
  if (rest != 0ull) top |= 1ull;
  return ldexp((double)top, 64 - lz);
}

// Sum over the workgroup; thread 0 holds it. s_red: LDS [AUC_WAVES].
__device__ __forceinline__ i64 auc_block_sum(i64 v, i64* s_red) {
  #pragma unroll
  for (int d = AUC_WAVE >> 1; d > 0; d >>= 1) v += __shfl_down(v, d, AUC_WAVE);
  if ((threadIdx.x & (AUC_WAVE - 1)) == 0) s_red[threadIdx.x / AUC_WAVE] = v;
  __syncthreads();
  i64 r = 0;
  #pragma unroll
  for (int i = 0; i < AUC_WAVES; ++i) r += s_red[i];
  __syncthreads();
  return r;
}

// Exclusive prefix sum of v over the workgroup's threads; total: the sum.
__device__ __forceinline__ i64 auc_block_scan(i64 v, i64* s_red, i64& total) {
  const int lane = threadIdx.x & (AUC_WAVE - 1);
  const int wave = threadIdx.x / AUC_WAVE;
  i64 incl = v;
  #pragma unroll
  for (int d = 1; d < AUC_WAVE; d <<= 1) {
    const i64 o = __shfl_up(incl, d, AUC_WAVE);
    if (lane >= d) incl += o;
  }
  if (lane == AUC_WAVE - 1) s_red[wave] = incl;
  __syncthreads();
  i64 base = 0, tot = 0;
  #pragma unroll
  for (int w = 0; w < AUC_WAVES; ++w) {
    const i64 x = s_red[w];
    if (w < wave) base += x;
    tot += x;
  }
  __syncthreads();
  total = tot;
  return base + incl - v;
}

// max of v over the threads before this one (-1 for thread 0 or none).
__device__ __forceinline__ int auc_block_max_before(int v, int* s_red) {
  const int lane = threadIdx.x & (AUC_WAVE - 1);
  const int wave = threadIdx.x / AUC_WAVE;
  int incl = v;
  #pragma unroll
  for (int d = 1; d < AUC_WAVE; d <<= 1) {
    const int o = __shfl_up(incl, d, AUC_WAVE);
    if (lane >= d) incl = max(incl, o);
  }
  if (lane == AUC_WAVE - 1) s_red[wave] = incl;
  int r = __shfl_up(incl, 1, AUC_WAVE);
  if (lane == 0) r = -1;
  __syncthreads();
  #pragma unroll
  for (int w = 0; w < AUC_WAVES; ++w)
    if (w < wave) r = max(r, s_red[w]);
  __syncthreads();
  return r;
}

// min of v over the threads after this one (`none` for the last or none).
__device__ __forceinline__ int auc_block_min_after(int v, int none, int* s_red) {
  const int lane = threadIdx.x & (AUC_WAVE - 1);
  const int wave = threadIdx.x / AUC_WAVE;
  int incl = v;
  #pragma unroll
  for (int d = 1; d < AUC_WAVE; d <<= 1) {
    const int o = __shfl_down(incl, d, AUC_WAVE);
    if (lane + d < AUC_WAVE) incl = min(incl, o);
  }
  if (lane == 0) s_red[wave] = incl;
  int r = __shfl_down(incl, 1, AUC_WAVE);
  if (lane == AUC_WAVE - 1) r = none;
  __syncthreads();
  #pragma unroll
  for (int w = 0; w < AUC_WAVES; ++w)
    if (w > wave) r = min(r, s_red[w]);
  __syncthreads();
  return r;
}

__device__ __forceinline__ i64 auc_neg(i64 packed) { return (packed & 1) ? 0 : (packed >> 1); }
__device__ __forceinline__ i64 auc_pos(i64 packed) { return (packed & 1) ? (packed >> 1) : 0; }
__device__ __forceinline__ int auc_hi(i64 key) { return (int)(key >> 32); }

// ---------------------------------------------------------------------------
// Plan
// ---------------------------------------------------------------------------
// state: int64 [AUC_ST_WORDS], zero on entry. w: null without weights.
__global__ __launch_bounds__(AUC_BLOCK) void auc_plan_stats_kernel(
    const float* __restrict__ y, const float* __restrict__ w, i64 n, u64* __restrict__ state) {
  unsigned flags = 0u, wmax = 0u;
  const i64 step = (i64)gridDim.x * AUC_BLOCK;
  for (i64 i = (i64)blockIdx.x * AUC_BLOCK + threadIdx.x; i < n; i += step) {
    const float yi = y[i];
    const float wi = w ? w[i] : 1.0f;
    const bool w_ok = wi >= 0.0f && wi < INFINITY;  // false for a NaN
    if (!(yi == 0.0f || yi == 1.0f)) flags |= AUC_BAD_LABEL;
    if (!w_ok) flags |= AUC_BAD_WEIGHT;
    else {
      wmax = max(wmax, __float_as_uint(wi + 0.0f));  // non-negative: bit order is value order
      if (wi > 0.0f) flags |= yi == 1.0f ? AUC_HAS_POS : (yi == 0.0f ? AUC_HAS_NEG : 0u);
    }
  }
  #pragma unroll
  for (int d = AUC_WAVE >> 1; d > 0; d >>= 1) {
    flags |= __shfl_xor(flags, d, AUC_WAVE);
    wmax = max(wmax, __shfl_xor(wmax, d, AUC_WAVE));
  }
  if ((threadIdx.x & (AUC_WAVE - 1)) == 0) {
    if (flags) atomicOr(&state[AUC_ST_FLAGS], (u64)flags);
    if (wmax) atomicMax(&state[AUC_ST_WMAX], (u64)wmax);
  }
}

// e_n: ceil(log2(n)). packed[i] = round(w_i * 2^s) << 1 | y_i with
// s = AUC_WEIGHT_BITS - e_n - e_w, max w < 2^e_w (ops/hip.leaf_quantile_weight_scale);
// an invalid weight packs as 0, the plan is refused on its flag.
__global__ __launch_bounds__(AUC_BLOCK) void auc_plan_pack_kernel(
    const float* __restrict__ y, const float* __restrict__ w, i64 n, int e_n,
    u64* __restrict__ state, i64* __restrict__ packed) {
  __shared__ i64 s_red[AUC_WAVES];
  int s = 0;
  if (w) {
    int e_w = 0;
    const float wmax = __uint_as_float((unsigned)state[AUC_ST_WMAX]);
    if (wmax > 0.0f) frexpf(wmax, &e_w);
    s = AUC_WEIGHT_BITS - e_n - e_w;
  }
  const double scale = ldexp(1.0, s);
  i64 P = 0, N = 0, n_pos = 0;
  const i64 step = (i64)gridDim.x * AUC_BLOCK;
  for (i64 i = (i64)blockIdx.x * AUC_BLOCK + threadIdx.x; i < n; i += step) {
    const bool pos = y[i] == 1.0f;
    i64 q = 1;
    if (w) {
      const float wi = w[i];
      q = (wi >= 0.0f && wi < INFINITY) ? llrint((double)wi * scale) : 0;
    }
    packed[i] = (q << 1) | (pos ? 1 : 0);
    if (pos) { P += q; ++n_pos; } else N += q;
  }
  P = auc_block_sum(P, s_red);
  N = auc_block_sum(N, s_red);
  n_pos = auc_block_sum(n_pos, s_red);
  if (threadIdx.x == 0) {
    if (n_pos) atomicAdd(&state[AUC_ST_NPOS], (u64)n_pos);
    if (P) atomicAdd(&state[AUC_ST_P], (u64)P);
    if (N) atomicAdd(&state[AUC_ST_N], (u64)N);
    if (blockIdx.x == 0) state[AUC_ST_S] = (u64)(i64)s;
  }
}

// ---------------------------------------------------------------------------
// Per call
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(AUC_BLOCK) void auc_keys_kernel(
    const float* __restrict__ margin, i64 n, i64* __restrict__ keys) {
  const i64 step = (i64)gridDim.x * AUC_BLOCK;
  for (i64 i = (i64)blockIdx.x * AUC_BLOCK + threadIdx.x; i < n; i += step) {
    const unsigned k = qz_key(__float_as_uint(margin[i])) ^ 0x80000000u;
    keys[i] = (i64)(((u64)k << 32) | (u64)i);
  }
}

// gathered[q] = packed[row at sorted position q]; chunk_neg[c] = the
// negative weight of chunk c.
__global__ __launch_bounds__(AUC_BLOCK) void auc_gather_kernel(
    const i64* __restrict__ skeys, const i64* __restrict__ packed, i64 n,
    i64* __restrict__ gathered, i64* __restrict__ chunk_neg) {
  __shared__ i64 s_red[AUC_WAVES];
  const i64 base = (i64)blockIdx.x * AUC_CHUNK;
  i64 neg = 0;
  #pragma unroll
  for (int j = 0; j < AUC_PER; ++j) {
    const i64 q = base + j * AUC_BLOCK + threadIdx.x;
    if (q < n) {
      i64 row = skeys[q] & 0xffffffffll;
      if (row >= n) row = n - 1;  // cannot happen: the keys hold each row < n once
      const i64 v = packed[row];
      gathered[q] = v;
      neg += auc_neg(v);
    }
  }
  neg = auc_block_sum(neg, s_red);
  if (threadIdx.x == 0) chunk_neg[blockIdx.x] = neg;
}

// chunk_base[c] = sum of chunk_neg before c, for c in [0, chunks].
__global__ __launch_bounds__(AUC_BLOCK) void auc_chunk_scan_kernel(
    const i64* __restrict__ chunk_neg, i64 chunks, i64* __restrict__ chunk_base) {
  __shared__ i64 s_red[AUC_WAVES];
  i64 carry = 0;
  for (i64 c0 = 0; c0 < chunks; c0 += AUC_BLOCK) {  // uniform
    const i64 c = c0 + threadIdx.x;
    const i64 v = c < chunks ? chunk_neg[c] : 0;
    i64 total;
    const i64 excl = auc_block_scan(v, s_red, total);
    if (c < chunks) chunk_base[c] = carry + excl;
    carry += total;
  }
  if (threadIdx.x == 0) chunk_base[chunks] = carry;
}

// prefix[q] = negative weight at the sorted positions below q, q in [0, n].
__global__ __launch_bounds__(AUC_BLOCK) void auc_prefix_kernel(
    const i64* __restrict__ gathered, const i64* __restrict__ chunk_base, i64 n, i64 chunks,
    i64* __restrict__ prefix) {
  __shared__ i64 s_val[AUC_CHUNK];
  __shared__ i64 s_red[AUC_WAVES];
  const int t = threadIdx.x;
  const i64 base = (i64)blockIdx.x * AUC_CHUNK;
  #pragma unroll
  for (int j = 0; j < AUC_PER; ++j) {
    const i64 q = base + j * AUC_BLOCK + t;
    s_val[j * AUC_BLOCK + t] = q < n ? auc_neg(gathered[q]) : 0;
  }
  __syncthreads();
  i64 v[AUC_PER], sum = 0;
  #pragma unroll
  for (int j = 0; j < AUC_PER; ++j) {
    v[j] = s_val[t * AUC_PER + j];
    sum += v[j];
  }
  i64 total;
  i64 run = chunk_base[blockIdx.x] + auc_block_scan(sum, s_red, total);
  #pragma unroll
  for (int j = 0; j < AUC_PER; ++j) {
    s_val[t * AUC_PER + j] = run;
    run += v[j];
  }
  __syncthreads();
  #pragma unroll
  for (int j = 0; j < AUC_PER; ++j) {
    const i64 q = base + j * AUC_BLOCK + t;
    if (q < n) prefix[q] = s_val[j * AUC_BLOCK + t];
  }
  if (blockIdx.x == chunks - 1 && t == 0) prefix[n] = chunk_base[chunks];
}

// part[3c], part[3c + 1]: lo and hi word of the chunk's sum of
// p * (N_< + N_<=); part[3c + 2]: 1 where the chunk holds a NaN margin.
__global__ __launch_bounds__(AUC_BLOCK) void auc_sum_kernel(
    const i64* __restrict__ skeys, const i64* __restrict__ gathered,
    const i64* __restrict__ prefix, i64 n, u64* __restrict__ part) {
  __shared__ int s_hi[AUC_CHUNK + 2];  // [0]: the position before the chunk
  __shared__ i64 s_p[AUC_CHUNK];
  __shared__ int s_red[AUC_WAVES];
  __shared__ u64 s_acc[2 * AUC_WAVES];
  __shared__ i64 s_ext[2];  // run start of the first, run end of the last position

  const int t = threadIdx.x;
  const int lane = t & (AUC_WAVE - 1);
  const i64 base = (i64)blockIdx.x * AUC_CHUNK;
  const int cnt = (int)min((i64)AUC_CHUNK, n - base);  // >= 1 by the grid size

  #pragma unroll
  for (int j = 0; j < AUC_PER; ++j) {
    const int l = j * AUC_BLOCK + t;
    if (l < cnt) {
      s_hi[l + 1] = auc_hi(skeys[base + l]);
      s_p[l] = auc_pos(gathered[base + l]);
    }
  }
  if (t == 0 && base > 0) s_hi[0] = auc_hi(skeys[base - 1]);
  if (t == 1 && base + cnt < n) s_hi[cnt + 1] = auc_hi(skeys[base + cnt]);
  __syncthreads();

  // a run that begins before the chunk, or ends after it: one search each
  const bool open_left = base > 0 && s_hi[0] == s_hi[1];
  const bool open_right = base + cnt < n && s_hi[cnt + 1] == s_hi[cnt];
  if (t == 0) {
    i64 lo = 0, hi = base;  // the first position whose word is not below s_hi[1]
    if (open_left) {
      const int want = s_hi[1];
      while (lo < hi) {
        const i64 mid = lo + ((hi - lo) >> 1);
        if (auc_hi(skeys[mid]) < want) lo = mid + 1; else hi = mid;
      }
    }
    s_ext[0] = hi;
  }
  if (t == AUC_WAVE) {
    i64 lo = base + cnt, hi = n;  // the first position whose word is above s_hi[cnt]
    if (open_right) {
      const int want = s_hi[cnt];
      while (lo < hi) {
        const i64 mid = lo + ((hi - lo) >> 1);
        if (auc_hi(skeys[mid]) <= want) lo = mid + 1; else hi = mid;
      }
    }
    s_ext[1] = lo;
  }

  // heads bit j: this thread's position l = t * AUC_PER + j starts a run
  // (its word differs from the one on its left)
  unsigned heads = 0u;
  int last_head = -1, first_head = AUC_NONE;  // among this thread's positions
  int nan = 0;
  #pragma unroll
  for (int j = 0; j < AUC_PER; ++j) {
    const int l = t * AUC_PER + j;
    if (l < cnt) {
      const int word = s_hi[l + 1];
      if (l == 0 ? !open_left : s_hi[l] != word) {
        heads |= 1u << j;
        last_head = l;
        if (first_head == AUC_NONE) first_head = l;
      }
      // back to qz_key's pattern, then to the float's bits
      const unsigned key = (unsigned)word ^ 0x80000000u;
      if (qz_is_nan((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key)) nan = 1;
    }
  }
  // the last head at or before a position, the first one after it; the
  // barriers inside also publish s_ext
  int start = auc_block_max_before(last_head, s_red);        // -1: before the chunk
  int after = auc_block_min_after(first_head, AUC_NONE, s_red);  // AUC_NONE: after the chunk
  const i64 ext_start = s_ext[0], ext_end = s_ext[1];
  int end_l[AUC_PER];
  #pragma unroll
  for (int j = AUC_PER - 1; j >= 0; --j) {
    end_l[j] = after;
    if (heads & (1u << j)) after = t * AUC_PER + j;
  }

  auc_u128 acc = {0ull, 0ull};
  #pragma unroll
  for (int j = 0; j < AUC_PER; ++j) {
    const int l = t * AUC_PER + j;
    if (heads & (1u << j)) start = l;
    const u64 p = l < cnt ? (u64)s_p[l] : 0ull;
    if (p != 0ull) {
      const i64 q0 = start < 0 ? ext_start : base + start;
      const i64 q1 = end_l[j] == AUC_NONE ? ext_end : base + end_l[j];
      const u64 m = (u64)(prefix[q0] + prefix[q1]);  // <= 2^51
      auc_add(acc, p * m, __umul64hi(p, m));
    }
  }

  #pragma unroll
  for (int d = AUC_WAVE >> 1; d > 0; d >>= 1) {
    const u64 lo = __shfl_down(acc.lo, d, AUC_WAVE);
    const u64 hi = __shfl_down(acc.hi, d, AUC_WAVE);
    auc_add(acc, lo, hi);
  }
  nan = __syncthreads_or(nan);
  if (lane == 0) {
    s_acc[2 * (t / AUC_WAVE)] = acc.lo;
    s_acc[2 * (t / AUC_WAVE) + 1] = acc.hi;
  }
  __syncthreads();
  if (t == 0) {
    auc_u128 r = {0ull, 0ull};
    #pragma unroll
    for (int w = 0; w < AUC_WAVES; ++w) auc_add(r, s_acc[2 * w], s_acc[2 * w + 1]);
    part[3 * (i64)blockIdx.x] = r.lo;
    part[3 * (i64)blockIdx.x + 1] = r.hi;
    part[3 * (i64)blockIdx.x + 2] = nan ? 1ull : 0ull;
  }
}

// out[0] = sum of the chunks' partials / (2 * P * N); NaN with a NaN margin.
__global__ __launch_bounds__(AUC_BLOCK) void auc_finish_kernel(
    const u64* __restrict__ part, i64 chunks, u64 P, u64 N, double* __restrict__ out) {
  __shared__ u64 s_acc[2 * AUC_WAVES];
  const int t = threadIdx.x;
  auc_u128 acc = {0ull, 0ull};
  int nan = 0;
  for (i64 c = t; c < chunks; c += AUC_BLOCK) {
    auc_add(acc, part[3 * c], part[3 * c + 1]);
    nan |= part[3 * c + 2] != 0ull;
  }
  #pragma unroll
  for (int d = AUC_WAVE >> 1; d > 0; d >>= 1) {
    const u64 lo = __shfl_down(acc.lo, d, AUC_WAVE);
    const u64 hi = __shfl_down(acc.hi, d, AUC_WAVE);
    auc_add(acc, lo, hi);
  }
  nan = __syncthreads_or(nan);
  if ((t & (AUC_WAVE - 1)) == 0) {
    s_acc[2 * (t / AUC_WAVE)] = acc.lo;
    s_acc[2 * (t / AUC_WAVE) + 1] = acc.hi;
  }
  __syncthreads();
  if (t == 0) {
    auc_u128 num = {0ull, 0ull};
    #pragma unroll
    for (int w = 0; w < AUC_WAVES; ++w) auc_add(num, s_acc[2 * w], s_acc[2 * w + 1]);
    const u64 p2 = 2ull * P;  // <= 2^51
    const auc_u128 den = {p2 * N, __umul64hi(p2, N)};
    const bool ok = !nan && P != 0ull && N != 0ull;
    out[0] = ok ? auc_to_double(num) / auc_to_double(den) : __longlong_as_double(0x7ff8000000000000ll);
  }
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
static hipStream_t auc_stream() { return at::hip::getCurrentHIPStream().stream(); }

static void auc_check_launch(const char* what) {
  const hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, what, " launch failed: ", hipGetErrorString(err));
}

static unsigned auc_stride_grid(int64_t n) {
  return (unsigned)std::min<int64_t>((n + AUC_BLOCK - 1) / AUC_BLOCK, AUC_GRID);
}

int64_t auc_chunk() { return AUC_CHUNK; }

// y: [n] labels; w: [n] weights or empty; state: [6] int64 of zeros; packed:
// [n]. On return (in stream order) state holds the flags, the bits of the
// largest weight, P, N, s and the rows of label 1.
void auc_plan(torch::Tensor y, torch::Tensor w, torch::Tensor state, torch::Tensor packed) {
  CHECK_DEV(y, torch::kFloat32);
  CHECK_DEV(w, torch::kFloat32);
  CHECK_DEV(state, torch::kInt64);
  CHECK_DEV(packed, torch::kInt64);
  const int64_t n = y.numel();
  TORCH_CHECK_VALUE(n >= 1 && n < (1ll << 31), "row count must be in [1, 2^31)");
  TORCH_CHECK_VALUE(w.numel() == 0 || w.numel() == n, "weight must be empty or match y");
  TORCH_CHECK_VALUE(state.numel() == AUC_ST_WORDS && packed.numel() == n,
                    "state must hold 6 words and packed one per row");
  int e_n = 0;
  while ((1ll << e_n) < n) ++e_n;
  const float* wp = w.numel() ? w.data_ptr<float>() : nullptr;
  u64* st = (u64*)state.data_ptr<int64_t>();
  hipLaunchKernelGGL(auc_plan_stats_kernel, dim3(auc_stride_grid(n)), dim3(AUC_BLOCK), 0,
                     auc_stream(), y.data_ptr<float>(), wp, (i64)n, st);
  auc_check_launch("auc_plan_stats_kernel");
  hipLaunchKernelGGL(auc_plan_pack_kernel, dim3(auc_stride_grid(n)), dim3(AUC_BLOCK), 0,
                     auc_stream(), y.data_ptr<float>(), wp, (i64)n, e_n, st,
                     (i64*)packed.data_ptr<int64_t>());
  auc_check_launch("auc_plan_pack_kernel");
}

void auc_keys(torch::Tensor margin, torch::Tensor keys) {
  CHECK_DEV(margin, torch::kFloat32);
  CHECK_DEV(keys, torch::kInt64);
  const int64_t n = margin.numel();
  TORCH_CHECK_VALUE(n >= 1 && n < (1ll << 31) && keys.numel() == n,
                    "keys must match margin, with fewer than 2^31 rows");
  hipLaunchKernelGGL(auc_keys_kernel, dim3(auc_stride_grid(n)), dim3(AUC_BLOCK), 0, auc_stream(),
                     margin.data_ptr<float>(), (i64)n, (i64*)keys.data_ptr<int64_t>());
  auc_check_launch("auc_keys_kernel");
}

// skeys: the sorted keys; packed: the plan's rows. gathered [n], prefix
// [n + 1], chunk_neg [chunks], chunk_base [chunks + 1], part [3 * chunks]:
// scratch, overwritten. out: [1] float64.
void auc_scan(torch::Tensor skeys, torch::Tensor packed, int64_t P, int64_t N,
              torch::Tensor gathered, torch::Tensor prefix, torch::Tensor chunk_neg,
              torch::Tensor chunk_base, torch::Tensor part, torch::Tensor out) {
  CHECK_DEV(skeys, torch::kInt64);
  CHECK_DEV(packed, torch::kInt64);
  CHECK_DEV(gathered, torch::kInt64);
  CHECK_DEV(prefix, torch::kInt64);
  CHECK_DEV(chunk_neg, torch::kInt64);
  CHECK_DEV(chunk_base, torch::kInt64);
  CHECK_DEV(part, torch::kInt64);
  CHECK_DEV(out, torch::kFloat64);
  const int64_t n = skeys.numel();
  TORCH_CHECK_VALUE(n >= 1 && n < (1ll << 31), "row count must be in [1, 2^31)");
  const int64_t chunks = (n + AUC_CHUNK - 1) / AUC_CHUNK;
  TORCH_CHECK_VALUE(packed.numel() == n && gathered.numel() >= n && prefix.numel() >= n + 1,
                    "packed, gathered and prefix must cover the rows");
  TORCH_CHECK_VALUE(chunk_neg.numel() >= chunks && chunk_base.numel() >= chunks + 1 &&
                        part.numel() >= 3 * chunks && out.numel() >= 1,
                    "the chunk tables are too small");
  TORCH_CHECK_VALUE(P >= 0 && N >= 0 && P <= (1ll << AUC_WEIGHT_BITS) && N <= (1ll << AUC_WEIGHT_BITS),
                    "P and N must be in [0, 2^50]");
  const i64* sk = (const i64*)skeys.data_ptr<int64_t>();
  i64* ga = (i64*)gathered.data_ptr<int64_t>();
  i64* pre = (i64*)prefix.data_ptr<int64_t>();
  i64* cn = (i64*)chunk_neg.data_ptr<int64_t>();
  i64* cb = (i64*)chunk_base.data_ptr<int64_t>();
  u64* pa = (u64*)part.data_ptr<int64_t>();
  hipStream_t stream = auc_stream();
  const dim3 grid((unsigned)chunks), block(AUC_BLOCK);
  hipLaunchKernelGGL(auc_gather_kernel, grid, block, 0, stream, sk,
                     (const i64*)packed.data_ptr<int64_t>(), (i64)n, ga, cn);
  auc_check_launch("auc_gather_kernel");
  hipLaunchKernelGGL(auc_chunk_scan_kernel, dim3(1), block, 0, stream, cn, (i64)chunks, cb);
  auc_check_launch("auc_chunk_scan_kernel");
  hipLaunchKernelGGL(auc_prefix_kernel, grid, block, 0, stream, ga, cb, (i64)n, (i64)chunks, pre);
  auc_check_launch("auc_prefix_kernel");
  hipLaunchKernelGGL(auc_sum_kernel, grid, block, 0, stream, sk, ga, pre, (i64)n, pa);
  auc_check_launch("auc_sum_kernel");
  hipLaunchKernelGGL(auc_finish_kernel, dim3(1), block, 0, stream, pa, (i64)chunks, (u64)P, (u64)N,
                     out.data_ptr<double>());
  auc_check_launch("auc_finish_kernel");
}

void init_auc_kernels(pybind11::module_& m) {
  m.def("auc_chunk", &auc_chunk, "sorted positions per workgroup of the auc scan");
  m.def("auc_plan", &auc_plan, "validate labels and weights, pack fixed-point weight | label");
  m.def("auc_keys", &auc_keys, "sortable int64 keys, orderable margin << 32 | row");
  m.def("auc_scan", &auc_scan, "exact tie-aware binary auc from the sorted keys");
}
