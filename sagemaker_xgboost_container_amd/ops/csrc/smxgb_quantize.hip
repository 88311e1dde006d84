// MI355X (gfx950 / CDNA4) kernels that quantize a dense float32 matrix:
// per-feature cut finding without a sort, and the bin matrix.
//
// Cut finding is a radix select with many targets per feature. A value's
// key is its orderable u32 pattern (see qz_key; -0.0 is folded into +0.0,
// NaN takes no part, +-inf order like any value), cut into three digits of
// 11, 11 and 10 bits. For every feature a sorted list of *active prefixes*
// says which buckets of the pass before are still followed; pass 1 has the
// one empty prefix. Per pass:
//
//   hist    counts[feature][slot of the prefix][digit] += 1 for every element
//           whose prefix is active (int32, exact, order-independent)
//   refine  one workgroup per feature: prefix sums of the counters in key
//           order, the bucket and the offset inside it of every target rank,
//           the number of non-empty buckets, and the next active list: all
//           non-empty buckets while there are at most max_bin of them,
//           otherwise (the feature is then "many" for good) only the buckets
//           that hold a target rank
//
// A bucket that holds a rank is not empty, so a list never has more than
// max_bin entries. After pass 3 a bucket is one float value: a feature that
// never became "many" lists all its distinct values (cuts are the float32
// midpoints of neighbours), a "many" feature lists the distinct values at
// the target ranks, which are its cuts. Nothing is read back between the
// refine of pass 1 and the final kernel.
//
// The histogram kernel reads X row-major in tiles of QZ_ROWS rows by up to
// QZ_FW features and turns the tile through LDS, so that a wave works on one
// feature at a time and a lane owns QZ_PER consecutive rows of it. The lane
// first joins equal neighbours into runs; the wave then elects up to
// QZ_ELECT leaders whose counter address is shared by other lanes and adds
// their runs up before the atomic, so that a binary or constant column sends
// two atomics per wave instead of 256. Pass 1 has one slot per feature: its
// 2048 counters per feature live in LDS and are flushed once per block.

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

// qz_key, qz_value, qz_is_nan, qz_wave_add, qz_block_scan and the block shape
#include "smxgb_quantize.h"

#define CHECK_DEV(x, dt)                                                       \
  TORCH_CHECK_VALUE(x.is_cuda() && x.is_contiguous() && x.scalar_type() == dt, \
                    #x " must be a contiguous ROCm device tensor of the expected dtype")

#define QZ_ROWS 256                     // rows of a tile
#define QZ_PER (QZ_ROWS / QZ_WAVE)      // consecutive rows of a lane
#define QZ_FW 8                         // most features of a tile
// a feature's rows in the LDS tile: one pad word every QZ_PER rows (a lane's
// reads are then 5 words apart) and 8 more between features
#define QZ_TILE_STRIDE (QZ_ROWS + QZ_ROWS / QZ_PER + 8)
#define QZ_TILE_WORDS (QZ_FW * QZ_TILE_STRIDE)
#define QZ_LDS_BYTES (64 * 1024)
#define QZ_MANY 1                       // flag: more than max_bin distinct values
#define QZ_NAN_BITS 0x7fc00000u

static hipStream_t quantize_stream() { return at::hip::getCurrentHIPStream().stream(); }

// X: [n][f] row-major. The launch covers features [f0, f0 + fcount); counts,
// active and nactive are indexed from f0. Block (x, y): the x-th group of fw
// features and the y-th run of rows_per_block rows (a multiple of QZ_ROWS).
//   PASS 1: counts[fl][2048]
//   PASS 2, 3: counts[fl][A][2048], active[fl][A] sorted, nactive[fl] <= A
// Dynamic LDS: the tile, then fw * 2048 counters (pass 1) or fw * A prefixes.
template <int PASS>
__global__ __launch_bounds__(QZ_BLOCK) void qz_hist_kernel(
    const unsigned* __restrict__ X, long long n, int f, int f0, int fcount, int fw,
    int rows_per_block, const unsigned* __restrict__ active, const int* __restrict__ nactive,
    int A, int* __restrict__ counts) {
  extern __shared__ unsigned qz_lds[];
  unsigned* s_tile = qz_lds;
  unsigned* s_aux = qz_lds + QZ_TILE_WORDS;
  __shared__ int s_nact[QZ_FW];

  const int tf0 = blockIdx.x * fw;            // first feature of the block, from f0
  const int cw = min(fw, fcount - tf0);       // its features, 1..fw
  if (cw <= 0) return;
  const int lane = threadIdx.x & (QZ_WAVE - 1);
  const int wave = threadIdx.x / QZ_WAVE;

  if (PASS == 1) {
    for (int i = threadIdx.x; i < cw * QZ_DIGITS; i += QZ_BLOCK) s_aux[i] = 0u;
  } else {
    if (threadIdx.x < QZ_FW) {
      int na = threadIdx.x < cw ? nactive[tf0 + threadIdx.x] : 0;
      s_nact[threadIdx.x] = na < 0 ? 0 : (na > A ? A : na);
    }
    __syncthreads();
    for (int c = 0; c < cw; ++c)
      for (int i = threadIdx.x; i < s_nact[c]; i += QZ_BLOCK)
        s_aux[c * A + i] = active[(long long)(tf0 + c) * A + i];
  }
  __syncthreads();

  const long long row_lo = (long long)blockIdx.y * rows_per_block;
  long long row_hi = row_lo + rows_per_block;
  if (row_hi > n) row_hi = n;
  const int tile_elems = QZ_ROWS * cw;

  for (long long r0 = row_lo; r0 < row_hi; r0 += QZ_ROWS) {
    // coalesced read of the tile's cw-word row segments, transposed store
    for (int e = threadIdx.x; e < tile_elems; e += QZ_BLOCK) {
      const int row = e / cw;
      const int col = e - row * cw;
      const long long r = r0 + row;
      unsigned b = QZ_NAN_BITS;
      if (r < row_hi) b = X[r * f + (f0 + tf0 + col)];
      s_tile[col * QZ_TILE_STRIDE + row + row / QZ_PER] = b;
    }
    __syncthreads();
    for (int c = wave; c < cw; c += QZ_WAVES) {  // uniform over the wave
      int addr[QZ_PER];
      #pragma unroll
      for (int k = 0; k < QZ_PER; ++k) {
        const int row = lane * QZ_PER + k;
        const unsigned b = s_tile[c * QZ_TILE_STRIDE + row + lane];
        int a = -1;
        if (!qz_is_nan(b)) {
          const unsigned key = qz_key(b);
          if (PASS == 1) {
            a = c * QZ_DIGITS + (int)(key >> 21);
          } else {
            const unsigned pre = PASS == 2 ? key >> 21 : key >> 10;
            const int dig = PASS == 2 ? (int)((key >> 10) & 2047u) : (int)(key & 1023u);
            const unsigned* list = s_aux + c * A;
            int lo = 0, hi = s_nact[c];
            while (lo < hi) {
              const int mid = (lo + hi) >> 1;
              if (list[mid] < pre) lo = mid + 1; else hi = mid;
            }
            if (lo < s_nact[c] && list[lo] == pre)
              a = ((tf0 + c) * A + lo) * QZ_DIGITS + dig;
          }
        }
        addr[k] = a;
      }
      // a run ends where the next row of the lane has another address
      int run = 0;
      #pragma unroll
      for (int k = 0; k < QZ_PER; ++k) {
        ++run;
        const bool ends = k == QZ_PER - 1 || addr[k + 1 < QZ_PER ? k + 1 : k] != addr[k];
        const bool pending = ends && addr[k] >= 0;
        if (PASS == 1) qz_wave_add((int*)s_aux, addr[k], run, pending);
        else qz_wave_add(counts, addr[k], run, pending);
        if (ends) run = 0;
      }
    }
    __syncthreads();
  }

  if (PASS == 1) {
    for (int i = threadIdx.x; i < cw * QZ_DIGITS; i += QZ_BLOCK) {
      const int v = (int)s_aux[i];
      if (v != 0) atomicAdd(&counts[(long long)tf0 * QZ_DIGITS + i], v);
    }
  }
}

// One workgroup per feature fl (all arrays indexed from the launch's first
// feature). pass p reads counts[fl][S][2048] (S = 1 in pass 1, else A) with
// the nact_in[fl] slots of active_in[fl][A] (pass 1: one slot, prefix 0),
// `bits` key bits per digit, and writes active_out / nact_out, the flag, and
// per target rank t < T: rank_slot (its slot in active_out) and rank_off
// (its offset inside that bucket). Pass 1 takes the ranks themselves from
// ranks[ridx[fl]][T]. The counters are left as inclusive prefix sums.
__global__ __launch_bounds__(QZ_BLOCK) void qz_refine_kernel(
    int pass, int bits, int* __restrict__ counts, int S, const unsigned* __restrict__ active_in,
    const int* __restrict__ nact_in, unsigned* __restrict__ active_out,
    int* __restrict__ nact_out, int A, int max_bin, const int* __restrict__ mcount,
    const int* __restrict__ ranks, const int* __restrict__ ridx, int n_rank_rows, int T,
    int* __restrict__ rank_slot, int* __restrict__ rank_off, unsigned* __restrict__ rank_key,
    int* __restrict__ flag) {
  __shared__ int s_w[QZ_WAVES];
  const int fl = blockIdx.x;
  const int m = mcount[fl];
  if (m <= 0) {  // uniform: a feature without a finite value
    if (threadIdx.x == 0) {
      nact_out[fl] = 0;
      flag[fl] = 0;
    }
    return;
  }
  const int ND = 1 << bits;
  const int per = ND / QZ_BLOCK;  // 8 or 4
  int nact = 1;
  if (pass > 1) {
    nact = nact_in[fl];
    nact = nact < 0 ? 0 : (nact > A ? A : nact);
    if (nact > S) nact = S;
  }
  if (nact <= 0) {  // uniform; a feature with a finite value has a bucket
    if (threadIdx.x == 0) {
      nact_out[fl] = 0;
      flag[fl] = 0;
    }
    return;
  }
  int* tab = counts + (long long)fl * S * QZ_DIGITS;
  const unsigned* act_in = active_in + (long long)fl * A;
  unsigned* act_out = active_out + (long long)fl * A;
  const int d0 = threadIdx.x * per;

  // A: inclusive prefix sums inside every slot; the non-empty buckets
  int nne_mine = 0;
  for (int s = 0; s < nact; ++s) {
    int* row = tab + (long long)s * QZ_DIGITS;
    int v[8];
    int sum = 0;
    #pragma unroll
    for (int k = 0; k < 8; ++k) {
      v[k] = 0;
      if (k < per) {
        const int c = row[d0 + k];
        nne_mine += c != 0;
        sum += c;
        v[k] = sum;
      }
    }
    int total;
    const int excl = qz_block_scan(sum, s_w, total);
    #pragma unroll
    for (int k = 0; k < 8; ++k)
      if (k < per) row[d0 + k] = excl + v[k];
  }
  int nne;
  qz_block_scan(nne_mine, s_w, nne);  // also the barrier after the stores of A
  const bool many = (pass > 1 && (flag[fl] & QZ_MANY)) || nne > max_bin;

  // B: the bucket of every target rank and the offset inside it
  const long long tb = (long long)fl * T;
  for (int t = threadIdx.x; t < T; t += QZ_BLOCK) {
    int s = 0, o;
    if (pass == 1) {
      int rr = ridx[fl];
      rr = rr < 0 ? 0 : (rr >= n_rank_rows ? n_rank_rows - 1 : rr);
      o = ranks[(long long)rr * T + t];
    } else {
      s = rank_slot[tb + t];
      o = rank_off[tb + t];
    }
    s = s < 0 ? 0 : (s >= nact ? nact - 1 : s);
    const int* row = tab + (long long)s * QZ_DIGITS;
    const int cnt = row[ND - 1];
    o = o < 0 ? 0 : (o >= cnt ? cnt - 1 : o);  // holds by construction
    int lo = 0, hi = ND - 1;                   // first d with row[d] > o
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (row[mid] > o) hi = mid; else lo = mid + 1;
    }
    const unsigned pre = pass == 1 ? 0u : act_in[s];
    rank_key[tb + t] = (pre << bits) | (unsigned)lo;
    rank_off[tb + t] = o - (lo > 0 ? row[lo - 1] : 0);
  }
  __syncthreads();

  // C: the next active list
  int nout = 0;
  if (!many) {
    // every non-empty bucket, in key order; nne <= max_bin <= A of them
    for (int s = 0; s < nact; ++s) {
      const int* row = tab + (long long)s * QZ_DIGITS;
      const unsigned pre = pass == 1 ? 0u : act_in[s];
      int prev = d0 > 0 ? row[d0 - 1] : 0;
      int c[8];
      int mine = 0;
      #pragma unroll
      for (int k = 0; k < 8; ++k) {
        c[k] = prev;
        if (k < per) {
          c[k] = row[d0 + k];
          mine += c[k] != prev;
          prev = c[k];
        }
      }
      int total;
      int pos = nout + qz_block_scan(mine, s_w, total);
      prev = d0 > 0 ? row[d0 - 1] : 0;
      #pragma unroll
      for (int k = 0; k < 8; ++k) {
        if (k < per) {
          if (c[k] != prev) {
            if (pos < A) act_out[pos] = (pre << bits) | (unsigned)(d0 + k);
            ++pos;
          }
          prev = c[k];
        }
      }
      nout += total;
    }
    if (nout > A) nout = A;
    __syncthreads();
    for (int t = threadIdx.x; t < T; t += QZ_BLOCK) {
      const unsigned key = rank_key[tb + t];
      int lo = 0, hi = nout;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (act_out[mid] < key) lo = mid + 1; else hi = mid;
      }
      rank_slot[tb + t] = lo < nout ? lo : nout - 1;
    }
  } else {
    // the rank buckets without repeats: the keys rise with the rank
    for (int t0 = 0; t0 < T; t0 += QZ_BLOCK) {
      const int t = t0 + threadIdx.x;
      unsigned key = 0u;
      int first = 0;
      if (t < T) {
        key = rank_key[tb + t];
        first = t == 0 || rank_key[tb + t - 1] != key;
      }
      int total;
      const int pos = nout + qz_block_scan(first, s_w, total);
      if (t < T) {
        if (first && pos < A) act_out[pos] = key;
        const int slot = pos + first - 1;
        rank_slot[tb + t] = slot < A ? slot : A - 1;
      }
      nout += total;
    }
    if (nout > A) nout = A;
  }
  if (threadIdx.x == 0) {
    nact_out[fl] = nout;
    flag[fl] = many ? QZ_MANY : 0;
  }
}

// One workgroup per feature: after pass 3 an active key is a value. Writes
// ncut[fl] and the cuts into cuts_pad[fl][Tpad] (Tpad >= max_bin - 1).
__global__ __launch_bounds__(QZ_BLOCK) void qz_final_kernel(
    const unsigned* __restrict__ active, const int* __restrict__ nact, int A,
    const int* __restrict__ mcount, const int* __restrict__ flag, float* __restrict__ cuts_pad,
    int Tpad, int* __restrict__ ncut) {
  const int fl = blockIdx.x;
  const unsigned* act = active + (long long)fl * A;
  float* out = cuts_pad + (long long)fl * Tpad;
  int nc = 0;
  if (mcount[fl] > 0) {
    int na = nact[fl];
    na = na < 0 ? 0 : (na > A ? A : na);
    if (flag[fl] & QZ_MANY) {
      nc = na < Tpad ? na : Tpad;
      for (int i = threadIdx.x; i < nc; i += QZ_BLOCK) out[i] = qz_value(act[i]);
    } else {
      nc = na - 1 < Tpad ? na - 1 : Tpad;
      if (nc < 0) nc = 0;
      for (int i = threadIdx.x; i < nc; i += QZ_BLOCK)
        out[i] = (qz_value(act[i]) + qz_value(act[i + 1])) * 0.5f;
    }
  }
  if (threadIdx.x == 0) ncut[fl] = nc;
}

// cuts_flat[cut_ptr[j] + i] = cuts_pad[j][i], i < ncut[j]
__global__ __launch_bounds__(QZ_BLOCK) void qz_compact_kernel(
    const float* __restrict__ cuts_pad, int Tpad, const int* __restrict__ ncut,
    const long long* __restrict__ cut_ptr, float* __restrict__ cuts_flat, long long total) {
  const int j = blockIdx.x;
  const long long base = cut_ptr[j];
  const int nc = min(ncut[j], Tpad);
  for (int i = threadIdx.x; i < nc; i += QZ_BLOCK)
    if (base + i >= 0 && base + i < total) cuts_flat[base + i] = cuts_pad[(long long)j * Tpad + i];
}

// bins[r][g0 + c] = #{cuts of feature g0 + c that are <= X[r][g0 + c]}, or
// missing_bin for NaN, for the gw features from g0 whose cuts (cut_ptr[g0] to
// cut_ptr[g0 + gw], at most the LDS the launch gives) are staged once per
// block. A block bins rows_per_block rows; reads and stores are row-major.
template <typename OutT>
__global__ __launch_bounds__(QZ_BLOCK) void qz_bin_kernel(
    const float* __restrict__ X, long long n, int f, int g0, int gw, int rows_per_block,
    const float* __restrict__ cuts, const long long* __restrict__ cut_ptr, int ncuts_group,
    long long ncuts_all, int missing_bin, OutT* __restrict__ bins) {
  extern __shared__ unsigned qz_lds[];
  int* s_ptr = (int*)qz_lds;                  // gw + 1 offsets into s_cuts
  float* s_cuts = (float*)(qz_lds + gw + 1);  // ncuts_group values
  const long long cbase = cut_ptr[g0];
  for (int c = threadIdx.x; c <= gw; c += QZ_BLOCK) {
    long long p = cut_ptr[g0 + c] - cbase;
    s_ptr[c] = (int)(p < 0 ? 0 : (p > ncuts_group ? ncuts_group : p));
  }
  for (int i = threadIdx.x; i < ncuts_group; i += QZ_BLOCK)
    s_cuts[i] = cbase >= 0 && cbase + i < ncuts_all ? cuts[cbase + i] : 0.0f;
  __syncthreads();
  const long long row_lo = (long long)blockIdx.x * rows_per_block;
  long long row_hi = row_lo + rows_per_block;
  if (row_hi > n) row_hi = n;
  if (row_lo >= row_hi) return;
  const int elems = (int)(row_hi - row_lo) * gw;  // the launch keeps this below 2^31
  for (int e = threadIdx.x; e < elems; e += QZ_BLOCK) {
    const int row = e / gw;
    const int col = e - row * gw;
    const long long at = (row_lo + row) * f + g0 + col;
    const float v = X[at];
    int b = missing_bin;
    if (v == v) {
      const float* c = s_cuts + s_ptr[col];
      int lo = 0, hi = s_ptr[col + 1] - s_ptr[col];
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (c[mid] <= v) lo = mid + 1; else hi = mid;
      }
      b = lo;
    }
    bins[at] = (OutT)b;
  }
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

static void qz_check_launch(const char* what) {
  const hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, what, " launch failed: ", hipGetErrorString(err));
}

// Features of a histogram block: as many as the LDS holds next to the tile.
static int qz_features_per_block(int pass, int A) {
  const long long room = QZ_LDS_BYTES - (long long)QZ_TILE_WORDS * 4 - 64;  // 64: static LDS
  const long long per = pass == 1 ? (long long)QZ_DIGITS * 4 : (long long)std::max(A, 1) * 4;
  return (int)std::max<long long>(0, std::min<long long>(QZ_FW, room / per));
}

// pass 1: counts int32 [fcount][2048]; active and nactive are not read.
// pass 2, 3: counts int32 [fcount][A][2048], active int32 [fcount][A],
// nactive int32 [fcount]. All indexed from feature f0 of X.
void quantize_hist(torch::Tensor X, int64_t f0, int64_t fcount, int64_t pass,
                   torch::Tensor active, torch::Tensor nactive, int64_t A, torch::Tensor counts) {
  CHECK_DEV(X, torch::kFloat32);
  CHECK_DEV(active, torch::kInt32);
  CHECK_DEV(nactive, torch::kInt32);
  CHECK_DEV(counts, torch::kInt32);
  TORCH_CHECK_VALUE(X.dim() == 2, "X must be [n][f]");
  const long long n = X.size(0);
  const long long f = X.size(1);
  TORCH_CHECK_VALUE(n >= 1 && n < (1ll << 31), "row count must be in [1, 2^31)");
  TORCH_CHECK_VALUE(f < (1ll << 31) && f0 >= 0 && fcount >= 1 && f0 + fcount <= f,
                    "feature range out of X");
  TORCH_CHECK_VALUE(pass >= 1 && pass <= 3, "pass must be 1, 2 or 3");
  TORCH_CHECK_VALUE(A >= 1, "A must be positive");
  if (pass == 1) {
    TORCH_CHECK_VALUE(counts.numel() == fcount * QZ_DIGITS, "counts must be [fcount][2048]");
  } else {
    TORCH_CHECK_VALUE(fcount * A * QZ_DIGITS < (1ll << 31) &&
                          counts.numel() == fcount * A * QZ_DIGITS,
                      "counts must be [fcount][A][2048] with fewer than 2^31 counters");
    TORCH_CHECK_VALUE(active.numel() == fcount * A && nactive.numel() == fcount,
                      "active must be [fcount][A] and nactive [fcount]");
  }
  const int fw = qz_features_per_block((int)pass, (int)A);
  TORCH_CHECK_VALUE(fw >= 1, "the active list of one feature does not fit the LDS");
  const int fwb = (int)std::min<long long>(fw, fcount);
  const long long ftiles = (fcount + fwb - 1) / fwb;
  const long long tiles = (n + QZ_ROWS - 1) / QZ_ROWS;
  // about 2048 blocks in all, each a whole number of row tiles
  long long gy = std::max<long long>(1, std::min<long long>(tiles, 2048 / std::min<long long>(ftiles, 2048)));
  const long long rows_per_block = ((tiles + gy - 1) / gy) * QZ_ROWS;
  gy = (n + rows_per_block - 1) / rows_per_block;
  TORCH_CHECK_VALUE(ftiles < (1ll << 31) && gy <= 65535, "grid out of range");
  const size_t lds = (size_t)QZ_TILE_WORDS * 4 +
                     (pass == 1 ? (size_t)fwb * QZ_DIGITS * 4 : (size_t)fwb * A * 4);
  const dim3 grid((unsigned)ftiles, (unsigned)gy);
  const unsigned* Xp = (const unsigned*)X.data_ptr<float>();
  const unsigned* act = (const unsigned*)active.data_ptr<int>();
  hipStream_t stream = quantize_stream();
  if (pass == 1)
    hipLaunchKernelGGL(qz_hist_kernel<1>, grid, dim3(QZ_BLOCK), lds, stream, Xp, n, (int)f, (int)f0,
                       (int)fcount, fwb, (int)rows_per_block, act, nactive.data_ptr<int>(), (int)A,
                       counts.data_ptr<int>());
  else if (pass == 2)
    hipLaunchKernelGGL(qz_hist_kernel<2>, grid, dim3(QZ_BLOCK), lds, stream, Xp, n, (int)f, (int)f0,
                       (int)fcount, fwb, (int)rows_per_block, act, nactive.data_ptr<int>(), (int)A,
                       counts.data_ptr<int>());
  else
    hipLaunchKernelGGL(qz_hist_kernel<3>, grid, dim3(QZ_BLOCK), lds, stream, Xp, n, (int)f, (int)f0,
                       (int)fcount, fwb, (int)rows_per_block, act, nactive.data_ptr<int>(), (int)A,
                       counts.data_ptr<int>());
  qz_check_launch("qz_hist_kernel");
}

// state: int32 [3][fcount][T] (rank_slot, rank_off, rank_key). See
// qz_refine_kernel; fcount is mcount's length.
void quantize_refine(int64_t pass, torch::Tensor counts, torch::Tensor active_in,
                     torch::Tensor nact_in, torch::Tensor active_out, torch::Tensor nact_out,
                     int64_t A, int64_t max_bin, torch::Tensor mcount, torch::Tensor ranks,
                     torch::Tensor ridx, int64_t T, torch::Tensor state, torch::Tensor flag) {
  CHECK_DEV(counts, torch::kInt32);
  CHECK_DEV(active_in, torch::kInt32);
  CHECK_DEV(nact_in, torch::kInt32);
  CHECK_DEV(active_out, torch::kInt32);
  CHECK_DEV(nact_out, torch::kInt32);
  CHECK_DEV(mcount, torch::kInt32);
  CHECK_DEV(ranks, torch::kInt32);
  CHECK_DEV(ridx, torch::kInt32);
  CHECK_DEV(state, torch::kInt32);
  CHECK_DEV(flag, torch::kInt32);
  const long long fc = mcount.numel();
  TORCH_CHECK_VALUE(pass >= 1 && pass <= 3, "pass must be 1, 2 or 3");
  TORCH_CHECK_VALUE(fc >= 1 && fc < (1ll << 31) && A >= 1 && max_bin >= 1 && max_bin <= A && T >= 0 &&
                        T < A + 1,
                    "need 1 <= max_bin <= A and T <= A");
  const long long S = pass == 1 ? 1 : A;
  TORCH_CHECK_VALUE(counts.numel() == fc * S * QZ_DIGITS, "counts must be [fcount][S][2048]");
  TORCH_CHECK_VALUE(active_in.numel() == fc * A && active_out.numel() == fc * A &&
                        nact_in.numel() == fc && nact_out.numel() == fc && flag.numel() == fc &&
                        ridx.numel() == fc && state.numel() == 3 * fc * std::max<long long>(T, 1),
                    "per-feature buffers do not match the feature count");
  const long long nrr = T > 0 ? ranks.numel() / T : 1;
  TORCH_CHECK_VALUE(T == 0 || (nrr >= 1 && ranks.numel() == nrr * T), "ranks must be [rows][T]");
  int* st = state.data_ptr<int>();
  const long long plane = fc * std::max<long long>(T, 1);
  hipLaunchKernelGGL(qz_refine_kernel, dim3((unsigned)fc), dim3(QZ_BLOCK), 0, quantize_stream(),
                     (int)pass, pass == 3 ? 10 : 11, counts.data_ptr<int>(), (int)S,
                     (const unsigned*)active_in.data_ptr<int>(), nact_in.data_ptr<int>(),
                     (unsigned*)active_out.data_ptr<int>(), nact_out.data_ptr<int>(), (int)A,
                     (int)max_bin, mcount.data_ptr<int>(), ranks.data_ptr<int>(),
                     ridx.data_ptr<int>(), (int)nrr, (int)T, st, st + plane,
                     (unsigned*)(st + 2 * plane), flag.data_ptr<int>());
  qz_check_launch("qz_refine_kernel");
}

// cuts_pad: float32 [fcount][Tpad], ncut: int32 [fcount], both written.
void quantize_final(torch::Tensor active, torch::Tensor nact, int64_t A, torch::Tensor mcount,
                    torch::Tensor flag, torch::Tensor cuts_pad, int64_t Tpad, torch::Tensor ncut) {
  CHECK_DEV(active, torch::kInt32);
  CHECK_DEV(nact, torch::kInt32);
  CHECK_DEV(mcount, torch::kInt32);
  CHECK_DEV(flag, torch::kInt32);
  CHECK_DEV(cuts_pad, torch::kFloat32);
  CHECK_DEV(ncut, torch::kInt32);
  const long long fc = mcount.numel();
  TORCH_CHECK_VALUE(fc >= 1 && fc < (1ll << 31) && A >= 1 && Tpad >= 1, "empty launch");
  TORCH_CHECK_VALUE(active.numel() == fc * A && nact.numel() == fc && flag.numel() == fc &&
                        cuts_pad.numel() == fc * Tpad && ncut.numel() == fc,
                    "per-feature buffers do not match the feature count");
  hipLaunchKernelGGL(qz_final_kernel, dim3((unsigned)fc), dim3(QZ_BLOCK), 0, quantize_stream(),
                     (const unsigned*)active.data_ptr<int>(), nact.data_ptr<int>(), (int)A,
                     mcount.data_ptr<int>(), flag.data_ptr<int>(), cuts_pad.data_ptr<float>(),
                     (int)Tpad, ncut.data_ptr<int>());
  qz_check_launch("qz_final_kernel");
}

// cut_ptr: int64 [f + 1] on the device, the running sum of ncut.
void quantize_compact(torch::Tensor cuts_pad, int64_t Tpad, torch::Tensor ncut,
                      torch::Tensor cut_ptr, torch::Tensor cuts_flat) {
  CHECK_DEV(cuts_pad, torch::kFloat32);
  CHECK_DEV(ncut, torch::kInt32);
  CHECK_DEV(cut_ptr, torch::kInt64);
  CHECK_DEV(cuts_flat, torch::kFloat32);
  const long long fc = ncut.numel();
  TORCH_CHECK_VALUE(fc >= 1 && fc < (1ll << 31) && Tpad >= 1 && cuts_pad.numel() == fc * Tpad &&
                        cut_ptr.numel() == fc + 1,
                    "buffers do not match the feature count");
  hipLaunchKernelGGL(qz_compact_kernel, dim3((unsigned)fc), dim3(QZ_BLOCK), 0, quantize_stream(),
                     cuts_pad.data_ptr<float>(), (int)Tpad, ncut.data_ptr<int>(),
                     (const long long*)cut_ptr.data_ptr<int64_t>(), cuts_flat.data_ptr<float>(),
                     (long long)cuts_flat.numel());
  qz_check_launch("qz_compact_kernel");
}

int64_t quantize_bin_lds_words() { return QZ_LDS_BYTES / 4; }

// Bins features [g0, g0 + gw) of X into bins (uint8, or int16). cut_ptr is the
// device copy (int64 [f + 1]); ncuts_group = cut_ptr[g0 + gw] - cut_ptr[g0],
// which the caller knows from its host copy, with gw + 1 + ncuts_group words
// inside quantize_bin_lds_words().
void quantize_bin(torch::Tensor X, torch::Tensor cuts, torch::Tensor cut_ptr, int64_t g0,
                  int64_t gw, int64_t ncuts_group, int64_t missing_bin, torch::Tensor bins) {
  CHECK_DEV(X, torch::kFloat32);
  CHECK_DEV(cuts, torch::kFloat32);
  CHECK_DEV(cut_ptr, torch::kInt64);
  TORCH_CHECK_VALUE(bins.is_cuda() && bins.is_contiguous(), "bins must be a contiguous device tensor");
  TORCH_CHECK_VALUE(X.dim() == 2, "X must be [n][f]");
  const long long n = X.size(0);
  const long long f = X.size(1);
  TORCH_CHECK_VALUE(n >= 1 && f >= 1 && f < (1ll << 31) && bins.numel() == n * f,
                    "bins must have X's shape");
  TORCH_CHECK_VALUE(g0 >= 0 && gw >= 1 && g0 + gw <= f && cut_ptr.numel() == f + 1,
                    "feature group out of X");
  TORCH_CHECK_VALUE(ncuts_group >= 0 && ncuts_group <= cuts.numel() &&
                        gw + 1 + ncuts_group <= quantize_bin_lds_words(),
                    "the group's cuts do not fit the LDS");
  const bool wide = bins.scalar_type() == torch::kInt16;
  TORCH_CHECK_VALUE(wide || bins.scalar_type() == torch::kUInt8, "bins must be uint8 or int16");
  TORCH_CHECK_VALUE(missing_bin >= 0 && missing_bin <= (wide ? 32767 : 255),
                    "missing_bin does not fit the bin type");
  // about 64k elements a block, so that staging the cuts is a small part
  const long long rows_per_block = std::max<long long>(1, 65536 / gw);  // times gw: < 2^31
  const long long grid = (n + rows_per_block - 1) / rows_per_block;
  TORCH_CHECK_VALUE(grid < (1ll << 31), "grid out of range");
  const size_t lds = (size_t)(gw + 1 + ncuts_group) * 4;
  hipStream_t stream = quantize_stream();
  if (wide)
    hipLaunchKernelGGL(qz_bin_kernel<short>, dim3((unsigned)grid), dim3(QZ_BLOCK), lds, stream,
                       X.data_ptr<float>(), n, (int)f, (int)g0, (int)gw, (int)rows_per_block,
                       cuts.data_ptr<float>(), (const long long*)cut_ptr.data_ptr<int64_t>(),
                       (int)ncuts_group, (long long)cuts.numel(), (int)missing_bin, (short*)bins.data_ptr<int16_t>());
  else
    hipLaunchKernelGGL(qz_bin_kernel<unsigned char>, dim3((unsigned)grid), dim3(QZ_BLOCK), lds,
                       stream, X.data_ptr<float>(), n, (int)f, (int)g0, (int)gw,
                       (int)rows_per_block, cuts.data_ptr<float>(),
                       (const long long*)cut_ptr.data_ptr<int64_t>(), (int)ncuts_group,
                       (long long)cuts.numel(), (int)missing_bin, bins.data_ptr<unsigned char>());
  qz_check_launch("qz_bin_kernel");
}

void init_quantize_kernels(pybind11::module_& m) {
  m.def("quantize_hist", &quantize_hist, "one radix pass of the per-feature digit counters");
  m.def("quantize_refine", &quantize_refine,
        "rank buckets, non-empty buckets and the next active prefixes of every feature");
  m.def("quantize_final", &quantize_final, "cuts of every feature from its final active list");
  m.def("quantize_compact", &quantize_compact, "padded per-feature cuts to the flat array");
  m.def("quantize_bin_lds_words", &quantize_bin_lds_words, "LDS words of a binning launch");
  m.def("quantize_bin", &quantize_bin, "bin a feature group of a dense float32 matrix");
}
