// MI355X (gfx950 / CDNA4) kernels for gradient-based row sampling
// (sampling_method=gradient_based: Minimal Variance Sampling).
//
// For one tree's (n, 2) gradient pairs, r_i = sqrt(g_i^2 + h_i^2) and
// S = subsample * n. The threshold mu solves
//     F(mu) = sum_i min(1, r_i / mu) = S,
// row i is kept when u_i < p_i = min(1, r_i / mu), and a kept pair is
// multiplied by 1 / p_i.
//
// mu is found without a sort. r >= 0, so float32 bit patterns order like
// unsigned integers: a radix select over the pattern (8 exponent bits, then
// 8 + 8 + 7 significand bits) narrows the bucket that holds mu in four
// streaming passes over gh; r is recomputed from gh in every pass. A pass
// builds a row count and a sum per bucket in LDS and adds them to a small
// global table. The rows of one bucket share their exponent (the first pass
// buckets ON the exponent), so a bucket's sum is the exact u64 sum of 24-bit
// significands: it does not depend on the order of the adds, and neither
// does mu. A single-workgroup select kernel then sums the 256 buckets in
// float64 and in a fixed order and finds, from the top, the one where
//     count(r >= t) + sum(r < t) / t
// crosses S (t = the bucket's lower edge), and leaves the next pass's prefix
// in device memory. Nothing is read back by the host.
//
// Rows with r == 0 take no part: they are never kept.

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <algorithm>

typedef unsigned long long u64;

#define CHECK_DEV(x, dt)                                                       \
  TORCH_CHECK_VALUE(x.is_cuda() && x.is_contiguous() && x.scalar_type() == dt, \
                    #x " must be a contiguous ROCm device tensor of the expected dtype")

static hipStream_t sampling_stream() { return at::hip::getCurrentHIPStream().stream(); }

#define MVS_BLOCK 256
#define MVS_WAVE 64
#define MVS_BUCKETS 256  // per pass (the last pass uses 128 of them)
#define MVS_PASSES 4
// LDS replicas of the bucket table: the gradients of one objective crowd
// into a few exponents, and lanes adding to one LDS address serialize.
// Lane l adds to replica l % 8, which cuts that 64-way conflict to 8-way.
#define MVS_REP 8
// state words behind the bucket tables (int64 each)
#define MVS_STATE_PREFIX 0  // pattern bits fixed so far (the chosen buckets)
#define MVS_STATE_DONE 1    // mu is final: later passes return at once
#define MVS_STATE_ABOVE 2   // rows in buckets above the chosen ones
#define MVS_STATE_BELOW 3   // float64 bits: sum of r over the buckets below
#define MVS_STATE_WORDS 4

// One definition of r for every pass and for the apply kernel: the select
// is only right when all of them see the same bits.
__device__ __forceinline__ float mvs_norm(const float2 p) {
  return __fsqrt_rn(__fmaf_rn(p.x, p.x, __fmul_rn(p.y, p.y)));
}

// table: this pass's [MVS_BUCKETS][2] u64 (count, significand sum). Rows
// take part when the pattern bits above this pass's field equal the prefix.
__global__ __launch_bounds__(MVS_BLOCK) void mvs_hist_kernel(
    const float2* __restrict__ gh, long long n, const long long* __restrict__ state,
    u64* __restrict__ table, int shift, int nbits) {
  __shared__ unsigned s_cnt[MVS_BUCKETS * MVS_REP];
  __shared__ u64 s_sum[MVS_BUCKETS * MVS_REP];
  if (state[MVS_STATE_DONE] != 0) return;  // uniform over the grid
  const unsigned prefix = (unsigned)state[MVS_STATE_PREFIX];
  for (int s = threadIdx.x; s < MVS_BUCKETS * MVS_REP; s += MVS_BLOCK) {
    s_cnt[s] = 0u;
    s_sum[s] = 0ull;
  }
  __syncthreads();
  const unsigned mask = (1u << nbits) - 1u;
  const int hi = shift + nbits;
  const int rep = threadIdx.x & (MVS_REP - 1);
  const long long step = (long long)gridDim.x * MVS_BLOCK;
  for (long long i = (long long)blockIdx.x * MVS_BLOCK + threadIdx.x; i < n; i += step) {
    const unsigned bits = __float_as_uint(mvs_norm(gh[i]));
    if (bits == 0u || (bits >> hi) != prefix) continue;
    const unsigned mant = bits & 0x7fffffu;
    const unsigned sig = (bits >> 23) != 0u ? (mant | 0x800000u) : mant;
    const int slot = (int)((bits >> shift) & mask) * MVS_REP + rep;  // < MVS_BUCKETS * MVS_REP
    atomicAdd(&s_cnt[slot], 1u);
    atomicAdd(&s_sum[slot], (u64)sig);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < MVS_BUCKETS; b += MVS_BLOCK) {
    u64 c = 0ull, s = 0ull;
    #pragma unroll
    for (int k = 0; k < MVS_REP; ++k) {
      c += s_cnt[b * MVS_REP + k];
      s += s_sum[b * MVS_REP + k];
    }
    if (c != 0ull) {
      atomicAdd(&table[2 * b], c);
      atomicAdd(&table[2 * b + 1], s);
    }
  }
}

// float64 value of a significand sum whose rows carry biased exponent e
__device__ __forceinline__ double mvs_sum_value(u64 sig_sum, unsigned e) {
  return ldexp((double)sig_sum, (int)(e != 0u ? e : 1u) - 150);
}

// One workgroup, one thread per bucket. The loads, the float64 bucket values
// and the crossing test run in parallel; the running sums in between are
// thread 0's alone, in a fixed order, so that mu does not depend on a
// schedule.
__global__ __launch_bounds__(MVS_BUCKETS) void mvs_select_kernel(
    const u64* __restrict__ table, long long* __restrict__ state, float* __restrict__ mu,
    double S, int shift, int nbits, int first, int last) {
  __shared__ u64 s_cnt[MVS_BUCKETS];
  __shared__ double s_val[MVS_BUCKETS];    // sum of r over the bucket
  __shared__ double s_below[MVS_BUCKETS];  // sum of r over everything below the bucket
  __shared__ u64 s_ge[MVS_BUCKETS];        // rows at or above the bucket's lower edge
  __shared__ int s_chosen;
  __shared__ int s_stop;
  if (state[MVS_STATE_DONE] != 0) return;  // uniform; written only behind the first barrier
  const unsigned prefix = (unsigned)state[MVS_STATE_PREFIX];
  const u64 count_above = (u64)state[MVS_STATE_ABOVE];
  const double sum_below = __longlong_as_double(state[MVS_STATE_BELOW]);
  const int nb = 1 << nbits;
  const int b = threadIdx.x;
  const bool live = b < nb;
  const unsigned edge = ((prefix << nbits) | (unsigned)b) << shift;  // the bucket's lower edge
  s_cnt[b] = live ? table[2 * b] : 0ull;
  s_val[b] = live ? mvs_sum_value(table[2 * b + 1], edge >> 23) : 0.0;
  if (b == 0) {
    s_chosen = 0;
    s_stop = 0;
  }
  __syncthreads();

  if (b == 0) {
    u64 ge = count_above;
    for (int k = nb - 1; k >= 0; --k) {
      ge += s_cnt[k];
      s_ge[k] = ge;
    }
    if (first && (double)ge <= S) {
      // mu = 0: no more rows with r > 0 than S, every one of them is kept
      mu[0] = 0.0f;
      state[MVS_STATE_DONE] = 1;
      s_stop = 1;
    } else {
      double run = sum_below;
      for (int k = 0; k < nb; ++k) {
        s_below[k] = run;
        run += s_val[k];
      }
    }
  }
  __syncthreads();
  if (s_stop) return;

  // The highest bucket whose lower edge t has F(t) >= S holds mu (F falls
  // as t grows). Bucket 0 needs no test: its edge is the edge of the bucket
  // this pass refines, where F >= S is already known (t = 0 in the first
  // pass).
  if (live && b > 0) {
    const double t = (double)__uint_as_float(edge);
    if ((double)s_ge[b] + s_below[b] / t >= S) atomicMax(&s_chosen, b);
  }
  __syncthreads();
  if (b != 0) return;

  const int chosen = s_chosen;
  const unsigned chosen_bits = (prefix << nbits) | (unsigned)chosen;
  const u64 above = s_ge[chosen] - s_cnt[chosen];
  double below = s_below[chosen];
  if (s_cnt[chosen] == 0ull || last) {
    // nothing left to resolve: no row lies between mu and the bucket's edge
    // (an empty bucket, e.g. mu above max r when all rows are equal), or
    // the bucket is one float32 value, whose rows have p = r / mu <= 1
    below += s_val[chosen];
    const double den = S - (double)above;
    mu[0] = den > 0.0 ? (float)(below / den) : INFINITY;
    state[MVS_STATE_DONE] = 1;
    return;
  }
  state[MVS_STATE_PREFIX] = (long long)chosen_bits;
  state[MVS_STATE_ABOVE] = (long long)above;
  state[MVS_STATE_BELOW] = __double_as_longlong(below);
}

// Keep / rescale in one pass. pmax: [gridDim.x] per-block (|g|, |h|) maxima
// of the rescaled pairs; every block writes its entry.
__global__ __launch_bounds__(MVS_BLOCK) void mvs_apply_kernel(
    const float2* __restrict__ gh, const float* __restrict__ u, const float* __restrict__ mu_p,
    long long n, float2* __restrict__ out, unsigned char* __restrict__ keep,
    float2* __restrict__ pmax) {
  __shared__ float s_g[MVS_BLOCK / MVS_WAVE];
  __shared__ float s_h[MVS_BLOCK / MVS_WAVE];
  const float mu = mu_p[0];
  float mg = 0.0f, mh = 0.0f;
  const long long step = (long long)gridDim.x * MVS_BLOCK;
  for (long long i = (long long)blockIdx.x * MVS_BLOCK + threadIdx.x; i < n; i += step) {
    const float2 p = gh[i];
    const float r = mvs_norm(p);
    const float prob = mu > 0.0f ? fminf(1.0f, __fdiv_rn(r, mu)) : (r > 0.0f ? 1.0f : 0.0f);
    const bool kept = u[i] < prob;
    float2 o = make_float2(0.0f, 0.0f);
    if (kept) {
      const float inv = __fdiv_rn(1.0f, prob);  // 1 for a certain row: bits unchanged
      o.x = __fmul_rn(p.x, inv);
      o.y = __fmul_rn(p.y, inv);
    }
    out[i] = o;
    keep[i] = kept ? 1 : 0;
    mg = fmaxf(mg, fabsf(o.x));
    mh = fmaxf(mh, fabsf(o.y));
  }
  #pragma unroll
  for (int d = MVS_WAVE >> 1; d > 0; d >>= 1) {
    mg = fmaxf(mg, __shfl_xor(mg, d, MVS_WAVE));
    mh = fmaxf(mh, __shfl_xor(mh, d, MVS_WAVE));
  }
  const int lane = threadIdx.x & (MVS_WAVE - 1);
  const int wave = threadIdx.x / MVS_WAVE;
  if (lane == 0) {
    s_g[wave] = mg;
    s_h[wave] = mh;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    #pragma unroll
    for (int w = 1; w < MVS_BLOCK / MVS_WAVE; ++w) {
      mg = fmaxf(mg, s_g[w]);
      mh = fmaxf(mh, s_h[w]);
    }
    pmax[blockIdx.x] = make_float2(mg, mh);
  }
}

static void check_launch(const char* what) {
  const hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, what, " launch failed: ", hipGetErrorString(err));
}

// work: zeroed int64 [MVS_PASSES * MVS_BUCKETS * 2 + MVS_STATE_WORDS] (the
// bucket tables, then the select state); mu: float32 [1], written.
void mvs_threshold(torch::Tensor gh, double S, torch::Tensor work, torch::Tensor mu) {
  CHECK_DEV(gh, torch::kFloat32);
  CHECK_DEV(work, torch::kInt64);
  CHECK_DEV(mu, torch::kFloat32);
  TORCH_CHECK_VALUE(gh.dim() == 2 && gh.size(1) == 2, "gh must be (n, 2)");
  TORCH_CHECK_VALUE(work.numel() == MVS_PASSES * MVS_BUCKETS * 2 + MVS_STATE_WORDS,
                    "work must hold the bucket tables and the select state");
  TORCH_CHECK_VALUE(mu.numel() == 1, "mu must hold one value");
  const long long n = gh.size(0);
  TORCH_CHECK_VALUE(n >= 1, "gh is empty");
  TORCH_CHECK_VALUE(S > 0.0, "the sample size S must be positive");
  const float2* gh_p = (const float2*)gh.data_ptr<float>();
  u64* tables = (u64*)work.data_ptr<int64_t>();
  long long* state = (long long*)(tables + MVS_PASSES * MVS_BUCKETS * 2);
  const int grid = (int)std::min<long long>((n + 4 * MVS_BLOCK - 1) / (4 * MVS_BLOCK), 1024);
  const int shifts[MVS_PASSES] = {23, 15, 7, 0};
  const int widths[MVS_PASSES] = {8, 8, 8, 7};
  hipStream_t stream = sampling_stream();
  for (int p = 0; p < MVS_PASSES; ++p) {
    u64* table = tables + p * MVS_BUCKETS * 2;
    hipLaunchKernelGGL(mvs_hist_kernel, dim3(grid), dim3(MVS_BLOCK), 0, stream, gh_p, n,
                       (const long long*)state, table, shifts[p], widths[p]);
    check_launch("mvs_hist_kernel");
    hipLaunchKernelGGL(mvs_select_kernel, dim3(1), dim3(MVS_BUCKETS), 0, stream, (const u64*)table,
                       state, mu.data_ptr<float>(), S, shifts[p], widths[p], p == 0 ? 1 : 0,
                       p == MVS_PASSES - 1 ? 1 : 0);
    check_launch("mvs_select_kernel");
  }
}

void mvs_apply(torch::Tensor gh, torch::Tensor u, torch::Tensor mu, torch::Tensor out,
               torch::Tensor keep, torch::Tensor pmax) {
  CHECK_DEV(gh, torch::kFloat32);
  CHECK_DEV(u, torch::kFloat32);
  CHECK_DEV(mu, torch::kFloat32);
  CHECK_DEV(out, torch::kFloat32);
  CHECK_DEV(keep, torch::kUInt8);
  CHECK_DEV(pmax, torch::kFloat32);
  TORCH_CHECK_VALUE(gh.dim() == 2 && gh.size(1) == 2, "gh must be (n, 2)");
  const long long n = gh.size(0);
  TORCH_CHECK_VALUE(n >= 1, "gh is empty");
  TORCH_CHECK_VALUE(u.numel() == n && keep.numel() == n && out.numel() == 2 * n,
                    "u, keep and out must match gh's rows");
  TORCH_CHECK_VALUE(mu.numel() == 1, "mu must hold one value");
  TORCH_CHECK_VALUE(pmax.dim() == 2 && pmax.size(1) == 2 && pmax.size(0) >= 1 &&
                        pmax.size(0) <= 65535,
                    "pmax must be (blocks, 2) with 1..65535 blocks");
  hipLaunchKernelGGL(mvs_apply_kernel, dim3((int)pmax.size(0)), dim3(MVS_BLOCK), 0,
                     sampling_stream(), (const float2*)gh.data_ptr<float>(), u.data_ptr<float>(),
                     mu.data_ptr<float>(), n, (float2*)out.data_ptr<float>(),
                     keep.data_ptr<uint8_t>(), (float2*)pmax.data_ptr<float>());
  check_launch("mvs_apply_kernel");
}

void init_sampling_kernels(pybind11::module_& m) {
  m.def("mvs_threshold", &mvs_threshold,
        "gradient-based sampling threshold mu by radix select over float32 bit patterns");
  m.def("mvs_apply", &mvs_apply,
        "keep flags, rescaled gradient pairs and their per-block absmax for a threshold mu");
}
