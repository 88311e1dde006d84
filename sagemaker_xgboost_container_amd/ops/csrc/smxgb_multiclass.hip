// MI355X (gfx950 / CDNA4) kernels for the multiclass objective
// (multi:softprob / multi:softmax) and its two eval metrics. The rule is
// models/objectives.Softmax.gradients:
//   p = exp(m - max_row) / sum exp(m - max_row)          (float32)
//   g = (p - [c == y]) * w,  h = max(2 p (1 - p), 1e-16) * w
// and models/eval_metrics.mlogloss / merror.
//
// margin is (n, k) row-major, the gradients leave class-major, (k, n, 2), so
// that the slice of one class, which is what a tree grows on, is contiguous.
// A lane per row would read margins k floats apart and write gradients n
// pairs apart, so a workgroup moves a tile of R rows through LDS instead:
//   stage     R * k consecutive margins, read in address order, go to LDS
//             rows of k | 1 floats (an odd stride: lanes that walk down a
//             column, one row each, fall on different banks); labels and
//             weights of the R rows beside them
//   reduce    W lanes per row (1 up to k = 16, 8 up to k = 64, a wave
//             above): row maximum, e = expf(m - max) written back over the
//             margin, row sum, both through an xor butterfly, which gives
//             every lane of the row the same bits
//   store     a wave takes one class and 64 consecutive rows at a time: lane
//             l divides e by the row sum once, forms (g, h) and writes it as
//             one 8-byte store next to its neighbours'. |g| and |h| are kept
//             as the bit patterns of non-negative floats, whose unsigned
//             order is the value order with NaN on top: a shuffle tree per
//             wave, then an integer max per class in LDS. A maximum does
//             not depend on the order it is taken in, so the partials are
//             the same from run to run, and a NaN gradient makes its class's
//             maximum NaN as abs().amax() would.
// A workgroup walks tiles blockIdx.x, blockIdx.x + grid, ... and writes its
// (k, 2) maxima once at the end; the host takes one amax over the grid.
//
// softmax_metric_kernel stages the same tile and never forms p: per row the
// maximum with the lowest class index that holds it, and for mlogloss
//   -log(max(p_y, 1e-16)) = min(log sum exp(m - max) + (max - m_y), -log 1e-16)
// in float64. The weighted terms and the weights are added per thread in row
// order, per wave by shuffles, per workgroup through LDS, and the per-block
// (numerator, denominator) pairs by softmax_metric_finish_kernel in index
// order: no atomics, the same bits from call to call.

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <algorithm>

typedef long long i64;

// Built without packed float32 instructions, as ops/csrc/smxgb_rank.hip is
// (and says why).
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#define SMX_BLOCK 256
#define SMX_WAVE 64
#define SMX_WAVES (SMX_BLOCK / SMX_WAVE)
#define SMX_MIN_ROWS SMX_WAVE    // tile rows: a multiple of the wave, so that
#define SMX_MAX_ROWS 512         // a store segment never straddles two classes
#define SMX_GRID 2048            // workgroups at most; each walks its tiles
#define SMX_MAX_LDS (64 * 1024)  // dynamic LDS a launch may ask for
#define SMX_RED_BYTES 64         // static LDS of the metric kernels' reduction
#define SMX_LOG_CLAMP 36.841361487904734  // -log(1e-16)

enum { SMX_MLOGLOSS = 0, SMX_MERROR = 1 };

#define CHECK_DEV(x, dt)                                                       \
  TORCH_CHECK_VALUE(x.is_cuda() && x.is_contiguous() && x.scalar_type() == dt, \
                    #x " must be a contiguous ROCm device tensor of the expected dtype")

__host__ __device__ __forceinline__ int smx_stride(int k) { return k | 1; }

// dynamic LDS of both kernels: the tile, then per row the sum, the weight
// and the label, then 2 * k words of class maxima
struct SmxLds {
  float* tile;
  float* sum;
  float* w;
  int* y;
  unsigned* amax;
};

__device__ __forceinline__ SmxLds smx_carve(float* base, int k, int R) {
  SmxLds s;
  s.tile = base;
  s.sum = s.tile + R * smx_stride(k);
  s.w = s.sum + R;
  s.y = (int*)(s.w + R);
  s.amax = (unsigned*)(s.y + R);
  return s;
}

// rows row0 .. row0 + rows - 1 of margin into the tile, with their labels
// and weights (1 without weights). rows * k <= SMX_MAX_ROWS * cap: an int.
__device__ __forceinline__ void smx_stage_tile(
    const float* __restrict__ margin, const float* __restrict__ y, const float* __restrict__ w,
    i64 row0, int rows, int k, const SmxLds& s) {
  const float* src = margin + row0 * k;
  const int ks = smx_stride(k), cnt = rows * k;
  int r = threadIdx.x / k, c = threadIdx.x % k;
  const int dr = SMX_BLOCK / k, dc = SMX_BLOCK % k;
  for (int e = threadIdx.x; e < cnt; e += SMX_BLOCK) {
    s.tile[r * ks + c] = src[e];
    r += dr;
    c += dc;
    if (c >= k) {
      c -= k;
      ++r;
    }
  }
  for (int i = threadIdx.x; i < rows; i += SMX_BLOCK) {
    s.y[i] = (int)y[row0 + i];
    s.w[i] = w ? w[row0 + i] : 1.0f;
  }
}

// tile[r][c] <- expf(m - max_r), sum[r] <- their sum, W lanes per row. The
// trip count is the same for every thread: all lanes reach the shuffles.
template <int W>
__device__ __forceinline__ void smx_row_exp(const SmxLds& s, int rows, int k) {
  const int ks = smx_stride(k);
  const int j = threadIdx.x % W, g = threadIdx.x / W;
  for (int r0 = 0; r0 < rows; r0 += SMX_BLOCK / W) {
    const int r = r0 + g;
    const bool live = r < rows;
    float* row = s.tile + (live ? r : 0) * ks;
    float mx = -INFINITY;
    if (live)
      for (int c = j; c < k; c += W) mx = fmaxf(mx, row[c]);
    #pragma unroll
    for (int d = W >> 1; d > 0; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d, W));
    float sum = 0.0f;
    if (live)
      for (int c = j; c < k; c += W) {
        const float e = expf(row[c] - mx);
        row[c] = e;
        sum += e;
      }
    #pragma unroll
    for (int d = W >> 1; d > 0; d >>= 1) sum += __shfl_xor(sum, d, W);
    if (live && j == 0) s.sum[r] = sum;
  }
}

// gh: (k, n) pairs. pmax: (grid, k, 2) bit patterns of |g|, |h| maxima.
// R: tile rows, a multiple of SMX_WAVE.
template <int W>
__global__ __launch_bounds__(SMX_BLOCK) void softmax_grad_kernel(
    const float* __restrict__ margin, const float* __restrict__ y, const float* __restrict__ w,
    float2* __restrict__ gh, unsigned* __restrict__ pmax, i64 n, int k, int R) {
  extern __shared__ float smx_lds[];
  const SmxLds s = smx_carve(smx_lds, k, R);
  const int t = threadIdx.x, lane = t & (SMX_WAVE - 1), wave = t / SMX_WAVE;
  const int ks = smx_stride(k), nseg = R / SMX_WAVE;
  for (int i = t; i < 2 * k; i += SMX_BLOCK) s.amax[i] = 0u;
  __syncthreads();

  const i64 tiles = (n + R - 1) / R;
  for (i64 tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
    const i64 row0 = tl * R;
    const int rows = (int)min((i64)R, n - row0);
    smx_stage_tile(margin, y, w, row0, rows, k, s);
    __syncthreads();
    smx_row_exp<W>(s, rows, k);
    __syncthreads();

    // item = (class, segment of 64 rows); uniform within a wave
    for (int item = wave; item < k * nseg; item += SMX_WAVES) {
      const int c = item / nseg, seg0 = (item - c * nseg) * SMX_WAVE;
      if (seg0 >= rows) continue;
      const int r = seg0 + lane;
      unsigned gm = 0u, hm = 0u;
      if (r < rows) {
        const float p = s.tile[r * ks + c] / s.sum[r];
        const float wi = s.w[r];
        const float h0 = 2.0f * p * (1.0f - p);
        const float g = (p - (c == s.y[r] ? 1.0f : 0.0f)) * wi;
        const float h = (h0 < 1e-16f ? 1e-16f : h0) * wi;  // keeps a NaN, as torch.clamp does
        gh[(i64)c * n + row0 + r] = make_float2(g, h);
        gm = __float_as_uint(fabsf(g));
        hm = __float_as_uint(fabsf(h));
      }
      #pragma unroll
      for (int d = SMX_WAVE >> 1; d > 0; d >>= 1) {
        gm = max(gm, __shfl_xor(gm, d, SMX_WAVE));
        hm = max(hm, __shfl_xor(hm, d, SMX_WAVE));
      }
      if (lane == 0) {
        atomicMax(&s.amax[2 * c], gm);
        atomicMax(&s.amax[2 * c + 1], hm);
      }
    }
    __syncthreads();  // the tile is free again; the maxima are in LDS
  }
  for (int i = t; i < 2 * k; i += SMX_BLOCK) pmax[(i64)blockIdx.x * 2 * k + i] = s.amax[i];
}

// Sums of a and b over the workgroup; thread 0 holds them. s_red: LDS
// [2 * SMX_WAVES].
__device__ __forceinline__ void smx_block_sum2(double& a, double& b, double* s_red) {
  #pragma unroll
  for (int d = SMX_WAVE >> 1; d > 0; d >>= 1) {
    a += __shfl_down(a, d, SMX_WAVE);
    b += __shfl_down(b, d, SMX_WAVE);
  }
  const int wave = threadIdx.x / SMX_WAVE;
  if ((threadIdx.x & (SMX_WAVE - 1)) == 0) {
    s_red[2 * wave] = a;
    s_red[2 * wave + 1] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    a = b = 0.0;
    #pragma unroll
    for (int i = 0; i < SMX_WAVES; ++i) {
      a += s_red[2 * i];
      b += s_red[2 * i + 1];
    }
  }
}

// part: (grid, 2) float64, the workgroup's sum of w * term and of w. A label
// outside [0, k) makes the term, and with it the metric, NaN.
template <int W>
__global__ __launch_bounds__(SMX_BLOCK) void softmax_metric_kernel(
    const float* __restrict__ margin, const float* __restrict__ y, const float* __restrict__ w,
    double* __restrict__ part, i64 n, int k, int R, int kind) {
  extern __shared__ float smx_lds[];
  __shared__ double s_red[2 * SMX_WAVES];
  static_assert(sizeof(double) * 2 * SMX_WAVES <= SMX_RED_BYTES, "static LDS above what the host counts");
  const SmxLds s = smx_carve(smx_lds, k, R);
  const int ks = smx_stride(k);
  const int j = threadIdx.x % W, g = threadIdx.x / W;
  double num = 0.0, den = 0.0;

  const i64 tiles = (n + R - 1) / R;
  for (i64 tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
    const i64 row0 = tl * R;
    const int rows = (int)min((i64)R, n - row0);
    smx_stage_tile(margin, y, w, row0, rows, k, s);
    __syncthreads();
    for (int r0 = 0; r0 < rows; r0 += SMX_BLOCK / W) {  // uniform: see smx_row_exp
      const int r = r0 + g;
      const bool live = r < rows;
      const float* row = s.tile + (live ? r : 0) * ks;
      // the row maximum and the lowest class that holds it
      float mx = -INFINITY;
      int am = k;
      if (live)
        for (int c = j; c < k; c += W) {
          const float v = row[c];
          if (v > mx || am == k) {
            mx = v;
            am = c;
          }
        }
      #pragma unroll
      for (int d = W >> 1; d > 0; d >>= 1) {
        const float om = __shfl_xor(mx, d, W);
        const int oa = __shfl_xor(am, d, W);
        if (oa < k && (am == k || om > mx || (om == mx && oa < am))) {
          mx = om;
          am = oa;
        }
      }
      const int yi = live ? s.y[r] : 0;
      const bool y_ok = (unsigned)yi < (unsigned)k;
      double term;
      if (kind == SMX_MERROR) {
        term = am != yi ? 1.0 : 0.0;
      } else {
        double sum = 0.0;
        if (live)
          for (int c = j; c < k; c += W) sum += exp((double)row[c] - (double)mx);
        #pragma unroll
        for (int d = W >> 1; d > 0; d >>= 1) sum += __shfl_xor(sum, d, W);
        term = log(sum) + ((double)mx - (double)row[y_ok ? yi : 0]);
        if (term > SMX_LOG_CLAMP) term = SMX_LOG_CLAMP;
      }
      if (!y_ok) term = __longlong_as_double(0x7ff8000000000000ll);
      if (live && j == 0) {
        const double wi = (double)s.w[r];
        num += wi * term;
        den += wi;
      }
    }
    __syncthreads();
  }
  smx_block_sum2(num, den, s_red);
  if (threadIdx.x == 0) {
    part[2 * (i64)blockIdx.x] = num;
    part[2 * (i64)blockIdx.x + 1] = den;
  }
}

// out[0], out[1] = the sums of the blocks' numerators and denominators.
__global__ __launch_bounds__(SMX_BLOCK) void softmax_metric_finish_kernel(
    const double* __restrict__ part, int blocks, double* __restrict__ out) {
  __shared__ double s_red[2 * SMX_WAVES];
  double num = 0.0, den = 0.0;
  for (int b = threadIdx.x; b < blocks; b += SMX_BLOCK) {
    num += part[2 * b];
    den += part[2 * b + 1];
  }
  smx_block_sum2(num, den, s_red);
  if (threadIdx.x == 0) {
    out[0] = num;
    out[1] = den;
  }
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
static hipStream_t smx_stream() { return at::hip::getCurrentHIPStream().stream(); }

static void smx_check_launch(const char* what) {
  const hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, what, " launch failed: ", hipGetErrorString(err));
}

static int64_t smx_lds_bytes(int64_t k, int64_t rows) {
  return rows * (4 * (int64_t)smx_stride((int)k) + 12) + 8 * k;
}

// Tile rows for k classes within `budget` bytes of LDS per workgroup: the
// largest multiple of SMX_MIN_ROWS up to SMX_MAX_ROWS that fits; 0 where
// not even SMX_MIN_ROWS do (k is above the cap).
int64_t softmax_tile_rows(int64_t k, int64_t budget) {
  if (k < 2 || k > (1 << 20)) return 0;
  budget = std::min<int64_t>(budget, SMX_MAX_LDS) - SMX_RED_BYTES;
  for (int64_t rows = SMX_MAX_ROWS; rows >= SMX_MIN_ROWS; rows -= SMX_MIN_ROWS)
    if (smx_lds_bytes(k, rows) <= budget) return rows;
  return 0;
}

int64_t softmax_max_grid() { return SMX_GRID; }

struct SmxShape {
  int64_t n, k, tiles;
  const float* w;
};

static SmxShape smx_check_inputs(const torch::Tensor& margin, const torch::Tensor& y,
                                 const torch::Tensor& w, int64_t rows, int64_t grid) {
  CHECK_DEV(margin, torch::kFloat32);
  CHECK_DEV(y, torch::kFloat32);
  CHECK_DEV(w, torch::kFloat32);
  TORCH_CHECK_VALUE(margin.dim() == 2, "margin must be (rows, classes)");
  SmxShape s;
  s.n = margin.size(0);
  s.k = margin.size(1);
  TORCH_CHECK_VALUE(s.n >= 1 && s.n < (1ll << 31), "row count must be in [1, 2^31)");
  TORCH_CHECK_VALUE(y.numel() == s.n && (w.numel() == 0 || w.numel() == s.n),
                    "y must hold one label per row, weight none or one per row");
  TORCH_CHECK_VALUE(s.k >= 2 && rows >= SMX_MIN_ROWS && rows <= SMX_MAX_ROWS &&
                        rows % SMX_MIN_ROWS == 0 &&
                        smx_lds_bytes(s.k, rows) <= SMX_MAX_LDS - SMX_RED_BYTES,
                    "tile rows must come from softmax_tile_rows for this class count");
  s.tiles = (s.n + rows - 1) / rows;
  TORCH_CHECK_VALUE(grid >= 1 && grid <= s.tiles && grid <= SMX_GRID,
                    "one block of partials per workgroup, at most one workgroup per tile");
  s.w = w.numel() ? w.data_ptr<float>() : nullptr;
  return s;
}

#define SMX_LAUNCH(kernel, k, ...)                                             \
  do {                                                                         \
    if ((k) <= 16) hipLaunchKernelGGL(kernel<1>, __VA_ARGS__);                 \
    else if ((k) <= 64) hipLaunchKernelGGL(kernel<8>, __VA_ARGS__);            \
    else hipLaunchKernelGGL(kernel<SMX_WAVE>, __VA_ARGS__);                    \
    smx_check_launch(#kernel);                                                 \
  } while (0)

// margin: (n, k); y: [n] class ids; w: [n] or empty. gh: (k, n, 2), written.
// pmax: (grid, k, 2) float32, written: per workgroup the largest |g|, |h| of
// each class. rows: softmax_tile_rows(k, budget).
void softmax_grad(torch::Tensor margin, torch::Tensor y, torch::Tensor w, torch::Tensor gh,
                  torch::Tensor pmax, int64_t rows) {
  CHECK_DEV(gh, torch::kFloat32);
  CHECK_DEV(pmax, torch::kFloat32);
  TORCH_CHECK_VALUE(pmax.dim() == 3, "pmax must be (grid, classes, 2)");
  const SmxShape s = smx_check_inputs(margin, y, w, rows, pmax.size(0));
  TORCH_CHECK_VALUE(gh.numel() == 2 * s.n * s.k && pmax.numel() == pmax.size(0) * 2 * s.k,
                    "gh must be (classes, rows, 2) and pmax (grid, classes, 2)");
  SMX_LAUNCH(softmax_grad_kernel, s.k, dim3((unsigned)pmax.size(0)), dim3(SMX_BLOCK),
             (size_t)smx_lds_bytes(s.k, rows), smx_stream(), margin.data_ptr<float>(),
             y.data_ptr<float>(), s.w, (float2*)gh.data_ptr<float>(),
             (unsigned*)pmax.data_ptr<float>(), (i64)s.n, (int)s.k, (int)rows);
}

// part: (grid, 2) float64 scratch; out: [2] float64, written: the sum of
// w * term and the sum of w. kind: 0 mlogloss, 1 merror.
void softmax_metric(torch::Tensor margin, torch::Tensor y, torch::Tensor w, torch::Tensor part,
                    torch::Tensor out, int64_t rows, int64_t kind) {
  CHECK_DEV(part, torch::kFloat64);
  CHECK_DEV(out, torch::kFloat64);
  TORCH_CHECK_VALUE(part.dim() == 2 && part.size(1) == 2 && out.numel() == 2,
                    "part must be (grid, 2) and out hold 2 values");
  TORCH_CHECK_VALUE(kind == SMX_MLOGLOSS || kind == SMX_MERROR, "kind must be 0 (mlogloss) or 1 (merror)");
  const SmxShape s = smx_check_inputs(margin, y, w, rows, part.size(0));
  SMX_LAUNCH(softmax_metric_kernel, s.k, dim3((unsigned)part.size(0)), dim3(SMX_BLOCK),
             (size_t)smx_lds_bytes(s.k, rows), smx_stream(), margin.data_ptr<float>(),
             y.data_ptr<float>(), s.w, part.data_ptr<double>(), (i64)s.n, (int)s.k, (int)rows,
             (int)kind);
  hipLaunchKernelGGL(softmax_metric_finish_kernel, dim3(1), dim3(SMX_BLOCK), 0, smx_stream(),
                     part.data_ptr<double>(), (int)part.size(0), out.data_ptr<double>());
  smx_check_launch("softmax_metric_finish_kernel");
}

void init_multiclass_kernels(pybind11::module_& m) {
  m.def("softmax_tile_rows", &softmax_tile_rows, "tile rows for a class count and an LDS budget; 0 above the cap");
  m.def("softmax_max_grid", &softmax_max_grid, "most workgroups of a softmax launch");
  m.def("softmax_grad", &softmax_grad, "class-major softmax gradients + per-class absmax partials");
  m.def("softmax_metric", &softmax_metric, "mlogloss / merror sums without the softmax tensor");
}
