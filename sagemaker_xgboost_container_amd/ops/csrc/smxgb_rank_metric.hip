// MI355X (gfx950 / CDNA4) kernels for the ranking metrics ndcg[@k] and
// map[@k] over all query groups of a data set. The rule and its float64
// reference are ops/torch_ref.rank_metric.
//
// Per query group, documents are ranked by margin (descending, a NaN above
// +inf, ties by row index) and one float64 value per group is written:
//   ndcg  sum_{p < top} (2^y_p - 1) / log2(p + 2), over the group's IDCG
//   map   sum_{p < top} hit_p * hits_through_p / (p + 1), over the group's
//         relevant documents
// top = min(k, m), or m without a cut-off (k == 0 here). Nothing adds into
// another thread's sum with an atomic: every sum has one fixed order that
// depends on the position p alone, so the bits do not change from call to
// call or with the packing of groups into tiles.
//
// Tile kernel. Groups are fixed for a data set, so the host packs runs of
// consecutive groups into tiles of at most RM_CAP documents and RM_MAXG
// groups (ops/hip.rank_metric_plan). One 256-thread workgroup sorts its
// whole tile with a bitonic network over u64 keys
//     group-in-tile (8) | orderable(-margin) (32) | index-in-tile (12)
// in LDS (32 KiB). The sorted keys are then replaced in place by what the
// sums read by position: the float64 gain (ndcg) or the hit flag (map).
// After that a wavefront owns a group: lane l takes the positions l, l + 64,
// ... in rising order, and the 64 partial sums meet in a fixed shuffle tree.
// A tile of 256 two-document groups and a tile of one 4096-document group
// run through the same code; a group never waits at a workgroup barrier for
// another one. map carries an exact integer hit count from one 64-position
// step to the next (a shuffle scan inside the step).
//
// IDCG depends on labels and k only: the plan runs the ndcg kernels once
// with the labels as the margin and no `idcg` table, which makes them write
// the plain DCG, and keeps the result on the device. The per-round launch
// divides by it.
//
// Stream path, for a group of more than RM_CAP documents (among them a data
// set without group info, which is one query). rank_metric_keys_kernel
// writes int64 keys orderable(-margin) << 31 | row, which torch sorts (no
// readback); rank_metric_stream_kernel reads the first `top` sorted keys in
// chunks of RM_SCHUNK positions, four consecutive positions a thread, and
// writes one float64 partial sum per chunk; rank_metric_stream_finish_kernel
// adds the chunks in a fixed order. For map, rank_metric_stream_hits_kernel
// first counts the hits of every chunk; a chunk's carry is the integer sum
// of the counts before it.
//
// rank_metric_mean_kernel reduces the per-group values to their mean with
// one workgroup, so the host reads one scalar per metric.

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <algorithm>

typedef unsigned long long u64;

// Built without packed float32 instructions, as ops/csrc/smxgb_rank.hip is
// (and says why).
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#define RM_BLOCK 256
#define RM_WAVE 64
#define RM_WAVES (RM_BLOCK / RM_WAVE)
#define RM_CAP 4096  // documents per tile
#define RM_SLOTS (RM_CAP / RM_BLOCK)
#define RM_MAXG 256  // groups per tile (8 key bits)
#define RM_SCHUNK 1024  // positions per workgroup of the stream kernels
#define RM_PER (RM_SCHUNK / RM_BLOCK)
#define RM_KEYS_GRID 2048
#define RM_ROW_MASK 0x7fffffffll

enum { RM_NDCG = 0, RM_MAP = 1 };

#define CHECK_DEV(x, dt)                                                       \
  TORCH_CHECK_VALUE(x.is_cuda() && x.is_contiguous() && x.scalar_type() == dt, \
                    #x " must be a contiguous ROCm device tensor of the expected dtype")

// Rising in the rank: the largest margin gives the smallest value. -0.0
// ranks equal to +0.0; every NaN gives 0, which no other margin does (+inf
// gives 0x007fffff), so NaNs lead and tie among themselves.
__device__ __forceinline__ unsigned rm_order_bits(float s) {
  s += 0.0f;  // -0.0 -> +0.0
  if (s != s) return 0u;
  const unsigned b = __float_as_uint(-s);
  return b ^ ((b & 0x80000000u) ? 0xffffffffu : 0x80000000u);
}

__device__ __forceinline__ double rm_gain(float y) { return exp2((double)y) - 1.0; }

template <typename T>
__device__ __forceinline__ T rm_wave_sum(T v) {
  #pragma unroll
  for (int d = RM_WAVE >> 1; d > 0; d >>= 1) v += __shfl_down(v, d, RM_WAVE);
  return v;  // lane 0 holds the sum
}

__device__ __forceinline__ int rm_wave_scan(int v, int lane) {
  #pragma unroll
  for (int d = 1; d < RM_WAVE; d <<= 1) {
    const int o = __shfl_up(v, d, RM_WAVE);
    if (lane >= d) v += o;
  }
  return v;  // inclusive
}

// Shuffle tree per wavefront, then the wavefronts in order; every thread
// gets the sum (float64 terms, or int hit counts). red: LDS [RM_WAVES], free
// again on return.
template <typename T>
__device__ __forceinline__ T rm_block_sum(T v, T* red) {
  v = rm_wave_sum(v);
  if ((threadIdx.x & (RM_WAVE - 1)) == 0) red[threadIdx.x / RM_WAVE] = v;
  __syncthreads();
  T r = red[0];
  #pragma unroll
  for (int i = 1; i < RM_WAVES; ++i) r += red[i];
  __syncthreads();
  return r;
}

__device__ __forceinline__ double rm_ndcg_value(double dcg, const double* idcg, long long g) {
  if (idcg == nullptr) return dcg;  // the plan's IDCG pass
  const double ideal = idcg[g];
  return ideal > 0.0 ? dcg / ideal : 1.0;
}

// ---------------------------------------------------------------------------
// Tile kernel
// ---------------------------------------------------------------------------
// tiles: int32 [T][2] (first group, group count). disc: float64 [RM_CAP],
// 1 / log2(p + 2). idcg: float64 [n_groups], or null to write the DCG.
// value: float64 [n_groups].
template <int KIND>
__global__ __launch_bounds__(RM_BLOCK) void rank_metric_tile_kernel(
    const float* __restrict__ margin, const float* __restrict__ label,
    const int* __restrict__ group_ptr, const int* __restrict__ tiles,
    const double* __restrict__ disc, const double* __restrict__ idcg, int n, int n_groups, int k,
    double* __restrict__ value) {
  // the sorted keys, then gain (float64) or hit (int32) by sorted slot
  __shared__ __align__(16) unsigned char s_raw[RM_CAP * 8];
  __shared__ int s_gstart[RM_MAXG + 1];
  u64* s_keys = (u64*)s_raw;
  double* s_gain = (double*)s_raw;
  int* s_hit = (int*)s_raw;

  const int t = threadIdx.x;
  const int lane = t & (RM_WAVE - 1);
  const int w = t / RM_WAVE;
  const int g0 = tiles[2 * blockIdx.x];
  const int ng = tiles[2 * blockIdx.x + 1];
  if (g0 < 0 || ng < 1 || ng > RM_MAXG || g0 > n_groups - ng) return;  // uniform
  const int base = group_ptr[g0];
  const int N = group_ptr[g0 + ng] - base;
  if (base < 0 || N < 0 || N > RM_CAP || base > n - N) return;  // uniform

  for (int i = t; i <= ng; i += RM_BLOCK) {
    const int v = group_ptr[g0 + i] - base;
    s_gstart[i] = v < 0 ? 0 : (v > N ? N : v);
  }
  __syncthreads();

  // -- 1. keys and one bitonic sort over the tile ---------------------------
  int P = 2;
  while (P < N) P <<= 1;
  for (int i = t; i < P; i += RM_BLOCK) {
    u64 key = ~0ull;
    if (i < N) {
      int lo = 0, hi = ng;  // the last group that starts at or before slot i
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (s_gstart[mid] <= i) lo = mid; else hi = mid;
      }
      key = ((u64)lo << 44) | ((u64)rm_order_bits(margin[base + i]) << 12) | (u64)i;
    }
    s_keys[i] = key;
  }
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int i = t; i < (P >> 1); i += RM_BLOCK) {
        const int lo = 2 * i - (i & (stride - 1));
        const int hi = lo + stride;
        const u64 a = s_keys[lo];
        const u64 b = s_keys[hi];
        if ((a > b) == ((lo & size) == 0)) {
          s_keys[lo] = b;
          s_keys[hi] = a;
        }
      }
    }
  }
  __syncthreads();

  // -- 2. keys -> gain or hit, in place: thread t owns slots t, t + 256, ... -
  int row[RM_SLOTS];
  #pragma unroll
  for (int j = 0; j < RM_SLOTS; ++j) {
    const int slot = j * RM_BLOCK + t;
    int i = slot < N ? (int)(s_keys[slot] & 0xfffull) : 0;
    if (i >= N) i = N - 1;  // cannot happen: the keys hold each i < N once
    row[j] = i;
  }
  __syncthreads();
  #pragma unroll
  for (int j = 0; j < RM_SLOTS; ++j) {
    const int slot = j * RM_BLOCK + t;
    if (slot < N) {
      const float y = label[base + row[j]];
      if (KIND == RM_NDCG) s_gain[slot] = rm_gain(y);
      else s_hit[slot] = y > 0.0f ? 1 : 0;
    }
  }
  __syncthreads();

  // -- 3. one wavefront per group -------------------------------------------
  for (int gi = w; gi < ng; gi += RM_WAVES) {
    const int gs = s_gstart[gi];
    const int m = s_gstart[gi + 1] - gs;
    const int top = (k > 0 && k < m) ? k : m;
    double acc = 0.0;
    if (KIND == RM_NDCG) {
      for (int p = lane; p < top; p += RM_WAVE) acc += s_gain[gs + p] * disc[p];
      acc = rm_wave_sum(acc);
      if (lane == 0) value[g0 + gi] = rm_ndcg_value(acc, idcg, g0 + gi);
    } else {
      int carry = 0;  // hits before this step, then of the group
      for (int p0 = 0; p0 < m; p0 += RM_WAVE) {  // m is uniform over the wave
        const int p = p0 + lane;
        const int hit = p < m ? s_hit[gs + p] : 0;
        const int hs = carry + rm_wave_scan(hit, lane);
        if (hit && p < top) acc += (double)hs / (double)(p + 1);
        carry = __shfl(hs, RM_WAVE - 1, RM_WAVE);
      }
      acc = rm_wave_sum(acc);
      if (lane == 0) value[g0 + gi] = carry > 0 ? acc / (double)carry : 1.0;
    }
  }
}

// ---------------------------------------------------------------------------
// Stream path: one group of m > RM_CAP documents
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(RM_BLOCK) void rank_metric_keys_kernel(
    const float* __restrict__ s, int m, long long* __restrict__ keys) {
  const long long step = (long long)gridDim.x * RM_BLOCK;
  for (long long i = (long long)blockIdx.x * RM_BLOCK + threadIdx.x; i < m; i += step)
    keys[i] = ((long long)rm_order_bits(s[i]) << 31) | i;
}

// Label at sorted position p of the group whose rows start at `label`.
__device__ __forceinline__ float rm_stream_label(const long long* __restrict__ skeys,
                                                 const float* __restrict__ label, int p, int m) {
  long long r = skeys[p] & RM_ROW_MASK;
  if (r >= m) r = m - 1;  // cannot happen: the keys hold each row < m once
  return label[r];
}

// chunk_h[c] = relevant documents among the positions of chunk c below top.
__global__ __launch_bounds__(RM_BLOCK) void rank_metric_stream_hits_kernel(
    const long long* __restrict__ skeys, const float* __restrict__ label, int m, int top,
    int* __restrict__ chunk_h) {
  __shared__ int s_red[RM_WAVES];
  const int p0 = blockIdx.x * RM_SCHUNK + threadIdx.x * RM_PER;
  int h = 0;
  #pragma unroll
  for (int j = 0; j < RM_PER; ++j)
    if (p0 + j < top && rm_stream_label(skeys, label, p0 + j, m) > 0.0f) ++h;
  h = rm_block_sum(h, s_red);
  if (threadIdx.x == 0) chunk_h[blockIdx.x] = h;
}

// part[c] = the chunk's terms, summed position by position inside a thread,
// then over the workgroup in rm_block_sum's order. chunk_h: map only.
template <int KIND>
__global__ __launch_bounds__(RM_BLOCK) void rank_metric_stream_kernel(
    const long long* __restrict__ skeys, const float* __restrict__ label, int m, int top,
    const int* __restrict__ chunk_h, double* __restrict__ part) {
  __shared__ double s_red[RM_WAVES];
  __shared__ int s_cnt[RM_WAVES];
  __shared__ int s_h[RM_WAVES];
  const int t = threadIdx.x;
  const int lane = t & (RM_WAVE - 1);
  const int w = t / RM_WAVE;
  const int p0 = blockIdx.x * RM_SCHUNK + t * RM_PER;
  double acc = 0.0;
  if (KIND == RM_NDCG) {
    #pragma unroll
    for (int j = 0; j < RM_PER; ++j) {
      const int p = p0 + j;
      if (p < top) acc += rm_gain(rm_stream_label(skeys, label, p, m)) * (1.0 / log2((double)p + 2.0));
    }
  } else {
    int hit[RM_PER];
    int th = 0;
    #pragma unroll
    for (int j = 0; j < RM_PER; ++j) {
      const int p = p0 + j;
      hit[j] = (p < top && rm_stream_label(skeys, label, p, m) > 0.0f) ? 1 : 0;
      th += hit[j];
    }
    // hits before this thread: the chunks before, the wavefronts before, the
    // lanes before; integers, so exact in any order
    int before = 0;
    for (int c = t; c < (int)blockIdx.x; c += RM_BLOCK) before += chunk_h[c];
    before = rm_block_sum(before, s_cnt);
    const int incl = rm_wave_scan(th, lane);
    if (lane == RM_WAVE - 1) s_h[w] = incl;
    __syncthreads();
    int h = before + incl - th;
    for (int i = 0; i < w; ++i) h += s_h[i];
    #pragma unroll
    for (int j = 0; j < RM_PER; ++j) {
      h += hit[j];
      if (hit[j]) acc += (double)h / (double)(p0 + j + 1);
    }
  }
  acc = rm_block_sum(acc, s_red);
  if (t == 0) part[blockIdx.x] = acc;
}

// One workgroup: value[g] from the chunks' partial sums, thread t adding
// the chunks t, t + 256, ... in rising order. n_pos: map, relevant documents
// of the whole group.
template <int KIND>
__global__ __launch_bounds__(RM_BLOCK) void rank_metric_stream_finish_kernel(
    const double* __restrict__ part, int chunks, int n_pos, const double* __restrict__ idcg,
    long long g, double* __restrict__ value) {
  __shared__ double s_red[RM_WAVES];
  double acc = 0.0;
  for (int c = threadIdx.x; c < chunks; c += RM_BLOCK) acc += part[c];
  acc = rm_block_sum(acc, s_red);
  if (threadIdx.x == 0) {
    if (KIND == RM_NDCG) value[g] = rm_ndcg_value(acc, idcg, g);
    else value[g] = n_pos > 0 ? acc / (double)n_pos : 1.0;
  }
}

// out[0] = mean of value[0, G), one workgroup, the order of the finish kernel.
__global__ __launch_bounds__(RM_BLOCK) void rank_metric_mean_kernel(
    const double* __restrict__ value, long long G, double* __restrict__ out) {
  __shared__ double s_red[RM_WAVES];
  double acc = 0.0;
  for (long long g = threadIdx.x; g < G; g += RM_BLOCK) acc += value[g];
  acc = rm_block_sum(acc, s_red);
  if (threadIdx.x == 0) out[0] = acc / (double)G;
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
static hipStream_t rm_stream() { return at::hip::getCurrentHIPStream().stream(); }

static void rm_check_launch(const char* what) {
  const hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, what, " launch failed: ", hipGetErrorString(err));
}

static void rm_check_common(int64_t k, int64_t kind) {
  TORCH_CHECK_VALUE(k >= 0 && k < (1ll << 31), "k must be in [0, 2^31), 0 for no cut-off");
  TORCH_CHECK_VALUE(kind == RM_NDCG || kind == RM_MAP, "unknown ranking metric kind");
}

int64_t rank_metric_cap() { return RM_CAP; }
int64_t rank_metric_max_groups() { return RM_MAXG; }
int64_t rank_metric_stream_chunk() { return RM_SCHUNK; }

// idcg: [G], or empty to write the DCG (kind 0). tiles: [T, 2]. value: [G].
void rank_metric_tile(torch::Tensor margin, torch::Tensor label, torch::Tensor group_ptr,
                      torch::Tensor tiles, torch::Tensor disc, torch::Tensor idcg, int64_t k,
                      int64_t kind, torch::Tensor value) {
  CHECK_DEV(margin, torch::kFloat32);
  CHECK_DEV(label, torch::kFloat32);
  CHECK_DEV(group_ptr, torch::kInt32);
  CHECK_DEV(tiles, torch::kInt32);
  CHECK_DEV(disc, torch::kFloat64);
  CHECK_DEV(idcg, torch::kFloat64);
  CHECK_DEV(value, torch::kFloat64);
  rm_check_common(k, kind);
  const int64_t n = margin.numel();
  const int64_t T = tiles.numel() / 2;
  const int64_t G = group_ptr.numel() - 1;
  TORCH_CHECK_VALUE(n >= 1 && n < (1ll << 31), "row count must be in [1, 2^31)");
  TORCH_CHECK_VALUE(label.numel() == n, "label must match margin");
  TORCH_CHECK_VALUE(G >= 1 && T >= 1 && tiles.numel() == 2 * T, "tiles must be [T, 2]");
  TORCH_CHECK_VALUE(value.numel() == G && (idcg.numel() == 0 || idcg.numel() == G),
                    "value and idcg must hold one entry per group");
  TORCH_CHECK_VALUE(disc.numel() >= RM_CAP, "disc must hold a discount per tile position");
  const double* ideal = idcg.numel() ? idcg.data_ptr<double>() : nullptr;
#define RM_LAUNCH_TILE(KIND)                                                                 \
  hipLaunchKernelGGL(rank_metric_tile_kernel<KIND>, dim3((unsigned)T), dim3(RM_BLOCK), 0,    \
                     rm_stream(), margin.data_ptr<float>(), label.data_ptr<float>(),         \
                     group_ptr.data_ptr<int>(), tiles.data_ptr<int>(),                       \
                     disc.data_ptr<double>(), ideal, (int)n, (int)G, (int)k,                 \
                     value.data_ptr<double>())
  if (kind == RM_NDCG) RM_LAUNCH_TILE(RM_NDCG);
  else RM_LAUNCH_TILE(RM_MAP);
#undef RM_LAUNCH_TILE
  rm_check_launch("rank_metric_tile_kernel");
}

// keys[i] = orderable(-s[i]) << 31 | i; sorted ascending they give the rows
// of one group by rank.
void rank_metric_keys(torch::Tensor s, torch::Tensor keys) {
  CHECK_DEV(s, torch::kFloat32);
  CHECK_DEV(keys, torch::kInt64);
  const int64_t m = s.numel();
  TORCH_CHECK_VALUE(m >= 1 && m < (1ll << 31) && keys.numel() == m,
                    "keys must match s, with fewer than 2^31 rows");
  const int64_t grid = std::min<int64_t>((m + RM_BLOCK - 1) / RM_BLOCK, RM_KEYS_GRID);
  hipLaunchKernelGGL(rank_metric_keys_kernel, dim3((unsigned)grid), dim3(RM_BLOCK), 0,
                     rm_stream(), s.data_ptr<float>(), (int)m,
                     (long long*)keys.data_ptr<int64_t>());
  rm_check_launch("rank_metric_keys_kernel");
}

// Group g: rows [gs, gs + m) of label, skeys its sorted keys (at least the
// first min(k, m)). n_pos: relevant documents of the group (map). chunk_h,
// part: scratch with an entry per chunk of the first `top` positions.
void rank_metric_stream(torch::Tensor skeys, torch::Tensor label, int64_t gs, int64_t m,
                        int64_t k, int64_t kind, int64_t n_pos, torch::Tensor idcg, int64_t g,
                        torch::Tensor chunk_h, torch::Tensor part, torch::Tensor value) {
  CHECK_DEV(skeys, torch::kInt64);
  CHECK_DEV(label, torch::kFloat32);
  CHECK_DEV(idcg, torch::kFloat64);
  CHECK_DEV(chunk_h, torch::kInt32);
  CHECK_DEV(part, torch::kFloat64);
  CHECK_DEV(value, torch::kFloat64);
  rm_check_common(k, kind);
  const int64_t G = value.numel();
  TORCH_CHECK_VALUE(m >= 1 && m < (1ll << 31), "group size must be in [1, 2^31)");
  TORCH_CHECK_VALUE(gs >= 0 && gs + m <= label.numel(), "the group must lie inside label");
  TORCH_CHECK_VALUE(g >= 0 && g < G && (idcg.numel() == 0 || idcg.numel() == G),
                    "value and idcg must hold one entry per group");
  TORCH_CHECK_VALUE(n_pos >= 0 && n_pos <= m, "n_pos must be in [0, m]");
  const int64_t top = (k > 0 && k < m) ? k : m;
  const int64_t chunks = (top + RM_SCHUNK - 1) / RM_SCHUNK;
  TORCH_CHECK_VALUE(skeys.numel() >= top && chunk_h.numel() >= chunks && part.numel() >= chunks,
                    "skeys, chunk_h and part are too small");
  const double* ideal = idcg.numel() ? idcg.data_ptr<double>() : nullptr;
  const long long* sk = (const long long*)skeys.data_ptr<int64_t>();
  const float* lab = label.data_ptr<float>() + gs;
  hipStream_t stream = rm_stream();
  if (kind == RM_MAP) {
    hipLaunchKernelGGL(rank_metric_stream_hits_kernel, dim3((unsigned)chunks), dim3(RM_BLOCK), 0,
                       stream, sk, lab, (int)m, (int)top, chunk_h.data_ptr<int>());
    rm_check_launch("rank_metric_stream_hits_kernel");
  }
#define RM_LAUNCH_STREAM(KIND)                                                                \
  hipLaunchKernelGGL(rank_metric_stream_kernel<KIND>, dim3((unsigned)chunks), dim3(RM_BLOCK), \
                     0, stream, sk, lab, (int)m, (int)top, chunk_h.data_ptr<int>(),           \
                     part.data_ptr<double>());                                                \
  rm_check_launch("rank_metric_stream_kernel");                                               \
  hipLaunchKernelGGL(rank_metric_stream_finish_kernel<KIND>, dim3(1), dim3(RM_BLOCK), 0,      \
                     stream, part.data_ptr<double>(), (int)chunks, (int)n_pos, ideal,         \
                     (long long)g, value.data_ptr<double>());                                 \
  rm_check_launch("rank_metric_stream_finish_kernel")
  if (kind == RM_NDCG) { RM_LAUNCH_STREAM(RM_NDCG); }
  else { RM_LAUNCH_STREAM(RM_MAP); }
#undef RM_LAUNCH_STREAM
}

void rank_metric_mean(torch::Tensor value, torch::Tensor out) {
  CHECK_DEV(value, torch::kFloat64);
  CHECK_DEV(out, torch::kFloat64);
  TORCH_CHECK_VALUE(value.numel() >= 1 && out.numel() >= 1, "value and out must not be empty");
  hipLaunchKernelGGL(rank_metric_mean_kernel, dim3(1), dim3(RM_BLOCK), 0, rm_stream(),
                     value.data_ptr<double>(), (long long)value.numel(), out.data_ptr<double>());
  rm_check_launch("rank_metric_mean_kernel");
}

void init_rank_metric_kernels(pybind11::module_& m) {
  m.def("rank_metric_cap", &rank_metric_cap, "documents per tile of the ranking metric kernel");
  m.def("rank_metric_max_groups", &rank_metric_max_groups, "groups per tile");
  m.def("rank_metric_stream_chunk", &rank_metric_stream_chunk, "positions per stream workgroup");
  m.def("rank_metric_tile", &rank_metric_tile, "ndcg / map of every tile of groups");
  m.def("rank_metric_keys", &rank_metric_keys, "sortable keys of one group larger than a tile");
  m.def("rank_metric_stream", &rank_metric_stream, "ndcg / map of one group larger than a tile");
  m.def("rank_metric_mean", &rank_metric_mean, "fixed-order mean of the per-group values");
}
