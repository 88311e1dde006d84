// MI355X (gfx950 / CDNA4) kernels for the histogram tree updater.
//
// Replaces the CUDA gpu_hist kernel set the reference reaches through
// xgb.train: per-node gradient histograms, row partition,
// leaf scatter and batched forest prediction. Written directly for CDNA4:
// 64-wide wavefronts, 160 KiB LDS per CU, device-scope atomics, grids capped
// and grid-strided per Guideline 11 of the CDNA HIP programming guide.
//
// Histogram accumulation uses int64 fixed point (value * 2^33 / max_abs)
// in LDS with one global flush per block: bit-deterministic regardless of
// atomic ordering (the `deterministic_histogram` contract) and exactly
// summable across ranks by an RCCL int64 allreduce.
//
// All launchers are batched: one launch covers every node of a tree level,
// with a host-built block -> (job, chunk) map so the grid stays near the
// 256-CU sweet spot regardless of how many nodes/rows each level has.

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <vector>

#include "smxgb_cat.h"   // CAT_WORDS, cat_bit, cat_goes_left (categorical nodes)
#include "smxgb_jobs.h"  // WAVE, HIST_BLOCK, CHECK_GPU, HistJob / PartJob / LeafJob
#include "smxgb_shap.h"  // SHAP_BLOCK, shap_one_fraction, shap_unwound_sum

// LDS histogram layout: separate g and h arrays (SoA). A 16-B interleaved
// (g,h) slot can only start on 8 of the 32 bank groups (measured 75% of
// LDS cycles lost to conflicts: SQ_LDS_BANK_CONFLICT 0.74G vs
// SQ_LDS_IDX_ACTIVE 1.0G); 8-B-strided u64 arrays reach 16 groups, halving
// intrinsic conflict pressure. lds_pad_slot adds a skew word per 8 slots.
__device__ __host__ inline int lds_pad_slot(int s) { return s + (s >> 3); }
__device__ __host__ inline long long lds_padded_words(long long pairs) {
  // per array: pairs + pairs/8 + 1 u64 words; x2 for the g and h arrays
  return (pairs + (pairs >> 3) + 1) * 2;
}
__device__ inline long long lds_half_words(long long pairs) {
  return pairs + (pairs >> 3) + 1;
}

// ---------------------------------------------------------------------------
// histogram build
// ---------------------------------------------------------------------------

template <typename BinT>
__global__ __launch_bounds__(HIST_BLOCK) void hist_kernel(
    const BinT* __restrict__ bins, const float2* __restrict__ gh,
    const int* __restrict__ rowbuf, const HistJob* __restrict__ jobs,
    const int* __restrict__ block_job, unsigned long long* __restrict__ out,
    int nfeat, int stride, float scale_g, float scale_h) {
  extern __shared__ unsigned long long lhist[];

  const HistJob job = jobs[block_job[blockIdx.x]];
  const int nf_group = job.fg_end - job.fg_start;
  const int lds_words = nf_group * stride * 2;
  const int hofs = (int)lds_half_words(nf_group * stride);
  const int lds_padded = 2 * hofs;
  for (int i = threadIdx.x; i < lds_padded; i += blockDim.x) lhist[i] = 0ull;
  __syncthreads();

  const int chunk = blockIdx.x - job.first_block;
  const long long step = (long long)job.num_blocks * blockDim.x;
  for (long long r = job.start + (long long)chunk * blockDim.x + threadIdx.x; r < job.end; r += step) {
    const int row = rowbuf[r];
    const float2 gp = gh[row];
    const unsigned long long gfix = (unsigned long long)(long long)llrintf(gp.x * scale_g);
    const unsigned long long hfix = (unsigned long long)(long long)llrintf(gp.y * scale_h);
    const BinT* rp = bins + (long long)row * nfeat + job.fg_start;
    if constexpr (sizeof(BinT) == 1) {
      // vectorized path: 4 bins per dword load (valid when the group is
      // 4-aligned in the row — guaranteed by host packing for nfeat%4==0)
      if ((nf_group & 3) == 0 && ((((long long)row * nfeat + job.fg_start) & 3) == 0)) {
        const uchar4* rp4 = reinterpret_cast<const uchar4*>(rp);
        #pragma unroll 2
        for (int f4 = 0; f4 < (nf_group >> 2); ++f4) {
          const uchar4 b4 = rp4[f4];
          const int base = (f4 << 2) * stride;
          const int s0 = lds_pad_slot(base + (int)b4.x);
          const int s1 = lds_pad_slot(base + stride + (int)b4.y);
          const int s2 = lds_pad_slot(base + 2 * stride + (int)b4.z);
          const int s3 = lds_pad_slot(base + 3 * stride + (int)b4.w);
          atomicAdd(&lhist[s0], gfix);
          atomicAdd(&lhist[hofs + s0], hfix);
          atomicAdd(&lhist[s1], gfix);
          atomicAdd(&lhist[hofs + s1], hfix);
          atomicAdd(&lhist[s2], gfix);
          atomicAdd(&lhist[hofs + s2], hfix);
          atomicAdd(&lhist[s3], gfix);
          atomicAdd(&lhist[hofs + s3], hfix);
        }
        continue;
      }
    }
    #pragma unroll 4
    for (int f = 0; f < nf_group; ++f) {
      const int slot = lds_pad_slot(f * stride + (int)rp[f]);
      atomicAdd(&lhist[slot], gfix);
      atomicAdd(&lhist[hofs + slot], hfix);
    }
  }
  __syncthreads();

  unsigned long long* gout =
      out + ((long long)job.hist_idx * nfeat + job.fg_start) * (long long)stride * 2;
  for (int i = threadIdx.x; i < lds_words; i += blockDim.x) {
    const int pair = i >> 1;
    const int idx = lds_pad_slot(pair) + ((i & 1) ? hofs : 0);
    const unsigned long long v = lhist[idx];
    if (v) atomicAdd(&gout[i], v);
  }
}

__global__ void hist_convert_kernel(const unsigned long long* __restrict__ in,
                                    float* __restrict__ out, long long n_pairs,
                                    float inv_g, float inv_h) {
  const long long step = (long long)gridDim.x * blockDim.x;
  const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (long long i = i0; i < n_pairs; i += step) {
    const long long j = i * 2;
    out[j] = (float)((double)(long long)in[j] * (double)inv_g);
    out[j + 1] = (float)((double)(long long)in[j + 1] * (double)inv_h);
  }
}

__global__ void hist_convert_dev_kernel(const unsigned long long* __restrict__ in,
                                        float* __restrict__ out, long long n_pairs,
                                        const float* __restrict__ gh_max) {
  const double inv_g = (double)fmaxf(gh_max[0], 1e-30f) / 8589934592.0;
  const double inv_h = (double)fmaxf(gh_max[1], 1e-30f) / 8589934592.0;
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_pairs; i += step) {
    const long long j = i * 2;
    out[j] = (float)((double)(long long)in[j] * (double)inv_g);
    out[j + 1] = (float)((double)(long long)in[j + 1] * (double)inv_h);
  }
}

// ---------------------------------------------------------------------------
// COMPACT-LAYOUT pipeline (v2)
//
// The gather-based hist kernel reads each scattered row through a full
// 128-B cache line (28 useful bytes): at depth>0 the updater is bound by
// that amplification. v2 keeps rows PHYSICALLY node-contiguous: partition
// rewrites each surviving row's (row id, bin bytes, gradient pair) into
// ping-pong compact SoA buffers, so every level's histogram build is a
// perfectly coalesced stream and no kernel gathers by row id again.
// ---------------------------------------------------------------------------

// hist over compact buffers: rows are positions [start,end) in bins_c/gh_c.
template <typename BinT>
__global__ __launch_bounds__(HIST_BLOCK) void hist_compact_kernel(
    const BinT* __restrict__ bins_c, const float2* __restrict__ gh_c,
    const HistJob* __restrict__ jobs, const int* __restrict__ block_job,
    unsigned long long* __restrict__ out, int nfeat, int stride,
    const float* __restrict__ gh_max) {
  extern __shared__ unsigned long long lhist[];

  // fixed-point scale derived on device (2^33 / max_abs): no host sync
  const float scale_g = 8589934592.0f / fmaxf(gh_max[0], 1e-30f);
  const float scale_h = 8589934592.0f / fmaxf(gh_max[1], 1e-30f);
  const HistJob job = jobs[block_job[blockIdx.x]];
  const int nf_group = job.fg_end - job.fg_start;
  const int lds_words = nf_group * stride * 2;
  const int hofs = (int)lds_half_words(nf_group * stride);
  const int lds_padded = 2 * hofs;
  for (int i = threadIdx.x; i < lds_padded; i += blockDim.x) lhist[i] = 0ull;
  __syncthreads();

  const int chunk = blockIdx.x - job.first_block;
  const long long step = (long long)job.num_blocks * blockDim.x;
  for (long long r = job.start + (long long)chunk * blockDim.x + threadIdx.x; r < job.end; r += step) {
    const float2 gp = gh_c[r];
    const unsigned long long gfix = (unsigned long long)(long long)llrintf(gp.x * scale_g);
    const unsigned long long hfix = (unsigned long long)(long long)llrintf(gp.y * scale_h);
    const BinT* rp = bins_c + (long long)r * nfeat + job.fg_start;
    if constexpr (sizeof(BinT) == 1) {
      if ((nf_group & 3) == 0 && ((((long long)r * nfeat + job.fg_start) & 3) == 0)) {
        const uchar4* rp4 = reinterpret_cast<const uchar4*>(rp);
        #pragma unroll 2
        for (int f4 = 0; f4 < (nf_group >> 2); ++f4) {
          const uchar4 b4 = rp4[f4];
          const int base = (f4 << 2) * stride;
          const int s0 = lds_pad_slot(base + (int)b4.x);
          const int s1 = lds_pad_slot(base + stride + (int)b4.y);
          const int s2 = lds_pad_slot(base + 2 * stride + (int)b4.z);
          const int s3 = lds_pad_slot(base + 3 * stride + (int)b4.w);
          atomicAdd(&lhist[s0], gfix);
          atomicAdd(&lhist[hofs + s0], hfix);
          atomicAdd(&lhist[s1], gfix);
          atomicAdd(&lhist[hofs + s1], hfix);
          atomicAdd(&lhist[s2], gfix);
          atomicAdd(&lhist[hofs + s2], hfix);
          atomicAdd(&lhist[s3], gfix);
          atomicAdd(&lhist[hofs + s3], hfix);
        }
        continue;
      }
    }
    #pragma unroll 4
    for (int f = 0; f < nf_group; ++f) {
      const int slot = lds_pad_slot(f * stride + (int)rp[f]);
      atomicAdd(&lhist[slot], gfix);
      atomicAdd(&lhist[hofs + slot], hfix);
    }
  }
  __syncthreads();

  unsigned long long* gout =
      out + ((long long)job.hist_idx * nfeat + job.fg_start) * (long long)stride * 2;
  for (int i = threadIdx.x; i < lds_words; i += blockDim.x) {
    const int pair = i >> 1;
    const int idx = lds_pad_slot(pair) + ((i & 1) ? hofs : 0);
    const unsigned long long v = lhist[idx];
    if (v) atomicAdd(&gout[i], v);
  }
}

// compact partition: decide per row from src bins (sequential read), then
// copy the whole record (row id + bin bytes + gh) to its contiguous
// destination run. Destinations inside one tile form two coalesced runs.
#define CPART_TILE 2048

// jobs carry segments only; the split decision (gain, feature, bin,
// missing direction) is read from the on-device packed split tensor
// ([k, 6] float32 from the split kernels), so no host round-trip sits
// between split search and partition. gain <= 0 jobs are skipped.
// HAS_CAT (a matrix with categorical columns): a split on a feature with
// is_cat[feature] set sends the bins in the node's category set
// (cat_bits[node row], smxgb_cat.h) right and the others left.
template <typename BinT, bool HAS_CAT>
__global__ __launch_bounds__(HIST_BLOCK) void partition_compact_kernel(
    const BinT* __restrict__ src_bins, const float2* __restrict__ src_gh,
    const int* __restrict__ src_rows, BinT* __restrict__ dst_bins,
    float2* __restrict__ dst_gh, int* __restrict__ dst_rows,
    const PartJob* __restrict__ jobs, const int* __restrict__ block_job,
    const float* __restrict__ split_packed,  // [n_nodes, 6]; job.feature = node row
    int* __restrict__ counters, int nfeat, int missing_bin,
    const unsigned char* __restrict__ is_cat,  // [nfeat]; read only with HAS_CAT
    const unsigned int* __restrict__ cat_bits) {  // [n_nodes, CAT_WORDS]
  __shared__ int ldest[CPART_TILE];  // destination index per tile row
  __shared__ int lcnt, rcnt, lbase, rbase;

  const int j = block_job[blockIdx.x];
  const PartJob job = jobs[j];
  const float* sp6 = split_packed + job.feature * 6;
  if (sp6[0] <= 0.0f) return;  // no split for this node
  const int feature = (int)sp6[1];
  const int split_bin = (int)sp6[2];
  const int default_left = sp6[3] > 0.5f ? 1 : 0;
  __shared__ unsigned int cset[CAT_WORDS];  // the node's category set
  bool cat_split = false;
  if (HAS_CAT) {
    cat_split = is_cat[feature] != 0;  // block-uniform
    if (cat_split && threadIdx.x < CAT_WORDS) {
      cset[threadIdx.x] = cat_bits[(long long)job.feature * CAT_WORDS + threadIdx.x];
    }
    // the tile loop's first barrier orders these stores before any read
  }

  const int chunk = blockIdx.x - job.first_block;
  const long long tile_step = (long long)job.num_blocks * CPART_TILE;

  for (long long tile = job.start + (long long)chunk * CPART_TILE; tile < job.end; tile += tile_step) {
    if (threadIdx.x == 0) {
      lcnt = 0;
      rcnt = 0;
    }
    __syncthreads();
    const int tile_n = (int)min((long long)CPART_TILE, job.end - tile);
    for (int i = threadIdx.x; i < tile_n; i += blockDim.x) {
      const int b = (int)src_bins[(tile + i) * (long long)nfeat + feature];
      bool left;
      if (HAS_CAT && cat_split) {
        left = (b == missing_bin) ? (default_left != 0)
                                  : !((unsigned)b < (unsigned)CAT_MAX && cat_bit(cset, b));
      } else {
        left = (b == missing_bin) ? (default_left != 0) : (b <= split_bin);
      }
      ldest[i] = left ? atomicAdd(&lcnt, 1) : ~atomicAdd(&rcnt, 1);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      lbase = atomicAdd(&counters[j * 2], lcnt);
      rbase = atomicAdd(&counters[j * 2 + 1], rcnt);
    }
    __syncthreads();
    // copy phase, (row, dword) work units: consecutive threads move
    // consecutive dwords so stores coalesce into the two destination runs.
    // Work units are padded to a power of two per row so the row index is a
    // shift, not an integer division (a div per dword dominated this loop).
    if ((nfeat & 3) == 0 && sizeof(BinT) == 1) {
      const int nd = nfeat >> 2;  // bin dwords per row
      int log2p = 0;
      while ((1 << log2p) < nd) ++log2p;
      const int mask = (1 << log2p) - 1;
      const uchar4* sb4 = reinterpret_cast<const uchar4*>(src_bins);
      uchar4* db4 = reinterpret_cast<uchar4*>(dst_bins);
      for (int u = threadIdx.x; u < (tile_n << log2p); u += blockDim.x) {
        const int i = u >> log2p;
        const int f4 = u & mask;
        if (f4 >= nd) continue;
        const int d = ldest[i];
        const long long dst =
            d >= 0 ? (long long)job.start + lbase + d : (long long)job.end - 1 - rbase - (~d);
        db4[dst * nd + f4] = sb4[(tile + i) * (long long)nd + f4];
      }
    } else {
      int log2p = 0;
      while ((1 << log2p) < nfeat) ++log2p;
      const int mask = (1 << log2p) - 1;
      for (int u = threadIdx.x; u < (tile_n << log2p); u += blockDim.x) {
        const int i = u >> log2p;
        const int f = u & mask;
        if (f >= nfeat) continue;
        const int d = ldest[i];
        const long long dst =
            d >= 0 ? (long long)job.start + lbase + d : (long long)job.end - 1 - rbase - (~d);
        dst_bins[dst * (long long)nfeat + f] = src_bins[(tile + i) * (long long)nfeat + f];
      }
    }
    for (int u = threadIdx.x; u < tile_n * 2; u += blockDim.x) {
      const int i = u >> 1;
      const int half = u & 1;
      const int d = ldest[i];
      const long long dst =
          d >= 0 ? (long long)job.start + lbase + d : (long long)job.end - 1 - rbase - (~d);
      reinterpret_cast<float*>(dst_gh)[dst * 2 + half] =
          reinterpret_cast<const float*>(src_gh)[(tile + i) * 2 + half];
    }
    for (int i = threadIdx.x; i < tile_n; i += blockDim.x) {
      const int d = ldest[i];
      const long long dst =
          d >= 0 ? (long long)job.start + lbase + d : (long long)job.end - 1 - rbase - (~d);
      dst_rows[dst] = src_rows[tile + i];
    }
    __syncthreads();
  }
}

// fused per-round gradient computation: one HBM pass writes the packed
// (g, h) pairs AND per-block |g|/|h| maxima (for the fixed-point histogram
// scale), replacing ~5 torch elementwise/reduce passes (~250 us/round on the
// 12.5M-row bench; this kernel is ~35 us).
// mode 0: binary:logistic / reg:logistic — g = sigmoid(m) - y,
//         h = max(p(1-p), 1e-16), scale_pos_weight applied to y == 1
// mode 1: reg:squarederror — g = m - y, h = 1
__global__ __launch_bounds__(HIST_BLOCK) void grad_fused_kernel(
    const float* __restrict__ margin, const float* __restrict__ y,
    const float* __restrict__ w, float2* __restrict__ gh,
    float2* __restrict__ pmax, double2* __restrict__ psum, long long n, int mode,
    float spw) {
  __shared__ float red[HIST_BLOCK * 2];
  __shared__ double dred[HIST_BLOCK * 2];
  float gmax = 0.f, hmax = 0.f;
  double gsum = 0.0, hsum = 0.0;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float m = margin[i];
    const float yi = y[i];
    float g, h;
    if (mode == 0) {
      const float p = 1.0f / (1.0f + expf(-m));
      g = p - yi;
      h = fmaxf(p * (1.0f - p), 1e-16f);
      if (spw != 1.0f && yi == 1.0f) {
        g *= spw;
        h *= spw;
      }
    } else {
      g = m - yi;
      h = 1.0f;
    }
    if (w) {
      const float wi = w[i];
      g *= wi;
      h *= wi;
    }
    gh[i] = make_float2(g, h);
    gmax = fmaxf(gmax, fabsf(g));
    hmax = fmaxf(hmax, fabsf(h));
    gsum += (double)g;
    hsum += (double)h;
  }
  red[threadIdx.x] = gmax;
  red[threadIdx.x + HIST_BLOCK] = hmax;
  dred[threadIdx.x] = gsum;
  dred[threadIdx.x + HIST_BLOCK] = hsum;
  __syncthreads();
  for (int off = HIST_BLOCK / 2; off > 0; off >>= 1) {
    if (threadIdx.x < off) {
      red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + off]);
      red[threadIdx.x + HIST_BLOCK] =
          fmaxf(red[threadIdx.x + HIST_BLOCK], red[threadIdx.x + HIST_BLOCK + off]);
      dred[threadIdx.x] += dred[threadIdx.x + off];
      dred[threadIdx.x + HIST_BLOCK] += dred[threadIdx.x + HIST_BLOCK + off];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    pmax[blockIdx.x] = make_float2(red[0], red[HIST_BLOCK]);
    psum[blockIdx.x] = make_double2(dred[0], dred[HIST_BLOCK]);
  }
}

// leaf scatter from compact row-id buffers. The random 4-B RMW is
// latency-bound; 4 rows in flight per iteration overlap the line fetches
// (leaf row sets are disjoint by construction, so the += needs no atomics).
__global__ __launch_bounds__(HIST_BLOCK) void leaf_update_compact_kernel(
    const int* __restrict__ rows0, const int* __restrict__ rows1,
    float* __restrict__ margin, const LeafJob* __restrict__ jobs,
    const int* __restrict__ block_job, long long col_stride) {
  const LeafJob job = jobs[block_job[blockIdx.x]];
  const int* src = job.parity ? rows1 : rows0;
  const int chunk = blockIdx.x - job.first_block;
  const long long step = (long long)job.num_blocks * blockDim.x;
  long long r = job.start + (long long)chunk * blockDim.x + threadIdx.x;
  constexpr int LROWS = 4;
  for (; r + (LROWS - 1) * step < job.end; r += LROWS * step) {
    int rid[LROWS];
    #pragma unroll
    for (int u = 0; u < LROWS; ++u) rid[u] = src[r + u * step];
    #pragma unroll
    for (int u = 0; u < LROWS; ++u) margin[(long long)rid[u] * col_stride] += job.value;
  }
  for (; r < job.end; r += step) {
    margin[(long long)src[r] * col_stride] += job.value;
  }
}

// Margin update by streaming traversal (full-data device-grown trees). Every
// row of the ORIGINAL bin matrix walks the finished tree's split heap with
// the partition's predicate and adds its leaf's value to its own margin
// cell: one coalesced pass over bins and margin, no row ids, no scatter and
// no partition of the deepest level. The add is the same float32 add of the
// same host-computed value the scatter does, so margins stay bit-identical.
//
// splits: the grower's [2^D - 1, 6] heap (gain, feature, split_bin,
// default_left, lg, lh); a node with gain <= 0 is a leaf, as in
// make_level_kernel. values: [2^(D+1) - 1] leaf values by heap index. Both
// are staged in LDS once per block (split records packed to two ints), so
// the row loop touches no float record.
//
// STAGED (u8 bins, nfeat % 4 == 0): each 256-row tile is copied into LDS
// with 16-B coalesced loads and traversed from there — a thread-per-row read
// of nfeat-byte rows would fetch with an nfeat-byte lane stride. The LDS
// byte reads have a lane stride of nfeat/4 dwords: conflict-free when that
// is odd (28 features -> 7). Otherwise rows are read in place.
#define TRAV_TILE 256

__device__ inline int traverse_step(int2 rec, int b, int missing_bin) {
  const bool left = (b == missing_bin) ? ((rec.y & 1) != 0) : (b <= (rec.y >> 1));
  return left ? 1 : 2;
}

template <typename BinT, bool STAGED>
__global__ __launch_bounds__(HIST_BLOCK) void leaf_update_traverse_kernel(
    const BinT* __restrict__ bins, const float* __restrict__ splits,
    const float* __restrict__ values, float* __restrict__ margin, long long n, int nfeat,
    int D, int missing_bin, long long col_stride) {
  extern __shared__ __align__(16) unsigned char trav_smem[];
  const int heap = (1 << D) - 1;
  const int nvals = 2 * heap + 1;
  int2* lnode = reinterpret_cast<int2*>(trav_smem);      // [heap]
  float* lval = reinterpret_cast<float*>(lnode + heap);  // [nvals]
  for (int h = threadIdx.x; h < heap; h += blockDim.x) {
    const float* sp = splits + h * 6;
    int2 rec = make_int2(-1, 0);
    // slots no row reaches hold whatever the split scan left there: keep
    // any feature outside the matrix from ever forming an address
    if (sp[0] > 0.0f && sp[1] >= 0.0f && sp[1] < (float)nfeat) {
      rec.x = (int)sp[1];
      rec.y = ((int)sp[2] << 1) | (sp[3] > 0.5f ? 1 : 0);
    }
    lnode[h] = rec;
  }
  for (int h = threadIdx.x; h < nvals; h += blockDim.x) lval[h] = values[h];
  __syncthreads();

  if (STAGED) {
    // tables take 16 * heap + 4 bytes; the tile starts on the next 16
    unsigned* ltile = reinterpret_cast<unsigned*>(trav_smem + 16 * (heap + 1));
    const unsigned char* lbytes = reinterpret_cast<const unsigned char*>(ltile);
    const int nd = nfeat >> 2;
    const long long ntiles = (n + TRAV_TILE - 1) / TRAV_TILE;
    for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
      const long long row0 = t * TRAV_TILE;
      const int tile_n = (int)min((long long)TRAV_TILE, n - row0);
      const long long r = row0 + threadIdx.x;
      float m = 0.f;
      if ((int)threadIdx.x < tile_n) m = margin[r * col_stride];  // in flight during the copy
      const unsigned char* src = reinterpret_cast<const unsigned char*>(bins) + row0 * nfeat;
      if (tile_n == TRAV_TILE) {
        const uint4* s4 = reinterpret_cast<const uint4*>(src);
        uint4* l4 = reinterpret_cast<uint4*>(ltile);
        for (int u = threadIdx.x; u < (TRAV_TILE >> 2) * nd; u += blockDim.x) l4[u] = s4[u];
      } else {
        const unsigned* s1 = reinterpret_cast<const unsigned*>(src);
        for (int u = threadIdx.x; u < tile_n * nd; u += blockDim.x) ltile[u] = s1[u];
      }
      __syncthreads();
      if ((int)threadIdx.x < tile_n) {
        const unsigned char* row = lbytes + (int)threadIdx.x * nfeat;
        int h = 0;
        for (int d = 0; d < D; ++d) {
          const int2 rec = lnode[h];
          if (rec.x < 0) break;
          h = 2 * h + traverse_step(rec, (int)row[rec.x], missing_bin);
        }
        margin[r * col_stride] = m + lval[h];
      }
      __syncthreads();
    }
  } else {
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += step) {
      const BinT* row = bins + r * nfeat;
      int h = 0;
      for (int d = 0; d < D; ++d) {
        const int2 rec = lnode[h];
        if (rec.x < 0) break;
        h = 2 * h + traverse_step(rec, (int)row[rec.x], missing_bin);
      }
      margin[r * col_stride] += lval[h];
    }
  }
}

// ---------------------------------------------------------------------------
// DEVICE-AUTONOMOUS depthwise grow (v3)
//
// The per-level host round-trip (drain -> python job packing -> launches)
// costs ~2-3 ms of a 7 ms round. v3 removes it: the whole tree's kernel
// sequence is enqueued up front; a tiny single-block `make_level` kernel
// builds the next level's node table and block-assignment prefixes ON
// DEVICE, hist/partition kernels walk virtual-block work lists found by
// binary search, and the host reads back ONE packed buffer per tree
// (split records + child counts + node sums) to build the tree object.
//
// Heap indexing: level d slot i lives at heap index (2^d - 1 + i);
// children of (d, i) are (d+1, 2i) and (d+1, 2i+1). Dead slots have
// start == end.
// ---------------------------------------------------------------------------

struct LevelNode {
  int start;
  int end;
  int build;  // 1 = histogram built from rows, 0 = derived by subtraction
};

// prefix tables for one level's virtual-block work distribution
struct LevelWork {
  int hist_total;   // total hist virtual blocks
  int part_total;   // total partition virtual blocks
};

#define GROW_MAX_SLOTS 1024  // max nodes per level for the device driver

// Single-block kernel: build level d+1's node table from level d's
// splits/counts, choose build children (smaller hessian), compute
// per-slot virtual-block counts + exclusive prefixes for hist & partition.
//
// filtered != 0: level d was NOT partitioned (its counts are zero). Both
// children of a live parent get the parent's own [start, end); the build
// child's histogram launch streams that range and keeps the rows the
// parent's split sends to its side (hist_device_kernel, FILTER), so its
// block count comes from the parent's row count.
__global__ __launch_bounds__(GROW_MAX_SLOTS) void make_level_kernel(
    const LevelNode* __restrict__ cur,    // [k] level d nodes
    const float* __restrict__ splits,     // [k, 6] level d split records
    const int* __restrict__ counts,       // [k, 2] level d partition counts
    const float* __restrict__ node_gh,    // [k, 2] level d node sums
    LevelNode* __restrict__ nxt,          // [2k] level d+1 nodes
    float* __restrict__ nxt_gh,           // [2k, 2]
    int* __restrict__ hist_prefix,        // [2k + 1]
    int* __restrict__ part_prefix,        // [2k + 1]
    LevelWork* __restrict__ work, int k, int rows_per_block, int max_blocks, int filtered) {
  __shared__ int h_counts[2 * GROW_MAX_SLOTS];
  __shared__ int p_counts[2 * GROW_MAX_SLOTS];
  const int tid = threadIdx.x;

  for (int i = tid; i < k; i += blockDim.x) {
    const float* sp = splits + i * 6;
    const LevelNode node = cur[i];
    LevelNode lft = {0, 0, 0}, rgt = {0, 0, 0};
    float lg = 0.f, lh = 0.f, rg = 0.f, rh = 0.f;
    if (node.end > node.start && sp[0] > 0.0f) {
      const int lc = filtered ? node.end - node.start : counts[i * 2];
      lft.start = node.start;
      lft.end = node.start + lc;
      rgt.start = filtered ? node.start : lft.end;
      rgt.end = node.end;
      lg = sp[4];
      lh = sp[5];
      rg = node_gh[i * 2] - lg;
      rh = node_gh[i * 2 + 1] - lh;
      // subtraction trick: build the smaller-hessian child
      if (lh <= rh) {
        lft.build = 1;
      } else {
        rgt.build = 1;
      }
    }
    nxt[2 * i] = lft;
    nxt[2 * i + 1] = rgt;
    nxt_gh[4 * i] = lg;
    nxt_gh[4 * i + 1] = lh;
    nxt_gh[4 * i + 2] = rg;
    nxt_gh[4 * i + 3] = rh;
    for (int c = 0; c < 2; ++c) {
      const LevelNode child = c ? rgt : lft;
      const int rows = child.end - child.start;
      h_counts[2 * i + c] =
          (child.build && rows > 0)
              ? (int)min((long long)(rows + rows_per_block - 1) / rows_per_block, (long long)max_blocks)
              : 0;
      p_counts[2 * i + c] =
          rows > 0 ? (int)min((long long)(rows + rows_per_block - 1) / rows_per_block,
                              (long long)max_blocks)
                   : 0;
    }
  }
  __syncthreads();
  if (tid == 0) {  // serial scan: 2k <= 2048 entries, negligible
    int hs = 0, ps = 0;
    for (int i = 0; i < 2 * k; ++i) {
      hist_prefix[i] = hs;
      part_prefix[i] = ps;
      hs += h_counts[i];
      ps += p_counts[i];
    }
    hist_prefix[2 * k] = hs;
    part_prefix[2 * k] = ps;
    work->hist_total = hs;
    work->part_total = ps;
  }
}

// Root bootstrap: one node covering [0, cap); also its hist job prefix.
__global__ void make_root_kernel(LevelNode* root, int* hist_prefix, int* part_prefix,
                                 LevelWork* work, int cap, int rows_per_block, int max_blocks) {
  root->start = 0;
  root->end = cap;
  root->build = 1;
  const int nb = (int)min((long long)(cap + rows_per_block - 1) / rows_per_block, (long long)max_blocks);
  hist_prefix[0] = 0;
  hist_prefix[1] = nb;
  part_prefix[0] = 0;
  part_prefix[1] = nb;
  work->hist_total = nb;
  work->part_total = nb;
}

// Interaction constraints on the device path. A node may only split on
// features that share a constraint set with every feature split on along
// its path; that path is known on device only. Allowed sets are bitsets
// (W = ceil(f/32) words per node, heap-indexed like `nodes`, root all ones):
//   allowed[child] = allowed[parent] & inter_union[parent's split feature]
// where inter_union[j] = {j} | (every constraint set containing j), built
// once on the host. One workgroup per slot of level d >= 1 writes the
// child's bitset and the level's [k, f] uint8 node mask (level-mask row AND
// allowed bit) that split_scan_kernel consumes with mask_per_node = 1.
// Every word and byte of the level is written (dead slots get zeros): the
// buffers are uninitialised between trees.
#define NODE_MASK_BLOCK 256

__global__ __launch_bounds__(NODE_MASK_BLOCK) void node_mask_kernel(
    const LevelNode* __restrict__ par_nodes,       // [k/2] level d-1 nodes
    const float* __restrict__ par_splits,          // [k/2, 6] level d-1 split records
    const unsigned* __restrict__ par_allowed,      // [k/2, W]
    const unsigned* __restrict__ inter_union,      // [f, W]
    const unsigned char* __restrict__ level_mask,  // [f] row of level d, or null
    unsigned* __restrict__ allowed,                // [k, W] level d bitsets
    unsigned char* __restrict__ node_mask,         // [k, f]
    int k, int f, int W) {
  const int slot = blockIdx.x;
  if (slot >= k) return;
  const int par = slot >> 1;
  const LevelNode pn = par_nodes[par];
  const float* sp = par_splits + par * 6;
  const int feat = (int)sp[1];
  // same liveness rule as make_level_kernel: the parent holds rows and split
  const bool live = pn.end > pn.start && sp[0] > 0.0f && feat >= 0 && feat < f;
  for (int j = threadIdx.x; j < f; j += blockDim.x) {
    const int w = j >> 5;
    const unsigned bits =
        live ? (par_allowed[(long long)par * W + w] & inter_union[(long long)feat * W + w]) : 0u;
    if ((j & 31) == 0) allowed[(long long)slot * W + w] = bits;
    const bool on = ((bits >> (j & 31)) & 1u) && (level_mask == nullptr || level_mask[j] != 0);
    node_mask[(long long)slot * f + j] = on ? 1 : 0;
  }
}

__device__ inline int find_slot(const int* __restrict__ prefix, int k, int vb) {
  int lo = 0, hi = k;  // find i with prefix[i] <= vb < prefix[i+1]
  while (lo + 1 < hi) {
    const int mid = (lo + hi) >> 1;
    if (prefix[mid] <= vb) {
      lo = mid;
    } else {
      hi = mid;
    }
  }
  return lo;
}

// hist over compact buffers driven by a device job table.
// BLOCK=256 pairs with grouped 56 KB slabs (2 blocks/CU); BLOCK=512 runs a
// SINGLE full-feature slab (up to ~158 KB, 1 block/CU — the same 8 waves,
// but bins/gh stream ONCE per row instead of once per feature group).
//
// FILTER (the deepest level when the level above it was not partitioned):
// nodes[slot] holds the PARENT's row range and par_splits the parent
// level's [k/2, 6] split records. Slot s accumulates only the rows the
// partition's own predicate would have moved to side (s & 1) of parent
// s >> 1, classified by one byte load per row. The same rows contribute the
// same fixed-point values as after a partition, so the sums are bit-equal.
//   PREDICATE: rows stay lane-consecutive; bin loads and atomics of the
//     other rows are predicated off. Every LDS atomic instruction still
//     issues with about half its lanes idle.
//   COMPACT: each wave classifies tiles of 64 consecutive rows, ballots and
//     queues the kept row indices in its own LDS queue behind the slab; once
//     4 x 64 rows wait they go through the 4-rows-in-flight loop with full
//     lanes. The wave walks the block-strided loop as a whole, so the
//     classify loads stay coalesced and the queued rows stay close together.
//     Needs HIST_QUEUE_ROWS ints per wave behind the slab (queue_ofs, in
//     u64 words); the host picks it only where that does not cost occupancy.
#define HIST_FILTER_OFF 0
#define HIST_FILTER_PREDICATE 1
#define HIST_FILTER_COMPACT 2
#define HIST_ROWS_IN_FLIGHT 4
// a wave classifies this many 64-row tiles per step, their byte loads all in
// flight together: with one load per step the 8 waves of a CU wait out the
// memory latency once per 64 rows
#define HIST_CLASSIFY_TILES 4
// one drain (4 x 64 rows) plus what a step can add to a queue just short of it
#define HIST_QUEUE_ROWS (HIST_ROWS_IN_FLIGHT * 64 + HIST_CLASSIFY_TILES * 64)
static_assert(HIST_CLASSIFY_TILES <= HIST_ROWS_IN_FLIGHT,
              "one drain per step must bring the queue back under a drain's worth");

__device__ inline bool hist_row_kept(int b, int missing_bin, int split_bin, bool default_left,
                                     bool want_left) {
  const bool left = (b == missing_bin) ? default_left : (b <= split_bin);
  return left == want_left;
}

// 4 bins per dword load (rows are 4-aligned when nfeat % 4 == 0);
// HIST_ROWS_IN_FLIGHT rows per lane in flight so the gathers overlap
template <typename BinT, bool PRED>
__device__ inline void hist_add_rows_vec4(unsigned long long* lhist, int hofs,
                                          const BinT* __restrict__ bins_c,
                                          const float2* __restrict__ gh_c,
                                          const long long (&ru)[HIST_ROWS_IN_FLIGHT],
                                          const bool (&keep)[HIST_ROWS_IN_FLIGHT], int nfeat,
                                          int fg_start, int nd, int stride, float scale_g,
                                          float scale_h) {
  constexpr int HROWS = HIST_ROWS_IN_FLIGHT;
  unsigned long long gf[HROWS], hf[HROWS];
  const uchar4* rp[HROWS];
  #pragma unroll
  for (int u = 0; u < HROWS; ++u) {
    const float2 gp = gh_c[ru[u]];
    gf[u] = (unsigned long long)(long long)llrintf(gp.x * scale_g);
    hf[u] = (unsigned long long)(long long)llrintf(gp.y * scale_h);
    rp[u] = reinterpret_cast<const uchar4*>(bins_c + ru[u] * nfeat + fg_start);
  }
  #pragma unroll 2
  for (int f4 = 0; f4 < nd; ++f4) {
    const int base = (f4 << 2) * stride;
    uchar4 b4[HROWS];
    #pragma unroll
    for (int u = 0; u < HROWS; ++u) {
      if (!PRED || keep[u]) b4[u] = rp[u][f4];
    }
    #pragma unroll
    for (int u = 0; u < HROWS; ++u) {
      if (PRED && !keep[u]) continue;
      const int s0 = lds_pad_slot(base + (int)b4[u].x);
      const int s1 = lds_pad_slot(base + stride + (int)b4[u].y);
      const int s2 = lds_pad_slot(base + 2 * stride + (int)b4[u].z);
      const int s3 = lds_pad_slot(base + 3 * stride + (int)b4[u].w);
      atomicAdd(&lhist[s0], gf[u]);
      atomicAdd(&lhist[hofs + s0], hf[u]);
      atomicAdd(&lhist[s1], gf[u]);
      atomicAdd(&lhist[hofs + s1], hf[u]);
      atomicAdd(&lhist[s2], gf[u]);
      atomicAdd(&lhist[hofs + s2], hf[u]);
      atomicAdd(&lhist[s3], gf[u]);
      atomicAdd(&lhist[hofs + s3], hf[u]);
    }
  }
}

// one row per lane: the tail of a range, and every row of a scalar-loop slab
template <typename BinT>
__device__ inline void hist_add_row(unsigned long long* lhist, int hofs,
                                    const BinT* __restrict__ bins_c,
                                    const float2* __restrict__ gh_c, long long r, bool vec4,
                                    int nfeat, int fg_start, int nf_group, int stride,
                                    float scale_g, float scale_h) {
  const float2 gp = gh_c[r];
  const unsigned long long gfix = (unsigned long long)(long long)llrintf(gp.x * scale_g);
  const unsigned long long hfix = (unsigned long long)(long long)llrintf(gp.y * scale_h);
  const BinT* rp = bins_c + r * nfeat + fg_start;
  if (vec4) {
    const uchar4* rp4 = reinterpret_cast<const uchar4*>(rp);
    #pragma unroll 2
    for (int f4 = 0; f4 < (nf_group >> 2); ++f4) {
      const uchar4 b4 = rp4[f4];
      const int base = (f4 << 2) * stride;
      const int s0 = lds_pad_slot(base + (int)b4.x);
      const int s1 = lds_pad_slot(base + stride + (int)b4.y);
      const int s2 = lds_pad_slot(base + 2 * stride + (int)b4.z);
      const int s3 = lds_pad_slot(base + 3 * stride + (int)b4.w);
      atomicAdd(&lhist[s0], gfix);
      atomicAdd(&lhist[hofs + s0], hfix);
      atomicAdd(&lhist[s1], gfix);
      atomicAdd(&lhist[hofs + s1], hfix);
      atomicAdd(&lhist[s2], gfix);
      atomicAdd(&lhist[hofs + s2], hfix);
      atomicAdd(&lhist[s3], gfix);
      atomicAdd(&lhist[hofs + s3], hfix);
    }
    return;
  }
  #pragma unroll 4
  for (int f = 0; f < nf_group; ++f) {
    const int slot2 = lds_pad_slot(f * stride + (int)rp[f]);
    atomicAdd(&lhist[slot2], gfix);
    atomicAdd(&lhist[hofs + slot2], hfix);
  }
}

// queue writes of some lanes are read by other lanes of the same wave
__device__ inline void hist_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

template <typename BinT, int BLOCK, int FILTER>
__global__ __launch_bounds__(BLOCK) void hist_device_kernel(
    const BinT* __restrict__ bins_c, const float2* __restrict__ gh_c,
    const LevelNode* __restrict__ nodes, const int* __restrict__ hist_prefix,
    const LevelWork* __restrict__ work, unsigned long long* __restrict__ out,
    int k, int nfeat, int stride, int n_groups, int feats_per_group,
    const float* __restrict__ gh_max, int rows_per_block, int slot_lo, int slot_hi,
    const float* __restrict__ par_splits, int missing_bin, int queue_ofs) {
  extern __shared__ unsigned long long lhist[];
  constexpr int HROWS = HIST_ROWS_IN_FLIGHT;
  const float scale_g = 8589934592.0f / fmaxf(gh_max[0], 1e-30f);
  const float scale_h = 8589934592.0f / fmaxf(gh_max[1], 1e-30f);
  const int total = work->hist_total * n_groups;

  for (int vb = blockIdx.x; vb < total; vb += gridDim.x) {
    const int fg = vb % n_groups;
    const int hvb = vb / n_groups;
    const int slot = find_slot(hist_prefix, k, hvb);
    if (slot < slot_lo || slot >= slot_hi) continue;  // comm-overlap slot window
    const int chunk = hvb - hist_prefix[slot];
    const int nb = hist_prefix[slot + 1] - hist_prefix[slot];
    const LevelNode node = nodes[slot];
    int flt_feat = 0, flt_bin = 0;
    bool flt_dl = false;
    const bool flt_left = (slot & 1) == 0;
    if (FILTER != HIST_FILTER_OFF) {
      const float* sp = par_splits + (slot >> 1) * 6;
      flt_feat = (int)sp[1];
      flt_bin = (int)sp[2];
      flt_dl = sp[3] > 0.5f;
      // a slot has blocks only under a live parent, whose feature is valid;
      // never form an address from anything else
      if (flt_feat < 0 || flt_feat >= nfeat) continue;
    }
    const int fg_start = fg * feats_per_group;
    const int nf_group = min(feats_per_group, nfeat - fg_start);
    const int lds_words = nf_group * stride * 2;
    const int hofs = (int)lds_half_words(nf_group * stride);
    const int lds_padded = 2 * hofs;

    for (int i = threadIdx.x; i < lds_padded; i += blockDim.x) lhist[i] = 0ull;
    __syncthreads();

    const long long step = (long long)nb * blockDim.x;
    const bool vec4 = sizeof(BinT) == 1 && (nf_group & 3) == 0 && (nfeat & 3) == 0 &&
                      (fg_start & 3) == 0;
    const int nd = nf_group >> 2;
    long long r = node.start + (long long)chunk * blockDim.x + threadIdx.x;
    if (FILTER == HIST_FILTER_COMPACT) {
      int* queue =
          reinterpret_cast<int*>(lhist + queue_ofs) + (threadIdx.x >> 6) * HIST_QUEUE_ROWS;
      const int lane = threadIdx.x & 63;
      const bool all_true[HROWS] = {true, true, true, true};
      int qn = 0;  // the same in every lane: it only adds ballot counts
      constexpr int CT = HIST_CLASSIFY_TILES;
      for (long long r0 = r - lane; r0 < node.end; r0 += CT * step) {
        int b[CT];
        #pragma unroll
        for (int c = 0; c < CT; ++c) {
          const long long rr = r0 + c * step + lane;
          b[c] = rr < node.end ? (int)bins_c[rr * nfeat + flt_feat] : 0;
        }
        #pragma unroll
        for (int c = 0; c < CT; ++c) {
          const long long rr = r0 + c * step + lane;
          const bool kept =
              rr < node.end && hist_row_kept(b[c], missing_bin, flt_bin, flt_dl, flt_left);
          const unsigned long long m = __ballot(kept);
          if (kept) queue[qn + __popcll(m & ((1ull << lane) - 1ull))] = (int)rr;
          qn += __popcll(m);
        }
        hist_wave_sync();
        // at most 4 x 64 - 1 rows waited and CT x 64 came: one drain leaves
        // fewer than 4 x 64 again
        if (qn >= HROWS * 64) {
          qn -= HROWS * 64;  // the newest rows: nothing has to move down
          long long ru[HROWS];
          #pragma unroll
          for (int u = 0; u < HROWS; ++u) ru[u] = queue[qn + u * 64 + lane];
          if (vec4) {
            hist_add_rows_vec4<BinT, false>(lhist, hofs, bins_c, gh_c, ru, all_true, nfeat,
                                            fg_start, nd, stride, scale_g, scale_h);
          } else {
            #pragma unroll
            for (int u = 0; u < HROWS; ++u)
              hist_add_row<BinT>(lhist, hofs, bins_c, gh_c, ru[u], false, nfeat, fg_start,
                                 nf_group, stride, scale_g, scale_h);
          }
          hist_wave_sync();
        }
      }
      // what is left (fewer than 4 x 64 rows) goes through the same loop;
      // only its last 64-row batch runs with idle lanes
      if (vec4 && qn > 0) {
        long long ru[HROWS];
        bool keep[HROWS];
        #pragma unroll
        for (int u = 0; u < HROWS; ++u) {
          keep[u] = u * 64 + lane < qn;
          ru[u] = keep[u] ? queue[u * 64 + lane] : node.start;
        }
        hist_add_rows_vec4<BinT, true>(lhist, hofs, bins_c, gh_c, ru, keep, nfeat, fg_start, nd,
                                       stride, scale_g, scale_h);
      } else {
        for (int i = lane; i < qn; i += 64)
          hist_add_row<BinT>(lhist, hofs, bins_c, gh_c, (long long)queue[i], false, nfeat,
                             fg_start, nf_group, stride, scale_g, scale_h);
      }
    } else {
      if (vec4) {
        for (; r + (HROWS - 1) * step < node.end; r += HROWS * step) {
          long long ru[HROWS];
          bool keep[HROWS];
          #pragma unroll
          for (int u = 0; u < HROWS; ++u) {
            ru[u] = r + u * step;
            keep[u] = FILTER == HIST_FILTER_OFF ||
                      hist_row_kept((int)bins_c[ru[u] * nfeat + flt_feat], missing_bin, flt_bin,
                                    flt_dl, flt_left);
          }
          hist_add_rows_vec4<BinT, FILTER != HIST_FILTER_OFF>(lhist, hofs, bins_c, gh_c, ru, keep,
                                                              nfeat, fg_start, nd, stride, scale_g,
                                                              scale_h);
        }
      }
      for (; r < node.end; r += step) {
        if (FILTER != HIST_FILTER_OFF &&
            !hist_row_kept((int)bins_c[r * nfeat + flt_feat], missing_bin, flt_bin, flt_dl,
                           flt_left))
          continue;
        hist_add_row<BinT>(lhist, hofs, bins_c, gh_c, r, vec4, nfeat, fg_start, nf_group, stride,
                           scale_g, scale_h);
      }
    }
    __syncthreads();
    unsigned long long* gout =
        out + ((long long)slot * nfeat + fg_start) * (long long)stride * 2;
    for (int i = threadIdx.x; i < lds_words; i += blockDim.x) {
      const int pair = i >> 1;
      const int idx = lds_pad_slot(pair) + ((i & 1) ? hofs : 0);
      const unsigned long long v = lhist[idx];
      if (v) atomicAdd(&gout[i], v);
    }
    __syncthreads();
  }
}

// convert built slots (int64 acc -> f32 heap) and fill node sums from the
// feature-0 bin range; one block per (slot, chunk of slots_total)
__global__ __launch_bounds__(HIST_BLOCK) void convert_level_kernel(
    const unsigned long long* __restrict__ acc, float* __restrict__ hist_f32,
    const LevelNode* __restrict__ nodes, int k, long long slots2,
    const float* __restrict__ gh_max) {
  const double inv_g = (double)fmaxf(gh_max[0], 1e-30f) / 8589934592.0;
  const double inv_h = (double)fmaxf(gh_max[1], 1e-30f) / 8589934592.0;
  for (long long u = (long long)blockIdx.x * blockDim.x + threadIdx.x; u < (long long)k * slots2;
       u += (long long)gridDim.x * blockDim.x) {
    const int slot = (int)(u / slots2);
    if (!nodes[slot].build || nodes[slot].end <= nodes[slot].start) continue;
    const long long j = u - (long long)slot * slots2;
    const double inv = (j & 1) ? inv_h : inv_g;
    hist_f32[u] = (float)((double)(long long)acc[u] * inv);
  }
}

// derived slots: hist = parent - sibling (all f32, same heap layout);
// also node sums for EVERY alive slot from the feature-0 bins
__global__ __launch_bounds__(HIST_BLOCK) void derive_level_kernel(
    float* __restrict__ level_hist, const float* __restrict__ parent_hist,
    const LevelNode* __restrict__ nodes, int k, long long slots2) {
  for (long long u = (long long)blockIdx.x * blockDim.x + threadIdx.x; u < (long long)k * slots2;
       u += (long long)gridDim.x * blockDim.x) {
    const int slot = (int)(u / slots2);
    const LevelNode node = nodes[slot];
    if (node.build || node.end <= node.start) continue;
    const long long j = u - (long long)slot * slots2;
    const int sib = slot ^ 1;
    const int parent = slot >> 1;
    level_hist[u] = parent_hist[(long long)parent * slots2 + j] -
                    level_hist[(long long)sib * slots2 + j];
  }
}

// partition driven by the device job table (virtual blocks)
template <typename BinT>
__global__ __launch_bounds__(HIST_BLOCK) void partition_device_kernel(
    const BinT* __restrict__ src_bins, const float2* __restrict__ src_gh,
    const int* __restrict__ src_rows, BinT* __restrict__ dst_bins,
    float2* __restrict__ dst_gh, int* __restrict__ dst_rows,
    const LevelNode* __restrict__ nodes, const int* __restrict__ part_prefix,
    const LevelWork* __restrict__ work, const float* __restrict__ split_packed,
    int* __restrict__ counters, int k, int nfeat, int missing_bin,
    int copy_payload, int copy_rows) {
  __shared__ int ldest[CPART_TILE];
  __shared__ int lcnt, rcnt, lbase, rbase;
  const int total = work->part_total;

  for (int vb = blockIdx.x; vb < total; vb += gridDim.x) {
    const int slot = find_slot(part_prefix, k, vb);
    const LevelNode node = nodes[slot];
    const float* sp6 = split_packed + slot * 6;
    if (sp6[0] <= 0.0f || node.end <= node.start) continue;
    const int feature = (int)sp6[1];
    const int split_bin = (int)sp6[2];
    const int default_left = sp6[3] > 0.5f ? 1 : 0;
    const int chunk = vb - part_prefix[slot];
    const int nb = part_prefix[slot + 1] - part_prefix[slot];
    const long long tile_step = (long long)nb * CPART_TILE;

    for (long long tile = node.start + (long long)chunk * CPART_TILE; tile < node.end;
         tile += tile_step) {
      if (threadIdx.x == 0) {
        lcnt = 0;
        rcnt = 0;
      }
      __syncthreads();
      const int tile_n = (int)min((long long)CPART_TILE, node.end - tile);
      for (int i = threadIdx.x; i < tile_n; i += blockDim.x) {
        const int b = (int)src_bins[(tile + i) * (long long)nfeat + feature];
        const bool left = (b == missing_bin) ? (default_left != 0) : (b <= split_bin);
        ldest[i] = left ? atomicAdd(&lcnt, 1) : ~atomicAdd(&rcnt, 1);
      }
      __syncthreads();
      if (threadIdx.x == 0) {
        lbase = atomicAdd(&counters[slot * 2], lcnt);
        rbase = atomicAdd(&counters[slot * 2 + 1], rcnt);
      }
      __syncthreads();
      // the deepest level's partition only feeds leaf_update (row ids +
      // counts): bins/gh copies are skipped there (copy_payload == 0),
      // dropping ~90% of that level's partition traffic.
      if (copy_payload && (nfeat & 3) == 0 && sizeof(BinT) == 1) {
        const int nd = nfeat >> 2;
        int log2p = 0;
        while ((1 << log2p) < nd) ++log2p;
        const int mask = (1 << log2p) - 1;
        const uchar4* sb4 = reinterpret_cast<const uchar4*>(src_bins);
        uchar4* db4 = reinterpret_cast<uchar4*>(dst_bins);
        for (int u = threadIdx.x; u < (tile_n << log2p); u += blockDim.x) {
          const int i = u >> log2p;
          const int f4 = u & mask;
          if (f4 >= nd) continue;
          const int d = ldest[i];
          const long long dst =
              d >= 0 ? (long long)node.start + lbase + d : (long long)node.end - 1 - rbase - (~d);
          db4[dst * nd + f4] = sb4[(tile + i) * (long long)nd + f4];
        }
      } else if (copy_payload) {
        int log2p = 0;
        while ((1 << log2p) < nfeat) ++log2p;
        const int mask = (1 << log2p) - 1;
        for (int u = threadIdx.x; u < (tile_n << log2p); u += blockDim.x) {
          const int i = u >> log2p;
          const int f = u & mask;
          if (f >= nfeat) continue;
          const int d = ldest[i];
          const long long dst =
              d >= 0 ? (long long)node.start + lbase + d : (long long)node.end - 1 - rbase - (~d);
          dst_bins[dst * (long long)nfeat + f] = src_bins[(tile + i) * (long long)nfeat + f];
        }
      }
      if (copy_payload) {
        for (int u = threadIdx.x; u < tile_n * 2; u += blockDim.x) {
          const int i = u >> 1;
          const int half = u & 1;
          const int d = ldest[i];
          const long long dst =
              d >= 0 ? (long long)node.start + lbase + d : (long long)node.end - 1 - rbase - (~d);
          reinterpret_cast<float*>(dst_gh)[dst * 2 + half] =
              reinterpret_cast<const float*>(src_gh)[(tile + i) * 2 + half];
        }
      }
      // row ids feed the leaf scatter only: a tree whose margins are updated
      // by traversal never reads them (copy_rows == 0)
      if (copy_rows) {
        for (int i = threadIdx.x; i < tile_n; i += blockDim.x) {
          const int d = ldest[i];
          const long long dst =
              d >= 0 ? (long long)node.start + lbase + d : (long long)node.end - 1 - rbase - (~d);
          dst_rows[dst] = src_rows[tile + i];
        }
      }
      __syncthreads();
    }
  }
}

// Single-read partition: every tile's payload is loaded ONCE into registers,
// classified from the register that holds the split feature's byte, and
// stored from those registers after the tile's two global atomics. The
// classic kernel re-reads the whole tile for the copy; at the flagship shape
// ~15 MB of tiles are live per XCD between the two reads (3.5x its L2), so
// the second read goes to memory again.
//
// Lane mapping: 8 lanes per row, lane `sub` holds dword `sub` of the row
// (nd = nfeat/4 <= 8; lanes sub >= nd idle, as in the classic copy loop), a
// pass covers BLOCK/8 rows and a lane holds R passes: TILE = R * BLOCK / 8.
// gh (and the row id with ROWS) of tile row g*BLOCK + tid sit in lane tid.
// Source addresses are a block-uniform tile base plus one 32-bit lane
// offset; the passes differ by a uniform step, so no per-load address lives
// in VGPRs. u8 bins, nfeat % 4 == 0, nfeat <= 32, payload always copied.
template <int BLOCK, int R, bool ROWS, bool FULL>
__device__ __forceinline__ void partition_staged_tile(
    const unsigned* __restrict__ sb, const float2* __restrict__ sgh,
    const int* __restrict__ srows, unsigned* __restrict__ db, float2* __restrict__ dgh,
    int* __restrict__ drows, int* ldest, int* lcnt, int* rcnt, int* lbase, int* rbase,
    int* __restrict__ counter, long long left0, long long right0, int tile_n, int nd,
    int fdw, int fsh, int split_bin, int missing_bin, bool default_left) {
  constexpr int RPP = BLOCK / 8;
  constexpr int G = R / 8;
  const int sub = threadIdx.x & 7;
  const int rlane = threadIdx.x >> 3;
  const unsigned lane_off = (unsigned)(rlane * nd + sub);
  const int pass_step = RPP * nd;
  unsigned v[R];
  float2 gh[G];
  int rid[G];
  // 1. the whole tile, loads issued back to back
  // (a tail tile leaves the registers of rows past its end at zero)
  if (sub < nd) {
#pragma unroll
    for (int j = 0; j < R; ++j) {
      v[j] = 0u;
      if (FULL || j * RPP + rlane < tile_n) v[j] = (sb + (long long)j * pass_step)[lane_off];
    }
  }
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int i = g * BLOCK + (int)threadIdx.x;
    gh[g] = make_float2(0.f, 0.f);
    rid[g] = 0;
    if (FULL || i < tile_n) {
      gh[g] = sgh[i];
      if (ROWS) rid[g] = srows[i];
    }
  }
  // 2. classify from the register holding the split feature's byte
  if (sub == fdw) {
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int i = j * RPP + rlane;
      if (FULL || i < tile_n) {
        const int b = (int)((v[j] >> fsh) & 0xffu);
        const bool left = (b == missing_bin) ? default_left : (b <= split_bin);
        ldest[i] = left ? atomicAdd(lcnt, 1) : ~atomicAdd(rcnt, 1);
      }
    }
  }
  __syncthreads();
  // 3. one returning global atomic per side; the LDS counters are zeroed
  // for the next tile here (nothing touches them before the closing barrier)
  if (threadIdx.x == 0) {
    *lbase = atomicAdd(&counter[0], *lcnt);
    *rbase = atomicAdd(&counter[1], *rcnt);
    *lcnt = 0;
    *rcnt = 0;
  }
  __syncthreads();
  // 4. store the registers; destinations are computed just before each store
  const long long lb = left0 + *lbase;
  const long long rb = right0 - *rbase;
  if (sub < nd) {
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int i = j * RPP + rlane;
      if (FULL || i < tile_n) {
        const int d = ldest[i];
        const long long dst = d >= 0 ? lb + d : rb - (~d);
        db[dst * nd + sub] = v[j];
      }
    }
  }
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int i = g * BLOCK + (int)threadIdx.x;
    if (FULL || i < tile_n) {
      const int d = ldest[i];
      const long long dst = d >= 0 ? lb + d : rb - (~d);
      dgh[dst] = gh[g];
      if (ROWS) drows[dst] = rid[g];
    }
  }
  __syncthreads();
}

template <int BLOCK, int R, bool ROWS>
__global__ __launch_bounds__(BLOCK) void partition_device_staged_kernel(
    const unsigned char* __restrict__ src_bins, const float2* __restrict__ src_gh,
    const int* __restrict__ src_rows, unsigned char* __restrict__ dst_bins,
    float2* __restrict__ dst_gh, int* __restrict__ dst_rows,
    const LevelNode* __restrict__ nodes, const int* __restrict__ part_prefix,
    const LevelWork* __restrict__ work, const float* __restrict__ split_packed,
    int* __restrict__ counters, int k, int nfeat, int missing_bin) {
  constexpr int TILE = R * BLOCK / 8;
  __shared__ int ldest[TILE];
  __shared__ int lcnt, rcnt, lbase, rbase;
  const int total = work->part_total;
  const int nd = nfeat >> 2;
  if (threadIdx.x == 0) {
    lcnt = 0;
    rcnt = 0;
  }
  __syncthreads();

  for (int vb = blockIdx.x; vb < total; vb += gridDim.x) {
    const int slot = find_slot(part_prefix, k, vb);
    const LevelNode node = nodes[slot];
    const float* sp6 = split_packed + slot * 6;
    if (sp6[0] <= 0.0f || node.end <= node.start) continue;
    const int feature = (int)sp6[1];
    const int split_bin = (int)sp6[2];
    const bool default_left = sp6[3] > 0.5f;
    const int fdw = feature >> 2;
    const int fsh = (feature & 3) * 8;
    const int chunk = vb - part_prefix[slot];
    const int nb = part_prefix[slot + 1] - part_prefix[slot];
    const long long tile_step = (long long)nb * TILE;
    unsigned* db = reinterpret_cast<unsigned*>(dst_bins);

    for (long long tile = node.start + (long long)chunk * TILE; tile < node.end;
         tile += tile_step) {
      // tile < node.end, so both fit an int
      const int tile_n = min(TILE, node.end - (int)tile);
      const unsigned* sb = reinterpret_cast<const unsigned*>(src_bins) + tile * nd;
      if (tile_n == TILE) {
        partition_staged_tile<BLOCK, R, ROWS, true>(
            sb, src_gh + tile, src_rows + tile, db, dst_gh, dst_rows, ldest, &lcnt, &rcnt,
            &lbase, &rbase, counters + slot * 2, node.start, (long long)node.end - 1, tile_n,
            nd, fdw, fsh, split_bin, missing_bin, default_left);
      } else {
        partition_staged_tile<BLOCK, R, ROWS, false>(
            sb, src_gh + tile, src_rows + tile, db, dst_gh, dst_rows, ldest, &lcnt, &rcnt,
            &lbase, &rbase, counters + slot * 2, node.start, (long long)node.end - 1, tile_n,
            nd, fdw, fsh, split_bin, missing_bin, default_left);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// split-gain scan
//
// Kernel A: one 256-thread workgroup per (node, feature): inclusive scan of
// the feature's bin histogram in LDS, gain for every split position in both
// missing directions, block-reduce to the feature's best candidate.
// Kernel B: one workgroup per node reduces over features.
// Replaces ~30 small torch kernels + 6 D2H syncs per level.
// ---------------------------------------------------------------------------

struct SplitCand {
  float gain;
  int bin;
  int dir;  // 1 = missing left
  float left_g;
  float left_h;
};

__device__ inline float split_score(float g, float h, float alpha, float lam) {
  float ag = fabsf(g) - alpha;
  ag = ag > 0.f ? ag : 0.f;
  return ag * ag / (h + lam);
}

__device__ inline float split_weight(float g, float h, float alpha, float lam) {
  float ag = fabsf(g) - alpha;
  ag = ag > 0.f ? ag : 0.f;
  return -copysignf(ag, g) / (h + lam);
}

#define SPLIT_BLOCK 256

__global__ __launch_bounds__(SPLIT_BLOCK) void split_scan_kernel(
    const float* __restrict__ hist,      // [k, f, stride, 2]
    const float2* __restrict__ parent,   // [k]
    const int* __restrict__ nbins,       // [f]
    const unsigned char* __restrict__ feat_mask,  // [k*f], [f] or null
    const signed char* __restrict__ monotone,     // [f] or null
    SplitCand* __restrict__ out,         // [k, f]
    int k, int f, int stride, int has_missing, int mask_per_node,
    float reg_lambda, float reg_alpha, float gamma_, float min_child_weight) {
  __shared__ float sg[SPLIT_BLOCK];
  __shared__ float sh[SPLIT_BLOCK];
  __shared__ float red_gain[SPLIT_BLOCK / WAVE];
  __shared__ int red_idx[SPLIT_BLOCK / WAVE];

  const int node = blockIdx.x / f;
  const int feat = blockIdx.x % f;
  const int tid = threadIdx.x;
  SplitCand best = {-1.0f, -1, 0, 0.f, 0.f};

  bool masked = false;
  if (feat_mask != nullptr) {
    masked = feat_mask[mask_per_node ? (node * f + feat) : feat] == 0;
  }
  const int nb = nbins[feat];  // real bins
  if (!masked && nb >= 2 && nb <= SPLIT_BLOCK) {
    const float* hbase = hist + (((long long)node * f + feat) * stride) * 2;
    const float2 psum = parent[node];

    // load + inclusive block scan of real bins (nb <= 256)
    float g = 0.f, h = 0.f;
    if (tid < nb) {
      g = hbase[tid * 2];
      h = hbase[tid * 2 + 1];
    }
    // scan in LDS (Hillis-Steele; nb small)
    sg[tid] = g;
    sh[tid] = h;
    __syncthreads();
    for (int ofs = 1; ofs < nb; ofs <<= 1) {
      float ag = 0.f, ah = 0.f;
      if (tid >= ofs) {
        ag = sg[tid - ofs];
        ah = sh[tid - ofs];
      }
      __syncthreads();
      sg[tid] += ag;
      sh[tid] += ah;
      __syncthreads();
    }

    float miss_g = 0.f, miss_h = 0.f;
    if (has_missing) {
      miss_g = hbase[(stride - 1) * 2];
      miss_h = hbase[(stride - 1) * 2 + 1];
    }
    const float parent_score = split_score(psum.x, psum.y, reg_alpha, reg_lambda);
    const int cons = (monotone != nullptr) ? (int)monotone[feat] : 0;

    // split after bin j valid for j in [0, nb-2]
    if (tid <= nb - 2) {
      const float gl0 = sg[tid];
      const float hl0 = sh[tid];
      for (int dir = 0; dir < 2; ++dir) {
        const float gl = gl0 + (dir ? miss_g : 0.f);
        const float hl = hl0 + (dir ? miss_h : 0.f);
        const float gr = psum.x - gl;
        const float hr = psum.y - hl;
        if (hl < min_child_weight || hr < min_child_weight) continue;
        if (cons != 0) {
          const float wl = split_weight(gl, hl, reg_alpha, reg_lambda);
          const float wr = split_weight(gr, hr, reg_alpha, reg_lambda);
          if ((cons > 0 && wl > wr) || (cons < 0 && wl < wr)) continue;
        }
        const float gain =
            0.5f * (split_score(gl, hl, reg_alpha, reg_lambda) +
                    split_score(gr, hr, reg_alpha, reg_lambda) - parent_score) - gamma_;
        if (gain > best.gain) {
          best = {gain, tid, dir, gl, hl};
        }
      }
    }
  }
  __syncthreads();

  // block argmax reduce over candidates (pack gain+lane via wave shuffle)
  float bg = best.gain;
  int bidx = tid;
  for (int ofs = WAVE / 2; ofs > 0; ofs >>= 1) {
    const float og = __shfl_down(bg, ofs);
    const int oi = __shfl_down(bidx, ofs);
    if (og > bg) {
      bg = og;
      bidx = oi;
    }
  }
  const int wid = tid / WAVE;
  if ((tid & (WAVE - 1)) == 0) {
    red_gain[wid] = bg;
    red_idx[wid] = bidx;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < SPLIT_BLOCK / WAVE; ++w) {
      if (red_gain[w] > red_gain[0]) {
        red_gain[0] = red_gain[w];
        red_idx[0] = red_idx[w];
      }
    }
  }
  __syncthreads();
  // winning thread writes its candidate
  if (tid == red_idx[0] && best.gain == red_gain[0]) {
    out[(long long)node * f + feat] = best;
  }
}

__global__ __launch_bounds__(SPLIT_BLOCK) void split_reduce_kernel(
    const SplitCand* __restrict__ cands,  // [k, f]
    float* __restrict__ out,              // [k, 6]: gain, feat, bin, dir, lg, lh
    int k, int f) {
  __shared__ float rg[SPLIT_BLOCK / WAVE];
  __shared__ int ri[SPLIT_BLOCK / WAVE];
  const int node = blockIdx.x;
  const int tid = threadIdx.x;
  float bg = -1.0f;
  int bf = -1;
  for (int j = tid; j < f; j += blockDim.x) {
    const float gn = cands[(long long)node * f + j].gain;
    if (gn > bg) {
      bg = gn;
      bf = j;
    }
  }
  for (int ofs = WAVE / 2; ofs > 0; ofs >>= 1) {
    const float og = __shfl_down(bg, ofs);
    const int of_ = __shfl_down(bf, ofs);
    if (og > bg) {
      bg = og;
      bf = of_;
    }
  }
  const int wid = tid / WAVE;
  if ((tid & (WAVE - 1)) == 0) {
    rg[wid] = bg;
    ri[wid] = bf;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < SPLIT_BLOCK / WAVE; ++w) {
      if (rg[w] > rg[0]) {
        rg[0] = rg[w];
        ri[0] = ri[w];
      }
    }
    float* o = out + node * 6;
    if (ri[0] < 0 || rg[0] <= 0.f) {
      o[0] = -1.0f;
      o[1] = -1.f;
      o[2] = -1.f;
      o[3] = 0.f;
      o[4] = 0.f;
      o[5] = 0.f;
    } else {
      const SplitCand c = cands[(long long)node * f + ri[0]];
      o[0] = c.gain;
      o[1] = (float)ri[0];
      o[2] = (float)c.bin;
      o[3] = (float)c.dir;
      o[4] = c.left_g;
      o[5] = c.left_h;
    }
  }
}

// ---------------------------------------------------------------------------
// categorical split search (ops/torch_ref.py find_splits states the rule)
// ---------------------------------------------------------------------------
//
// One workgroup per (node, categorical feature); thread t owns category t of
// the feature's histogram (bin = category code, at most 255 of them). A
// candidate is a set R of categories that go right:
//   one-hot (nbins < max_cat_to_onehot): thread t proposes R = {t};
//   partition: the non-empty categories are bitonic-sorted in LDS by
//   (g / (h + lambda), category), empty and out-of-range lanes last; after
//   a Hillis-Steele scan of the sorted sums thread t proposes the cut after
//   p = t + 1 sorted categories, R being the shorter side.
// Both missing directions are tried, the block argmax keeps the lowest
// candidate among equal gains, the winner writes the feature's SplitCand
// (bin 0) and the block writes the winner's R to cand_bits[node, feat, :]
// with one ballot per wave. No atomics; every output word has one writer.
// split_scan_kernel has been launched before with these features masked
// (gain -1 candidates), split_reduce_kernel runs after over all features.
__global__ __launch_bounds__(SPLIT_BLOCK) void split_scan_cat_kernel(
    const float* __restrict__ hist,      // [k, f, stride, 2]
    const float2* __restrict__ parent,   // [k]
    const int* __restrict__ nbins,       // [f]
    const int* __restrict__ cat_feats,   // [n_cat] indices of the categorical features
    const unsigned char* __restrict__ feat_mask,  // [k*f], [f] or null
    SplitCand* __restrict__ out,         // [k, f]
    unsigned int* __restrict__ cand_bits,  // [k, f, CAT_WORDS]
    int k, int f, int n_cat, int stride, int has_missing, int mask_per_node,
    float reg_lambda, float reg_alpha, float gamma_, float min_child_weight,
    int max_cat_to_onehot, int max_cat_threshold) {
  __shared__ float sg[SPLIT_BLOCK];
  __shared__ float sh[SPLIT_BLOCK];
  __shared__ float skey[SPLIT_BLOCK];
  __shared__ int scat[SPLIT_BLOCK];   // category of a sorted position; bit 8: empty
  __shared__ int srank[SPLIT_BLOCK];  // sorted position of a category
  __shared__ float red_gain[SPLIT_BLOCK / WAVE];
  __shared__ int red_idx[SPLIT_BLOCK / WAVE];
  __shared__ int win_cand;

  const int node = blockIdx.x / n_cat;
  const int feat = cat_feats[blockIdx.x % n_cat];
  const int tid = threadIdx.x;
  SplitCand best = {-1.0f, 0, 0, 0.f, 0.f};
  int best_cand = -1;

  bool masked = false;
  if (feat_mask != nullptr) {
    masked = feat_mask[mask_per_node ? (node * f + feat) : feat] == 0;
  }
  const int nb = nbins[feat];
  if (nb > SPLIT_BLOCK || nb >= stride + (has_missing ? 0 : 1)) masked = true;

  const float* hbase = hist + (((long long)node * f + feat) * stride) * 2;
  float g = 0.f, h = 0.f;
  if (!masked && tid < nb) {
    g = hbase[tid * 2];
    h = hbase[tid * 2 + 1];
  }
  const bool nonempty = !masked && tid < nb && !(g == 0.f && h == 0.f);
  const int m = __syncthreads_count(nonempty ? 1 : 0);  // non-empty categories
  const bool onehot = nb < max_cat_to_onehot;

  if (m >= 2) {  // block-uniform
    float key = nonempty ? g / (h + reg_lambda) : INFINITY;
    if (isnan(key)) key = INFINITY;
    sg[tid] = g;
    sh[tid] = h;
    skey[tid] = key;
    scat[tid] = tid | (nonempty ? 0 : 256);
    __syncthreads();
    if (!onehot) {
      // bitonic sort, ascending by (empty, key, category): a total order
      for (int size = 2; size <= SPLIT_BLOCK; size <<= 1) {
        for (int j = size >> 1; j > 0; j >>= 1) {
          const int other = tid ^ j;
          if (other > tid) {
            const int ca = scat[tid], cb = scat[other];
            const float ka = skey[tid], kb = skey[other];
            const int ea = ca >> 8, eb = cb >> 8;
            // does the entry at `other` sort before the one at `tid`?
            const bool b_first = (eb != ea) ? (eb < ea) : ((kb != ka) ? (kb < ka) : (cb < ca));
            const bool ascending = (tid & size) == 0;
            if (b_first == ascending) {
              const float ga = sg[tid], ha = sh[tid];
              sg[tid] = sg[other];
              sh[tid] = sh[other];
              skey[tid] = kb;
              scat[tid] = cb;
              sg[other] = ga;
              sh[other] = ha;
              skey[other] = ka;
              scat[other] = ca;
            }
          }
          __syncthreads();
        }
      }
      srank[scat[tid] & 255] = tid;
    }
    // inclusive Hillis-Steele scan of the (sorted) per-category sums
    for (int ofs = 1; ofs < SPLIT_BLOCK; ofs <<= 1) {
      float ag = 0.f, ah = 0.f;
      if (tid >= ofs) {
        ag = sg[tid - ofs];
        ah = sh[tid - ofs];
      }
      __syncthreads();
      sg[tid] += ag;
      sh[tid] += ah;
      __syncthreads();
    }
    const float tot_g = sg[SPLIT_BLOCK - 1];
    const float tot_h = sh[SPLIT_BLOCK - 1];

    // the left child's sums, missing aside, of this thread's candidate
    bool valid;
    float lg0, lh0;
    if (onehot) {
      valid = nonempty;
      lg0 = tot_g - g;
      lh0 = tot_h - h;
    } else {
      const int p = tid + 1;
      valid = p <= m - 1 && min(p, m - p) <= max_cat_threshold;
      const bool prefix_right = p <= m - p;
      lg0 = prefix_right ? tot_g - sg[tid] : sg[tid];
      lh0 = prefix_right ? tot_h - sh[tid] : sh[tid];
    }
    if (valid) {
      const float2 psum = parent[node];
      float miss_g = 0.f, miss_h = 0.f;
      if (has_missing) {
        miss_g = hbase[(stride - 1) * 2];
        miss_h = hbase[(stride - 1) * 2 + 1];
      }
      const float parent_score = split_score(psum.x, psum.y, reg_alpha, reg_lambda);
      for (int dir = 0; dir < 2; ++dir) {
        const float gl = lg0 + (dir ? miss_g : 0.f);
        const float hl = lh0 + (dir ? miss_h : 0.f);
        const float gr = psum.x - gl;
        const float hr = psum.y - hl;
        if (hl < min_child_weight || hr < min_child_weight) continue;
        const float gain =
            0.5f * (split_score(gl, hl, reg_alpha, reg_lambda) +
                    split_score(gr, hr, reg_alpha, reg_lambda) - parent_score) - gamma_;
        if (gain > best.gain) {
          best = {gain, 0, dir, gl, hl};
          best_cand = tid;
        }
      }
    }
  }
  __syncthreads();

  // block argmax, lowest candidate first among equal gains
  float bg = best.gain;
  int bidx = tid;
  for (int ofs = WAVE / 2; ofs > 0; ofs >>= 1) {
    const float og = __shfl_down(bg, ofs);
    const int oi = __shfl_down(bidx, ofs);
    if (og > bg) {
      bg = og;
      bidx = oi;
    }
  }
  const int wid = tid / WAVE;
  if ((tid & (WAVE - 1)) == 0) {
    red_gain[wid] = bg;
    red_idx[wid] = bidx;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < SPLIT_BLOCK / WAVE; ++w) {
      if (red_gain[w] > red_gain[0]) {
        red_gain[0] = red_gain[w];
        red_idx[0] = red_idx[w];
      }
    }
  }
  __syncthreads();
  if (tid == red_idx[0] && best.gain == red_gain[0]) {
    out[(long long)node * f + feat] = best;
    win_cand = best_cand;  // -1: the feature has no candidate
  }
  __syncthreads();

  // thread t: is category t in the winner's R?
  const int wc = win_cand;
  bool member = false;
  if (wc >= 0 && nonempty) {
    if (onehot) {
      member = tid == wc;
    } else {
      const int p = wc + 1;
      const int r = srank[tid];
      member = (p <= m - p) ? (r < p) : (r >= p && r < m);
    }
  }
  // one 64-bit ballot per wave fills two words: the block's waves cover the set
  static_assert(SPLIT_BLOCK / WAVE * 2 == CAT_WORDS && SPLIT_BLOCK == CAT_MAX,
                "split_scan_cat_kernel: one thread per category, two set words per wave");
  const unsigned long long ballot = __ballot(member ? 1 : 0);
  if ((tid & (WAVE - 1)) == 0) {
    unsigned int* bits = cand_bits + ((long long)node * f + feat) * CAT_WORDS;
    bits[wid * 2] = (unsigned int)(ballot & 0xffffffffull);
    bits[wid * 2 + 1] = (unsigned int)(ballot >> 32);
  }
}

// cat_bits[node] = the winning feature's set when it is categorical and the
// node splits, else zeros. One thread per node.
__global__ void split_cat_gather_kernel(const float* __restrict__ packed,  // [k, 6]
                                        const unsigned char* __restrict__ is_cat,  // [f]
                                        const unsigned int* __restrict__ cand_bits,
                                        unsigned int* __restrict__ cat_bits,  // [k, CAT_WORDS]
                                        int k, int f) {
  const int node = blockIdx.x * blockDim.x + threadIdx.x;
  if (node >= k) return;
  const float gain = packed[node * 6];
  const int feat = (int)packed[node * 6 + 1];
  const bool cat = gain > 0.f && feat >= 0 && feat < f && is_cat[feat] != 0;
  for (int w = 0; w < CAT_WORDS; ++w) {
    cat_bits[node * CAT_WORDS + w] =
        cat ? cand_bits[((long long)node * f + feat) * CAT_WORDS + w] : 0u;
  }
}

// ---------------------------------------------------------------------------
// row partition (two-ended compaction within each segment)
// ---------------------------------------------------------------------------

// Rows are staged through LDS tiles so each block issues ONE global atomic
// per side per tile (vs one per row: a single counter word sustains only
// ~88 atomics/us even wave-aggregated — measured 2.9 ms/level before).
#define PART_TILE 4096

// HAS_CAT: job j on a feature with is_cat set splits by the category set
// cat_bits[j] (the bins that go right) instead of by split_bin.
template <typename BinT, bool HAS_CAT>
__global__ __launch_bounds__(HIST_BLOCK) void partition_kernel(
    const BinT* __restrict__ bins, const int* __restrict__ src, int* __restrict__ dst,
    const PartJob* __restrict__ jobs, const int* __restrict__ block_job,
    int* __restrict__ counters, int nfeat, int missing_bin,
    const unsigned char* __restrict__ is_cat,    // [nfeat]; read only with HAS_CAT
    const unsigned int* __restrict__ cat_bits) {  // [n_jobs, CAT_WORDS]
  __shared__ int lbuf[PART_TILE];
  __shared__ int rbuf[PART_TILE];
  __shared__ int lcnt, rcnt, lbase, rbase;
  __shared__ unsigned int cset[CAT_WORDS];  // the job's category set

  const int j = block_job[blockIdx.x];
  const PartJob job = jobs[j];
  bool cat_split = false;
  if (HAS_CAT) {
    cat_split = is_cat[job.feature] != 0;  // block-uniform
    if (cat_split && threadIdx.x < CAT_WORDS) {
      cset[threadIdx.x] = cat_bits[(long long)j * CAT_WORDS + threadIdx.x];
    }
    // the tile loop's first barrier orders these stores before any read
  }
  const int chunk = blockIdx.x - job.first_block;
  const long long tile_step = (long long)job.num_blocks * PART_TILE;

  for (long long tile = job.start + (long long)chunk * PART_TILE; tile < job.end; tile += tile_step) {
    if (threadIdx.x == 0) {
      lcnt = 0;
      rcnt = 0;
    }
    __syncthreads();
    const int tile_n = (int)min((long long)PART_TILE, job.end - tile);
    for (int i = threadIdx.x; i < tile_n; i += blockDim.x) {
      const int row = src[tile + i];
      const int b = (int)bins[(long long)row * nfeat + job.feature];
      bool left;
      if (HAS_CAT && cat_split) {
        left = (b == missing_bin) ? (job.default_left != 0)
                                  : !((unsigned)b < (unsigned)CAT_MAX && cat_bit(cset, b));
      } else {
        left = (b == missing_bin) ? (job.default_left != 0) : (b <= job.split_bin);
      }
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
// leaf value scatter into the margin vector
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(HIST_BLOCK) void leaf_update_kernel(
    const int* __restrict__ buf0, const int* __restrict__ buf1,
    float* __restrict__ margin, const LeafJob* __restrict__ jobs,
    const int* __restrict__ block_job, long long col_stride) {
  const LeafJob job = jobs[block_job[blockIdx.x]];
  const int* src = job.parity ? buf1 : buf0;
  const int chunk = blockIdx.x - job.first_block;
  const long long step = (long long)job.num_blocks * blockDim.x;
  for (long long r = job.start + (long long)chunk * blockDim.x + threadIdx.x; r < job.end; r += step) {
    margin[(long long)src[r] * col_stride] += job.value;
  }
}

// ---------------------------------------------------------------------------
// batched forest prediction (dense rows x trees traversal)
// ---------------------------------------------------------------------------

// Work item = (row, tree-chunk): small serving batches (1k rows) would
// otherwise launch ~4 blocks against 256 CUs and serialize 500 trees per
// thread (measured 1.36 ms for 1k x 500). Each (row, chunk) owns its
// exclusive out[chunk, row, :] slice — no atomics; the caller reduces the
// chunk axis with a fixed-order torch sum (deterministic).
//
// HAS_CAT (a forest with categorical nodes): cat_slot[node] >= 0 names the
// node's row of cat_table ([n_cat_nodes, CAT_WORDS]); such a node decides by
// cat_goes_left (smxgb_cat.h) instead of by its threshold.
template <bool HAS_CAT>
__device__ inline bool node_goes_left(float fv, int nid, const float* __restrict__ thresh,
                                      const int* __restrict__ cat_slot,
                                      const unsigned int* __restrict__ cat_table) {
  if (HAS_CAT) {
    const int slot = cat_slot[nid];
    if (slot >= 0) return cat_goes_left(fv, cat_table + (long long)slot * CAT_WORDS);
  }
  return fv < thresh[nid];
}

template <bool HAS_CAT>
__global__ __launch_bounds__(HIST_BLOCK) void predict_kernel(
    const float* __restrict__ X, long long n, int nfeat,
    const int* __restrict__ left, const int* __restrict__ right,
    const int* __restrict__ feat, const float* __restrict__ thresh,
    const unsigned char* __restrict__ defl, const float* __restrict__ value,
    const int* __restrict__ tree_root, const int* __restrict__ tree_cls,
    int t_begin, int t_end, float* __restrict__ out, int k, int n_chunks,
    int trees_per_chunk, const int* __restrict__ cat_slot,
    const unsigned int* __restrict__ cat_table) {
  const long long total = n * (long long)n_chunks;
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += step) {
    const long long row = idx / n_chunks;
    const int c = (int)(idx - row * n_chunks);
    const float* xr = X + row * nfeat;
    float* orow = out + ((long long)c * n + row) * k;
    const int ts = t_begin + c * trees_per_chunk;
    const int te = min(t_end, ts + trees_per_chunk);
    for (int t = ts; t < te; ++t) {
      int nid = tree_root[t];
      int l;
      while ((l = left[nid]) >= 0) {
        const float fv = xr[feat[nid]];
        const bool goleft = isnan(fv) ? (defl[nid] != 0)
                                      : node_goes_left<HAS_CAT>(fv, nid, thresh, cat_slot, cat_table);
        nid = goleft ? l : right[nid];
      }
      orow[tree_cls[t]] += value[nid];
    }
  }
}

// leaf index per (row, tree): the predict_kernel traversal writing the
// tree-local leaf id (xgboost pred_leaf semantics). One thread per
// (row, tree), grid-strided.
template <bool HAS_CAT>
__global__ __launch_bounds__(HIST_BLOCK) void pred_leaf_kernel(
    const float* __restrict__ X, long long n, int nfeat,
    const int* __restrict__ left, const int* __restrict__ right,
    const int* __restrict__ feat, const float* __restrict__ thresh,
    const unsigned char* __restrict__ defl, const int* __restrict__ tree_root,
    int t_begin, int T, int* __restrict__ out, const int* __restrict__ cat_slot,
    const unsigned int* __restrict__ cat_table) {
  const long long total = n * (long long)T;
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += step) {
    const long long row = idx / T;
    const int t = (int)(idx - row * T);
    const float* xr = X + row * nfeat;
    const int root = tree_root[t_begin + t];
    int nid = root;
    int l;
    while ((l = left[nid]) >= 0) {
      const float fv = xr[feat[nid]];
      const bool goleft = isnan(fv) ? (defl[nid] != 0)
                                    : node_goes_left<HAS_CAT>(fv, nid, thresh, cat_slot, cat_table);
      nid = goleft ? l : right[nid];
    }
    out[idx] = nid - root;
  }
}

// ---------------------------------------------------------------------------
// path-form exact TreeSHAP (contributions + interactions)
// ---------------------------------------------------------------------------
//
// The host (ops/shap_paths.py) turns every leaf into one path whose splits
// are merged per feature, so a path never holds a feature twice and the
// recursive algorithm's unwind-on-duplicate step disappears. A work item is
// one (row, tree-chunk); it is owned by a LANE GROUP of width W (power of
// two >= the longest path incl. the dummy root element), 64/W groups per
// wave, one lane per path element. Permutation weights are built with the
// EXTEND recurrence passed between lanes with __shfl/__shfl_up at width W;
// every lane then computes its own unwound sum. All arithmetic is fp64.
// No per-thread arrays: every path quantity is one scalar per lane.
//
// Every loop bound (paths per chunk, path length, Lmax) comes from the
// host-built tables; shuffles run unconditionally with a grid-uniform trip
// count (Lmax) and only the arithmetic is predicated on the path length,
// so all W lanes of a group always execute the same cross-lane ops.

// SHAP_BLOCK, the SHAP_F_* flags, shap_one_fraction and shap_unwound_sum
// live in smxgb_shap.h, shared with smxgb_shap_compact.hip.

// out: (n_chunks, n, k, nfeat+1) fp64 partials, bias column untouched.
// A group exclusively owns out[chunk, row, :, :] — nothing is shared
// between groups, so there are no atomics; the caller reduces the chunk
// axis with a fixed-order sum. The running phi slab lives in LDS (one
// slab of k*(nfeat+1) doubles per group) and is flushed once per item.
__global__ __launch_bounds__(SHAP_BLOCK) void shap_paths_kernel(
    const float* __restrict__ X, long long n, int nfeat,
    const int* __restrict__ elem_feat, const float* __restrict__ elem_lo,
    const float* __restrict__ elem_hi, const unsigned char* __restrict__ elem_flags,
    const double* __restrict__ elem_z, const int* __restrict__ path_off,
    const float* __restrict__ path_value, const int* __restrict__ path_cls,
    const int* __restrict__ tree_path_ptr, int t_begin, int t_end,
    double* __restrict__ out, int k, int n_chunks, int trees_per_chunk, int W, int lmax) {
  extern __shared__ double shap_slab[];
  const int gpb = SHAP_BLOCK / W;
  const int g = threadIdx.x / W;
  const int gl = threadIdx.x - g * W;
  const int ncols = nfeat + 1;
  const int slab_n = k * ncols;
  double* slab = shap_slab + (long long)g * slab_n;
  for (int i = gl; i < slab_n; i += W) slab[i] = 0.0;

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
    const float* xr = X + row * nfeat;
    for (int p = p0; p < p1; ++p) {
      const int off = path_off[p];
      const int len = path_off[p + 1] - off + 1;  // + dummy root element
      const bool mine = gl > 0 && gl < len;
      double z = 1.0, o = 1.0;
      int fidx = -1;
      if (mine) {
        const int e = off + gl - 1;
        fidx = elem_feat[e];
        z = elem_z[e];
        o = shap_one_fraction(xr[fidx], elem_lo[e], elem_hi[e], elem_flags[e]);
      }
      const double s = shap_unwound_sum(z, o, gl, len, lmax, W);
      // Plain LDS read-modify-write. Within one path no two lanes of a
      // group hit the same cell (merged paths hold a feature once) and
      // groups own disjoint slabs. Across paths a cell may be written by
      // one lane and read by another lane of the SAME wave: a wave's DS
      // instructions execute in issue order, and the wavefront fence +
      // wave barrier below keep the compiler from moving them.
      if (mine) slab[path_cls[p] * ncols + fidx] += s * (o - z) * (double)path_value[p];
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
    double* orow = out + item * slab_n;
    for (int i = gl; i < slab_n; i += W) {
      orow[i] = slab[i];
      slab[i] = 0.0;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

// out: (n_chunks, n, k, nfeat+1, nfeat+1) fp64 partials, off-diagonal
// cells only. For each path and each element j of it, the remaining
// elements' contributions are computed with j removed from the path
// (compacted across lanes); the leaf value scaled by o_j (j "on") minus
// z_j (j "off"), halved, lands in out[cls, d_i, d_j]. Paths without j
// cancel and are never touched: O(L^3) per path.
// The (nfeat+1)^2 slab is too large for LDS, so a group accumulates in its
// exclusively owned global slice. Within one path every (d_i, d_j) cell is
// written once; between paths a workgroup-scope fence (vmcnt(0): the
// group's stores have reached the CU's L1/L2 path that its later loads
// use) orders one lane's store before another lane's later load.
__global__ __launch_bounds__(SHAP_BLOCK) void shap_interactions_kernel(
    const float* __restrict__ X, long long n, int nfeat,
    const int* __restrict__ elem_feat, const float* __restrict__ elem_lo,
    const float* __restrict__ elem_hi, const unsigned char* __restrict__ elem_flags,
    const double* __restrict__ elem_z, const int* __restrict__ path_off,
    const float* __restrict__ path_value, const int* __restrict__ path_cls,
    const int* __restrict__ tree_path_ptr, int t_begin, int t_end,
    double* out, int k, int n_chunks, int trees_per_chunk, int W, int lmax) {
  const int gpb = SHAP_BLOCK / W;
  const int g = threadIdx.x / W;
  const int gl = threadIdx.x - g * W;
  const int ncols = nfeat + 1;
  const long long slab_n = (long long)k * ncols * ncols;
  const int lmax_c = lmax > 1 ? lmax - 1 : 1;  // longest path with one element removed

  const long long total = n * (long long)n_chunks;
  const long long ngroups = (long long)gridDim.x * gpb;
  for (long long item = (long long)blockIdx.x * gpb + g; item < total; item += ngroups) {
    const long long c = item / n;
    const long long row = item - c * n;
    const int ts = t_begin + (int)c * trees_per_chunk;
    const int te = min(t_end, ts + trees_per_chunk);
    const int p0 = tree_path_ptr[ts];
    const int p1 = tree_path_ptr[te];
    const float* xr = X + row * nfeat;
    double* oslab = out + item * slab_n;
    for (int p = p0; p < p1; ++p) {
      const int off = path_off[p];
      const int len = path_off[p + 1] - off + 1;
      double z = 1.0, o = 1.0;
      int fidx = -1;
      if (gl > 0 && gl < len) {
        const int e = off + gl - 1;
        fidx = elem_feat[e];
        z = elem_z[e];
        o = shap_one_fraction(xr[fidx], elem_lo[e], elem_hi[e], elem_flags[e]);
      }
      const double v = (double)path_value[p];
      double* cslab = oslab + (long long)path_cls[p] * ncols * ncols;
      for (int j = 1; j < lmax; ++j) {
        const double zj = __shfl(z, j, W);
        const double oj = __shfl(o, j, W);
        const int fj = __shfl(fidx, j, W);
        // compact the path around j: lane gl takes element gl (< j) or gl+1
        const int src = min(gl < j ? gl : gl + 1, W - 1);
        const double zc = __shfl(z, src, W);
        const double oc = __shfl(o, src, W);
        const int fc = __shfl(fidx, src, W);
        const bool act = j < len;
        const int len_c = act ? len - 1 : 1;
        const double s = shap_unwound_sum(zc, oc, gl, len_c, lmax_c, W);
        if (act && gl > 0 && gl < len_c && oj != zj) {
          cslab[(long long)fc * ncols + fj] += 0.5 * (oj - zj) * s * (oc - zc) * v;
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
      __builtin_amdgcn_wave_barrier();
    }
  }
}

// ---------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------

static hipStream_t current_stream() {
  return at::hip::getCurrentHIPStream().stream();
}

void hist_build(torch::Tensor bins, torch::Tensor gh, torch::Tensor rowbuf,
                torch::Tensor jobs, torch::Tensor block_job, torch::Tensor out,
                int64_t nfeat, int64_t stride, double scale_g, double scale_h,
                int64_t lds_words) {
  CHECK_GPU(bins);
  CHECK_GPU(out);
  const int grid = (int)block_job.size(0);
  const size_t lds_bytes = (size_t)lds_words * sizeof(unsigned long long);
  auto stream = current_stream();
  if (bins.scalar_type() == torch::kUInt8) {
    hipLaunchKernelGGL(hist_kernel<unsigned char>, dim3(grid), dim3(HIST_BLOCK), lds_bytes, stream,
                       bins.data_ptr<unsigned char>(), (const float2*)gh.data_ptr<float>(),
                       rowbuf.data_ptr<int>(), (const HistJob*)jobs.data_ptr<int>(),
                       block_job.data_ptr<int>(), (unsigned long long*)out.data_ptr<int64_t>(),
                       (int)nfeat, (int)stride, (float)scale_g, (float)scale_h);
  } else {
    hipLaunchKernelGGL(hist_kernel<short>, dim3(grid), dim3(HIST_BLOCK), lds_bytes, stream,
                       bins.data_ptr<short>(), (const float2*)gh.data_ptr<float>(),
                       rowbuf.data_ptr<int>(), (const HistJob*)jobs.data_ptr<int>(),
                       block_job.data_ptr<int>(), (unsigned long long*)out.data_ptr<int64_t>(),
                       (int)nfeat, (int)stride, (float)scale_g, (float)scale_h);
  }
}

void hist_convert(torch::Tensor in, torch::Tensor out, double inv_g, double inv_h) {
  CHECK_GPU(in);
  const long long n_pairs = in.numel() / 2;
  const int grid = (int)std::min<long long>((n_pairs + HIST_BLOCK - 1) / HIST_BLOCK, 2048);
  hipLaunchKernelGGL(hist_convert_kernel, dim3(std::max(grid, 1)), dim3(HIST_BLOCK), 0, current_stream(),
                     (const unsigned long long*)in.data_ptr<int64_t>(), out.data_ptr<float>(),
                     n_pairs, (float)inv_g, (float)inv_h);
}

#define CHECK_GPU_DENSE(x, dt)                                                          \
  TORCH_CHECK_VALUE(x.is_cuda() && x.is_contiguous() && x.scalar_type() == dt,          \
                    #x " must be a contiguous ROCm device tensor of the expected dtype")

// the side inputs of a partition with categorical columns: is_cat [nfeat]
// u8 and one CAT_WORDS-word category set per row of `rows` sets
static void check_cat_partition(const torch::Tensor& is_cat, const torch::Tensor& cat_bits,
                                int64_t nfeat, int64_t rows) {
  CHECK_GPU_DENSE(is_cat, torch::kUInt8);
  CHECK_GPU_DENSE(cat_bits, torch::kInt32);
  TORCH_CHECK_VALUE(is_cat.numel() == nfeat, "is_cat must have one entry per feature");
  TORCH_CHECK_VALUE(cat_bits.numel() >= rows * CAT_WORDS, "cat_bits must be (rows, 8)");
}

template <bool HAS_CAT>
static void launch_partition(torch::Tensor bins, torch::Tensor src, torch::Tensor dst,
                             torch::Tensor jobs, torch::Tensor block_job, torch::Tensor counters,
                             int64_t nfeat, int64_t missing_bin, const unsigned char* is_cat,
                             const unsigned int* cat_bits) {
  CHECK_GPU(bins);
  const int grid = (int)block_job.size(0);
  auto stream = current_stream();
  if (bins.scalar_type() == torch::kUInt8) {
    hipLaunchKernelGGL((partition_kernel<unsigned char, HAS_CAT>), dim3(grid), dim3(HIST_BLOCK), 0,
                       stream, bins.data_ptr<unsigned char>(), src.data_ptr<int>(),
                       dst.data_ptr<int>(), (const PartJob*)jobs.data_ptr<int>(),
                       block_job.data_ptr<int>(), counters.data_ptr<int>(), (int)nfeat,
                       (int)missing_bin, is_cat, cat_bits);
  } else {
    hipLaunchKernelGGL((partition_kernel<short, HAS_CAT>), dim3(grid), dim3(HIST_BLOCK), 0, stream,
                       bins.data_ptr<short>(), src.data_ptr<int>(), dst.data_ptr<int>(),
                       (const PartJob*)jobs.data_ptr<int>(), block_job.data_ptr<int>(),
                       counters.data_ptr<int>(), (int)nfeat, (int)missing_bin, is_cat, cat_bits);
  }
}

void partition(torch::Tensor bins, torch::Tensor src, torch::Tensor dst,
               torch::Tensor jobs, torch::Tensor block_job, torch::Tensor counters,
               int64_t nfeat, int64_t missing_bin) {
  launch_partition<false>(bins, src, dst, jobs, block_job, counters, nfeat, missing_bin, nullptr,
                          nullptr);
}

// partition() for a matrix with categorical columns; cat_bits: one set per job
void partition_cat(torch::Tensor bins, torch::Tensor src, torch::Tensor dst,
                   torch::Tensor jobs, torch::Tensor block_job, torch::Tensor counters,
                   int64_t nfeat, int64_t missing_bin, torch::Tensor is_cat,
                   torch::Tensor cat_bits) {
  check_cat_partition(is_cat, cat_bits, nfeat, counters.size(0));
  launch_partition<true>(bins, src, dst, jobs, block_job, counters, nfeat, missing_bin,
                         is_cat.data_ptr<unsigned char>(),
                         (const unsigned int*)cat_bits.data_ptr<int>());
}

void leaf_update(torch::Tensor buf0, torch::Tensor buf1, torch::Tensor margin_base,
                 torch::Tensor jobs, torch::Tensor block_job, int64_t col_stride) {
  CHECK_GPU(margin_base);
  const int grid = (int)block_job.size(0);
  hipLaunchKernelGGL(leaf_update_kernel, dim3(grid), dim3(HIST_BLOCK), 0, current_stream(),
                     buf0.data_ptr<int>(), buf1.data_ptr<int>(), margin_base.data_ptr<float>(),
                     (const LeafJob*)jobs.data_ptr<int>(), block_job.data_ptr<int>(), col_stride);
}

// The categorical side tables of a flat forest (cat_slot per node, -1 at a
// numeric node; cat_table [n_cat_nodes, CAT_WORDS]). The slots were built on
// the host (ops/torch_ref.py flat_cat_arrays) and must lie inside the table:
// `max_slot` is the host's largest slot.
static void check_cat_tables(const torch::Tensor& left, const torch::Tensor& cat_slot,
                             const torch::Tensor& cat_table, int64_t max_slot) {
  CHECK_GPU_DENSE(cat_slot, torch::kInt32);
  CHECK_GPU_DENSE(cat_table, torch::kInt32);
  TORCH_CHECK_VALUE(cat_slot.numel() == left.numel(), "cat_slot must have one entry per node");
  TORCH_CHECK_VALUE(cat_table.dim() == 2 && cat_table.size(1) == CAT_WORDS,
                    "cat_table must be (n_cat_nodes, 8)");
  TORCH_CHECK_VALUE(max_slot < cat_table.size(0), "cat_slot entry outside cat_table");
}

// Everything is checked on the host before the launch: a matrix narrower
// than the widest split feature, a class id beyond k or a tree range past
// the forest would otherwise index device memory out of bounds.
template <bool HAS_CAT>
static void launch_predict_forest(torch::Tensor X, torch::Tensor left, torch::Tensor right,
                    torch::Tensor feat, torch::Tensor thresh, torch::Tensor defl,
                    torch::Tensor value, torch::Tensor tree_root, torch::Tensor tree_cls,
                    int64_t t_begin, int64_t t_end, int64_t max_feature, int64_t tree_cls_max,
                    torch::Tensor out, int64_t k, int64_t n_chunks, int64_t trees_per_chunk,
                    const int* cat_slot, const unsigned int* cat_table) {
  CHECK_GPU_DENSE(X, torch::kFloat32);
  CHECK_GPU_DENSE(left, torch::kInt32);
  CHECK_GPU_DENSE(right, torch::kInt32);
  CHECK_GPU_DENSE(feat, torch::kInt32);
  CHECK_GPU_DENSE(thresh, torch::kFloat32);
  CHECK_GPU_DENSE(defl, torch::kUInt8);
  CHECK_GPU_DENSE(value, torch::kFloat32);
  CHECK_GPU_DENSE(tree_root, torch::kInt32);
  CHECK_GPU_DENSE(tree_cls, torch::kInt32);
  CHECK_GPU_DENSE(out, torch::kFloat32);
  TORCH_CHECK_VALUE(X.dim() == 2, "X must be (n, f)");
  const long long nodes = left.numel();
  TORCH_CHECK_VALUE(right.numel() == nodes && feat.numel() == nodes && thresh.numel() == nodes &&
                        defl.numel() == nodes && value.numel() == nodes,
                    "forest node arrays differ in size");
  TORCH_CHECK_VALUE(tree_cls.numel() == tree_root.numel(), "tree_root and tree_cls differ in size");
  TORCH_CHECK_VALUE(0 <= t_begin && t_begin <= t_end && t_end <= tree_root.numel(),
                    "tree range out of bounds");
  const long long n = X.size(0);
  const long long T = t_end - t_begin;
  TORCH_CHECK_VALUE(k >= 1 && n_chunks >= 1 && trees_per_chunk >= 1 &&
                        n_chunks * trees_per_chunk >= T &&
                        n_chunks * trees_per_chunk <= (1ll << 30) && t_end <= (1ll << 30),
                    "tree chunking does not cover the tree range");
  TORCH_CHECK_VALUE(out.numel() == n_chunks * n * k, "out must be (n_chunks, n, k)");
  TORCH_CHECK_VALUE(T == 0 || (0 <= tree_cls_max && tree_cls_max < k), "the forest holds class id ",
                    tree_cls_max, " but k is ", k);
  TORCH_CHECK_VALUE(T == 0 || max_feature < X.size(1), "X has ", X.size(1),
                    " columns but the forest splits on feature ", max_feature);
  if (n == 0 || T == 0) return;
  const long long total = n * n_chunks;
  const int grid = (int)std::min<long long>((total + HIST_BLOCK - 1) / HIST_BLOCK, 4096);
  hipLaunchKernelGGL(predict_kernel<HAS_CAT>, dim3(grid), dim3(HIST_BLOCK), 0, current_stream(),
                     X.data_ptr<float>(), n, (int)X.size(1), left.data_ptr<int>(),
                     right.data_ptr<int>(), feat.data_ptr<int>(), thresh.data_ptr<float>(),
                     defl.data_ptr<unsigned char>(), value.data_ptr<float>(),
                     tree_root.data_ptr<int>(), tree_cls.data_ptr<int>(),
                     (int)t_begin, (int)t_end, out.data_ptr<float>(), (int)k, (int)n_chunks,
                     (int)trees_per_chunk, cat_slot, cat_table);
}

void predict_forest(torch::Tensor X, torch::Tensor left, torch::Tensor right,
                    torch::Tensor feat, torch::Tensor thresh, torch::Tensor defl,
                    torch::Tensor value, torch::Tensor tree_root, torch::Tensor tree_cls,
                    int64_t t_begin, int64_t t_end, int64_t max_feature, int64_t tree_cls_max,
                    torch::Tensor out, int64_t k, int64_t n_chunks, int64_t trees_per_chunk) {
  launch_predict_forest<false>(X, left, right, feat, thresh, defl, value, tree_root, tree_cls,
                               t_begin, t_end, max_feature, tree_cls_max, out, k, n_chunks,
                               trees_per_chunk, nullptr, nullptr);
}

// predict_forest() for a forest with categorical nodes
void predict_forest_cat(torch::Tensor X, torch::Tensor left, torch::Tensor right,
                        torch::Tensor feat, torch::Tensor thresh, torch::Tensor defl,
                        torch::Tensor value, torch::Tensor tree_root, torch::Tensor tree_cls,
                        int64_t t_begin, int64_t t_end, int64_t max_feature,
                        int64_t tree_cls_max, torch::Tensor out, int64_t k, int64_t n_chunks,
                        int64_t trees_per_chunk, torch::Tensor cat_slot, torch::Tensor cat_table,
                        int64_t max_slot) {
  check_cat_tables(left, cat_slot, cat_table, max_slot);
  launch_predict_forest<true>(X, left, right, feat, thresh, defl, value, tree_root, tree_cls,
                              t_begin, t_end, max_feature, tree_cls_max, out, k, n_chunks,
                              trees_per_chunk, cat_slot.data_ptr<int>(),
                              (const unsigned int*)cat_table.data_ptr<int>());
}

template <bool HAS_CAT>
static void launch_pred_leaf(torch::Tensor X, torch::Tensor left, torch::Tensor right,
               torch::Tensor feat, torch::Tensor thresh, torch::Tensor defl,
               torch::Tensor tree_root, int64_t t_begin, int64_t t_end, int64_t max_feature,
               torch::Tensor out, const int* cat_slot, const unsigned int* cat_table) {
  CHECK_GPU_DENSE(X, torch::kFloat32);
  CHECK_GPU_DENSE(left, torch::kInt32);
  CHECK_GPU_DENSE(right, torch::kInt32);
  CHECK_GPU_DENSE(feat, torch::kInt32);
  CHECK_GPU_DENSE(thresh, torch::kFloat32);
  CHECK_GPU_DENSE(defl, torch::kUInt8);
  CHECK_GPU_DENSE(tree_root, torch::kInt32);
  CHECK_GPU_DENSE(out, torch::kInt32);
  TORCH_CHECK_VALUE(X.dim() == 2, "X must be (n, f)");
  TORCH_CHECK_VALUE(max_feature < X.size(1), "X has ", X.size(1),
                    " columns but the forest splits on feature ", max_feature);
  TORCH_CHECK_VALUE(0 <= t_begin && t_begin <= t_end && t_end <= tree_root.numel(),
                    "tree range out of bounds");
  const long long n = X.size(0);
  const long long T = t_end - t_begin;
  TORCH_CHECK_VALUE(out.numel() == n * T, "out must be (n, T)");
  const long long total = n * T;
  if (total == 0) return;
  const int grid = (int)std::min<long long>((total + HIST_BLOCK - 1) / HIST_BLOCK, 4096);
  hipLaunchKernelGGL(pred_leaf_kernel<HAS_CAT>, dim3(grid), dim3(HIST_BLOCK), 0, current_stream(),
                     X.data_ptr<float>(), n, (int)X.size(1), left.data_ptr<int>(),
                     right.data_ptr<int>(), feat.data_ptr<int>(), thresh.data_ptr<float>(),
                     defl.data_ptr<unsigned char>(), tree_root.data_ptr<int>(), (int)t_begin,
                     (int)T, out.data_ptr<int>(), cat_slot, cat_table);
}

void pred_leaf(torch::Tensor X, torch::Tensor left, torch::Tensor right, torch::Tensor feat,
               torch::Tensor thresh, torch::Tensor defl, torch::Tensor tree_root,
               int64_t t_begin, int64_t t_end, int64_t max_feature, torch::Tensor out) {
  launch_pred_leaf<false>(X, left, right, feat, thresh, defl, tree_root, t_begin, t_end,
                          max_feature, out, nullptr, nullptr);
}

// pred_leaf() for a forest with categorical nodes
void pred_leaf_cat(torch::Tensor X, torch::Tensor left, torch::Tensor right, torch::Tensor feat,
                   torch::Tensor thresh, torch::Tensor defl, torch::Tensor tree_root,
                   int64_t t_begin, int64_t t_end, int64_t max_feature, torch::Tensor out,
                   torch::Tensor cat_slot, torch::Tensor cat_table, int64_t max_slot) {
  check_cat_tables(left, cat_slot, cat_table, max_slot);
  launch_pred_leaf<true>(X, left, right, feat, thresh, defl, tree_root, t_begin, t_end,
                         max_feature, out, cat_slot.data_ptr<int>(),
                         (const unsigned int*)cat_table.data_ptr<int>());
}

// shared argument validation for the two path-form TreeSHAP launchers;
// returns the grid size. `cells` = doubles per (chunk, row) output slice.
static int shap_check(torch::Tensor X, torch::Tensor elem_feat, torch::Tensor elem_lo,
                      torch::Tensor elem_hi, torch::Tensor elem_flags, torch::Tensor elem_z,
                      torch::Tensor path_off, torch::Tensor path_value,
                      torch::Tensor path_cls, torch::Tensor tree_path_ptr, int64_t t_begin,
                      int64_t t_end, torch::Tensor out, int64_t k, int64_t n_chunks,
                      int64_t trees_per_chunk, int64_t W, int64_t lmax, int64_t max_feature,
                      int64_t cells) {
  CHECK_GPU_DENSE(X, torch::kFloat32);
  CHECK_GPU_DENSE(elem_feat, torch::kInt32);
  CHECK_GPU_DENSE(elem_lo, torch::kFloat32);
  CHECK_GPU_DENSE(elem_hi, torch::kFloat32);
  CHECK_GPU_DENSE(elem_flags, torch::kUInt8);
  CHECK_GPU_DENSE(elem_z, torch::kFloat64);
  CHECK_GPU_DENSE(path_off, torch::kInt32);
  CHECK_GPU_DENSE(path_value, torch::kFloat32);
  CHECK_GPU_DENSE(path_cls, torch::kInt32);
  CHECK_GPU_DENSE(tree_path_ptr, torch::kInt32);
  CHECK_GPU_DENSE(out, torch::kFloat64);
  TORCH_CHECK_VALUE(X.dim() == 2, "X must be (n, f)");
  TORCH_CHECK_VALUE(max_feature < X.size(1), "X has ", X.size(1),
                    " columns but the forest splits on feature ", max_feature);
  TORCH_CHECK_VALUE(lmax >= 1 && lmax <= WAVE, "path length ", lmax, " exceeds the wave width");
  TORCH_CHECK_VALUE(W >= lmax && W <= WAVE && (W & (W - 1)) == 0,
                    "lane-group width must be a power of two in [lmax, 64]");
  TORCH_CHECK_VALUE(0 <= t_begin && t_begin <= t_end && t_end < tree_path_ptr.numel(),
                    "tree range out of bounds");
  TORCH_CHECK_VALUE(k >= 1 && n_chunks >= 1 && trees_per_chunk >= 1 &&
                        n_chunks * trees_per_chunk >= t_end - t_begin &&
                        (n_chunks - 1) * trees_per_chunk <= t_end - t_begin,
                    "bad tree chunking");
  const int64_t n_paths = path_off.numel() - 1;
  TORCH_CHECK_VALUE(n_paths >= 0 && path_value.numel() == n_paths && path_cls.numel() == n_paths,
                    "path tables disagree");
  const int64_t n_elem = elem_feat.numel();
  TORCH_CHECK_VALUE(elem_lo.numel() == n_elem && elem_hi.numel() == n_elem &&
                        elem_flags.numel() == n_elem && elem_z.numel() == n_elem,
                    "element tables disagree");
  const long long total = (long long)X.size(0) * n_chunks;
  TORCH_CHECK_VALUE(out.numel() == total * cells, "partial buffer has the wrong size");
  const long long gpb = SHAP_BLOCK / W;
  return (int)std::max<long long>(1, std::min<long long>((total + gpb - 1) / gpb, 8192));
}

void tree_shap_paths(torch::Tensor X, torch::Tensor elem_feat, torch::Tensor elem_lo,
                     torch::Tensor elem_hi, torch::Tensor elem_flags, torch::Tensor elem_z,
                     torch::Tensor path_off, torch::Tensor path_value, torch::Tensor path_cls,
                     torch::Tensor tree_path_ptr, int64_t t_begin, int64_t t_end,
                     torch::Tensor out, int64_t k, int64_t n_chunks, int64_t trees_per_chunk,
                     int64_t W, int64_t lmax, int64_t max_feature) {
  const int64_t ncols = X.dim() == 2 ? X.size(1) + 1 : 1;
  const int grid = shap_check(X, elem_feat, elem_lo, elem_hi, elem_flags, elem_z, path_off,
                              path_value, path_cls, tree_path_ptr, t_begin, t_end, out, k,
                              n_chunks, trees_per_chunk, W, lmax, max_feature, k * ncols);
  const size_t lds_bytes = (size_t)(SHAP_BLOCK / W) * k * ncols * sizeof(double);
  TORCH_CHECK_VALUE(lds_bytes <= 64 * 1024, "phi slab does not fit the LDS budget");
  if (X.size(0) == 0 || t_end == t_begin) return;
  hipLaunchKernelGGL(shap_paths_kernel, dim3(grid), dim3(SHAP_BLOCK), lds_bytes,
                     current_stream(), X.data_ptr<float>(), (long long)X.size(0),
                     (int)X.size(1), elem_feat.data_ptr<int>(), elem_lo.data_ptr<float>(),
                     elem_hi.data_ptr<float>(), elem_flags.data_ptr<unsigned char>(),
                     elem_z.data_ptr<double>(), path_off.data_ptr<int>(),
                     path_value.data_ptr<float>(), path_cls.data_ptr<int>(),
                     tree_path_ptr.data_ptr<int>(), (int)t_begin, (int)t_end,
                     out.data_ptr<double>(), (int)k, (int)n_chunks, (int)trees_per_chunk,
                     (int)W, (int)lmax);
}

void tree_shap_interactions_paths(torch::Tensor X, torch::Tensor elem_feat,
                                  torch::Tensor elem_lo, torch::Tensor elem_hi,
                                  torch::Tensor elem_flags, torch::Tensor elem_z,
                                  torch::Tensor path_off, torch::Tensor path_value,
                                  torch::Tensor path_cls, torch::Tensor tree_path_ptr,
                                  int64_t t_begin, int64_t t_end, torch::Tensor out, int64_t k,
                                  int64_t n_chunks, int64_t trees_per_chunk, int64_t W,
                                  int64_t lmax, int64_t max_feature) {
  const int64_t ncols = X.dim() == 2 ? X.size(1) + 1 : 1;
  const int grid = shap_check(X, elem_feat, elem_lo, elem_hi, elem_flags, elem_z, path_off,
                              path_value, path_cls, tree_path_ptr, t_begin, t_end, out, k,
                              n_chunks, trees_per_chunk, W, lmax, max_feature,
                              k * ncols * ncols);
  if (X.size(0) == 0 || t_end == t_begin) return;
  hipLaunchKernelGGL(shap_interactions_kernel, dim3(grid), dim3(SHAP_BLOCK), 0,
                     current_stream(), X.data_ptr<float>(), (long long)X.size(0),
                     (int)X.size(1), elem_feat.data_ptr<int>(), elem_lo.data_ptr<float>(),
                     elem_hi.data_ptr<float>(), elem_flags.data_ptr<unsigned char>(),
                     elem_z.data_ptr<double>(), path_off.data_ptr<int>(),
                     path_value.data_ptr<float>(), path_cls.data_ptr<int>(),
                     tree_path_ptr.data_ptr<int>(), (int)t_begin, (int)t_end,
                     out.data_ptr<double>(), (int)k, (int)n_chunks, (int)trees_per_chunk,
                     (int)W, (int)lmax);
}

void hist_build_compact(torch::Tensor bins_c, torch::Tensor gh_c, torch::Tensor jobs,
                        torch::Tensor block_job, torch::Tensor out, int64_t nfeat,
                        int64_t stride, torch::Tensor gh_max, int64_t lds_words) {
  CHECK_GPU(bins_c);
  const int grid = (int)block_job.size(0);
  const size_t lds_bytes = (size_t)lds_words * sizeof(unsigned long long);
  auto stream = current_stream();
  if (bins_c.scalar_type() == torch::kUInt8) {
    hipLaunchKernelGGL(hist_compact_kernel<unsigned char>, dim3(grid), dim3(HIST_BLOCK), lds_bytes,
                       stream, bins_c.data_ptr<unsigned char>(),
                       (const float2*)gh_c.data_ptr<float>(), (const HistJob*)jobs.data_ptr<int>(),
                       block_job.data_ptr<int>(), (unsigned long long*)out.data_ptr<int64_t>(),
                       (int)nfeat, (int)stride, gh_max.data_ptr<float>());
  } else {
    hipLaunchKernelGGL(hist_compact_kernel<short>, dim3(grid), dim3(HIST_BLOCK), lds_bytes, stream,
                       bins_c.data_ptr<short>(), (const float2*)gh_c.data_ptr<float>(),
                       (const HistJob*)jobs.data_ptr<int>(), block_job.data_ptr<int>(),
                       (unsigned long long*)out.data_ptr<int64_t>(), (int)nfeat, (int)stride,
                       gh_max.data_ptr<float>());
  }
}

void hist_convert_dev(torch::Tensor in, torch::Tensor out, torch::Tensor gh_max) {
  CHECK_GPU(in);
  const long long n_pairs = in.numel() / 2;
  const int grid = (int)std::min<long long>((n_pairs + HIST_BLOCK - 1) / HIST_BLOCK, 2048);
  hipLaunchKernelGGL(hist_convert_dev_kernel, dim3(std::max(grid, 1)), dim3(HIST_BLOCK), 0,
                     current_stream(), (const unsigned long long*)in.data_ptr<int64_t>(),
                     out.data_ptr<float>(), n_pairs, gh_max.data_ptr<float>());
}

template <bool HAS_CAT>
static void launch_partition_compact(torch::Tensor src_bins, torch::Tensor src_gh,
                                     torch::Tensor src_rows, torch::Tensor dst_bins,
                                     torch::Tensor dst_gh, torch::Tensor dst_rows,
                                     torch::Tensor jobs, torch::Tensor block_job,
                                     torch::Tensor split_packed, torch::Tensor counters,
                                     int64_t nfeat, int64_t missing_bin,
                                     const unsigned char* is_cat, const unsigned int* cat_bits) {
  CHECK_GPU(src_bins);
  const int grid = (int)block_job.size(0);
  auto stream = current_stream();
  if (src_bins.scalar_type() == torch::kUInt8) {
    hipLaunchKernelGGL((partition_compact_kernel<unsigned char, HAS_CAT>), dim3(grid),
                       dim3(HIST_BLOCK), 0, stream, src_bins.data_ptr<unsigned char>(),
                       (const float2*)src_gh.data_ptr<float>(), src_rows.data_ptr<int>(),
                       dst_bins.data_ptr<unsigned char>(), (float2*)dst_gh.data_ptr<float>(),
                       dst_rows.data_ptr<int>(), (const PartJob*)jobs.data_ptr<int>(),
                       block_job.data_ptr<int>(), split_packed.data_ptr<float>(),
                       counters.data_ptr<int>(), (int)nfeat, (int)missing_bin, is_cat, cat_bits);
  } else {
    hipLaunchKernelGGL((partition_compact_kernel<short, HAS_CAT>), dim3(grid), dim3(HIST_BLOCK), 0,
                       stream, src_bins.data_ptr<short>(), (const float2*)src_gh.data_ptr<float>(),
                       src_rows.data_ptr<int>(), dst_bins.data_ptr<short>(),
                       (float2*)dst_gh.data_ptr<float>(), dst_rows.data_ptr<int>(),
                       (const PartJob*)jobs.data_ptr<int>(), block_job.data_ptr<int>(),
                       split_packed.data_ptr<float>(), counters.data_ptr<int>(), (int)nfeat,
                       (int)missing_bin, is_cat, cat_bits);
  }
}

void partition_compact(torch::Tensor src_bins, torch::Tensor src_gh, torch::Tensor src_rows,
                       torch::Tensor dst_bins, torch::Tensor dst_gh, torch::Tensor dst_rows,
                       torch::Tensor jobs, torch::Tensor block_job, torch::Tensor split_packed,
                       torch::Tensor counters, int64_t nfeat, int64_t missing_bin) {
  launch_partition_compact<false>(src_bins, src_gh, src_rows, dst_bins, dst_gh, dst_rows, jobs,
                                  block_job, split_packed, counters, nfeat, missing_bin, nullptr,
                                  nullptr);
}

// partition_compact() for a matrix with categorical columns; cat_bits: one
// category set per row of split_packed
void partition_compact_cat(torch::Tensor src_bins, torch::Tensor src_gh, torch::Tensor src_rows,
                           torch::Tensor dst_bins, torch::Tensor dst_gh, torch::Tensor dst_rows,
                           torch::Tensor jobs, torch::Tensor block_job,
                           torch::Tensor split_packed, torch::Tensor counters, int64_t nfeat,
                           int64_t missing_bin, torch::Tensor is_cat, torch::Tensor cat_bits) {
  check_cat_partition(is_cat, cat_bits, nfeat, split_packed.size(0));
  launch_partition_compact<true>(src_bins, src_gh, src_rows, dst_bins, dst_gh, dst_rows, jobs,
                                 block_job, split_packed, counters, nfeat, missing_bin,
                                 is_cat.data_ptr<unsigned char>(),
                                 (const unsigned int*)cat_bits.data_ptr<int>());
}

void leaf_update_compact(torch::Tensor rows0, torch::Tensor rows1, torch::Tensor margin_base,
                         torch::Tensor jobs, torch::Tensor block_job, int64_t col_stride) {
  CHECK_GPU(margin_base);
  const int grid = (int)block_job.size(0);
  hipLaunchKernelGGL(leaf_update_compact_kernel, dim3(grid), dim3(HIST_BLOCK), 0, current_stream(),
                     rows0.data_ptr<int>(), rows1.data_ptr<int>(), margin_base.data_ptr<float>(),
                     (const LeafJob*)jobs.data_ptr<int>(), block_job.data_ptr<int>(), col_stride);
}

template <typename BinT>
static void launch_leaf_traverse(bool staged, int grid, size_t lds, hipStream_t stream,
                                 const BinT* bins, const float* splits, const float* values,
                                 float* margin, long long n, int nfeat, int D, int missing_bin,
                                 long long col_stride) {
  if (staged) {
    hipLaunchKernelGGL((leaf_update_traverse_kernel<BinT, true>), dim3(grid), dim3(HIST_BLOCK),
                       lds, stream, bins, splits, values, margin, n, nfeat, D, missing_bin,
                       col_stride);
  } else {
    hipLaunchKernelGGL((leaf_update_traverse_kernel<BinT, false>), dim3(grid), dim3(HIST_BLOCK),
                       lds, stream, bins, splits, values, margin, n, nfeat, D, missing_bin,
                       col_stride);
  }
}

// margin[r * col_stride] += values[leaf(r)] for every row of the bin matrix
void leaf_update_traverse(torch::Tensor bins, torch::Tensor splits, torch::Tensor values,
                          torch::Tensor margin_base, int64_t D, int64_t missing_bin,
                          int64_t col_stride) {
  CHECK_GPU(bins);
  CHECK_GPU(splits);
  CHECK_GPU(values);
  CHECK_GPU(margin_base);
  TORCH_CHECK(D >= 1 && D <= 10, "leaf_update_traverse: depth must be 1..10");
  TORCH_CHECK(bins.dim() == 2 && bins.is_contiguous(), "leaf_update_traverse: bins must be [n, f]");
  const long long n = bins.size(0);
  const int nfeat = (int)bins.size(1);
  const long long heap = ((long long)1 << D) - 1;
  TORCH_CHECK(splits.scalar_type() == torch::kFloat32 && splits.is_contiguous() &&
                  splits.numel() >= heap * 6,
              "leaf_update_traverse: split heap too small");
  TORCH_CHECK(values.scalar_type() == torch::kFloat32 && values.is_contiguous() &&
                  values.numel() >= 2 * heap + 1,
              "leaf_update_traverse: value table too small");
  TORCH_CHECK(margin_base.scalar_type() == torch::kFloat32 && margin_base.dim() == 1 &&
                  margin_base.size(0) == n && margin_base.stride(0) == col_stride,
              "leaf_update_traverse: margin column does not match the bin matrix");
  if (n == 0) return;
  auto stream = current_stream();
  const size_t tables = (size_t)16 * (heap + 1);
  if (bins.scalar_type() == torch::kUInt8) {
    const unsigned char* ptr = bins.data_ptr<unsigned char>();
    const size_t tile = (size_t)TRAV_TILE * nfeat;
    const bool staged = (nfeat & 3) == 0 && tables + tile <= 48 * 1024 &&
                        (reinterpret_cast<uintptr_t>(ptr) & 15) == 0;
    const long long blocks =
        staged ? (n + TRAV_TILE - 1) / TRAV_TILE : (n + HIST_BLOCK - 1) / HIST_BLOCK;
    launch_leaf_traverse<unsigned char>(staged, (int)std::min<long long>(blocks, 2048),
                                        tables + (staged ? tile : 0), stream, ptr,
                                        splits.data_ptr<float>(), values.data_ptr<float>(),
                                        margin_base.data_ptr<float>(), n, nfeat, (int)D,
                                        (int)missing_bin, col_stride);
  } else {
    TORCH_CHECK(bins.scalar_type() == torch::kInt16, "leaf_update_traverse: bins must be u8 or i16");
    const long long blocks = (n + HIST_BLOCK - 1) / HIST_BLOCK;
    launch_leaf_traverse<short>(false, (int)std::min<long long>(blocks, 2048), tables, stream,
                                bins.data_ptr<short>(), splits.data_ptr<float>(),
                                values.data_ptr<float>(), margin_base.data_ptr<float>(), n, nfeat,
                                (int)D, (int)missing_bin, col_stride);
  }
}

void grow_make_root(torch::Tensor nodes, torch::Tensor hist_prefix, torch::Tensor part_prefix,
                    torch::Tensor work, int64_t cap, int64_t rows_per_block, int64_t max_blocks) {
  hipLaunchKernelGGL(make_root_kernel, dim3(1), dim3(1), 0, current_stream(),
                     (LevelNode*)nodes.data_ptr<int>(), hist_prefix.data_ptr<int>(),
                     part_prefix.data_ptr<int>(), (LevelWork*)work.data_ptr<int>(), (int)cap,
                     (int)rows_per_block, (int)max_blocks);
}

void grow_make_level(torch::Tensor cur, torch::Tensor splits, torch::Tensor counts,
                     torch::Tensor node_gh, torch::Tensor nxt, torch::Tensor nxt_gh,
                     torch::Tensor hist_prefix, torch::Tensor part_prefix, torch::Tensor work,
                     int64_t k, int64_t rows_per_block, int64_t max_blocks, int64_t filtered) {
  hipLaunchKernelGGL(make_level_kernel, dim3(1), dim3(GROW_MAX_SLOTS), 0, current_stream(),
                     (const LevelNode*)cur.data_ptr<int>(), splits.data_ptr<float>(),
                     counts.data_ptr<int>(), node_gh.data_ptr<float>(),
                     (LevelNode*)nxt.data_ptr<int>(), nxt_gh.data_ptr<float>(),
                     hist_prefix.data_ptr<int>(), part_prefix.data_ptr<int>(),
                     (LevelWork*)work.data_ptr<int>(), (int)k, (int)rows_per_block,
                     (int)max_blocks, (int)filtered);
}

// dispatch helper: BLOCK is a compile-time launch bound (256 grouped-slab,
// 512 single full-feature slab); FILTER: see hist_device_kernel
template <typename BinT, int FILTER>
static void launch_hist_device_impl(int grid, int hist_block, size_t lds_bytes, hipStream_t stream,
                               const BinT* bins_c, const float2* gh_c, const LevelNode* nodes,
                               const int* hist_prefix, const LevelWork* work,
                               unsigned long long* acc, int k, int nfeat, int stride,
                               int n_groups, int feats_per_group, const float* gh_max,
                               int rows_per_block, int slot_lo, int slot_hi,
                               const float* par_splits, int missing_bin, int queue_ofs) {
  // hipGraph kernel nodes validate dynamic LDS against the function's
  // max-dynamic-shared attribute (plain launches do not): without this
  // opt-in a captured full-slab launch (>64 KB) reads a truncated LDS
  // allocation and memory-faults on replay (gfx950 allows 160 KB).
  static bool lds_attr_set = [] {
    (void)hipFuncSetAttribute((const void*)(hist_device_kernel<BinT, 512, FILTER>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute((const void*)(hist_device_kernel<BinT, HIST_BLOCK, FILTER>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    return true;
  }();
  (void)lds_attr_set;
  if (hist_block == 512) {
    hipLaunchKernelGGL((hist_device_kernel<BinT, 512, FILTER>), dim3(grid), dim3(512),
                       lds_bytes, stream, bins_c, gh_c, nodes, hist_prefix, work, acc, k, nfeat,
                       stride, n_groups, feats_per_group, gh_max, rows_per_block, slot_lo,
                       slot_hi, par_splits, missing_bin, queue_ofs);
  } else {
    hipLaunchKernelGGL((hist_device_kernel<BinT, HIST_BLOCK, FILTER>), dim3(grid),
                       dim3(HIST_BLOCK), lds_bytes, stream, bins_c, gh_c, nodes, hist_prefix, work,
                       acc, k, nfeat, stride, n_groups, feats_per_group, gh_max, rows_per_block,
                       slot_lo, slot_hi, par_splits, missing_bin, queue_ofs);
  }
}

template <typename BinT>
static void launch_hist_device(int grid, int hist_block, size_t lds_bytes, hipStream_t stream,
                               const BinT* bins_c, const float2* gh_c, const LevelNode* nodes,
                               const int* hist_prefix, const LevelWork* work,
                               unsigned long long* acc, int k, int nfeat, int stride,
                               int n_groups, int feats_per_group, const float* gh_max,
                               int rows_per_block, int slot_lo = 0, int slot_hi = 1 << 30,
                               const float* par_splits = nullptr, int missing_bin = -1,
                               bool predicate_only = false) {
  // filter mode when parent split records are given. The per-wave row queues
  // of the compacting form go behind the slab: taken for the single-slab
  // block (one block per CU either way) when both fit, so they never cost
  // occupancy; grouped slabs keep plain predication.
  const size_t queue_bytes = (size_t)(hist_block / 64) * HIST_QUEUE_ROWS * sizeof(int);
  if (par_splits == nullptr) {
    launch_hist_device_impl<BinT, HIST_FILTER_OFF>(
        grid, hist_block, lds_bytes, stream, bins_c, gh_c, nodes, hist_prefix, work, acc, k,
        nfeat, stride, n_groups, feats_per_group, gh_max, rows_per_block, slot_lo, slot_hi,
        nullptr, missing_bin, 0);
  } else if (!predicate_only && hist_block == 512 && lds_bytes + queue_bytes <= 158 * 1024) {
    launch_hist_device_impl<BinT, HIST_FILTER_COMPACT>(
        grid, hist_block, lds_bytes + queue_bytes, stream, bins_c, gh_c, nodes, hist_prefix, work,
        acc, k, nfeat, stride, n_groups, feats_per_group, gh_max, rows_per_block, slot_lo,
        slot_hi, par_splits, missing_bin, (int)(lds_bytes / sizeof(unsigned long long)));
  } else {
    launch_hist_device_impl<BinT, HIST_FILTER_PREDICATE>(
        grid, hist_block, lds_bytes, stream, bins_c, gh_c, nodes, hist_prefix, work, acc, k,
        nfeat, stride, n_groups, feats_per_group, gh_max, rows_per_block, slot_lo, slot_hi,
        par_splits, missing_bin, 0);
  }
}

void grow_hist_level(torch::Tensor bins_c, torch::Tensor gh_c, torch::Tensor nodes,
                     torch::Tensor hist_prefix, torch::Tensor work, torch::Tensor acc,
                     int64_t k, int64_t nfeat, int64_t stride, int64_t n_groups,
                     int64_t feats_per_group, torch::Tensor gh_max, int64_t rows_per_block,
                     int64_t grid, int64_t lds_words, int64_t hist_block,
                     int64_t slot_lo, int64_t slot_hi, torch::Tensor par_splits,
                     int64_t missing_bin, int64_t predicate_only) {
  const size_t lds_bytes = (size_t)lds_words * sizeof(unsigned long long);
  auto stream = current_stream();
  // filter mode (see hist_device_kernel): the parent level's [k/2, 6] split
  // records; an empty tensor keeps the plain build
  const float* par_ptr = nullptr;
  if (par_splits.numel() > 0) {
    CHECK_GPU(par_splits);
    TORCH_CHECK(k >= 2 && par_splits.scalar_type() == torch::kFloat32 &&
                    par_splits.is_contiguous() && par_splits.numel() >= (k >> 1) * 6,
                "grow_hist_level: parent split records must be a contiguous float32 [k/2, 6]");
    par_ptr = par_splits.data_ptr<float>();
  }
  if (bins_c.scalar_type() == torch::kUInt8) {
    launch_hist_device<unsigned char>(
        (int)grid, (int)hist_block, lds_bytes, stream, bins_c.data_ptr<unsigned char>(),
        (const float2*)gh_c.data_ptr<float>(), (const LevelNode*)nodes.data_ptr<int>(),
        hist_prefix.data_ptr<int>(), (const LevelWork*)work.data_ptr<int>(),
        (unsigned long long*)acc.data_ptr<int64_t>(), (int)k, (int)nfeat, (int)stride,
        (int)n_groups, (int)feats_per_group, gh_max.data_ptr<float>(), (int)rows_per_block,
        (int)slot_lo, (int)slot_hi, par_ptr, (int)missing_bin, predicate_only != 0);
  } else {
    launch_hist_device<short>(
        (int)grid, (int)hist_block, lds_bytes, stream, bins_c.data_ptr<short>(),
        (const float2*)gh_c.data_ptr<float>(), (const LevelNode*)nodes.data_ptr<int>(),
        hist_prefix.data_ptr<int>(), (const LevelWork*)work.data_ptr<int>(),
        (unsigned long long*)acc.data_ptr<int64_t>(), (int)k, (int)nfeat, (int)stride,
        (int)n_groups, (int)feats_per_group, gh_max.data_ptr<float>(), (int)rows_per_block,
        (int)slot_lo, (int)slot_hi, par_ptr, (int)missing_bin, predicate_only != 0);
  }
}

void grow_convert_level(torch::Tensor acc, torch::Tensor hist_f32, torch::Tensor nodes,
                        int64_t k, int64_t slots2, torch::Tensor gh_max) {
  const long long total = (long long)k * slots2;
  const int grid = (int)std::min<long long>((total + HIST_BLOCK - 1) / HIST_BLOCK, 2048);
  hipLaunchKernelGGL(convert_level_kernel, dim3(std::max(grid, 1)), dim3(HIST_BLOCK), 0,
                     current_stream(), (const unsigned long long*)acc.data_ptr<int64_t>(),
                     hist_f32.data_ptr<float>(), (const LevelNode*)nodes.data_ptr<int>(), (int)k,
                     slots2, gh_max.data_ptr<float>());
}

void grow_derive_level(torch::Tensor level_hist, torch::Tensor parent_hist, torch::Tensor nodes,
                       int64_t k, int64_t slots2) {
  const long long total = (long long)k * slots2;
  const int grid = (int)std::min<long long>((total + HIST_BLOCK - 1) / HIST_BLOCK, 2048);
  hipLaunchKernelGGL(derive_level_kernel, dim3(std::max(grid, 1)), dim3(HIST_BLOCK), 0,
                     current_stream(), level_hist.data_ptr<float>(),
                     parent_hist.data_ptr<float>(), (const LevelNode*)nodes.data_ptr<int>(),
                     (int)k, slots2);
}

// Which kernel partitions a level (SMXGB_PARTITION, pushed in by ops/hip.py
// through set_partition_mode):
//   0                 the classic two-read kernel everywhere
//   1                 the staged single-read kernel where it applies
//   512 / 1024 / 2048 the staged kernel at that tile (A/B sweeps; 1 = 2048)
static int g_partition_mode = 1;

void set_partition_mode(int64_t mode) {
  TORCH_CHECK_VALUE(mode == 0 || mode == 1 || mode == 512 || mode == 1024 || mode == 2048,
                    "partition mode must be 0, 1, 512, 1024 or 2048, got ", mode);
  g_partition_mode = (int)mode;
}

// Rows per tile of the staged kernel, 0 where the classic kernel runs
// (int16 bins, widths the 8-lane row group does not cover, the payload-free
// last-level form). Measured at 12.5M x 28 (profiles/
// r11_partition_single_read.md): 580 / 318 / 190 us per launch at 512 / 1024 /
// 2048 rows per tile, at every level alike, so the barrier and atomic round
// trip that each tile pays sets the time, not the node's two counter words
// (rows / 2048 returning atomics per word at k = 1: 69 us of 190). Every
// level takes the 2048-row tile on a 512-thread block.
static int staged_partition_tile(int nfeat, bool u8, int copy_payload) {
  if (g_partition_mode == 0 || !u8 || !copy_payload || nfeat < 4 || nfeat > 32 ||
      (nfeat & 3) != 0)
    return 0;
  return g_partition_mode == 1 ? 2048 : g_partition_mode;
}

int64_t partition_tile(int64_t nfeat, int64_t u8, int64_t copy_payload) {
  return staged_partition_tile((int)nfeat, u8 != 0, (int)copy_payload);
}

static bool launch_part_staged(int grid, hipStream_t stream, const unsigned char* src_bins,
                               const float2* src_gh, const int* src_rows,
                               unsigned char* dst_bins, float2* dst_gh, int* dst_rows,
                               const LevelNode* nodes, const int* part_prefix,
                               const LevelWork* work, const float* split_packed, int* counters,
                               int k, int nfeat, int missing_bin, int copy_payload,
                               int copy_rows) {
  const int tile = staged_partition_tile(nfeat, true, copy_payload);
  if (tile == 0) return false;
#define SMXGB_LAUNCH_STAGED(BLOCK, R)                                                          \
  do {                                                                                         \
    if (copy_rows) {                                                                           \
      hipLaunchKernelGGL((partition_device_staged_kernel<BLOCK, R, true>), dim3(grid),         \
                         dim3(BLOCK), 0, stream, src_bins, src_gh, src_rows, dst_bins, dst_gh, \
                         dst_rows, nodes, part_prefix, work, split_packed, counters, k, nfeat, \
                         missing_bin);                                                         \
    } else {                                                                                   \
      hipLaunchKernelGGL((partition_device_staged_kernel<BLOCK, R, false>), dim3(grid),        \
                         dim3(BLOCK), 0, stream, src_bins, src_gh, src_rows, dst_bins, dst_gh, \
                         dst_rows, nodes, part_prefix, work, split_packed, counters, k, nfeat, \
                         missing_bin);                                                         \
    }                                                                                          \
  } while (0)
  if (tile == 2048) {
    SMXGB_LAUNCH_STAGED(512, 32);
  } else if (tile == 1024) {
    SMXGB_LAUNCH_STAGED(256, 32);
  } else {
    SMXGB_LAUNCH_STAGED(256, 16);
  }
#undef SMXGB_LAUNCH_STAGED
  return true;
}

void grow_partition_level(torch::Tensor src_bins, torch::Tensor src_gh, torch::Tensor src_rows,
                          torch::Tensor dst_bins, torch::Tensor dst_gh, torch::Tensor dst_rows,
                          torch::Tensor nodes, torch::Tensor part_prefix, torch::Tensor work,
                          torch::Tensor split_packed, torch::Tensor counters, int64_t k,
                          int64_t nfeat, int64_t missing_bin, int64_t grid,
                          int64_t copy_payload, int64_t copy_rows) {
  auto stream = current_stream();
  if (src_bins.scalar_type() == torch::kUInt8) {
    if (launch_part_staged((int)grid, stream, src_bins.data_ptr<unsigned char>(),
                           (const float2*)src_gh.data_ptr<float>(), src_rows.data_ptr<int>(),
                           dst_bins.data_ptr<unsigned char>(), (float2*)dst_gh.data_ptr<float>(),
                           dst_rows.data_ptr<int>(), (const LevelNode*)nodes.data_ptr<int>(),
                           part_prefix.data_ptr<int>(), (const LevelWork*)work.data_ptr<int>(),
                           split_packed.data_ptr<float>(), counters.data_ptr<int>(), (int)k,
                           (int)nfeat, (int)missing_bin, (int)copy_payload, (int)copy_rows))
      return;
    hipLaunchKernelGGL(partition_device_kernel<unsigned char>, dim3((int)grid), dim3(HIST_BLOCK),
                       0, stream, src_bins.data_ptr<unsigned char>(),
                       (const float2*)src_gh.data_ptr<float>(), src_rows.data_ptr<int>(),
                       dst_bins.data_ptr<unsigned char>(), (float2*)dst_gh.data_ptr<float>(),
                       dst_rows.data_ptr<int>(), (const LevelNode*)nodes.data_ptr<int>(),
                       part_prefix.data_ptr<int>(), (const LevelWork*)work.data_ptr<int>(),
                       split_packed.data_ptr<float>(), counters.data_ptr<int>(), (int)k,
                       (int)nfeat, (int)missing_bin, (int)copy_payload, (int)copy_rows);
  } else {
    hipLaunchKernelGGL(partition_device_kernel<short>, dim3((int)grid), dim3(HIST_BLOCK), 0,
                       stream, src_bins.data_ptr<short>(), (const float2*)src_gh.data_ptr<float>(),
                       src_rows.data_ptr<int>(), dst_bins.data_ptr<short>(),
                       (float2*)dst_gh.data_ptr<float>(), dst_rows.data_ptr<int>(),
                       (const LevelNode*)nodes.data_ptr<int>(), part_prefix.data_ptr<int>(),
                       (const LevelWork*)work.data_ptr<int>(), split_packed.data_ptr<float>(),
                       counters.data_ptr<int>(), (int)k, (int)nfeat, (int)missing_bin,
                       (int)copy_payload, (int)copy_rows);
  }
}

// One level's interaction-constraint step on its own (the whole-tree
// enqueue launches the same kernel inline).
void grow_node_mask(torch::Tensor par_nodes, torch::Tensor par_splits, torch::Tensor par_allowed,
                    torch::Tensor inter_union, torch::Tensor level_mask, torch::Tensor allowed,
                    torch::Tensor node_mask, int64_t k, int64_t nfeat) {
  CHECK_GPU(node_mask);
  const int64_t W = (nfeat + 31) / 32;
  const int64_t pk = k >> 1;
  TORCH_CHECK(k >= 2 && (k & 1) == 0, "grow_node_mask: k must be even and >= 2");
  TORCH_CHECK(par_nodes.numel() >= pk * 3 && par_splits.numel() >= pk * 6 &&
                  par_allowed.numel() >= pk * W && inter_union.numel() >= nfeat * W &&
                  allowed.numel() >= k * W && node_mask.numel() >= k * nfeat &&
                  (level_mask.numel() == 0 || level_mask.numel() >= nfeat),
              "grow_node_mask: buffer too small");
  hipLaunchKernelGGL(node_mask_kernel, dim3((int)k), dim3(NODE_MASK_BLOCK), 0, current_stream(),
                     (const LevelNode*)par_nodes.data_ptr<int>(), par_splits.data_ptr<float>(),
                     (const unsigned*)par_allowed.data_ptr<int>(),
                     (const unsigned*)inter_union.data_ptr<int>(),
                     level_mask.numel() ? level_mask.data_ptr<unsigned char>() : nullptr,
                     (unsigned*)allowed.data_ptr<int>(), node_mask.data_ptr<unsigned char>(),
                     (int)k, (int)nfeat, (int)W);
}

// Whole-tree enqueue: the entire depthwise grow issued from C++ in one
// Python call (single-process path; the distributed path keeps the Python
// per-level loop so torch.distributed can enqueue the allreduce).
void grow_tree_enqueue(
    torch::Tensor init_bins, torch::Tensor init_gh, torch::Tensor init_rows,
    torch::Tensor bins0, torch::Tensor gh0, torch::Tensor rows0,
    torch::Tensor bins1, torch::Tensor gh1, torch::Tensor rows1,
    torch::Tensor nodes, torch::Tensor node_gh, torch::Tensor splits, torch::Tensor counts,
    torch::Tensor hist_f32, torch::Tensor acc, torch::Tensor cands,
    std::vector<torch::Tensor> hp, std::vector<torch::Tensor> pp, torch::Tensor work,
    torch::Tensor nbins, torch::Tensor feat_mask, torch::Tensor monotone,
    torch::Tensor inter_union, torch::Tensor allowed, torch::Tensor node_mask,
    torch::Tensor gh_max, int64_t D, int64_t cap, int64_t nfeat, int64_t stride, int64_t n_groups,
    int64_t feats_per_group, int64_t lds_words, int64_t has_missing, int64_t missing_bin,
    int64_t rows_per_block, int64_t max_blocks, int64_t hist_grid, int64_t part_grid,
    double reg_lambda, double reg_alpha, double gamma_, double min_child_weight,
    int64_t hist_block, int64_t skip_last_partition, int64_t filter_deepest) {
  CHECK_GPU(init_bins);
  auto stream = current_stream();
  // Margins updated by traversal (skip_last_partition): nothing reads row
  // ids or the deepest level's ranges. With filter_deepest the partition of
  // level D-2 goes too: level D-1's histograms stream the ranges level D-2
  // read and keep each build child's rows by the parent's split
  // (filter_deepest == 2: by plain predication even where compaction fits).
  const bool filter_last = skip_last_partition && filter_deepest && D >= 2;
  const int copy_rows = skip_last_partition ? 0 : 1;
  const long long slots2 = (long long)nfeat * stride * 2;
  const bool u8 = init_bins.scalar_type() == torch::kUInt8;
  const size_t lds_bytes = (size_t)lds_words * sizeof(unsigned long long);
  // feat_mask: empty, [f] (one tree-wide mask) or [D, f] (row d = level d's
  // mask, tree/level/node draws already folded in by the host)
  const unsigned char* mask_base =
      feat_mask.numel() ? feat_mask.data_ptr<unsigned char>() : nullptr;
  const long long mask_row = feat_mask.dim() == 2 ? nfeat : 0;
  const signed char* mono_ptr =
      monotone.numel() ? (const signed char*)monotone.data_ptr<int8_t>() : nullptr;
  // interaction constraints: per-node allowed bitsets + [k, f] node masks
  const bool inter = inter_union.numel() > 0;
  const long long W = (nfeat + 31) / 32;
  const long long heap = ((long long)1 << D) - 1;
  TORCH_CHECK(feat_mask.numel() == 0 || feat_mask.numel() >= (mask_row ? D * nfeat : nfeat),
              "grow_tree_enqueue: feature mask too small");
  TORCH_CHECK(monotone.numel() == 0 || monotone.numel() >= nfeat,
              "grow_tree_enqueue: monotone vector too small");
  TORCH_CHECK(!inter || (inter_union.numel() >= nfeat * W && allowed.numel() >= heap * W &&
                         node_mask.numel() >= (heap + 1) / 2 * nfeat),
              "grow_tree_enqueue: interaction buffers too small");

  hipMemsetAsync(counts.data_ptr<int>(), 0, sizeof(int) * 2 * counts.size(0), stream);

  for (int d = 0; d < (int)D; ++d) {
    const int k = 1 << d;
    const int base = k - 1;
    LevelNode* nodes_d = (LevelNode*)nodes.data_ptr<int>() + base;
    float* gh_d = node_gh.data_ptr<float>() + (long long)base * 2;
    float* splits_d = splits.data_ptr<float>() + (long long)base * 6;
    int* counts_d = counts.data_ptr<int>() + (long long)base * 2;
    float* hist_d = hist_f32.data_ptr<float>() + (long long)base * slots2;
    int* hp_d = hp[d].data_ptr<int>();
    int* pp_d = pp[d].data_ptr<int>();
    LevelWork* work_d = (LevelWork*)(work.data_ptr<int>() + 2 * d);
    const bool filtered = filter_last && d == (int)D - 1;
    const float* par_splits =
        filtered ? splits.data_ptr<float>() + (long long)((k >> 1) - 1) * 6 : nullptr;

    if (d == 0) {
      hipLaunchKernelGGL(make_root_kernel, dim3(1), dim3(1), 0, stream, nodes_d, hp_d, pp_d,
                         work_d, (int)cap, (int)rows_per_block, (int)max_blocks);
    } else {
      const int pk = k >> 1;
      const int pbase = pk - 1;
      hipLaunchKernelGGL(make_level_kernel, dim3(1), dim3(GROW_MAX_SLOTS), 0, stream,
                         (const LevelNode*)nodes.data_ptr<int>() + pbase,
                         splits.data_ptr<float>() + (long long)pbase * 6,
                         counts.data_ptr<int>() + (long long)pbase * 2,
                         node_gh.data_ptr<float>() + (long long)pbase * 2, nodes_d, gh_d, hp_d,
                         pp_d, work_d, pk, (int)rows_per_block, (int)max_blocks,
                         filtered ? 1 : 0);
    }

    // a filtered level reads what the level above it read
    const int sd = filtered ? d - 1 : d;
    const bool level0 = sd == 0;
    const bool par = (sd % 2) == 1;
    const void* src_bins = level0 ? init_bins.data_ptr() : (par ? bins1.data_ptr() : bins0.data_ptr());
    const float2* src_gh = (const float2*)(level0 ? init_gh.data_ptr<float>()
                                                  : (par ? gh1.data_ptr<float>() : gh0.data_ptr<float>()));
    const int* src_rows = level0 ? init_rows.data_ptr<int>()
                                 : (par ? rows1.data_ptr<int>() : rows0.data_ptr<int>());
    const bool dpar = (d % 2) == 0;  // dst index = 1 - d%2
    void* dst_bins = dpar ? bins1.data_ptr() : bins0.data_ptr();
    float2* dst_gh = (float2*)(dpar ? gh1.data_ptr<float>() : gh0.data_ptr<float>());
    int* dst_rows = dpar ? rows1.data_ptr<int>() : rows0.data_ptr<int>();

    hipMemsetAsync(acc.data_ptr<int64_t>(), 0, sizeof(int64_t) * (size_t)k * slots2, stream);
    if (u8) {
      launch_hist_device<unsigned char>(
          (int)hist_grid, (int)hist_block, lds_bytes, stream, (const unsigned char*)src_bins,
          src_gh, nodes_d, hp_d, work_d, (unsigned long long*)acc.data_ptr<int64_t>(), k,
          (int)nfeat, (int)stride, (int)n_groups, (int)feats_per_group,
          gh_max.data_ptr<float>(), (int)rows_per_block, 0, 1 << 30, par_splits,
          (int)missing_bin, filter_deepest == 2);
    } else {
      launch_hist_device<short>(
          (int)hist_grid, (int)hist_block, lds_bytes, stream, (const short*)src_bins, src_gh,
          nodes_d, hp_d, work_d, (unsigned long long*)acc.data_ptr<int64_t>(), k, (int)nfeat,
          (int)stride, (int)n_groups, (int)feats_per_group, gh_max.data_ptr<float>(),
          (int)rows_per_block, 0, 1 << 30, par_splits, (int)missing_bin, filter_deepest == 2);
    }

    {
      const long long total = (long long)k * slots2;
      const int grid = (int)std::min<long long>((total + HIST_BLOCK - 1) / HIST_BLOCK, 2048);
      hipLaunchKernelGGL(convert_level_kernel, dim3(std::max(grid, 1)), dim3(HIST_BLOCK), 0,
                         stream, (const unsigned long long*)acc.data_ptr<int64_t>(), hist_d,
                         nodes_d, k, slots2, gh_max.data_ptr<float>());
      if (d > 0) {
        const int pbase = (k >> 1) - 1;
        hipLaunchKernelGGL(derive_level_kernel, dim3(std::max(grid, 1)), dim3(HIST_BLOCK), 0,
                           stream, hist_d, hist_f32.data_ptr<float>() + (long long)pbase * slots2,
                           nodes_d, k, slots2);
      }
    }

    const unsigned char* mask_ptr = mask_base ? mask_base + (long long)d * mask_row : nullptr;
    int mask_per_node = 0;
    if (inter && d > 0) {
      const int pbase = (k >> 1) - 1;
      unsigned* allowed_all = (unsigned*)allowed.data_ptr<int>();
      hipLaunchKernelGGL(node_mask_kernel, dim3(k), dim3(NODE_MASK_BLOCK), 0, stream,
                         (const LevelNode*)nodes.data_ptr<int>() + pbase,
                         splits.data_ptr<float>() + (long long)pbase * 6,
                         allowed_all + (long long)pbase * W,
                         (const unsigned*)inter_union.data_ptr<int>(), mask_ptr,
                         allowed_all + (long long)base * W, node_mask.data_ptr<unsigned char>(), k,
                         (int)nfeat, (int)W);
      mask_ptr = node_mask.data_ptr<unsigned char>();
      mask_per_node = 1;
    }
    hipLaunchKernelGGL(split_scan_kernel, dim3(k * (int)nfeat), dim3(SPLIT_BLOCK), 0, stream,
                       hist_d, (const float2*)gh_d, nbins.data_ptr<int>(), mask_ptr, mono_ptr,
                       (SplitCand*)cands.data_ptr<float>(), k, (int)nfeat, (int)stride,
                       (int)has_missing, mask_per_node, (float)reg_lambda, (float)reg_alpha, (float)gamma_,
                       (float)min_child_weight);
    hipLaunchKernelGGL(split_reduce_kernel, dim3(k), dim3(SPLIT_BLOCK), 0, stream,
                       (const SplitCand*)cands.data_ptr<float>(), splits_d, k, (int)nfeat);

    const int copy_payload = d < (int)D - 1 ? 1 : 0;  // last level: rows+counts only
    // margins updated by traversal: nothing consumes the deepest level's
    // row ids and counts, so that level is not partitioned at all
    if (!copy_payload && skip_last_partition) continue;
    // ... and with the filtered deepest histogram, neither is level D-2
    if (filter_last && d == (int)D - 2) continue;
    if (u8) {
      if (!launch_part_staged((int)part_grid, stream, (const unsigned char*)src_bins, src_gh,
                              src_rows, (unsigned char*)dst_bins, dst_gh, dst_rows, nodes_d,
                              pp_d, work_d, splits_d, counts_d, k, (int)nfeat,
                              (int)missing_bin, copy_payload, copy_rows))
        hipLaunchKernelGGL(partition_device_kernel<unsigned char>, dim3((int)part_grid),
                           dim3(HIST_BLOCK), 0, stream, (const unsigned char*)src_bins, src_gh,
                           src_rows, (unsigned char*)dst_bins, dst_gh, dst_rows, nodes_d, pp_d,
                           work_d, splits_d, counts_d, k, (int)nfeat, (int)missing_bin,
                           copy_payload, copy_rows);
    } else {
      hipLaunchKernelGGL(partition_device_kernel<short>, dim3((int)part_grid), dim3(HIST_BLOCK),
                         0, stream, (const short*)src_bins, src_gh, src_rows, (short*)dst_bins,
                         dst_gh, dst_rows, nodes_d, pp_d, work_d, splits_d, counts_d, k,
                         (int)nfeat, (int)missing_bin, copy_payload, copy_rows);
    }
  }
}

// `pmax` / `psum` hold one (|g|, |h|) maximum and one (g, h) sum per block:
// their first dimension is the grid size.
void grad_fused(torch::Tensor margin, torch::Tensor y, torch::Tensor w, torch::Tensor gh,
                torch::Tensor pmax, torch::Tensor psum, int64_t mode, double spw) {
  CHECK_GPU_DENSE(margin, torch::kFloat32);
  CHECK_GPU_DENSE(y, torch::kFloat32);
  CHECK_GPU_DENSE(w, torch::kFloat32);
  CHECK_GPU_DENSE(gh, torch::kFloat32);
  CHECK_GPU_DENSE(pmax, torch::kFloat32);
  CHECK_GPU_DENSE(psum, torch::kFloat64);
  const long long n = margin.numel();
  TORCH_CHECK_VALUE(y.numel() == n, "y holds ", y.numel(), " labels for ", n, " margins");
  TORCH_CHECK_VALUE(w.numel() == 0 || w.numel() == n, "w holds ", w.numel(), " weights for ", n,
                    " margins");
  TORCH_CHECK_VALUE(gh.numel() == 2 * n, "gh must be (n, 2)");
  TORCH_CHECK_VALUE(pmax.dim() == 2 && pmax.size(1) == 2 && pmax.size(0) >= 1 &&
                        pmax.size(0) <= 65536,
                    "pmax must be (grid, 2)");
  TORCH_CHECK_VALUE(psum.dim() == 2 && psum.size(1) == 2 && psum.size(0) == pmax.size(0),
                    "psum must be (grid, 2) like pmax");
  TORCH_CHECK_VALUE(mode == 0 || mode == 1, "mode must be 0 (logistic) or 1 (squared error)");
  const int grid = (int)pmax.size(0);
  hipLaunchKernelGGL(grad_fused_kernel, dim3(grid), dim3(HIST_BLOCK), 0, current_stream(),
                     margin.data_ptr<float>(), y.data_ptr<float>(),
                     w.numel() ? w.data_ptr<float>() : nullptr, (float2*)gh.data_ptr<float>(),
                     (float2*)pmax.data_ptr<float>(), (double2*)psum.data_ptr<double>(), n,
                     (int)mode, (float)spw);
}

void find_splits(torch::Tensor hist, torch::Tensor parent, torch::Tensor nbins,
                 torch::Tensor feat_mask, torch::Tensor monotone, torch::Tensor cands,
                 torch::Tensor out, int64_t k, int64_t f, int64_t stride, int64_t has_missing,
                 int64_t mask_per_node, double reg_lambda, double reg_alpha, double gamma_,
                 double min_child_weight) {
  CHECK_GPU(hist);
  auto stream = current_stream();
  const unsigned char* mask_ptr =
      feat_mask.numel() ? feat_mask.data_ptr<unsigned char>() : nullptr;
  const signed char* mono_ptr =
      monotone.numel() ? (const signed char*)monotone.data_ptr<int8_t>() : nullptr;
  hipLaunchKernelGGL(split_scan_kernel, dim3((int)(k * f)), dim3(SPLIT_BLOCK), 0, stream,
                     hist.data_ptr<float>(), (const float2*)parent.data_ptr<float>(),
                     nbins.data_ptr<int>(), mask_ptr, mono_ptr,
                     (SplitCand*)cands.data_ptr<float>(), (int)k, (int)f, (int)stride,
                     (int)has_missing, (int)mask_per_node, (float)reg_lambda, (float)reg_alpha,
                     (float)gamma_, (float)min_child_weight);
  hipLaunchKernelGGL(split_reduce_kernel, dim3((int)k), dim3(SPLIT_BLOCK), 0, stream,
                     (const SplitCand*)cands.data_ptr<float>(), out.data_ptr<float>(), (int)k,
                     (int)f);
}

// find_splits() for a matrix with categorical columns, on one stream:
// split_scan_kernel with the categorical features masked out of `num_mask`,
// split_scan_cat_kernel over (node, categorical feature) with the caller's
// own mask `cat_mask`, split_reduce_kernel over all features, then the
// gather of the winners' category sets into cat_bits [k, 8].
void find_splits_cat(torch::Tensor hist, torch::Tensor parent, torch::Tensor nbins,
                     torch::Tensor num_mask, int64_t num_mask_per_node, torch::Tensor cat_mask,
                     int64_t cat_mask_per_node, torch::Tensor monotone, torch::Tensor cands,
                     torch::Tensor out, torch::Tensor is_cat, torch::Tensor cat_feats,
                     torch::Tensor cand_bits, torch::Tensor cat_bits, int64_t k, int64_t f,
                     int64_t stride, int64_t has_missing, double reg_lambda, double reg_alpha,
                     double gamma_, double min_child_weight, int64_t max_cat_to_onehot,
                     int64_t max_cat_threshold) {
  CHECK_GPU_DENSE(hist, torch::kFloat32);
  CHECK_GPU_DENSE(parent, torch::kFloat32);
  CHECK_GPU_DENSE(nbins, torch::kInt32);
  CHECK_GPU_DENSE(num_mask, torch::kUInt8);
  CHECK_GPU_DENSE(cands, torch::kFloat32);
  CHECK_GPU_DENSE(out, torch::kFloat32);
  CHECK_GPU_DENSE(is_cat, torch::kUInt8);
  CHECK_GPU_DENSE(cat_feats, torch::kInt32);
  CHECK_GPU_DENSE(cand_bits, torch::kInt32);
  CHECK_GPU_DENSE(cat_bits, torch::kInt32);
  const int64_t n_cat = cat_feats.numel();
  TORCH_CHECK_VALUE(k >= 1 && f >= 1 && n_cat >= 1 && n_cat <= f && stride >= 1,
                    "bad split-search shape");
  TORCH_CHECK_VALUE(k * f <= (1ll << 30), "too many (node, feature) pairs");
  TORCH_CHECK_VALUE(hist.numel() == k * f * stride * 2, "hist must be (k, f * stride, 2)");
  TORCH_CHECK_VALUE(parent.numel() == k * 2 && nbins.numel() == f && is_cat.numel() == f,
                    "parent / nbins / is_cat differ from (k, f)");
  TORCH_CHECK_VALUE(num_mask.numel() == (num_mask_per_node ? k * f : f),
                    "num_mask must be (f,) or (k, f)");
  TORCH_CHECK_VALUE(cands.numel() == k * f * 5 && out.numel() == k * 6,
                    "cands must be (k, f, 5) and out (k, 6)");
  TORCH_CHECK_VALUE(cand_bits.numel() == k * f * CAT_WORDS && cat_bits.numel() == k * CAT_WORDS,
                    "cand_bits must be (k, f, 8) and cat_bits (k, 8)");
  const unsigned char* cat_mask_ptr = nullptr;
  if (cat_mask.numel()) {
    CHECK_GPU_DENSE(cat_mask, torch::kUInt8);
    TORCH_CHECK_VALUE(cat_mask.numel() == (cat_mask_per_node ? k * f : f),
                      "cat_mask must be (f,) or (k, f)");
    cat_mask_ptr = cat_mask.data_ptr<unsigned char>();
  }
  const signed char* mono_ptr =
      monotone.numel() ? (const signed char*)monotone.data_ptr<int8_t>() : nullptr;
  auto stream = current_stream();
  hipLaunchKernelGGL(split_scan_kernel, dim3((int)(k * f)), dim3(SPLIT_BLOCK), 0, stream,
                     hist.data_ptr<float>(), (const float2*)parent.data_ptr<float>(),
                     nbins.data_ptr<int>(), num_mask.data_ptr<unsigned char>(), mono_ptr,
                     (SplitCand*)cands.data_ptr<float>(), (int)k, (int)f, (int)stride,
                     (int)has_missing, (int)num_mask_per_node, (float)reg_lambda,
                     (float)reg_alpha, (float)gamma_, (float)min_child_weight);
  hipLaunchKernelGGL(split_scan_cat_kernel, dim3((int)(k * n_cat)), dim3(SPLIT_BLOCK), 0, stream,
                     hist.data_ptr<float>(), (const float2*)parent.data_ptr<float>(),
                     nbins.data_ptr<int>(), cat_feats.data_ptr<int>(), cat_mask_ptr,
                     (SplitCand*)cands.data_ptr<float>(),
                     (unsigned int*)cand_bits.data_ptr<int>(), (int)k, (int)f, (int)n_cat,
                     (int)stride, (int)has_missing, (int)cat_mask_per_node, (float)reg_lambda,
                     (float)reg_alpha, (float)gamma_, (float)min_child_weight,
                     (int)max_cat_to_onehot, (int)max_cat_threshold);
  hipLaunchKernelGGL(split_reduce_kernel, dim3((int)k), dim3(SPLIT_BLOCK), 0, stream,
                     (const SplitCand*)cands.data_ptr<float>(), out.data_ptr<float>(), (int)k,
                     (int)f);
  hipLaunchKernelGGL(split_cat_gather_kernel, dim3((int)((k + SPLIT_BLOCK - 1) / SPLIT_BLOCK)),
                     dim3(SPLIT_BLOCK), 0, stream, out.data_ptr<float>(),
                     is_cat.data_ptr<unsigned char>(),
                     (const unsigned int*)cand_bits.data_ptr<int>(),
                     (unsigned int*)cat_bits.data_ptr<int>(), (int)k, (int)f);
}

void init_text_parsers(pybind11::module_& m);
void init_sparse_kernels(pybind11::module_& m);
void init_shap_compact_kernels(pybind11::module_& m);
void init_sampling_kernels(pybind11::module_& m);
void init_quantile_kernels(pybind11::module_& m);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  init_text_parsers(m);
  init_sparse_kernels(m);
  init_shap_compact_kernels(m);
  init_sampling_kernels(m);
  init_quantile_kernels(m);
  m.def("hist_build", &hist_build, "batched LDS-staged fixed-point histogram build");
  m.def("hist_convert", &hist_convert, "fixed-point -> float32 histogram convert");
  m.def("partition", &partition, "batched two-ended row partition");
  m.def("find_splits", &find_splits, "fused split-gain scan + per-node reduce");
  m.def("find_splits_cat", &find_splits_cat,
        "split search with categorical features: numeric scan + category-set scan + reduce");
  m.def("partition_cat", &partition_cat, "two-ended row partition with category-set splits");
  m.def("partition_compact_cat", &partition_compact_cat,
        "compacting partition with category-set splits");
  m.def("predict_forest_cat", &predict_forest_cat,
        "batched dense forest traversal with categorical nodes");
  m.def("pred_leaf_cat", &pred_leaf_cat, "leaf index per (row, tree) with categorical nodes");
  m.def("hist_build_compact", &hist_build_compact, "streaming histogram over compact row buffers");
  m.def("hist_convert_dev", &hist_convert_dev, "fixed-point -> f32 convert with device-resident scale");
  m.def("grow_make_root", &grow_make_root);
  m.def("grow_make_level", &grow_make_level);
  m.def("grow_hist_level", &grow_hist_level);
  m.def("grow_convert_level", &grow_convert_level);
  m.def("grow_derive_level", &grow_derive_level);
  m.def("grow_partition_level", &grow_partition_level);
  m.def("set_partition_mode", &set_partition_mode,
        "0 classic, 1 staged, 512/1024/2048 staged at that tile");
  m.def("partition_tile", &partition_tile,
        "rows per tile of the staged partition for (nfeat, u8, copy_payload); 0 = classic");
  m.def("grow_node_mask", &grow_node_mask, "interaction-constraint bitsets + node mask of a level");
  m.def("grow_tree_enqueue", &grow_tree_enqueue, "whole depthwise tree enqueued from one call");
  m.def("partition_compact", &partition_compact, "compacting partition (rows+bins+gh rewrite)");
  m.def("leaf_update_compact", &leaf_update_compact, "leaf scatter from compact row ids");
  m.def("leaf_update_traverse", &leaf_update_traverse,
        "margin update by streaming traversal of the split heap");
  m.def("leaf_update", &leaf_update, "batched leaf value scatter into margins");
  m.def("predict_forest", &predict_forest, "batched dense forest traversal");
  m.def("grad_fused", &grad_fused, "one-pass gradient + absmax partials");
  m.def("pred_leaf", &pred_leaf, "leaf index per (row, tree)");
  m.def("tree_shap_paths", &tree_shap_paths, "path-form exact TreeSHAP contributions");
  m.def("tree_shap_interactions_paths", &tree_shap_interactions_paths,
        "path-form exact TreeSHAP interaction values (off-diagonal)");
  m.attr("_built_for") = "gfx950";
}
