// Device helpers shared by the quantization kernels: smxgb_quantize.hip
// (dense matrices) and smxgb_quantize_csr.hip (CSR matrices). Include inside
// the including file's no-packed-fp32-ops attribute region.
#pragma once

#include <hip/hip_runtime.h>

#define QZ_BLOCK 256
#define QZ_WAVE 64
#define QZ_WAVES (QZ_BLOCK / QZ_WAVE)
#define QZ_DIGITS 2048                  // counters of a slot (pass 3 uses 1024)
#define QZ_ELECT 2                      // leader elections per flush step

// The orderable u32 pattern of a float32's bits: unsigned order of the keys is
// the float order of the values.
__device__ __forceinline__ unsigned qz_key(unsigned b) {
  if (b == 0x80000000u) b = 0u;  // -0.0 is the value +0.0
  return b ^ ((b & 0x80000000u) ? 0xffffffffu : 0x80000000u);
}

__device__ __forceinline__ float qz_value(unsigned key) {
  return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}

__device__ __forceinline__ bool qz_is_nan(unsigned b) { return (b & 0x7fffffffu) > 0x7f800000u; }

// Adds cnt to tab[addr] for every lane with `pending`, all lanes of the wave
// calling. Lanes that share the address of an elected leader are summed and
// leave with one atomic.
__device__ __forceinline__ void qz_wave_add(int* tab, int addr, int cnt, bool pending) {
  const int lane = threadIdx.x & (QZ_WAVE - 1);
  unsigned long long pend = __ballot(pending);
  #pragma unroll
  for (int round = 0; round < QZ_ELECT; ++round) {
    if (pend == 0ull) break;  // uniform
    const int leader = __ffsll((long long)pend) - 1;
    const int la = __shfl(addr, leader, QZ_WAVE);
    const bool match = pending && addr == la;
    const unsigned long long mm = __ballot(match);
    if (__popcll(mm) > 1) {  // uniform
      int s = match ? cnt : 0;
      #pragma unroll
      for (int d = QZ_WAVE >> 1; d > 0; d >>= 1) s += __shfl_xor(s, d, QZ_WAVE);
      if (lane == leader) atomicAdd(&tab[la], s);
    } else if (lane == leader) {
      atomicAdd(&tab[la], cnt);
    }
    pending = pending && !match;
    pend &= ~mm;
  }
  if (pending) atomicAdd(&tab[addr], cnt);
}

// Exclusive prefix sum of v over the lanes of a wave; total: the wave's sum.
__device__ __forceinline__ int qz_wave_scan(int v, int& total) {
  const int lane = threadIdx.x & (QZ_WAVE - 1);
  int incl = v;
  #pragma unroll
  for (int d = 1; d < QZ_WAVE; d <<= 1) {
    const int o = __shfl_up(incl, d, QZ_WAVE);
    if (lane >= d) incl += o;
  }
  total = __shfl(incl, QZ_WAVE - 1, QZ_WAVE);
  return incl - v;
}

// Exclusive prefix sum of v over the block's threads; total: the block's sum.
// s_w: QZ_WAVES words of LDS, free again on return.
__device__ __forceinline__ int qz_block_scan(int v, int* s_w, int& total) {
  const int lane = threadIdx.x & (QZ_WAVE - 1);
  const int wave = threadIdx.x / QZ_WAVE;
  int incl = v;
  #pragma unroll
  for (int d = 1; d < QZ_WAVE; d <<= 1) {
    const int o = __shfl_up(incl, d, QZ_WAVE);
    if (lane >= d) incl += o;
  }
  if (lane == QZ_WAVE - 1) s_w[wave] = incl;
  __syncthreads();
  int base = 0, tot = 0;
  #pragma unroll
  for (int w = 0; w < QZ_WAVES; ++w) {
    const int x = s_w[w];
    if (w < wave) base += x;
    tot += x;
  }
  __syncthreads();
  total = tot;
  return base + incl - v;
}
