// The draw of the sampled (mean) LambdaRank pair method: a pure integer
// function of (seed, round, row, t), so the pair set is the same on every
// run, for every tile packing and whatever the margins are. Mirrored in
// numpy uint64 by ops/torch_ref.lambdarank_mix; all arithmetic is mod 2^64.
//
//   fin(z): z ^= z >> 30; z *= 0xbf58476d1ce4e5b9; z ^= z >> 27;
//           z *= 0x94d049bb133111eb; z ^= z >> 31      (splitmix64 finaliser)
//   key  = fin(seed + 0x9e3779b97f4a7c15 * (round + 1))
//   mix  = fin(key ^ ((row << 12) | t)),  row < 2^31, t < 4096
//   partner of local index a in a group of m >= 2 documents:
//     b = ((mix >> 32) * (m - 1)) >> 32;  b += (b >= a)
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define LR_MIX_FN __host__ __device__ static inline
#else
#define LR_MIX_FN static inline
#endif

LR_MIX_FN uint64_t lr_mix_fin(uint64_t z) {
  z ^= z >> 30;
  z *= 0xbf58476d1ce4e5b9ull;
  z ^= z >> 27;
  z *= 0x94d049bb133111ebull;
  z ^= z >> 31;
  return z;
}

// the part of the draw that a call shares: once per thread
LR_MIX_FN uint64_t lr_mix_key(uint64_t seed, uint64_t round) {
  return lr_mix_fin(seed + 0x9e3779b97f4a7c15ull * (round + 1ull));
}

LR_MIX_FN uint64_t lr_mix(uint64_t key, uint64_t row, uint64_t t) {
  return lr_mix_fin(key ^ ((row << 12) | t));
}

// local index of the partner that document a (< m) of a group of m >= 2
// draws from r = lr_mix(...): uniform over the other m - 1 documents
LR_MIX_FN uint32_t lr_mix_partner(uint64_t r, uint32_t a, uint32_t m) {
  const uint32_t b = (uint32_t)(((r >> 32) * (uint64_t)(m - 1u)) >> 32);
  return b + (b >= a ? 1u : 0u);
}
