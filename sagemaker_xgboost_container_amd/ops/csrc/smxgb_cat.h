// Categorical (set-valued) split nodes, shared by the device kernels and the
// host traversal. A node's set R holds the categories that go RIGHT, as 256
// bits in CAT_WORDS 32-bit words: bit (c & 31) of word (c >> 5).
#pragma once

#define CAT_WORDS 8
#define CAT_MAX 256  // categories are the integers [0, CAT_MAX)

#if defined(__HIPCC__)
#define SMXGB_HD __host__ __device__
#else
#define SMXGB_HD
#endif

// bin / category b in [0, CAT_MAX) is a member of the set
SMXGB_HD inline bool cat_bit(const unsigned int* bits, int b) {
  return (bits[b >> 5] >> (b & 31)) & 1u;
}

// Decision at a categorical node for a value that is not NaN (the caller
// sends NaN the default way): a value outside [0, CAT_MAX) goes left;
// otherwise the category is the value truncated, and members go right.
SMXGB_HD inline bool cat_goes_left(float fv, const unsigned int* bits) {
  if (!(fv >= 0.0f) || fv >= (float)CAT_MAX) return true;
  return !cat_bit(bits, (int)fv);
}
