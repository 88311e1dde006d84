// Device helpers shared by the path-form TreeSHAP kernels
// (smxgb_kernels.hip, smxgb_shap_compact.hip) and the CSR kernels
// (smxgb_sparse.hip). Each helper exists once, here.
#pragma once

#include <hip/hip_runtime.h>

#define SHAP_BLOCK 256
#define SHAP_F_NAN 1     // missing values follow this path on this feature
#define SHAP_F_LO 2      // path has a right turn on this feature (x >= lo)
#define SHAP_F_HI 4      // path has a left turn on this feature  (x <  hi)

__device__ inline double shap_one_fraction(float x, float lo, float hi, int flags) {
  if (isnan(x)) return (flags & SHAP_F_NAN) ? 1.0 : 0.0;
  const bool ok = (!(flags & SHAP_F_LO) || x >= lo) && (!(flags & SHAP_F_HI) || x < hi);
  return ok ? 1.0 : 0.0;
}

// Lane `gl` of a W-wide group holds element gl (z, o) of a path of `len`
// elements (element 0 = dummy root, z = o = 1). Returns the unwound
// permutation-weight sum for this lane's element. Must be called by all W
// lanes of the group; `lmax` (>= len, <= W) is the uniform shuffle bound.
__device__ inline double shap_unwound_sum(double z, double o, int gl, int len, int lmax,
                                          int W) {
  double w = gl == 0 ? 1.0 : 0.0;
  for (int d = 1; d < lmax; ++d) {
    const double zd = __shfl(z, d, W);
    const double od = __shfl(o, d, W);
    const double wl = __shfl_up(w, 1, W);
    if (d < len) {
      const double inv = 1.0 / (d + 1);
      double nw = 0.0;
      if (gl <= d) {
        nw = zd * w * (d - gl) * inv;
        if (gl > 0) nw += od * wl * gl * inv;
      }
      w = nw;
    }
  }
  const int D = len - 1;
  double next = __shfl(w, D > 0 ? D : 0, W);
  double total = 0.0;
  for (int j = lmax - 2; j >= 0; --j) {
    const double wj = __shfl(w, j, W);
    if (j < D) {
      if (o != 0.0) {
        const double tmp = next * (D + 1) / ((j + 1) * o);
        total += tmp;
        next = wj - tmp * z * (D - j) / (double)(D + 1);
      } else if (z != 0.0) {
        total += (wj / z) * (D + 1) / (double)(D - j);
      }
    }
  }
  return total;
}

// position of `feature` among the sorted column ids [lo, hi), or -1
__device__ inline long long csr_find(const int* __restrict__ indices, long long lo,
                                     long long hi, int feature) {
  while (lo < hi) {
    const long long mid = lo + ((hi - lo) >> 1);
    const int c = indices[mid];
    if (c < feature) {
      lo = mid + 1;
    } else if (c > feature) {
      hi = mid;
    } else {
      return mid;
    }
  }
  return -1;
}
