// The fp64 coordinate evaluation the bird's-eye kernels share (include/fastscnn.h: the coordinate
// laws of the mask warp, bev.hip, and of the frame warp, bev_image.hip).  Every operation is rounded
// on its own, so that a float64 numpy restatement gives the same integers.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>

namespace fscnn {

// hipcc contracts a * b + c into an fma by default, and through __dmul_rn / __dadd_rn too: their
// bodies are plain operators compiled under the same default (the ISA showed v_fma_f64 for
// m0*x + m1*y with them).  So the products and sums are written as operators inside blocks with
// contraction switched off, which is what keeps every operation rounded on its own; the ISA of
// these kernels holds no v_fma_f64 outside the division's refinement sequence.
__device__ __forceinline__ double bv_mul(double a, double b) {
#pragma clang fp contract(off)
  return a * b;
}

// Destination pixel (x, y) -> (rint(num * X / W), rint(num * Y / W)) as ints; m1y, m4y, m7y = the
// row's m1*y, m4*y, m7*y (bv_mul).  num = 1 gives the nearest source pixel, num = 32 the source
// position in 1/32 pixel.
__device__ __forceinline__ void bv_scaled(const double* m, int x, double m1y, double m4y,
                                          double m7y, double num, int& fxi, int& fyi) {
#pragma clang fp contract(off)
  const double dx = (double)x;
  const double X = (m[0] * dx + m1y) + m[2];
  const double Y = (m[3] * dx + m4y) + m[5];
  double W = (m[6] * dx + m7y) + m[8];
  W = W != 0.0 ? num / W : 0.0;  // (IEEE division: no fast-math flag in this build)
  // clamp to the int range the way std::max(INT_MIN, std::min(INT_MAX, v)) does (a NaN ends as
  // INT_MAX, which no source has), then round half to even
  double fx = X * W, fy = Y * W;
  fx = fx < (double)INT_MAX ? fx : (double)INT_MAX;
  fy = fy < (double)INT_MAX ? fy : (double)INT_MAX;
  fx = fx > (double)INT_MIN ? fx : (double)INT_MIN;
  fy = fy > (double)INT_MIN ? fy : (double)INT_MIN;
  fxi = (int)rint(fx);
  fyi = (int)rint(fy);
}

// The mask law for destination pixel (x, y): the nearest source pixel.
__device__ __forceinline__ void bv_source(const double* m, int x, double m1y, double m4y,
                                          double m7y, int& sx, int& sy) {
  bv_scaled(m, x, m1y, m4y, m7y, 1.0, sx, sy);
}

}  // namespace fscnn
