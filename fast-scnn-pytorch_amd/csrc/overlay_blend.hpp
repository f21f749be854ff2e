// The blend of the overlay law (include/fastscnn.h), shared by overlay.hip and bev_image.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace fscnn {

// t = ((a * fw) + (o * alpha)) + gamma, each operation rounded to fp32 on its own, then
// saturate_cast<uchar>: round half to even, clamp, NaN -> 0.  Plain operators under contract(off):
// hipcc's default contraction reaches through __fmul_rn / __fadd_rn (common.hpp lerp2), and a fused
// a * 1 + 127.5 would round differently from the law.
__device__ __forceinline__ uint8_t ov_blend(float a, float o, float fw, float alpha, float gamma) {
#pragma clang fp contract(off)
  const float p = a * fw;
  const float q = o * alpha;
  const float s = p + q;
  float t = rintf(s + gamma);
  t = t > 0.f ? t : 0.f;  // (a NaN fails the comparison)
  t = t < 255.f ? t : 255.f;
  return (uint8_t)(int)t;
}

}  // namespace fscnn
