// Host tables of the GPU augmentation (augment.hip): what PIL computes once per resize / blur
// before it touches a pixel, for the crop window only.  The reference's per-sample pipeline
// (CitySegmentation._sync_transform, data_loader/cityscapes.py:115-150) is PIL's
//   img.resize(BILINEAR)  : Resample.c precompute_coeffs (triangle filter) + normalize_coeffs_8bpc
//   mask.resize(NEAREST)  : Geometry.c ImagingScaleAffine (xo = a/2; xo += a per output)
//   GaussianBlur(radius)  : BoxBlur.c _gaussian_blur_radius(radius, 3) + ImagingLineBoxBlur8 weights
// restated here in the same arithmetic (double / float as PIL uses them, same operation order) so
// the integer tables, and therefore every pixel, are the same.
#include <cmath>
#include <cstring>

#include "kernels.hpp"

namespace fscnn {

constexpr int SYNC_PRECISION_BITS = 32 - 8 - 2;  // Resample.c PRECISION_BITS
constexpr double SYNC_MAX_SCALE = 8.0;

// No multiply-add may be fused anywhere below: PIL's builds round every operation.
#pragma clang fp contract(off)

int sync_tables(int in_size, int out_size, int start, int count, int kmax, int* bounds, int* coef,
                int* nearest, int* ksize_out) {
  if (in_size < 1 || out_size < 1 || start < 0 || count < 1) {
    set_error("sync_tables: in=%d out=%d start=%d count=%d", in_size, out_size, start, count);
    return E_INVALID;
  }
  // (double)(in1 - in0) / outSize with the box corners held as float
  const double scale = (double)((float)in_size - 0.0f) / out_size;
  if (scale > SYNC_MAX_SCALE) {
    set_error("sync_tables: %d -> %d shrinks by more than %g", in_size, out_size, SYNC_MAX_SCALE);
    return E_INVALID;
  }
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 1.0 * filterscale;  // bilinear support 1.0
  const int ksize = (int)ceil(support) * 2 + 1;
  if (ksize_out) *ksize_out = ksize;
  if (!bounds && !coef && !nearest) return OK;  // size query
  if (!bounds || !coef || !nearest || kmax < ksize) {
    set_error("sync_tables: null table or kmax %d < ksize %d", kmax, ksize);
    return E_INVALID;
  }
  const double ss = 1.0 / filterscale;
  double w[2 * ((int)SYNC_MAX_SCALE + 1) + 1];
  for (int j = 0; j < count; ++j) {
    const int xx = start + j;
    int* k = coef + (size_t)j * kmax;
    memset(k, 0, sizeof(int) * kmax);
    if (xx >= out_size) {  // zero pad: no taps -> pixel 0
      bounds[2 * j] = in_size;
      bounds[2 * j + 1] = 0;
      continue;
    }
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    const int cnt = xmax - xmin;
    double ww = 0.0;
    for (int x = 0; x < cnt; ++x) {
      double v = (x + xmin - center + 0.5) * ss;
      if (v < 0.0) v = -v;
      w[x] = v < 1.0 ? 1.0 - v : 0.0;
      ww += w[x];
    }
    for (int x = 0; x < cnt; ++x) {
      if (ww != 0.0) w[x] /= ww;
      k[x] = w[x] < 0 ? (int)(-0.5 + w[x] * (1 << SYNC_PRECISION_BITS))
                      : (int)(0.5 + w[x] * (1 << SYNC_PRECISION_BITS));
    }
    bounds[2 * j] = xmin;
    bounds[2 * j + 1] = cnt;
  }
  // nearest: sequential additions from output 0, as ImagingScaleAffine runs them
  const double a = (double)in_size / out_size;
  double xo = a * 0.5;
  for (int j = 0; j < count; ++j) nearest[j] = -1;
  const int end = out_size < start + count ? out_size : start + count;
  for (int xx = 0; xx < end; ++xx) {
    if (xx >= start) {
      int idx = (int)xo;
      nearest[xx - start] = idx < in_size ? idx : in_size - 1;
    }
    xo += a;
  }
  return OK;
}

int sync_blur_weights(float radius, unsigned* ww_out, unsigned* fw_out) {
  if (!(radius >= 0.f) || !(radius < 1.f) || !ww_out || !fw_out) {
    set_error("sync_blur_weights: radius %g (supported: 0 <= radius < 1)", (double)radius);
    return E_INVALID;
  }
  const int passes = 3;
  const float sigma2 = radius * radius / passes;
  const float L = (float)sqrt(12.0 * sigma2 + 1.0);
  const float l = (float)floor((L - 1.0) / 2.0);
  float a = (2 * l + 1) * (l * (l + 1) - 3 * sigma2);
  a /= 6 * (sigma2 - (l + 1) * (l + 1));
  const float fr = l + a;
  const int ir = (int)fr;
  if (ir != 0) {
    set_error("sync_blur_weights: box radius %g >= 1", (double)fr);
    return E_INVALID;
  }
  const uint32_t ww = (uint32_t)((float)(1u << 24) / (fr * 2 + 1));
  const uint32_t fw = ((1u << 24) - (uint32_t)(ir * 2 + 1) * ww) / 2;
  *ww_out = ww;
  *fw_out = fw;
  return OK;
}

}  // namespace fscnn
