// Colour bird's-eye view of the deployment pipeline: the camera frame warped to the bird's-eye
// view with the fixed-point bilinear law of include/fastscnn.h (what the reference's
// PerspectiveTransformer.transform_image_and_mask does to the image with cv2.INTER_LINEAR, border
// 0: kuruma/vision/transform.py:174-180), and in the same launch the segmented picture: that warped
// frame blended with the lane colour where a bird's-eye mask is set (create_visualization of the
// warped pair, kuruma/core/inference.py:275-287).
//
// A workgroup owns BI_T consecutive pixels of one view row of one image, a thread one pixel: the
// coordinates in fp64 exactly as bev.hip takes them (bv_scaled, bev_coord.hpp), four byte taps per
// channel from the frame (640 x 360 x 3 bytes: it stays in L2), integer weights.  The stores are
// the work: three bytes per pixel, and a row of the view starts on any byte (Wb * 3 is no multiple
// of 4 in general).  So the tile's bytes are staged in LDS behind a lead of as many bytes as the
// destination is past a dword boundary, which puts LDS dword d on global dword d, and are written
// as whole dwords; only the first and the last dword of a run go out byte by byte (bi_flush).
// channels_last tiles are one run of 3 * BI_T bytes, planar tiles three runs of BI_T bytes.
#include "bev_coord.hpp"
#include "common.hpp"
#include "kernels.hpp"
#include "overlay_blend.hpp"

#include <cmath>

namespace fscnn {

constexpr int BI_T = 256;                 // threads = pixels of a tile
constexpr int BI_PL = BI_T + 4;           // planar: LDS bytes of one plane's run (lead <= 3)
constexpr int BI_SEG = 3 * BI_PL;         // LDS bytes of one output's tile (channels_last: 3 + 3 * BI_T)
constexpr int BI_PD = 80;                 // planar flush: threads per plane, >= the run's dwords
static_assert(BI_PL % 4 == 0 && BI_SEG >= 3 + 3 * BI_T, "runs start on LDS dwords and fit");
static_assert(BI_PD * 4 >= 3 + BI_T + 3 && BI_PD * 3 <= BI_T, "a thread per dword of every plane");
static_assert(4 * BI_T >= 3 + 3 * BI_T + 3, "a thread per dword of a channels_last run");

// The run of len bytes that starts at g, staged at s + lead, lead = g's offset past a dword
// boundary (s itself on an LDS dword): thread d writes global dword d of the run's span, whole when
// all four bytes belong to the run, else its bytes one by one.
__device__ __forceinline__ int bi_lead(const uint8_t* g) { return (int)((uintptr_t)g & 3); }
__device__ __forceinline__ void bi_flush(const uint8_t* s, uint8_t* g, int len, int d) {
  const int lead = bi_lead(g);
  if (d * 4 >= lead + len) return;
  const int lo = max(d * 4, lead), hi = min(d * 4 + 4, lead + len);
  uint8_t* q = g - lead;  // the dword boundary at or before g; only bytes lo .. hi - 1 are touched
  if (hi - lo == 4) {
    *(uint32_t*)(q + d * 4) = *(const uint32_t*)(s + d * 4);
  } else {
    for (int b = lo; b < hi; ++b) q[b] = s[b];
  }
}

template <bool CL>
__global__ __launch_bounds__(BI_T) void bev_image_kernel(BevImageArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[2][BI_SEG];  // image, blended
  const int x0 = blockIdx.x * BI_T, y = blockIdx.y, n = blockIdx.z;
  const int t = threadIdx.x, x = x0 + t;
  const int cnt = min(BI_T, a.Wb - x0);  // >= 1
  const size_t hbwb = (size_t)a.Hb * a.Wb;
  const size_t pix0 = (size_t)n * hbwb + (size_t)y * a.Wb + x0;  // the tile's first view pixel
  // byte offset of the tile's run (channels_last) or of plane k's run in an output
  auto run = [&](int k) -> size_t {
    return CL ? pix0 * 3 : ((size_t)n * 3 + k) * hbwb + (size_t)y * a.Wb + x0;
  };
  if (t < cnt) {
    const double dy = (double)y;
    int fx, fy;
    bv_scaled(a.m, x, bv_mul(a.m[1], dy), bv_mul(a.m[4], dy), bv_mul(a.m[7], dy), 32.0, fx, fy);
    const int sx = fx >> 5, sy = fy >> 5, ax = fx & 31, ay = fy & 31;  // (sx + 1 <= 2^26)
    const size_t hw = (size_t)a.h * a.w;
    int S[3] = {0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int tx = sx + (j & 1), ty = sy + (j >> 1);
      const int wt = ((j & 1) ? ax : 32 - ax) * ((j >> 1) ? ay : 32 - ay);
      if (wt != 0 && tx >= 0 && tx < a.w && ty >= 0 && ty < a.h) {
        const size_t e = (size_t)ty * a.w + tx;
        const uint8_t* p = CL ? a.frames + ((size_t)n * hw + e) * 3 : a.frames + (size_t)n * 3 * hw + e;
#pragma unroll
        for (int k = 0; k < 3; ++k) S[k] += wt * (int)p[CL ? (size_t)k : (size_t)k * hw];
      }
    }
    const uint8_t L = a.blended ? a.bev_mask[pix0 + t] : 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const uint8_t v = (uint8_t)((S[k] + 512) >> 10);  // S <= 1024 * 255
      const int at = CL ? 3 * t + k : k * BI_PL + t;
      if (a.image) stage[0][at + bi_lead(a.image + run(k))] = v;
      if (a.blended)
        stage[1][at + bi_lead(a.blended + run(k))] =
            ov_blend((float)v, L ? (float)a.color[k] : 0.f, a.frame_weight, a.alpha, a.gamma);
    }
  }
  __syncthreads();
#pragma unroll
  for (int o = 0; o < 2; ++o) {
    uint8_t* out = o ? a.blended : a.image;
    if (!out) continue;
    if (CL) {
      bi_flush(stage[o], out + run(0), cnt * 3, t);
    } else {
      const int k = t / BI_PD;
      if (k < 3) bi_flush(stage[o] + k * BI_PL, out + run(k), cnt, t - k * BI_PD);
    }
  }
}

bool bev_image_ok(int N, int h, int w, int Hb, int Wb) {
  return N >= 1 && N <= 65535 && Hb >= 1 && Hb <= BEV_MAXH && Wb >= 1 && Wb <= BEV_MAXW &&
         h >= 2 && h <= E2E_MAXDIM && w >= 2 && w <= E2E_MAXDIM;
}

int bev_image(const BevImageArgs& a, hipStream_t st) {
  if (!a.frames || (!a.image && !a.blended)) {
    set_error("bev_image: null frames, or neither an image nor a blended output");
    return E_INVALID;
  }
  if (a.blended && !a.bev_mask) {
    set_error("bev_image: the blended output needs a bird's-eye mask and a color");
    return E_INVALID;
  }
  if (a.image == a.frames || a.blended == a.frames || a.image == a.blended ||
      (a.blended && (a.bev_mask == a.image || a.bev_mask == a.blended))) {
    set_error("bev_image: the outputs are fresh buffers; aliasing the frames, the mask or each "
              "other is refused");
    return E_INVALID;
  }
  for (int i = 0; i < 9; ++i)
    if (!std::isfinite(a.m[i])) {
      set_error("bev_image: m[%d] is not finite", i);
      return E_INVALID;
    }
  if (!bev_image_ok(a.N, a.h, a.w, a.Hb, a.Wb)) {
    set_error("bev_image: unsupported geometry (N=%d frame %dx%d view %dx%d; N <= 65535, frame "
              "sides 2 .. %d, view width 1 .. %d, height 1 .. %d)", a.N, a.w, a.h, a.Wb, a.Hb,
              E2E_MAXDIM, BEV_MAXW, BEV_MAXH);
    return E_UNSUPPORTED;
  }
  const dim3 grid((unsigned)cdiv(a.Wb, BI_T), (unsigned)a.Hb, (unsigned)a.N);
  if (a.channels_last) prof_launch(bev_image_kernel<true>, grid, BI_T, 0, st, a);
  else prof_launch(bev_image_kernel<false>, grid, BI_T, 0, st, a);
  return check_launch("bev_image");
}

}  // namespace fscnn
