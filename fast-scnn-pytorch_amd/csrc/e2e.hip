// Deployment pipeline around an inference plan (EndToEndFastSCNN, export_onnx_fixed.py:34-98):
//   e2e_pre   raw 0..255 frames -> the backbone's input: bilinear resize to base x base, / 255,
//             optional (v - mean) / std                       (EndToEndPreprocessing, :62-98)
//   e2e_head  the low-resolution logits -> probabilities / logits / labels at the frame size: the
//             backbone's final x8 upsample (align_corners=True, models/fast_scnn.py:40), the resize
//             back to the frame (:54-55) and the softmax (:57-58) or the host's argmax * 255
//             (kuruma/core/preprocessing.py:53-79) in one pass; nothing of base x base is written.
//
// Both resizes are F.interpolate(mode='bilinear', align_corners=False) without antialiasing:
// output position o of an in -> out resize reads the source position
//     s = max((o + 0.5) * in / out - 0.5, 0),   taps floor(s) and min(floor(s) + 1, in - 1).
// s is the rational ((2o + 1) in - out) / (2 out); cf_tap evaluates it in integers (quotient =
// first tap, remainder / (2 out) = weight), so the taps are exact and the weight carries one fp32
// rounding, and the host's tile bounds agree with the kernel's indices by construction.
#include "e2e_pixel.hpp"

#include <algorithm>

namespace fscnn {

__device__ __forceinline__ float ld1(const uint8_t* p) { return (float)*p; }

// ---- front end -------------------------------------------------------------------------------------
// One thread: 8 consecutive X of one output row, the 3 channels in turn (the taps are shared).
// The frame is small next to the output (a 640x360 frame is 0.7 MB against 12.6 MB of fp32 input)
// and stays in cache; the stores are what the launch costs, so they go out as 16-B vectors
// wherever the row offset allows (always when base is a multiple of 8).
constexpr int EP_V = 8;

template <typename TX, typename TY>
__global__ __launch_bounds__(256) void e2e_pre_kernel(E2ePreArgs a, double inv) {
  const int XG = cdiv(a.base, EP_V);
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)a.N * a.base * XG) return;
  const int xg = (int)(t % XG);
  const long long rest = t / XG;
  const int Y = (int)(rest % a.base), n = (int)(rest / a.base);
  const int X0 = xg * EP_V;
  const CfTap ty = cf_tap(Y, a.h, a.base, inv);
  long long o0[EP_V], o1[EP_V];
  float wx[EP_V];
#pragma unroll
  for (int j = 0; j < EP_V; ++j) {  // (columns past the row are computed on a clamped X, not stored)
    const CfTap tx = cf_tap(min(X0 + j, a.base - 1), a.w, a.base, inv);
    o0[j] = tx.i0 * a.sx;
    o1[j] = tx.i1 * a.sx;
    wx[j] = tx.w;
  }
  const float wy1 = ty.w, wy0 = 1.0f - ty.w;
  const TX* xb = (const TX*)a.x + (long long)n * a.sn;
#pragma unroll 1
  for (int c = 0; c < 3; ++c) {
    const TX* r0 = xb + (a.bgr ? 2 - c : c) * a.sc + ty.i0 * a.sy;
    const TX* r1 = xb + (a.bgr ? 2 - c : c) * a.sc + ty.i1 * a.sy;
    float o[EP_V];
#pragma unroll
    for (int j = 0; j < EP_V; ++j) {
      const float top = lerp2(1.0f - wx[j], ld1(r0 + o0[j]), wx[j], ld1(r0 + o1[j]));
      const float bot = lerp2(1.0f - wx[j], ld1(r1 + o0[j]), wx[j], ld1(r1 + o1[j]));
      const float v = lerp2(wy0, top, wy1, bot);
      o[j] = (float)fma((double)v, a.A[c], a.B[c]);  // / 255 and the normalisation, unrounded
    }
    TY* yp = (TY*)a.y + (((long long)n * 3 + c) * a.base + Y) * a.base + X0;
    if (X0 + EP_V <= a.base && ((uintptr_t)yp & 15) == 0) {
      if constexpr (sizeof(TY) == 4) {
        const float lo4[4] = {o[0], o[1], o[2], o[3]}, hi4[4] = {o[4], o[5], o[6], o[7]};
        stv(yp, lo4);
        stv(yp + 4, hi4);
      } else {
        stv(yp, o);
      }
    } else {
#pragma unroll
      for (int j = 0; j < EP_V; ++j)
        if (X0 + j < a.base) st1(yp + j, o[j]);
    }
  }
}

int e2e_pre(const E2ePreArgs& a, int x_dtype, int y_dtype, hipStream_t st) {
  if (a.N < 1 || a.h < 2 || a.w < 2 || a.base < 1 || a.h > E2E_MAXDIM || a.w > E2E_MAXDIM ||
      a.base > E2E_MAXDIM) {
    set_error("e2e_pre: N=%d frame %dx%d base %d (frame sides 2 .. %d, base 1 .. %d)", a.N, a.h,
              a.w, a.base, E2E_MAXDIM, E2E_MAXDIM);
    return E_INVALID;
  }
  if (x_dtype < DT_F32 || x_dtype > DT_U8 || y_dtype < DT_F32 || y_dtype > DT_F16) {
    set_error("e2e_pre: frame dtype %d (0 fp32, 1 bf16, 2 fp16, 3 uint8), output dtype %d (0 .. 2)",
              x_dtype, y_dtype);
    return E_INVALID;
  }
  const long long total = (long long)a.N * a.base * cdiv(a.base, EP_V);
  if ((total + 255) / 256 >= (1LL << 31)) {
    set_error("e2e_pre: N=%d base=%d is too large for one launch", a.N, a.base);
    return E_UNSUPPORTED;
  }
  const unsigned grid = (unsigned)((total + 255) / 256);
  const double inv = 1.0 / (2.0 * a.base);
#define EP_LAUNCH(TX)                                                                      \
  do {                                                                                     \
    if (y_dtype == DT_F32) prof_launch(e2e_pre_kernel<TX, float>, grid, 256, 0, st, a, inv); \
    else if (y_dtype == DT_F16) prof_launch(e2e_pre_kernel<TX, f16>, grid, 256, 0, st, a, inv); \
    else prof_launch(e2e_pre_kernel<TX, bf16>, grid, 256, 0, st, a, inv);                 \
  } while (0)
  if (x_dtype == DT_U8) EP_LAUNCH(uint8_t);
  else if (x_dtype == DT_F32) EP_LAUNCH(float);
  else if (x_dtype == DT_F16) EP_LAUNCH(f16);
  else EP_LAUNCH(bf16);
#undef EP_LAUNCH
  return check_launch("e2e_pre");
}

// ---- tail -----------------------------------------------------------------------------------------
// A workgroup owns EE_TH output rows x EE_TW output columns of one image, one thread per pixel.
// The base-grid rows / columns its pixels tap, and through them the low-resolution rows / columns
// those taps interpolate from, form one window (every index law here is monotone), staged once in
// LDS class-major [row][C][WP] in fp32 like up_argmax's rows.  Per class a thread forms its four
// base-grid taps exactly as up_nchw stores them (ac_lerp weights, lerp2 W-then-H, tap_as_stored),
// combines them in fp32 (ee_pixel, e2e_pixel.hpp: shared with the bird's-eye tail) and keeps the
// C values in registers (CB = the unrolled class bound) for the max-subtracted softmax or the
// argmax (strict >: the lowest class wins ties).
constexpr int EE_TW = 64, EE_TH = 4, EE_T = EE_TW * EE_TH;

struct EeGeom {
  int rows, cols;  // largest staged window of any tile
};
static EeGeom ee_geom(int Hl, int Wl, int base, int Ho, int Wo) {
  const float sl_h = ac_scale(Hl, base), sl_w = ac_scale(Wl, base);
  const double ih = 1.0 / (2.0 * Ho), iw = 1.0 / (2.0 * Wo);
  EeGeom g{0, 0};
  for (int y0 = 0; y0 < Ho; y0 += EE_TH) {
    const int y1 = std::min(y0 + EE_TH, Ho) - 1;
    const int lo = ac_lerp(cf_tap(y0, base, Ho, ih).i0, Hl, base, sl_h).i0;
    g.rows = std::max(g.rows, ac_lerp(cf_tap(y1, base, Ho, ih).i1, Hl, base, sl_h).i1 - lo + 1);
  }
  for (int x0 = 0; x0 < Wo; x0 += EE_TW) {
    const int x1 = std::min(x0 + EE_TW, Wo) - 1;
    const int lo = ac_lerp(cf_tap(x0, base, Wo, iw).i0, Wl, base, sl_w).i0;
    g.cols = std::max(g.cols, ac_lerp(cf_tap(x1, base, Wo, iw).i1, Wl, base, sl_w).i1 - lo + 1);
  }
  return g;
}

__device__ __forceinline__ void ee_store(void* p, int dtype, size_t i, float v) {
  if (dtype == DT_F32) ((float*)p)[i] = v;
  else if (dtype == DT_F16) st1((f16*)p + i, v);
  else st1((bf16*)p + i, v);
}

// the staged window as ee_pixel's row accessor: it starts at low-res row lo, column cl0
struct EeLdsRows {
  const float* w;
  int lo, cl0, CWP, WP;
  __device__ __forceinline__ int row(int r) const { return (r - lo) * CWP; }
  __device__ __forceinline__ float at(int row, int c, int col) const {
    return w[row + c * WP + (col - cl0)];
  }
};

template <typename TI, int CB>
__global__ __launch_bounds__(EE_T) void e2e_head_kernel(E2eHeadArgs a, int WP, double ih, double iw) {
  extern __shared__ float ee_rows[];  // [rows][C][WP]
  const int n = blockIdx.z, C = a.C;
  const int yo0 = blockIdx.y * EE_TH, xo0 = blockIdx.x * EE_TW;
  const int yo1 = min(yo0 + EE_TH, a.Ho) - 1, xo1 = min(xo0 + EE_TW, a.Wo) - 1;
  const float sl_h = ac_scale(a.Hl, a.base), sl_w = ac_scale(a.Wl, a.base);
  // the tile's low-res window (ee_geom bounds nrows x ncols by the LDS the launch got)
  const int lo = ac_lerp(cf_tap(yo0, a.base, a.Ho, ih).i0, a.Hl, a.base, sl_h).i0;
  const int nrows = ac_lerp(cf_tap(yo1, a.base, a.Ho, ih).i1, a.Hl, a.base, sl_h).i1 - lo + 1;
  const int cl0 = ac_lerp(cf_tap(xo0, a.base, a.Wo, iw).i0, a.Wl, a.base, sl_w).i0;
  const int ncols = ac_lerp(cf_tap(xo1, a.base, a.Wo, iw).i1, a.Wl, a.base, sl_w).i1 - cl0 + 1;
  const int CWP = C * WP, CN = C * ncols;
  {
    const TI* xb = (const TI*)a.logits + (((size_t)n * a.Hl + lo) * a.Wl + cl0) * a.ldx;
    for (int e = threadIdx.x; e < nrows * CN; e += EE_T) {
      const int r = e / CN;
      const int rem = e - r * CN;
      const int wi = rem / C, c = rem - wi * C;
      ee_rows[r * CWP + c * WP + wi] = ld1(xb + ((size_t)r * a.Wl + wi) * a.ldx + c);
    }
  }
  __syncthreads();
  const int xo = xo0 + threadIdx.x % EE_TW, yo = yo0 + threadIdx.x / EE_TW;
  if (xo > xo1 || yo > yo1) return;
  const EeGrid g{a.Hl, a.Wl, a.base, a.Ho, a.Wo, C, a.f16_once, ih, iw};
  const EeLdsRows rows{ee_rows, lo, cl0, CWP, WP};
  float v[CB];
  ee_pixel<TI, CB>(g, xo, yo, rows, v);
  float m;
  const int arg = ee_argmax<CB>(v, m);
  const size_t pix = ((size_t)n * a.Ho + yo) * a.Wo + xo;
  if (a.labels) a.labels[pix] = (uint8_t)(arg * a.label_scale);
  if (!a.probs) return;
  if (a.softmax) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < CB; ++c) {
      v[c] = c < C ? expf(v[c] - m) : 0.f;
      s += v[c];
    }
#pragma unroll
    for (int c = 0; c < CB; ++c) v[c] = v[c] / s;
  }
  const size_t plane = (size_t)a.Ho * a.Wo;
  const size_t o0 = (size_t)n * C * plane + (size_t)yo * a.Wo + xo;
#pragma unroll
  for (int c = 0; c < CB; ++c)
    if (c < C) ee_store(a.probs, a.probs_dtype, o0 + c * plane, v[c]);
}

int ee_f16_once(int N, int Hl, int Wl, int C, int base) {
  UpArgs u{};
  u.N = N; u.Hi = Hl; u.Wi = Wl; u.C = C; u.Ho = base; u.Wo = base;
  return !(up_nchw_rows_path(u) && base % 4 == 0);
}

bool e2e_head_ok(int N, int C, int Hl, int Wl, int base, int Ho, int Wo) {
  if (N < 1 || N > 65535 || C < 1 || C > EE_CMAX || Hl < 1 || Wl < 1 || base < 1 || Ho < 1 ||
      Wo < 1 || base > E2E_MAXDIM || Ho > E2E_MAXDIM || Wo > E2E_MAXDIM)
    return false;
  const EeGeom g = ee_geom(Hl, Wl, base, Ho, Wo);
  return (size_t)g.rows * C * (g.cols | 1) * sizeof(float) <= 64 * 1024;
}

int e2e_head(const E2eHeadArgs& a0, int dtype, hipStream_t st) {
  E2eHeadArgs a = a0;
  a.f16_once = ee_f16_once(a.N, a.Hl, a.Wl, a.C, a.base);
  if (a.probs && (a.probs_dtype < DT_F32 || a.probs_dtype > DT_F16)) {
    set_error("e2e_head: probs dtype %d (0 fp32, 1 bf16, 2 fp16)", a.probs_dtype);
    return E_INVALID;
  }
  if (a.ldx < a.C) {
    set_error("e2e_head: ldx=%d below C=%d", a.ldx, a.C);
    return E_INVALID;
  }
  if (!e2e_head_ok(a.N, a.C, a.Hl, a.Wl, a.base, a.Ho, a.Wo)) {
    set_error("e2e_head: unsupported geometry (N=%d C=%d low-res %dx%d base %d out %dx%d)", a.N,
              a.C, a.Hl, a.Wl, a.base, a.Ho, a.Wo);
    return E_UNSUPPORTED;
  }
  if (!a.probs && !a.labels) return OK;
  const EeGeom g = ee_geom(a.Hl, a.Wl, a.base, a.Ho, a.Wo);
  const int wp = g.cols | 1;  // odd plane stride: the staging stores walk c
  const size_t lds = (size_t)g.rows * a.C * wp * sizeof(float);
  const dim3 grid((unsigned)cdiv(a.Wo, EE_TW), (unsigned)cdiv(a.Ho, EE_TH), (unsigned)a.N);
  const double ih = 1.0 / (2.0 * a.Ho), iw = 1.0 / (2.0 * a.Wo);
#define EE_LAUNCH(TI)                                                                    \
  do {                                                                                   \
    if (a.C <= 2) prof_launch(e2e_head_kernel<TI, 2>, grid, EE_T, lds, st, a, wp, ih, iw); \
    else if (a.C <= 8) prof_launch(e2e_head_kernel<TI, 8>, grid, EE_T, lds, st, a, wp, ih, iw); \
    else prof_launch(e2e_head_kernel<TI, EE_CMAX>, grid, EE_T, lds, st, a, wp, ih, iw);  \
  } while (0)
  if (dtype == DT_F32) EE_LAUNCH(float);
  else if (dtype == DT_F16) EE_LAUNCH(f16);
  else if (dtype == DT_BF16) EE_LAUNCH(bf16);
  else {
    set_error("e2e_head: logits dtype %d (0 fp32, 1 bf16, 2 fp16)", dtype);
    return E_INVALID;
  }
#undef EE_LAUNCH
  return check_launch("e2e_head");
}

}  // namespace fscnn
