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
#include "kernels.hpp"

#include <algorithm>

namespace fscnn {

struct CfTap {
  int i0, i1;
  float w;  // weight of tap i1
};
// inv = 1.0 / (2 out): the double product lands within one of the quotient, which the remainder
// test then settles exactly (numerators stay below 2^30: E2E_MAXDIM)
__host__ __device__ __forceinline__ CfTap cf_tap(int o, int in, int out, double inv) {
  int num = (2 * o + 1) * in - out;
  num = num < 0 ? 0 : num;
  const int d = 2 * out;
  int q = (int)((double)num * inv);
  int r = num - q * d;
  if (r < 0) {
    --q;
    r += d;
  } else if (r >= d) {
    ++q;
    r -= d;
  }
  CfTap t;
  t.i0 = q;  // <= in - 1: num < 2 out in
  t.i1 = q + 1 < in ? q + 1 : in - 1;
  t.w = (float)r / (float)d;  // both exact in fp32 (d <= 2^15)
  return t;
}

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
// combines them in fp32 and keeps the C values in registers (CB = the unrolled class bound) for
// the max-subtracted softmax or the argmax (strict >: the lowest class wins ties).
constexpr int EE_TW = 64, EE_TH = 4, EE_T = EE_TW * EE_TH;
constexpr int EE_CMAX = 32;

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

// A tap as the forward stores it: lerp2(l0, x0, l1, x1) in the logits dtype.  fp32 and bf16 have
// one answer.  fp16 has two: the fp32 value converted (two roundings), or v_fma_mixlo_f16, which
// rounds the exact fma once, straight to fp16 -- what the compiler makes of f2h(fmaf(..)) where it
// can -- and they differ by one fp16 ulp at a few values in 10^5.  up_nchw's stores use both: its
// row-group kernel with vector stores (plans whose width is a multiple of 4) rounds once in column
// 0 of each 4-vector and twice in columns 1 .. 3; its other forms round once everywhere (read from
// the ISA of interp.hip; tests/test_gpu_e2e.py compares every tap with the stored logits).  Both
// forms are spelled out here so that this kernel's own codegen has no say.
template <typename TI>
__device__ __forceinline__ float tap_as_stored(float l0, float x0, float l1, float x1, bool once) {
  if constexpr (std::is_same<TI, f16>::value) {
    const float p = l1 * x1;
    if (once) {
      uint32_t h;  // (the instruction writes the low half only)
      asm("v_fma_mixlo_f16 %0, %1, %2, %3" : "=v"(h) : "v"(l0), "v"(x0), "v"(p));
      return h2f((uint16_t)(h & 0xFFFFu));
    }
    float v = fmaf(l0, x0, p);
    asm("" : "+v"(v));  // keeps the fp32 value apart from its conversion
    return h2f(f2h(v));
  } else {
    return round_as<TI>(lerp2(l0, x0, l1, x1));
  }
}

__device__ __forceinline__ void ee_store(void* p, int dtype, size_t i, float v) {
  if (dtype == DT_F32) ((float*)p)[i] = v;
  else if (dtype == DT_F16) st1((f16*)p + i, v);
  else st1((bf16*)p + i, v);
}

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
  const CfTap ty = cf_tap(yo, a.base, a.Ho, ih), tx = cf_tap(xo, a.base, a.Wo, iw);
  Lerp lh[2] = {ac_lerp(ty.i0, a.Hl, a.base, sl_h), ac_lerp(ty.i1, a.Hl, a.base, sl_h)};
  Lerp lw[2] = {ac_lerp(tx.i0, a.Wl, a.base, sl_w), ac_lerp(tx.i1, a.Wl, a.base, sl_w)};
#pragma unroll
  for (int k = 0; k < 2; ++k) {  // offsets into the staged window
    lh[k].i0 = (lh[k].i0 - lo) * CWP;
    lh[k].i1 = (lh[k].i1 - lo) * CWP;
    lw[k].i0 -= cl0;
    lw[k].i1 -= cl0;
  }
  const float wy0 = 1.0f - ty.w, wx0 = 1.0f - tx.w;
  const bool once[2] = {a.f16_once || (tx.i0 & 3) == 0, a.f16_once || (tx.i1 & 3) == 0};
  float v[CB];
#pragma unroll
  for (int c = 0; c < CB; ++c) {
    v[c] = -INFINITY;
    if (c < C) {
      const float* pc = ee_rows + c * WP;
      float t[2][2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const float* r0 = pc + lh[i].i0;
        const float* r1 = pc + lh[i].i1;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const float x0 = lerp2(lw[j].l0, r0[lw[j].i0], lw[j].l1, r0[lw[j].i1]);
          const float x1 = lerp2(lw[j].l0, r1[lw[j].i0], lw[j].l1, r1[lw[j].i1]);
          t[i][j] = tap_as_stored<TI>(lh[i].l0, x0, lh[i].l1, x1, once[j]);  // up_nchw's logit
        }
      }
      v[c] = lerp2(wy0, lerp2(wx0, t[0][0], tx.w, t[0][1]), ty.w, lerp2(wx0, t[1][0], tx.w, t[1][1]));
    }
  }
  float m = v[0];
  int arg = 0;
#pragma unroll
  for (int c = 1; c < CB; ++c) {
    const bool gt = v[c] > m;  // (classes >= C hold -inf and never win)
    m = gt ? v[c] : m;
    arg = gt ? c : arg;
  }
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

bool e2e_head_ok(int N, int C, int Hl, int Wl, int base, int Ho, int Wo) {
  if (N < 1 || N > 65535 || C < 1 || C > EE_CMAX || Hl < 1 || Wl < 1 || base < 1 || Ho < 1 ||
      Wo < 1 || base > E2E_MAXDIM || Ho > E2E_MAXDIM || Wo > E2E_MAXDIM)
    return false;
  const EeGeom g = ee_geom(Hl, Wl, base, Ho, Wo);
  return (size_t)g.rows * C * (g.cols | 1) * sizeof(float) <= 64 * 1024;
}

int e2e_head(const E2eHeadArgs& a0, int dtype, hipStream_t st) {
  E2eHeadArgs a = a0;
  {
    UpArgs u{};
    u.N = a.N; u.Hi = a.Hl; u.Wi = a.Wl; u.C = a.C; u.Ho = a.base; u.Wo = a.base;
    a.f16_once = !(up_nchw_rows_path(u) && a.base % 4 == 0);
  }
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
