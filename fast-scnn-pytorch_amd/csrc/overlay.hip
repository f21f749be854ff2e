// Overlay tail of the deployment pipeline: the picture every consumer of the exported model
// builds on the host from the frame and the lane mask (create_visualization,
// kuruma/core/preprocessing.py:85-104: green where mask > 0, cv2.addWeighted(frame, 1, green,
// alpha, 0); the evaluation scripts: a per-class colour image at 0.7 / 0.3 or 0.6 / 0.4), after the
// nearest-neighbour resize of the mask back to the camera frame (postprocess_matched_resolution,
// :53-79).  The law is stated in include/fastscnn.h; ov_src / ov_blend (overlay_blend.hpp) are its
// two halves.
//   overlay_mask   frames + a uint8 mask in memory: pure streaming, a thread owns 4 consecutive
//                  pixels of a frame row
//   e2e_overlay    frames + the low-resolution logits: a workgroup owns OV_TW x OV_TH frame pixels,
//                  stages the low-resolution window their source pixels tap in LDS exactly as
//                  e2e_head does (frame pixel -> source pixel is monotone too, so the window is
//                  still the span between the tile's corners), every thread takes the class of one
//                  frame pixel with ee_pixel / ee_argmax (the bits of predict), the tile's classes
//                  go through 256 bytes of LDS, and the first wave blends and stores 4 pixels per
//                  thread with the routine overlay_mask uses.  Neither a mask nor a probability is
//                  written unless the caller asks for the frame-size mask.
#include "e2e_pixel.hpp"
#include "overlay_blend.hpp"

#include <algorithm>

namespace fscnn {

constexpr int OV_G = 4;  // pixels per thread: NHWC stores are 3 dwords, NCHW plane stores 1
constexpr int OV_TW = 64, OV_TH = 4, OV_T = OV_TW * OV_TH;

// source index of frame index x: floor(x * M / w) as a rational (cv2.INTER_NEAREST), x * M < 2^28
__host__ __device__ __forceinline__ int ov_src(int x, int M, int w) {
  return M == w ? x : (int)((unsigned)(x * M) / (unsigned)w);
}

__device__ __forceinline__ float ov_ld(const uint8_t* p) { return (float)*p; }
__device__ __forceinline__ float ov_ld(const float* p) { return *p; }
__device__ __forceinline__ float ov_ld(const f16* p) { return ld1(p); }
__device__ __forceinline__ float ov_ld(const bf16* p) { return ld1(p); }

__device__ __forceinline__ uint32_t ov_pack(const uint8_t* r) {
  return (uint32_t)r[0] | ((uint32_t)r[1] << 8) | ((uint32_t)r[2] << 16) | ((uint32_t)r[3] << 24);
}
// nb bytes of r to q: dwords when the group is whole and q is dword-aligned (a row whose byte
// offset is not a multiple of 4 takes the byte path), else the first `valid` bytes one by one
template <int NB>
__device__ __forceinline__ void ov_store(uint8_t* q, const uint8_t (&r)[NB], int valid) {
  if (valid == NB && ((uintptr_t)q & 3) == 0) {
#pragma unroll
    for (int i = 0; i < NB / 4; ++i) ((uint32_t*)q)[i] = ov_pack(r + 4 * i);
  } else {
#pragma unroll
    for (int i = 0; i < NB; ++i)
      if (i < valid) q[i] = r[i];
  }
}

// The pixel routine both kernels share: pixels x0 .. x0 + OV_G - 1 (those below w) of row y of
// image n, o[j] = the colour and L[j] = the label byte of pixel x0 + j.
template <typename TX>
__device__ __forceinline__ void ov_group(const OverlayArgs& a, int n, int y, int x0,
                                         const uint8_t (&o)[OV_G][3], const uint8_t (&L)[OV_G]) {
  const int cnt = min(OV_G, a.w - x0);
  const size_t hw = (size_t)a.h * a.w;
  const size_t pix = ((size_t)n * a.h + y) * a.w + x0;
  if (a.channels_last) {
    const TX* f = (const TX*)a.frames + pix * 3;
    uint8_t r[OV_G * 3];
#pragma unroll
    for (int j = 0; j < OV_G; ++j)
#pragma unroll
      for (int k = 0; k < 3; ++k)
        r[j * 3 + k] = j < cnt ? ov_blend(ov_ld(f + j * 3 + k), (float)o[j][k], a.frame_weight,
                                          a.alpha, a.gamma)
                               : 0;
    ov_store(a.out + pix * 3, r, cnt * 3);
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const size_t e = ((size_t)n * 3 + k) * hw + (size_t)y * a.w + x0;
      const TX* f = (const TX*)a.frames + e;
      uint8_t r[OV_G];
#pragma unroll
      for (int j = 0; j < OV_G; ++j)
        r[j] = j < cnt ? ov_blend(ov_ld(f + j), (float)o[j][k], a.frame_weight, a.alpha, a.gamma)
                       : 0;
      ov_store(a.out + e, r, cnt);
    }
  }
  if (a.mask_out) ov_store(a.mask_out + pix, L, cnt);
}

__device__ __forceinline__ void ov_group_any(const OverlayArgs& a, int n, int y, int x0,
                                             const uint8_t (&o)[OV_G][3], const uint8_t (&L)[OV_G]) {
  if (a.frame_dtype == DT_U8) ov_group<uint8_t>(a, n, y, x0, o, L);
  else if (a.frame_dtype == DT_F32) ov_group<float>(a, n, y, x0, o, L);
  else if (a.frame_dtype == DT_F16) ov_group<f16>(a, n, y, x0, o, L);
  else ov_group<bf16>(a, n, y, x0, o, L);
}

// ---- a mask in memory ------------------------------------------------------------------------------
struct OvLaneColor {  // create_visualization: the colour where the mask byte is not 0
  uint8_t c[3];
  __device__ __forceinline__ uint8_t operator()(uint8_t L, int k) const { return L ? c[k] : 0; }
};
struct OvPalette {  // the mask byte is a class id: palette[id], 0 from row P on
  const uint8_t* p;
  int P;
  __device__ __forceinline__ uint8_t operator()(uint8_t L, int k) const {
    return L < P ? p[(int)L * 3 + k] : 0;
  }
};

template <typename Col>
__global__ __launch_bounds__(256) void overlay_mask_kernel(OverlayArgs a, const uint8_t* mask,
                                                           int Hm, int Wm, Col col) {
  const int XG = cdiv(a.w, OV_G);
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)a.N * a.h * XG) return;
  const int xg = (int)(t % XG);
  const long long rest = t / XG;
  const int y = (int)(rest % a.h), n = (int)(rest / a.h);
  const int x0 = xg * OV_G;
  const uint8_t* mrow = mask + ((size_t)n * Hm + ov_src(y, Hm, a.h)) * Wm;
  uint8_t L[OV_G], o[OV_G][3];
#pragma unroll
  for (int j = 0; j < OV_G; ++j) {  // (columns past the row read a clamped x and are not stored)
    L[j] = mrow[ov_src(min(x0 + j, a.w - 1), Wm, a.w)];
#pragma unroll
    for (int k = 0; k < 3; ++k) o[j][k] = col(L[j], k);
  }
  ov_group_any(a, n, y, x0, o, L);
}

static int ov_check(const char* who, const OverlayArgs& a) {
  if (!a.frames || !a.out) {
    set_error("%s: null frames or out", who);
    return E_INVALID;
  }
  if ((const void*)a.out == a.frames || (a.mask_out && (a.mask_out == a.out ||
                                                        (const void*)a.mask_out == a.frames))) {
    set_error("%s: the outputs are fresh buffers; aliasing the frames is refused", who);
    return E_INVALID;
  }
  if (a.frame_dtype < DT_F32 || a.frame_dtype > DT_U8) {
    set_error("%s: frame dtype %d (0 fp32, 1 bf16, 2 fp16, 3 uint8)", who, a.frame_dtype);
    return E_INVALID;
  }
  if (a.N < 1 || a.h < 2 || a.w < 2) {
    set_error("%s: N=%d frame %dx%d (N >= 1, frame sides >= 2)", who, a.N, a.h, a.w);
    return E_INVALID;
  }
  return OK;
}

int overlay_mask(const OverlayArgs& a, const uint8_t* mask, int Hm, int Wm,
                 const OverlayColors& colors, const uint8_t* palette, int P, hipStream_t st) {
  if (int rc = ov_check("overlay_mask", a)) return rc;
  if (!mask || Hm < 1 || Wm < 1 || (const void*)mask == (const void*)a.out) {
    set_error("overlay_mask: null, empty or aliased mask (%dx%d)", Hm, Wm);
    return E_INVALID;
  }
  if (palette && (P < 1 || P > 256)) {
    set_error("overlay_mask: a palette has 1 .. 256 rows, got %d", P);
    return E_INVALID;
  }
  const long long total = (long long)a.N * a.h * cdiv(a.w, OV_G);
  if (a.h > E2E_MAXDIM || a.w > E2E_MAXDIM || Hm > E2E_MAXDIM || Wm > E2E_MAXDIM ||
      (total + 255) / 256 >= (1LL << 31)) {
    set_error("overlay_mask: unsupported geometry (N=%d frame %dx%d mask %dx%d; every size <= %d)",
              a.N, a.h, a.w, Hm, Wm, E2E_MAXDIM);
    return E_UNSUPPORTED;
  }
  const unsigned grid = (unsigned)((total + 255) / 256);
  if (palette)
    prof_launch(overlay_mask_kernel<OvPalette>, grid, 256, 0, st, a, mask, Hm, Wm,
                OvPalette{palette, P});
  else
    prof_launch(overlay_mask_kernel<OvLaneColor>, grid, 256, 0, st, a, mask, Hm, Wm,
                OvLaneColor{{colors.c[0][0], colors.c[0][1], colors.c[0][2]}});
  return check_launch("overlay_mask");
}

// ---- the low-resolution logits ---------------------------------------------------------------------
struct OvGeom {
  int rows, cols;  // largest staged window of any tile
};
static OvGeom ov_geom(int Hl, int Wl, int base, int Ho, int Wo, int h, int w) {
  const float sl_h = ac_scale(Hl, base), sl_w = ac_scale(Wl, base);
  const double ih = 1.0 / (2.0 * Ho), iw = 1.0 / (2.0 * Wo);
  OvGeom g{0, 0};
  for (int y0 = 0; y0 < h; y0 += OV_TH) {
    const int yo0 = ov_src(y0, Ho, h), yo1 = ov_src(std::min(y0 + OV_TH, h) - 1, Ho, h);
    const int lo = ac_lerp(cf_tap(yo0, base, Ho, ih).i0, Hl, base, sl_h).i0;
    g.rows = std::max(g.rows, ac_lerp(cf_tap(yo1, base, Ho, ih).i1, Hl, base, sl_h).i1 - lo + 1);
  }
  for (int x0 = 0; x0 < w; x0 += OV_TW) {
    const int xo0 = ov_src(x0, Wo, w), xo1 = ov_src(std::min(x0 + OV_TW, w) - 1, Wo, w);
    const int lo = ac_lerp(cf_tap(xo0, base, Wo, iw).i0, Wl, base, sl_w).i0;
    g.cols = std::max(g.cols, ac_lerp(cf_tap(xo1, base, Wo, iw).i1, Wl, base, sl_w).i1 - lo + 1);
  }
  return g;
}

// the staged window as ee_pixel's row accessor (as e2e_head's)
struct OvLdsRows {
  const float* w;
  int lo, cl0, CWP, WP;
  __device__ __forceinline__ int row(int r) const { return (r - lo) * CWP; }
  __device__ __forceinline__ float at(int row, int c, int col) const {
    return w[row + c * WP + (col - cl0)];
  }
};

template <typename TI, int CB>
__global__ __launch_bounds__(OV_T) void e2e_overlay_kernel(E2eHeadArgs a, OverlayArgs f,
                                                           OverlayColors col, int WP, double ih,
                                                           double iw) {
  extern __shared__ float ov_rows[];  // [rows][C][WP]
  __shared__ uint8_t ids[OV_T];       // the tile's classes
  const int n = blockIdx.z, C = a.C;
  const int fy0 = blockIdx.y * OV_TH, fx0 = blockIdx.x * OV_TW;
  const int fy1 = min(fy0 + OV_TH, f.h) - 1, fx1 = min(fx0 + OV_TW, f.w) - 1;
  const int yo0 = ov_src(fy0, a.Ho, f.h), yo1 = ov_src(fy1, a.Ho, f.h);
  const int xo0 = ov_src(fx0, a.Wo, f.w), xo1 = ov_src(fx1, a.Wo, f.w);
  const float sl_h = ac_scale(a.Hl, a.base), sl_w = ac_scale(a.Wl, a.base);
  // the tile's low-res window (ov_geom bounds nrows x ncols by the LDS the launch got)
  const int lo = ac_lerp(cf_tap(yo0, a.base, a.Ho, ih).i0, a.Hl, a.base, sl_h).i0;
  const int nrows = ac_lerp(cf_tap(yo1, a.base, a.Ho, ih).i1, a.Hl, a.base, sl_h).i1 - lo + 1;
  const int cl0 = ac_lerp(cf_tap(xo0, a.base, a.Wo, iw).i0, a.Wl, a.base, sl_w).i0;
  const int ncols = ac_lerp(cf_tap(xo1, a.base, a.Wo, iw).i1, a.Wl, a.base, sl_w).i1 - cl0 + 1;
  const int CWP = C * WP, CN = C * ncols;
  {
    const TI* xb = (const TI*)a.logits + (((size_t)n * a.Hl + lo) * a.Wl + cl0) * a.ldx;
    for (int e = threadIdx.x; e < nrows * CN; e += OV_T) {
      const int r = e / CN;
      const int rem = e - r * CN;
      const int wi = rem / C, c = rem - wi * C;
      ov_rows[r * CWP + c * WP + wi] = ld1(xb + ((size_t)r * a.Wl + wi) * a.ldx + c);
    }
  }
  __syncthreads();
  {
    const int fx = fx0 + threadIdx.x % OV_TW, fy = fy0 + threadIdx.x / OV_TW;
    if (fx <= fx1 && fy <= fy1) {
      const EeGrid g{a.Hl, a.Wl, a.base, a.Ho, a.Wo, C, a.f16_once, ih, iw};
      const OvLdsRows rows{ov_rows, lo, cl0, CWP, WP};
      float v[CB], m;
      ee_pixel<TI, CB>(g, ov_src(fx, a.Wo, f.w), ov_src(fy, a.Ho, f.h), rows, v);
      ids[threadIdx.x] = (uint8_t)ee_argmax<CB>(v, m);
    }
  }
  __syncthreads();
  constexpr int GX = OV_TW / OV_G;  // groups per tile row: GX * OV_TH = one wave
  if (threadIdx.x >= GX * OV_TH) return;
  const int gy = threadIdx.x / GX, gx0 = (threadIdx.x % GX) * OV_G;
  const int y = fy0 + gy, x0 = fx0 + gx0;
  if (y > fy1 || x0 > fx1) return;
  uint8_t L[OV_G], o[OV_G][3];
#pragma unroll
  for (int j = 0; j < OV_G; ++j) {  // (columns past the tile read its last class and are not stored)
    const int id = ids[gy * OV_TW + min(gx0 + j, fx1 - fx0)];  // < C <= 32
    L[j] = (uint8_t)(id * a.label_scale);
    const bool on = (col.on >> id) & 1u;
#pragma unroll
    for (int k = 0; k < 3; ++k) o[j][k] = on ? col.c[id][k] : 0;
  }
  ov_group_any(f, n, y, x0, o, L);
}

bool e2e_overlay_ok(int N, int C, int Hl, int Wl, int base, int Ho, int Wo, int h, int w) {
  if (N < 1 || N > 65535 || C < 1 || C > EE_CMAX || Hl < 1 || Wl < 1 || base < 1 || Ho < 1 ||
      Wo < 1 || h < 1 || w < 1 || base > E2E_MAXDIM || Ho > E2E_MAXDIM || Wo > E2E_MAXDIM ||
      h > E2E_MAXDIM || w > E2E_MAXDIM)
    return false;
  const OvGeom g = ov_geom(Hl, Wl, base, Ho, Wo, h, w);
  return (size_t)g.rows * C * (g.cols | 1) * sizeof(float) <= 64 * 1024 - OV_T;
}

int e2e_overlay(const E2eHeadArgs& h0, const OverlayArgs& f, const OverlayColors& colors,
                int dtype, hipStream_t st) {
  static_assert(OV_CMAX == EE_CMAX, "the colour table holds one row per class the tail takes");
  E2eHeadArgs a = h0;
  if (!a.logits) {
    set_error("e2e_overlay: null logits");
    return E_INVALID;
  }
  if (int rc = ov_check("e2e_overlay", f)) return rc;
  if (f.N != a.N) {
    set_error("e2e_overlay: %d frames for %d images of logits", f.N, a.N);
    return E_INVALID;
  }
  if (a.ldx < a.C) {
    set_error("e2e_overlay: ldx=%d below C=%d", a.ldx, a.C);
    return E_INVALID;
  }
  if (dtype < DT_F32 || dtype > DT_F16) {
    set_error("e2e_overlay: logits dtype %d (0 fp32, 1 bf16, 2 fp16)", dtype);
    return E_INVALID;
  }
  if (!e2e_overlay_ok(a.N, a.C, a.Hl, a.Wl, a.base, a.Ho, a.Wo, f.h, f.w)) {
    set_error("e2e_overlay: unsupported geometry (N=%d C=%d low-res %dx%d base %d out %dx%d frame "
              "%dx%d)", a.N, a.C, a.Hl, a.Wl, a.base, a.Ho, a.Wo, f.h, f.w);
    return E_UNSUPPORTED;
  }
  a.f16_once = ee_f16_once(a.N, a.Hl, a.Wl, a.C, a.base);
  a.probs = nullptr; a.labels = nullptr;
  const OvGeom g = ov_geom(a.Hl, a.Wl, a.base, a.Ho, a.Wo, f.h, f.w);
  const int wp = g.cols | 1;  // odd plane stride: the staging stores walk c
  const size_t lds = (size_t)g.rows * a.C * wp * sizeof(float);
  const dim3 grid((unsigned)cdiv(f.w, OV_TW), (unsigned)cdiv(f.h, OV_TH), (unsigned)a.N);
  const double ih = 1.0 / (2.0 * a.Ho), iw = 1.0 / (2.0 * a.Wo);
#define OV_LAUNCH(TI)                                                                          \
  do {                                                                                         \
    if (a.C <= 2)                                                                              \
      prof_launch(e2e_overlay_kernel<TI, 2>, grid, OV_T, lds, st, a, f, colors, wp, ih, iw);   \
    else if (a.C <= 8)                                                                         \
      prof_launch(e2e_overlay_kernel<TI, 8>, grid, OV_T, lds, st, a, f, colors, wp, ih, iw);   \
    else                                                                                       \
      prof_launch(e2e_overlay_kernel<TI, EE_CMAX>, grid, OV_T, lds, st, a, f, colors, wp, ih,  \
                  iw);                                                                         \
  } while (0)
  if (dtype == DT_F32) OV_LAUNCH(float);
  else if (dtype == DT_F16) OV_LAUNCH(f16);
  else OV_LAUNCH(bf16);
#undef OV_LAUNCH
  return check_launch("e2e_overlay");
}

}  // namespace fscnn
