// One output pixel of the deployment tail, shared by e2e_head (e2e.hip, rows staged in LDS) and
// the bird's-eye tail (bev.hip, rows gathered from global memory): the exact align_corners=False
// tap law, the base-grid taps as the forward stores them, and their fp32 combination.  Both tails
// get the same bits for the same pixel because both call ee_pixel; only the row accessor differs.
#pragma once
#include "kernels.hpp"

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

constexpr int EE_CMAX = 32;

// A tap as the forward stores it: lerp2(l0, x0, l1, x1) in the logits dtype.  fp32 and bf16 have
// one answer.  fp16 has two: the fp32 value converted (two roundings), or v_fma_mixlo_f16, which
// rounds the exact fma once, straight to fp16 -- what the compiler makes of f2h(fmaf(..)) where it
// can -- and they differ by one fp16 ulp at a few values in 10^5.  up_nchw's stores use both: its
// row-group kernel with vector stores (plans whose width is a multiple of 4) rounds once in column
// 0 of each 4-vector and twice in columns 1 .. 3; its other forms round once everywhere (read from
// the ISA of interp.hip; tests/test_gpu_e2e.py compares every tap with the stored logits).  Both
// forms are spelled out here so that the calling kernel's own codegen has no say.
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

// The geometry of one tail: low-res Hl x Wl -> base x base (align_corners=True) -> Ho x Wo
// (align_corners=False); ih / iw = 1 / (2 Ho), 1 / (2 Wo).
struct EeGrid {
  int Hl, Wl, base, Ho, Wo, C, f16_once;
  double ih, iw;
};

// v[c] = the fp32 logit of class c at output pixel (xo, yo), -inf for c >= C.  `rows` is the row
// accessor: rows.row(r) names low-resolution row r, rows.at(row, c, col) is its class-c value at
// low-resolution column col, as fp32.
template <typename TI, int CB, typename Rows>
__device__ __forceinline__ void ee_pixel(const EeGrid& g, int xo, int yo, const Rows& rows,
                                         float (&v)[CB]) {
  const float sl_h = ac_scale(g.Hl, g.base), sl_w = ac_scale(g.Wl, g.base);
  const CfTap ty = cf_tap(yo, g.base, g.Ho, g.ih), tx = cf_tap(xo, g.base, g.Wo, g.iw);
  const Lerp lh[2] = {ac_lerp(ty.i0, g.Hl, g.base, sl_h), ac_lerp(ty.i1, g.Hl, g.base, sl_h)};
  const Lerp lw[2] = {ac_lerp(tx.i0, g.Wl, g.base, sl_w), ac_lerp(tx.i1, g.Wl, g.base, sl_w)};
  const auto r00 = rows.row(lh[0].i0), r01 = rows.row(lh[0].i1);
  const auto r10 = rows.row(lh[1].i0), r11 = rows.row(lh[1].i1);
  const float wy0 = 1.0f - ty.w, wx0 = 1.0f - tx.w;
  const bool once[2] = {g.f16_once || (tx.i0 & 3) == 0, g.f16_once || (tx.i1 & 3) == 0};
#pragma unroll
  for (int c = 0; c < CB; ++c) {
    v[c] = -INFINITY;
    if (c < g.C) {
      float t[2][2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const auto r0 = i ? r10 : r00;
        const auto r1 = i ? r11 : r01;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const float x0 = lerp2(lw[j].l0, rows.at(r0, c, lw[j].i0), lw[j].l1, rows.at(r0, c, lw[j].i1));
          const float x1 = lerp2(lw[j].l0, rows.at(r1, c, lw[j].i0), lw[j].l1, rows.at(r1, c, lw[j].i1));
          t[i][j] = tap_as_stored<TI>(lh[i].l0, x0, lh[i].l1, x1, once[j]);  // up_nchw's logit
        }
      }
      v[c] = lerp2(wy0, lerp2(wx0, t[0][0], tx.w, t[0][1]), ty.w, lerp2(wx0, t[1][0], tx.w, t[1][1]));
    }
  }
}

// argmax with strict >: the lowest class wins ties (classes >= C hold -inf and never win)
template <int CB>
__device__ __forceinline__ int ee_argmax(const float (&v)[CB], float& m) {
  m = v[0];
  int arg = 0;
#pragma unroll
  for (int c = 1; c < CB; ++c) {
    const bool gt = v[c] > m;
    m = gt ? v[c] : m;
    arg = gt ? c : arg;
  }
  return arg;
}

// whether fp16 taps round once in every column for this plan (e2e.hip)
int ee_f16_once(int N, int Hl, int Wl, int C, int base);

}  // namespace fscnn
