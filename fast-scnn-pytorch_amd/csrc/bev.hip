// Bird's-eye tail of the deployment pipeline: what the reference's consumers do to the lane mask
// before anything is steered (kuruma/vision/transform.py:130-201, path_planning.py:188-293):
//   the nearest-neighbour perspective warp of the mask to the bird's-eye view (border 0), and
//   per bird's-eye row the table both centreline flavours are read from: the longest run of
//   non-zero pixels of at least min_width (extract_centerline) and the count / index sum of the
//   non-zero pixels (extract_centerline_fast).
// A workgroup owns one bird's-eye row of one image, so the row scan needs no second launch: its
// threads walk the row 256 pixels at a time, each wave's ballot becomes one 64-bit word of the
// row's bitmask in LDS, and the table is a scan of that bitmask in a fixed order (no atomics).
// The source pixel comes from a functor: a mask in memory, or the (argmax * label_scale) that
// e2e_head would store at that frame pixel, evaluated from the low-resolution logits by the same
// ee_pixel (e2e_pixel.hpp) -- the frame-size mask is never written.  The gather reads the
// low-resolution logits from global memory: N x (base/8)^2 x C values, which stay in L2.
//
// Coordinate law (include/fastscnn.h), in fp64 with every operation rounded on its own (bv_source
// of bev_coord.hpp), so that a float64 numpy restatement gives the same integers.
#include "bev_coord.hpp"
#include "e2e_pixel.hpp"

#include <climits>
#include <cmath>

namespace fscnn {

constexpr int BV_T = 256;
constexpr int BV_WORDS = BEV_MAXW / 64;

struct BvMaskSrc {
  const uint8_t* mask;
  int Ho, Wo;
  __device__ __forceinline__ uint8_t operator()(int n, int sx, int sy) const {
    return mask[((size_t)n * Ho + sy) * Wo + sx];
  }
};

// low-resolution logits in global memory as ee_pixel's row accessor
template <typename TI>
struct BvGlobalRows {
  const TI* img;  // [Hl][Wl][ldx] of one image
  size_t row_stride;
  int ldx;
  __device__ __forceinline__ const TI* row(int r) const { return img + (size_t)r * row_stride; }
  __device__ __forceinline__ float at(const TI* row, int c, int col) const {
    return ld1(row + (size_t)col * ldx + c);
  }
};

template <typename TI, int CB>
struct BvLogitSrc {
  E2eHeadArgs h;
  double ih, iw;
  __device__ __forceinline__ uint8_t operator()(int n, int sx, int sy) const {
    const EeGrid g{h.Hl, h.Wl, h.base, h.Ho, h.Wo, h.C, h.f16_once, ih, iw};
    const size_t rs = (size_t)h.Wl * h.ldx;
    const BvGlobalRows<TI> rows{(const TI*)h.logits + (size_t)n * h.Hl * rs, rs, h.ldx};
    float v[CB], m;
    ee_pixel<TI, CB>(g, sx, sy, rows, v);
    return (uint8_t)(ee_argmax<CB>(v, m) * h.label_scale);
  }
};

// sum of the positions of the set bits of u
__device__ __forceinline__ int bv_possum(unsigned long long u) {
  return __popcll(u & 0xAAAAAAAAAAAAAAAAull) + 2 * __popcll(u & 0xCCCCCCCCCCCCCCCCull) +
         4 * __popcll(u & 0xF0F0F0F0F0F0F0F0ull) + 8 * __popcll(u & 0xFF00FF00FF00FF00ull) +
         16 * __popcll(u & 0xFFFF0000FFFF0000ull) + 32 * __popcll(u & 0xFFFFFFFF00000000ull);
}

template <typename Src>
__global__ __launch_bounds__(BV_T) void bev_rows_kernel(BevArgs a, Src src) {
  __shared__ unsigned long long bits[BV_WORDS];  // the row: bit x % 64 of word x / 64
  __shared__ int inner[BV_WORDS][2];             // per word: start, length of its longest inner run
  const int y = blockIdx.x, n = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double dy = (double)y;
  const double m1y = bv_mul(a.m[1], dy), m4y = bv_mul(a.m[4], dy), m7y = bv_mul(a.m[7], dy);
  uint8_t* out = a.bev ? a.bev + ((size_t)n * a.Hb + y) * a.Wb : nullptr;
  for (int x0 = 0; x0 < a.Wb; x0 += BV_T) {  // (uniform trip count: every wave ballots)
    const int x = x0 + threadIdx.x;
    uint8_t v = 0;
    if (x < a.Wb) {
      int sx, sy;
      bv_source(a.m, x, m1y, m4y, m7y, sx, sy);
      if (sx >= 0 && sx < a.Wo && sy >= 0 && sy < a.Ho) v = src(n, sx, sy);
      if (out) out[x] = v;
    }
    const unsigned long long b = __ballot(v != 0);
    if (lane == 0) bits[(x0 >> 6) + wave] = b;  // <= (BEV_MAXW - BV_T) / 64 + 3
  }
  __syncthreads();
  const int nw = (a.Wb + 63) >> 6;
  // runs that touch neither end of their word, one word per thread (leftmost of the longest)
  if ((int)threadIdx.x < nw) {
    const unsigned long long u = bits[threadIdx.x];
    int is = 0, il = 0;
    if (~u) {
      const int lead = __builtin_ctzll(~u), tail = __builtin_clzll(~u);
      unsigned long long wi = u & ~((1ull << lead) - 1ull);
      if (tail) wi &= ~(~0ull << (64 - tail));
      while (wi) {
        const int s = __builtin_ctzll(wi);  // >= 1: bit 0 belongs to the leading run or is clear
        const int l = __builtin_ctzll(~(wi >> s));
        if (l > il) {
          il = l;
          is = s;
        }
        wi &= ~(((1ull << l) - 1ull) << s);
      }
    }
    inner[threadIdx.x][0] = is;
    inner[threadIdx.x][1] = il;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  // candidates arrive in order of their start, so a strict > keeps the leftmost of the longest
  int best_s = 0, best_l = 0, cs = 0, cl = 0, cnt = 0, isum = 0;
  auto take = [&](int s, int l) {
    if (l >= a.min_width && l > best_l) {
      best_s = s;
      best_l = l;
    }
  };
  for (int w = 0; w < nw; ++w) {
    const unsigned long long u = bits[w];
    const int c = __popcll(u), x0 = w * 64;
    cnt += c;
    isum += x0 * c + bv_possum(u);
    if (!~u) {  // the open run goes on
      if (!cl) cs = x0;
      cl += 64;
      continue;
    }
    const int lead = __builtin_ctzll(~u), tail = __builtin_clzll(~u);
    if (cl + lead) take(cl ? cs : x0, cl + lead);
    take(x0 + inner[w][0], inner[w][1]);
    cl = tail;
    cs = x0 + 64 - tail;
  }
  if (cl) take(cs, cl);
  int* r = a.rows + ((size_t)n * a.Hb + y) * 4;
  r[0] = best_s;
  r[1] = best_s + best_l;
  r[2] = cnt;
  r[3] = isum;
}

bool bev_ok(int N, int Hb, int Wb, int min_width) {
  return N >= 1 && N <= 65535 && Hb >= 1 && Hb <= BEV_MAXH && Wb >= 1 && Wb <= BEV_MAXW &&
         min_width >= 1;
}

bool e2e_bev_ok(int N, int C, int Hl, int Wl, int base, int Ho, int Wo, int Hb, int Wb,
                int min_width) {
  return bev_ok(N, Hb, Wb, min_width) && C >= 1 && C <= EE_CMAX && Hl >= 1 && Wl >= 1 &&
         base >= 1 && Ho >= 1 && Wo >= 1 && base <= E2E_MAXDIM && Ho <= E2E_MAXDIM &&
         Wo <= E2E_MAXDIM;
}

static int bev_check(const char* who, const BevArgs& a) {
  if (!a.rows) {
    set_error("%s: null rows", who);
    return E_INVALID;
  }
  for (int i = 0; i < 9; ++i)
    if (!std::isfinite(a.m[i])) {
      set_error("%s: m[%d] is not finite", who, i);
      return E_INVALID;
    }
  return OK;
}

int bev_mask(const BevArgs& a, const uint8_t* mask, hipStream_t st) {
  if (!mask || a.Ho < 1 || a.Wo < 1) {
    set_error("bev_mask: null mask or empty source (%dx%d)", a.Ho, a.Wo);
    return E_INVALID;
  }
  if (int rc = bev_check("bev_mask", a)) return rc;
  if (!bev_ok(a.N, a.Hb, a.Wb, a.min_width)) {
    set_error("bev_mask: unsupported geometry (N=%d view %dx%d min_width %d; N <= 65535, width "
              "1 .. %d, height 1 .. %d, min_width >= 1)", a.N, a.Wb, a.Hb, a.min_width, BEV_MAXW,
              BEV_MAXH);
    return E_UNSUPPORTED;
  }
  const dim3 grid((unsigned)a.Hb, (unsigned)a.N);
  prof_launch(bev_rows_kernel<BvMaskSrc>, grid, BV_T, 0, st, a, BvMaskSrc{mask, a.Ho, a.Wo});
  return check_launch("bev_mask");
}

int e2e_bev(const E2eHeadArgs& h0, const BevArgs& a0, int dtype, hipStream_t st) {
  E2eHeadArgs h = h0;
  BevArgs a = a0;
  a.Ho = h.Ho; a.Wo = h.Wo; a.N = h.N;
  if (!h.logits) {
    set_error("e2e_bev: null logits");
    return E_INVALID;
  }
  if (int rc = bev_check("e2e_bev", a)) return rc;
  if (h.ldx < h.C) {
    set_error("e2e_bev: ldx=%d below C=%d", h.ldx, h.C);
    return E_INVALID;
  }
  if (dtype < DT_F32 || dtype > DT_F16) {
    set_error("e2e_bev: logits dtype %d (0 fp32, 1 bf16, 2 fp16)", dtype);
    return E_INVALID;
  }
  if (!e2e_bev_ok(h.N, h.C, h.Hl, h.Wl, h.base, h.Ho, h.Wo, a.Hb, a.Wb, a.min_width)) {
    set_error("e2e_bev: unsupported geometry (N=%d C=%d low-res %dx%d base %d frame %dx%d view "
              "%dx%d min_width %d)", h.N, h.C, h.Hl, h.Wl, h.base, h.Ho, h.Wo, a.Wb, a.Hb,
              a.min_width);
    return E_UNSUPPORTED;
  }
  h.f16_once = ee_f16_once(h.N, h.Hl, h.Wl, h.C, h.base);
  h.probs = nullptr; h.labels = nullptr;
  const dim3 grid((unsigned)a.Hb, (unsigned)a.N);
  const double ih = 1.0 / (2.0 * h.Ho), iw = 1.0 / (2.0 * h.Wo);
#define BV_LAUNCH(TI)                                                                         \
  do {                                                                                        \
    if (h.C <= 2)                                                                             \
      prof_launch(bev_rows_kernel<BvLogitSrc<TI, 2>>, grid, BV_T, 0, st, a,                   \
                  BvLogitSrc<TI, 2>{h, ih, iw});                                              \
    else if (h.C <= 8)                                                                        \
      prof_launch(bev_rows_kernel<BvLogitSrc<TI, 8>>, grid, BV_T, 0, st, a,                   \
                  BvLogitSrc<TI, 8>{h, ih, iw});                                              \
    else                                                                                      \
      prof_launch(bev_rows_kernel<BvLogitSrc<TI, EE_CMAX>>, grid, BV_T, 0, st, a,             \
                  BvLogitSrc<TI, EE_CMAX>{h, ih, iw});                                        \
  } while (0)
  if (dtype == DT_F32) BV_LAUNCH(float);
  else if (dtype == DT_F16) BV_LAUNCH(f16);
  else BV_LAUNCH(bf16);
#undef BV_LAUNCH
  return check_launch("e2e_bev");
}

}  // namespace fscnn
