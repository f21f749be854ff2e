// The work layout shared by the fused training loss heads of head.hip (ce_head_kernel,
// ce_head2_kernel, dice_head_kernel, ohem_head_kernel): the final F.interpolate(bilinear,
// align_corners=True) of the logits (models/fast_scnn.py:40) + a criterion and its gradient back
// to the LOW-resolution logits, in one pass that never writes full-resolution logits.
//
// Workgroup (hl, n) owns the full-resolution pixels whose bilinear row tap i0(h) is low-res row
// hl, across the whole width, in chunks of HD_T low-res columns; thread t owns the pixels whose
// column tap i0(w) is low-res column t.  Every pixel is therefore computed exactly once (no
// halo).  A pixel touches cells (i0h|i1h) x (i0w|i1w); its four contributions are accumulated in
// registers as packed pairs a0 = (acc00, acc01): own row, columns t / t+1, and a1 = (acc10,
// acc11): row hl+1, the row spill.  At the end of a chunk (hd_tile_epilogue) thread t adds its
// left neighbour's (*, t) share in a fixed order and writes the own-row plane; the spill plane
// (row hl+1) is written separately and summed by the *_scale kernels, so the result is
// deterministic without atomics.  The two low-res logit rows the workgroup interpolates from are
// staged in LDS (odd row stride: conflict-free per-thread class walks), and the full-resolution
// target rows go through a two-row int8 ring in LDS (HdTargetRows).
#pragma once
#include "kernels.hpp"

namespace fscnn {

constexpr int HD_T = 256;
constexpr int HD_CMAX = 32;
constexpr int HD_TMAX = 2048;  // max full-res row width whose targets are staged in LDS
constexpr float HD_LOG2E = 1.4426950408889634f;
constexpr float HD_LN2 = 0.6931471805599453f;
typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int hd_first_ge(int i, int Lin, int Lout, float sc) {
  int lo = 0, hi = Lout;
  while (lo < hi) {
    int mid = (lo + hi) >> 1;
    if (ac_lerp(mid, Lin, Lout, sc).i0 >= i) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// The per-workgroup geometry: low-res row hl of image n, its full-resolution rows [h_lo, h_hi).
struct HeadTile {
  int tid, hl, n, Hl, Wl, H, W, hl1, h_lo, h_hi;
  float sh, sw;
  __device__ __forceinline__ HeadTile(int Hl_, int Wl_, int H_, int W_)
      : tid(threadIdx.x), hl(blockIdx.x), n(blockIdx.y), Hl(Hl_), Wl(Wl_), H(H_), W(W_) {
    sh = ac_scale(Hl, H), sw = ac_scale(Wl, W);
    h_lo = hd_first_ge(hl, Hl, H, sh), h_hi = hd_first_ge(hl + 1, Hl, H, sh);
    hl1 = min(hl + 1, Hl - 1);
  }
  // image n's offset in an NHWC [N][Hl][Wl][ld] array
  __device__ __forceinline__ size_t image(int ld) const { return (size_t)n * Hl * Wl * ld; }
  // g0 is the own-row plane; the spill plane (row hl+1) follows it
  __device__ __forceinline__ float* spill_plane(float* g0, int N, int ld) const {
    return g0 + (size_t)N * Hl * Wl * ld;
  }
  __device__ __forceinline__ void zero_spill_row0(float* g1, int ld) const {
    if (hl == 0) {  // nothing spills into row 0
      for (int i = tid; i < Wl * ld; i += HD_T) g1[image(ld) + i] = 0.f;
    }
  }
};

// One chunk of HD_T low-res columns from cb: thread tid's column t and its full-resolution
// columns [w_lo, w_hi) (none for an inactive thread, which still takes every barrier).
struct HeadCols {
  int t, w_lo, w_hi;
  bool active;
  __device__ __forceinline__ HeadCols(const HeadTile& tl, int cb) {
    t = cb + tl.tid;
    active = t < tl.Wl;
    w_lo = active ? hd_first_ge(t, tl.Wl, tl.W, tl.sw) : 0;
    w_hi = active ? hd_first_ge(t + 1, tl.Wl, tl.W, tl.sw) : 0;
  }
};

// Both low-res rows (hl, hl1), columns [cb, cb + HD_T] (clamped), into s_L as fp32 in log2 units
// (x log2 e): the softmax runs on v_exp_f32 (2^x) directly.  Barriers before and after.
template <typename T, int CT, int SL>
__device__ __forceinline__ void hd_stage_rows_f32(float* s_L, const T* lg, const HeadTile& tl,
                                                  int cb, int Cm, int ldl) {
  __syncthreads();
  for (int i = tl.tid; i < 2 * (HD_T + 1) * CT; i += HD_T) {
    const int c = i % CT, jr = i / CT;
    const int j = jr % (HD_T + 1), r = jr / (HD_T + 1);
    const int col = min(cb + j, tl.Wl - 1);
    const int row = r ? tl.hl1 : tl.hl;
    s_L[(r * (HD_T + 1) + j) * SL + c] =
        c < Cm ? ld1(lg + ((size_t)row * tl.Wl + col) * ldl + c) * HD_LOG2E : 0.f;
  }
  __syncthreads();
}

// Validity rules of the target pipeline.  The packed int8 copy (ce_pack_targets) holds -1 for
// every target that is ignored or outside [0, C).
struct HdIgnoreAware {  // CE, OHEM: -1 = ignored
  long long ignore_index;
  static constexpr int NONE = -1;
  __device__ __forceinline__ bool ok(long long tg, int Cm) const {
    return tg != ignore_index && tg >= 0 && tg < Cm;
  }
  static __device__ __forceinline__ int staged(int ti) { return ti; }
};
struct HdClampZero {  // Dice: targets outside [0, C) count as class 0
  static constexpr int NONE = 0;
  __device__ __forceinline__ bool ok(long long tg, int Cm) const { return tg >= 0 && tg < Cm; }
  static __device__ __forceinline__ int staged(int ti) { return ti < 0 ? 0 : ti; }
};

// The full-resolution target rows of a tile.  With `lds` the whole workgroup loads row h with
// coalesced loads -- int64 rows, or with T8 the plan's packed int8 copy, 8 per thread, when
// there is one and W % 8 == 0 -- into registers while row h - 1 is being worked on, and commit()
// stores it as int8 class indices into a two-row LDS ring; without `lds` (rows wider than
// HD_TMAX) get() reads the int64 target per pixel.  commit() is uniform: every thread of the
// workgroup takes its barrier, active column or not.
template <class POL, bool T8>
struct HdTargetRows {
  static constexpr int TPT = HD_TMAX / HD_T;
  const long long* tgt;      // image n's int64 targets
  const signed char* tgt8;   // image n's packed targets (T8)
  signed char* s_t;          // [2][HD_TMAX]
  POL pol;
  int tid, W, Cm;
  bool lds, t8, t8own;
  int tnext[TPT];
  uint2 tq;
  signed char* trow_s;       // the current row in the ring / in global memory
  const long long* trow;
  __device__ __forceinline__ HdTargetRows(const HeadTile& tl, const long long* target,
                                          const signed char* target8, signed char* s_t_, POL pol_,
                                          int Cm_, bool lds_)
      : tgt(target + (size_t)tl.n * tl.H * tl.W), s_t(s_t_), pol(pol_), tid(tl.tid), W(tl.W),
        Cm(Cm_), lds(lds_) {
    t8 = T8 && target8 != nullptr && W <= HD_TMAX && W % 8 == 0;
    t8own = tid * 8 < W;
    tgt8 = T8 ? target8 + (size_t)tl.n * tl.H * tl.W : nullptr;
    tq = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
  }
  __device__ __forceinline__ int cls(long long tg) const {
    return pol.ok(tg, Cm) ? (int)tg : POL::NONE;
  }
  __device__ __forceinline__ void prefetch(int h) {
    if (T8 && t8) {
      if (t8own) tq = *reinterpret_cast<const uint2*>(tgt8 + (size_t)h * W + tid * 8);
      return;
    }
    const long long* tr = tgt + (size_t)h * W;
#pragma unroll
    for (int k = 0; k < TPT; ++k) {
      const int w = tid + HD_T * k;
      const long long tg = tr[w < W ? w : 0];
      tnext[k] = (w < W && pol.ok(tg, Cm)) ? (int)tg : POL::NONE;
    }
  }
  // the first row's loads, issued before the chunk's row loop
  __device__ __forceinline__ void start(int h_lo, int h_hi) {
    if (lds && h_lo < h_hi) prefetch(h_lo);
  }
  __device__ __forceinline__ void select(int h) {
    trow_s = s_t + (h & 1) * HD_TMAX;
    trow = tgt + (size_t)h * W;
  }
  // row h: registers -> ring, barrier, then the next row's loads go out
  __device__ __forceinline__ void commit(int h, int h_hi) {
    select(h);
    if (lds) {
      if (T8 && t8) {
        if (t8own) *reinterpret_cast<uint2*>(trow_s + tid * 8) = tq;
      } else {
#pragma unroll
        for (int k = 0; k < TPT; ++k)
          if (tid + HD_T * k < W) trow_s[tid + HD_T * k] = (signed char)tnext[k];
      }
      __syncthreads();
      if (h + 1 < h_hi) prefetch(h + 1);
    }
  }
  __device__ __forceinline__ int get(int w) const {
    return lds ? POL::staged(trow_s[w]) : cls(trow[w]);
  }
};

// Class pairs (v_pk_* f32) of one full-resolution row: v0 = the row-interpolated low-res logits
// of column t and dv = (column t+1) - v0 (log2 units), padded to an even class count with
// zeros; a pixel's logits are then ONE packed fma per pair, v0 + lw.l1 * dv.  L0 / L1 are the
// thread's column in the staged rows hl / hl1.
template <int CT, int SL>
__device__ __forceinline__ void hd_lerp_rows_pk(const float* L0, const float* L1, const Lerp& lh,
                                                f32x2 (&v0)[(CT + 1) / 2],
                                                f32x2 (&dv)[(CT + 1) / 2]) {
  const f32x2 h0 = {lh.l0, lh.l0}, h1 = {lh.l1, lh.l1};
#pragma unroll
  for (int p = 0; p < (CT + 1) / 2; ++p) {
    const int c = 2 * p, c1 = c + 1 < CT ? c + 1 : c;
    const f32x2 l00 = {L0[c], c + 1 < CT ? L0[c1] : 0.f};
    const f32x2 l10 = {L1[c], c + 1 < CT ? L1[c1] : 0.f};
    const f32x2 l01 = {L0[SL + c], c + 1 < CT ? L0[SL + c1] : 0.f};
    const f32x2 l11 = {L1[SL + c], c + 1 < CT ? L1[SL + c1] : 0.f};
    v0[p] = __builtin_elementwise_fma(h1, l10, h0 * l00);
    dv[p] = __builtin_elementwise_fma(h1, l11, h0 * l01) - v0[p];
  }
}

// A class weight, or at compile time none (the CE head multiplies by nothing).
struct HdNoWeight {};
__device__ __forceinline__ float hd_times(float x, HdNoWeight) { return x; }
__device__ __forceinline__ float hd_times(float x, float w) { return x * w; }
__device__ __forceinline__ float hd_onehot(HdNoWeight) { return 1.f; }
__device__ __forceinline__ float hd_onehot(float w) { return w; }

// One pixel's gradient wt (e inv - onehot(ti)) onto the four taps, as two packed pairs per class
// (v_pk_fma_f32: (00, 01) and (10, 11)); an invalid pixel comes with inv = 0.
template <int CT, class WT>
__device__ __forceinline__ void hd_tap_accum_pk(f32x2 (&a0)[CT], f32x2 (&a1)[CT],
                                                const f32x2 (&e)[(CT + 1) / 2], float inv, WT wt,
                                                int ti, bool valid, const Lerp& lh,
                                                const Lerp& lw) {
  const f32x2 k0 = {lh.l0 * lw.l0, lh.l0 * lw.l1};
  const f32x2 k1 = {lh.l1 * lw.l0, lh.l1 * lw.l1};
  const f32x2 iv = {hd_times(inv, wt), hd_times(inv, wt)};
#pragma unroll
  for (int p = 0; p < (CT + 1) / 2; ++p) {
    const f32x2 oh = {(valid && 2 * p == ti) ? hd_onehot(wt) : 0.f,
                      (valid && 2 * p + 1 == ti) ? hd_onehot(wt) : 0.f};
    const f32x2 g = e[p] * iv - oh;
    const f32x2 gx = {g.x, g.x}, gy = {g.y, g.y};
    a0[2 * p] = __builtin_elementwise_fma(k0, gx, a0[2 * p]);
    a1[2 * p] = __builtin_elementwise_fma(k1, gx, a1[2 * p]);
    if (2 * p + 1 < CT) {
      a0[2 * p + 1] = __builtin_elementwise_fma(k0, gy, a0[2 * p + 1]);
      a1[2 * p + 1] = __builtin_elementwise_fma(k1, gy, a1[2 * p + 1]);
    }
  }
}

// s_carry[2 * NA]: the last thread's (*, t+1) shares, handed to the next chunk's thread 0.
template <int NA>
__device__ __forceinline__ void hd_carry_zero(float* s_carry, int tid) {
  if (tid < 2 * NA) s_carry[tid] = 0.f;
}

// The end of a column chunk, NA accumulated scalars per tap.  Folds the last column (i1(w) ==
// i0(w): both column taps are t) and the last row (both row taps are hl), hands the (*, t+1)
// shares to thread t+1 through LDS -- s_h[tid * stride + c] for the own row, base1 further for
// row hl+1; the logit rows are dead by now and lend their LDS -- and writes scalars [0, nw) of
// the own-row plane g0 and the spill plane g1 (leading dimension ld) in a fixed order; the last
// thread's shares are carried to the next chunk.  Every thread takes the three barriers.
template <int NA>
__device__ __forceinline__ void hd_tile_epilogue(const f32x2 (&a0)[NA], const f32x2 (&a1)[NA],
                                                 const HeadTile& tl, const HeadCols& cl, float* s_h,
                                                 int base1, int stride, float* s_carry, float* g0,
                                                 float* g1, int ld, int nw) {
  const int tid = tl.tid;
  float acc00[NA], acc01[NA], acc10[NA], acc11[NA];
#pragma unroll
  for (int c = 0; c < NA; ++c) {
    acc00[c] = a0[c].x;
    acc01[c] = a0[c].y;
    acc10[c] = a1[c].x;
    acc11[c] = a1[c].y;
  }
  if (cl.active) {
    if (cl.t == tl.Wl - 1) {
#pragma unroll
      for (int c = 0; c < NA; ++c) {
        acc00[c] += acc01[c];
        acc10[c] += acc11[c];
        acc01[c] = acc11[c] = 0.f;
      }
    }
    if (tl.hl1 == tl.hl) {
#pragma unroll
      for (int c = 0; c < NA; ++c) {
        acc00[c] += acc10[c];
        acc01[c] += acc11[c];
        acc10[c] = acc11[c] = 0.f;
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < NA; ++c) {
    s_h[tid * stride + c] = acc01[c];
    s_h[base1 + tid * stride + c] = acc11[c];
  }
  __syncthreads();
  if (cl.active) {
    float* o0 = g0 + (((size_t)tl.n * tl.Hl + tl.hl) * tl.Wl + cl.t) * ld;
    float* o1 = g1 + (((size_t)tl.n * tl.Hl + tl.hl + 1) * tl.Wl + cl.t) * ld;
    // the left neighbour's shares, or the previous chunk's for thread 0 (one select per row)
    const float* left0 = tid > 0 ? s_h + (tid - 1) * stride : s_carry;
    const float* left1 = tid > 0 ? s_h + base1 + (tid - 1) * stride : s_carry + NA;
#pragma unroll
    for (int c = 0; c < NA; ++c) {
      if (c < nw) {
        o0[c] = acc00[c] + left0[c];
        if (tl.hl1 != tl.hl) o1[c] = acc10[c] + left1[c];
      }
    }
  }
  __syncthreads();
  if (tid == HD_T - 1) {  // column cb + HD_T starts the next chunk
#pragma unroll
    for (int c = 0; c < NA; ++c) {
      s_carry[c] = acc01[c];
      s_carry[NA + c] = acc11[c];
    }
  }
}

// The workgroup's per-thread partials, already stored at s_f[k][tid] (KF floats) and s_u[k][tid]
// (KU unsigned counters), reduced in a fixed order by one tree; the sums land in s_f[k][0] /
// s_u[k][0].
template <int KF, int KU>
__device__ __forceinline__ void hd_block_reduce(float (*s_f)[HD_T], unsigned (*s_u)[HD_T],
                                                int tid) {
  __syncthreads();
  for (int off = HD_T / 2; off > 0; off >>= 1) {
    if (tid < off) {
#pragma unroll
      for (int k = 0; k < KF; ++k) s_f[k][tid] += s_f[k][tid + off];
#pragma unroll
      for (int k = 0; k < KU; ++k) s_u[k][tid] += s_u[k][tid + off];
    }
    __syncthreads();
  }
}

}  // namespace fscnn
