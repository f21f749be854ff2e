// The fused training loss heads: upsample + criterion + gradient to the low-resolution logits in
// one pass (8 x 19 x 1024 x 2048 full-resolution logits would be 637 MB bf16 written, read,
// re-written and re-read by the unfused path).  The work layout all four kernels share -- tile
// geometry, logit staging, target rows, tap accumulation, chunk epilogue, block reduce -- is
// head_tile.hpp; a kernel here holds only its own per-pixel arithmetic.
#include <type_traits>

#include "head_tile.hpp"

namespace fscnn {

constexpr int HD_PD = 4;  // int8 target rows in flight per thread (ce_head2_kernel)

// nn.CrossEntropyLoss(ignore_index=-1) (utils/loss.py:103-124) with a per-pixel softmax: fp32
// plans, and 16-bit plans with class counts other than 19 and 2.
template <typename T, int CT, bool EXACT>
__global__ __launch_bounds__(HD_T) void ce_head_kernel(CeHeadArgs a) {
  constexpr int SL = (CT % 2 == 0) ? CT + 1 : CT;  // odd LDS stride per column
  constexpr int CP = (CT + 1) / 2;
  __shared__ float s_L[2 * (HD_T + 1) * SL];
  __shared__ float s_carry[2 * CT];
  __shared__ signed char s_t[2 * HD_TMAX];
  __shared__ float s_r[2][HD_T];
  const HeadTile tl(a.Hl, a.Wl, a.H, a.W);
  const int tid = tl.tid, ldl = a.ldl;
  const int Cm = EXACT ? CT : a.C;
  const T* lg = (const T*)a.logits + tl.image(ldl);
  float* g1 = tl.spill_plane(a.g_raw, a.N, ldl);
  float loss = 0.f, cnt = 0.f;
  hd_carry_zero<CT>(s_carry, tid);
  tl.zero_spill_row0(g1, ldl);
  for (int cb = 0; cb < tl.Wl; cb += HD_T) {
    hd_stage_rows_f32<T, CT, SL>(s_L, lg, tl, cb, Cm, ldl);
    const HeadCols cl(tl, cb);
    f32x2 a0[CT], a1[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) a0[c] = a1[c] = f32x2{0.f, 0.f};
    HdTargetRows<HdIgnoreAware, false> tr(tl, a.target, nullptr, s_t, HdIgnoreAware{a.ignore_index},
                                          Cm, tl.W <= HD_TMAX);
    tr.start(tl.h_lo, tl.h_hi);
    const float* L0 = &s_L[tid * SL];
    const float* L1 = &s_L[((HD_T + 1) + tid) * SL];
    for (int h = tl.h_lo; h < tl.h_hi; ++h) {
      tr.commit(h, tl.h_hi);
      if (cl.active) {
        const Lerp lh = ac_lerp(h, tl.Hl, tl.H, tl.sh);
        f32x2 v0[CP], dv[CP];
        hd_lerp_rows_pk<CT, SL>(L0, L1, lh, v0, dv);
        for (int w = cl.w_lo; w < cl.w_hi; ++w) {
          const Lerp lw = ac_lerp(w, tl.Wl, tl.W, tl.sw);
          const int ti = tr.get(w);
          const bool valid = ti >= 0;
          const f32x2 w1 = {lw.l1, lw.l1};
          f32x2 e[CP];
#pragma unroll
          for (int p = 0; p < CP; ++p) e[p] = __builtin_elementwise_fma(w1, dv[p], v0[p]);
          // class max as a tree of 3-input maxima (v_max3_f32): a short dependency chain
          float mx;
          {
            float m[2 * CP];
#pragma unroll
            for (int p = 0; p < CP; ++p) {
              m[2 * p] = 2 * p < Cm ? e[p].x : -INFINITY;
              m[2 * p + 1] = 2 * p + 1 < Cm ? e[p].y : -INFINITY;
            }
            int k = 2 * CP;
#pragma unroll
            for (int lvl = 0; lvl < 6; ++lvl) {
              if (k == 1) break;
              const int k3 = (k + 2) / 3;
#pragma unroll
              for (int i = 0; i < k3; ++i) {
                const float x0 = m[3 * i];
                const float x1 = 3 * i + 1 < k ? m[3 * i + 1] : x0;
                const float x2 = 3 * i + 2 < k ? m[3 * i + 2] : x0;
                m[i] = fmaxf(fmaxf(x0, x1), x2);
              }
              k = k3;
            }
            mx = m[0];
          }
          // the target's logit, re-interpolated from the staged rows with the same operations
          // (an LDS gather instead of a select over every class)
          float lt;
          {
            const int tc = valid ? ti : 0;
            const float v0t = fmaf(lh.l1, L1[tc], lh.l0 * L0[tc]);
            const float v1t = fmaf(lh.l1, L1[SL + tc], lh.l0 * L0[SL + tc]);
            lt = fmaf(lw.l1, v1t - v0t, v0t);
          }
          // v_exp_f32 (2^x) of packed differences; the loss takes v_log_f32 (log2) of the sum
          const f32x2 mm = {mx, mx};
#pragma unroll
          for (int p = 0; p < CP; ++p) {
            const f32x2 d = e[p] - mm;
            e[p].x = 2 * p < Cm ? __builtin_amdgcn_exp2f(d.x) : 0.f;
            e[p].y = 2 * p + 1 < Cm ? __builtin_amdgcn_exp2f(d.y) : 0.f;
          }
          // packed pair sums as a tree (fixed order; short dependency chain)
          float se;
          {
            f32x2 sp[CP];
#pragma unroll
            for (int p = 0; p < CP; ++p) sp[p] = e[p];
            int k = CP;
#pragma unroll
            for (int lvl = 0; lvl < 6; ++lvl) {
              if (k == 1) break;
              const int k2 = (k + 1) / 2;
#pragma unroll
              for (int i = 0; i < k / 2; ++i) sp[i] = sp[2 * i] + sp[2 * i + 1];
              if (k & 1) sp[k / 2] = sp[k - 1];
              k = k2;
            }
            se = sp[0].x + sp[0].y;
          }
          const float inv = valid ? __builtin_amdgcn_rcpf(se) : 0.f;  // v_rcp_f32 (1 ulp)
          if (valid) {
            loss += (mx - lt + __builtin_amdgcn_logf(se)) * HD_LN2;  // v_log_f32: log2
            cnt += 1.f;
          }
          hd_tap_accum_pk<CT>(a0, a1, e, inv, HdNoWeight{}, ti, valid, lh, lw);
        }
      }
    }
    hd_tile_epilogue<CT>(a0, a1, tl, cl, s_L, (HD_T + 1) * SL, SL, s_carry, a.g_raw, g1, ldl, Cm);
  }
  s_r[0][tid] = loss;
  s_r[1][tid] = cnt;
  hd_block_reduce<2, 0>(s_r, nullptr, tid);
  if (tid == 0) {
    const size_t pi = (size_t)tl.n * tl.Hl + tl.hl;
    a.part[2 * pi] = s_r[0][0];
    a.part[2 * pi + 1] = s_r[1][0];
  }
}

// 16-bit plans, exact class counts.  Along one full-resolution row segment of a thread (h fixed,
// w in [w_lo, w_hi): the columns whose left tap is low-res column t) every logit is linear in
// lw.l1 = w * sw - t, which steps by sw, so
//   * exponentials are walked, not evaluated: e_c(w + 1) = e_c(w) * q_c with q_c = 2^(sw dv_c),
//     seeded at the segment's first pixel against the segment bound M = max_c logit_c(first) --
//     the true per-pixel max is within max|dv| * span of M, and a segment whose spread could take
//     exp2 below 2^-60 re-seeds every pixel (exactly the per-pixel evaluation);
//   * the gradient is accumulated row-factored: a pixel adds inv * (e_c, lw.l1 e_c) to per-class
//     row sums (S, R) -- one packed fma per class -- and the segment's end folds lh.l0 (S - R, R)
//     and lh.l1 (S - R, R) into the four tap accumulators;
//   * the target's -1 is not selected per class: (1, lw.l1) is added to a per-thread LDS slot of
//     its class (fixed order) and subtracted from (S, R) at the segment's end;
//   * the low-res logit rows are staged as raw 16-bit values (exact): half the LDS.
// The walk's exponent follows w * sw in real arithmetic where the weights use fl(w * sw): at most
// a few fp32 ulps of W/Wl in lw.l1, i.e. ~1e-4 relative in a probability at |dv| ~ 3 -- well
// inside one 16-bit rounding of the stored gradient (tests/test_gpu_literal.py).
// Of head_tile.hpp this kernel shares the tile geometry only.  At C = 19 it sits at 256 VGPRs with
// ~64 spilled, and each further shared piece moved it: the int64 target rows and the epilogue
// change its scratch (HdTargetRows: +8 B; hd_tile_epilogue: 264 -> 188 B), and HeadCols plus
// hd_block_reduce measured 1.5 - 3 us slower on the cfg3 step (profiles/head_refactor_time.txt).
// So the column bounds, the int64 target rows, the epilogue and the reduce stay inline below.
template <typename T, int CT>
__global__ __launch_bounds__(HD_T, 2) void ce_head2_kernel(CeHeadArgs a) {
  constexpr int CP = (CT + 1) / 2;
  constexpr int VPP = (CT + 7) / 8;                 // 16-byte vectors per pixel (ldl == 8 VPP)
  constexpr int SLW = CP % 2 == 0 ? CP + 1 : CP;    // odd 32-bit word stride per pixel
  constexpr int SL = 2 * SLW;                       // ... in 16-bit elements
  constexpr int NSV = (2 * (HD_T + 1) * VPP + HD_T - 1) / HD_T;  // staged vectors per thread
  __shared__ __attribute__((aligned(16))) uint16_t s_L[2 * (HD_T + 1) * SL];
  __shared__ __attribute__((aligned(16))) f32x2 s_oh[CT * HD_T];  // [class][thread] (1, lw.l1) sums
  __shared__ float s_carry[2 * CT];
  __shared__ signed char s_t[2 * HD_TMAX];
  __shared__ float s_r1[HD_T], s_r2[HD_T];
  const HeadTile tl(a.Hl, a.Wl, a.H, a.W);
  const int tid = tl.tid, hl = tl.hl, n = tl.n, hl1 = tl.hl1, h_lo = tl.h_lo, h_hi = tl.h_hi;
  const int Hl = tl.Hl, Wl = tl.Wl, H = tl.H, W = tl.W, ldl = a.ldl;
  const float sh = tl.sh, sw = tl.sw;
  const uint16_t* lg = (const uint16_t*)a.logits + (size_t)n * Hl * Wl * ldl;
  float* g0 = a.g_raw;                              // own-row plane
  float* g1 = a.g_raw + (size_t)a.N * Hl * Wl * ldl;  // spill plane (row hl+1)
  const long long* tgt = a.target + (size_t)n * H * W;
  float loss = 0.f, cnt = 0.f;
  stamp(a.stamps, 0);
  hd_carry_zero<CT>(s_carry, tid);
  tl.zero_spill_row0(g1, ldl);
  // int8 targets (a.tgt8): 8 bytes per thread and row, HD_PD rows in flight (register ring)
  const bool t8 = a.tgt8 != nullptr && W <= HD_TMAX && W % 8 == 0;
  const bool t8own = tid * 8 < W;
  const signed char* trow8 = a.tgt8 + (size_t)n * H * W + tid * 8;
  uint2 tq[HD_PD];
  auto load8 = [&](int h, uint2& d) {
    d = (h < h_hi && t8own) ? *reinterpret_cast<const uint2*>(trow8 + (size_t)h * W)
                            : make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
  };
  for (int cb = 0; cb < Wl; cb += HD_T) {
    __syncthreads();
    if (t8) {  // the first target rows' loads go out with the logit staging below
#pragma unroll
      for (int j = 0; j < HD_PD; ++j) load8(h_lo + j, tq[j]);
    }
    {  // both low-res rows, columns cb .. cb + HD_T: 16-byte loads all in flight, then LDS
      uint4 v[NSV];
#pragma unroll
      for (int k = 0; k < NSV; ++k) {
        const int i = tid + HD_T * k;
        const int q = i % VPP, jr = i / VPP;
        const int j = jr % (HD_T + 1), r = jr / (HD_T + 1);
        const int col = min(cb + j, Wl - 1), row = r ? hl1 : hl;
        v[k] = i < 2 * (HD_T + 1) * VPP
                   ? *(const uint4*)(lg + ((size_t)row * Wl + col) * ldl + 8 * q)
                   : uint4{0, 0, 0, 0};
      }
#pragma unroll
      for (int k = 0; k < NSV; ++k) {
        const int i = tid + HD_T * k;
        if (i < 2 * (HD_T + 1) * VPP) {
          const int q = i % VPP, jr = i / VPP;
          uint32_t* d = (uint32_t*)s_L + jr * SLW + 4 * q;
          if (4 * q + 0 < CP) d[0] = v[k].x;
          if (4 * q + 1 < CP) d[1] = v[k].y;
          if (4 * q + 2 < CP) d[2] = v[k].z;
          if (4 * q + 3 < CP) d[3] = v[k].w;
        }
      }
    }
#pragma unroll
    for (int c = 0; c < CT; ++c) s_oh[c * HD_T + tid] = f32x2{0.f, 0.f};
    __syncthreads();
    if (cb == 0) stamp(a.stamps, 1);
    const int t = cb + tid;
    const bool active = t < Wl;
    f32x2 a0[CT], a1[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) a0[c] = a1[c] = f32x2{0.f, 0.f};
    const int w_lo = active ? hd_first_ge(t, Wl, W, sw) : 0;
    const int w_hi = active ? hd_first_ge(t + 1, Wl, W, sw) : 0;
    const bool lds_t = W <= HD_TMAX;
    constexpr int TPT = HD_TMAX / HD_T;
    int tnext[TPT];
    auto load_trow = [&](int h) {
      const long long* tr = tgt + (size_t)h * W;
#pragma unroll
      for (int k = 0; k < TPT; ++k) {
        const int w = tid + HD_T * k;
        const long long tg = tr[w < W ? w : 0];
        tnext[k] = (w < W && tg != a.ignore_index && tg >= 0 && tg < CT) ? (int)tg : -1;
      }
    };
    if (lds_t && !t8 && h_lo < h_hi) load_trow(h_lo);
    const uint32_t* W0 = (const uint32_t*)s_L + tid * SLW;                 // row hl, column t
    const uint32_t* W1 = (const uint32_t*)s_L + ((HD_T + 1) + tid) * SLW;  // row hl + 1
    const uint16_t* L0 = &s_L[tid * SL];
    const uint16_t* L1 = &s_L[((HD_T + 1) + tid) * SL];
    auto unpack = [](uint32_t w) {
      return f32x2{s16_to<T>((uint16_t)(w & 0xFFFFu)), s16_to<T>((uint16_t)(w >> 16))};
    };
#pragma unroll 1
    for (int h = h_lo; h < h_hi; ++h) {
      signed char* trow_s = s_t + (h & 1) * HD_TMAX;
      if (t8) {
        if (t8own) *reinterpret_cast<uint2*>(trow_s + tid * 8) = tq[0];
#pragma unroll
        for (int j = 0; j + 1 < HD_PD; ++j) tq[j] = tq[j + 1];
        load8(h + HD_PD, tq[HD_PD - 1]);
        __syncthreads();
      } else if (lds_t) {
#pragma unroll
        for (int k = 0; k < TPT; ++k)
          if (tid + HD_T * k < W) trow_s[tid + HD_T * k] = (signed char)tnext[k];
        __syncthreads();
        if (h + 1 < h_hi) load_trow(h + 1);
      }
      if (active && w_lo < w_hi) {
        const Lerp lh = ac_lerp(h, Hl, H, sh);
        const f32x2 h0 = {lh.l0 * HD_LOG2E, lh.l0 * HD_LOG2E};
        const f32x2 h1 = {lh.l1 * HD_LOG2E, lh.l1 * HD_LOG2E};
        const long long* trow = tgt + (size_t)h * W;
        auto target = [&](int w) -> int {
          if (lds_t) return trow_s[w];
          const long long tg = trow[w];
          return (tg != a.ignore_index && tg >= 0 && tg < CT) ? (int)tg : -1;
        };
        // class pair p's logits (log2 units) at column taps 0 / 1 of row h
        auto taps = [&](int p, f32x2& v0, f32x2& dv) {
          v0 = __builtin_elementwise_fma(h1, unpack(W1[p]), h0 * unpack(W0[p]));
          dv = __builtin_elementwise_fma(h1, unpack(W1[SLW + p]), h0 * unpack(W0[SLW + p])) - v0;
          if (2 * p + 1 >= CT) v0.y = -INFINITY, dv.y = 0.f;  // padding class of an odd count
        };
        float l1 = ac_lerp(w_lo, Wl, W, sw).l1;
        f32x2 e[CP], q[CP];
        float M = -INFINITY, dvmax = 0.f;
        {
          const f32x2 L1v = {l1, l1}, SWv = {sw, sw};
#pragma unroll
          for (int p = 0; p < CP; ++p) {
            asm volatile("" ::: "memory");  // one class pair's staged reads at a time
            f32x2 v0, dv;
            taps(p, v0, dv);
            e[p] = __builtin_elementwise_fma(L1v, dv, v0);
            q[p] = dv * SWv;
            M = fmaxf(M, fmaxf(e[p].x, e[p].y));
            dvmax = fmaxf(dvmax, fmaxf(fabsf(dv.x), fabsf(dv.y)));
          }
#pragma unroll
          for (int p = 0; p < CP; ++p) {
            e[p].x = __builtin_amdgcn_exp2f(e[p].x - M);
            e[p].y = __builtin_amdgcn_exp2f(e[p].y - M);
            q[p].x = __builtin_amdgcn_exp2f(q[p].x);
            q[p].y = __builtin_amdgcn_exp2f(q[p].y);
          }
        }
        const bool reseed = dvmax * ((w_hi - 1 - w_lo) * sw) > 60.f;
        if (cb == 0 && h == h_lo) stamp(a.stamps, 5);
        f32x2 S[CP], R[CP];  // per class pair: the segment's sum inv e, sum lw.l1 inv e
#pragma unroll
        for (int p = 0; p < CP; ++p) S[p] = R[p] = f32x2{0.f, 0.f};
        int ti = target(w_lo);
#pragma unroll 1
        for (int w = w_lo; w < w_hi; ++w) {
          if (reseed && w > w_lo) {  // wide logit spread: evaluate this pixel directly
            M = -INFINITY;
            const f32x2 L1v = {l1, l1};
#pragma unroll
            for (int p = 0; p < CP; ++p) {
              asm volatile("" ::: "memory");
              f32x2 v0, dv;
              taps(p, v0, dv);
              e[p] = __builtin_elementwise_fma(L1v, dv, v0);
              M = fmaxf(M, fmaxf(e[p].x, e[p].y));
            }
#pragma unroll
            for (int p = 0; p < CP; ++p) {
              e[p].x = __builtin_amdgcn_exp2f(e[p].x - M);
              e[p].y = __builtin_amdgcn_exp2f(e[p].y - M);
            }
          }
          const int tcur = ti;
          if (w + 1 < w_hi) ti = target(w + 1);  // next pixel's target, in flight meanwhile
          const bool valid = tcur >= 0;
          float se;
          {
            f32x2 sp[CP];
#pragma unroll
            for (int p = 0; p < CP; ++p) sp[p] = e[p];
            int k = CP;
#pragma unroll
            for (int lvl = 0; lvl < 6; ++lvl) {
              if (k == 1) break;
              const int k2 = (k + 1) / 2;
#pragma unroll
              for (int i = 0; i < k / 2; ++i) sp[i] = sp[2 * i] + sp[2 * i + 1];
              if (k & 1) sp[k / 2] = sp[k - 1];
              k = k2;
            }
            se = sp[0].x + sp[0].y;
          }
          const float inv = valid ? __builtin_amdgcn_rcpf(se) : 0.f;
          if (valid) {
            const float v0t = fmaf(h1.x, s16_to<T>(L1[tcur]), h0.x * s16_to<T>(L0[tcur]));
            const float v1t = fmaf(h1.x, s16_to<T>(L1[SL + tcur]), h0.x * s16_to<T>(L0[SL + tcur]));
            loss += M - fmaf(l1, v1t - v0t, v0t) + __builtin_amdgcn_logf(se);  // log2 units
            cnt += 1.f;
            s_oh[tcur * HD_T + tid] = s_oh[tcur * HD_T + tid] + f32x2{1.f, l1};
          }
          const f32x2 iv = {inv, inv}, lv = {l1 * inv, l1 * inv};
#pragma unroll
          for (int p = 0; p < CP; ++p) {
            S[p] = __builtin_elementwise_fma(iv, e[p], S[p]);
            R[p] = __builtin_elementwise_fma(lv, e[p], R[p]);
            e[p] = e[p] * q[p];
          }
          l1 += sw;
        }
        if (cb == 0 && h == h_lo) stamp(a.stamps, 6);
        // the segment's end: target -1 terms, then the two row taps
        const f32x2 r0 = {lh.l0, lh.l0}, r1 = {lh.l1, lh.l1};
#pragma unroll
        for (int c = 0; c < CT; ++c) {
          const float Sc = (c & 1) ? S[c / 2].y : S[c / 2].x;
          const float Rc = (c & 1) ? R[c / 2].y : R[c / 2].x;
          const f32x2 oh = s_oh[c * HD_T + tid];
          s_oh[c * HD_T + tid] = f32x2{0.f, 0.f};
          const float d1 = Rc - oh.y;
          const f32x2 u = {(Sc - oh.x) - d1, d1};
          a0[c] = __builtin_elementwise_fma(r0, u, a0[c]);
          a1[c] = __builtin_elementwise_fma(r1, u, a1[c]);
        }
      }
    }
    if (cb == 0) stamp(a.stamps, 2);
    // hd_tile_epilogue<CT>, inline (above), with the hand-off through s_oh as [2][HD_T][CT] floats
    float acc00[CT], acc01[CT], acc10[CT], acc11[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      acc00[c] = a0[c].x;
      acc01[c] = a0[c].y;
      acc10[c] = a1[c].x;
      acc11[c] = a1[c].y;
    }
    if (active) {
      if (t == Wl - 1) {
#pragma unroll
        for (int c = 0; c < CT; ++c) {
          acc00[c] += acc01[c];
          acc10[c] += acc11[c];
          acc01[c] = acc11[c] = 0.f;
        }
      }
      if (hl1 == hl) {
#pragma unroll
        for (int c = 0; c < CT; ++c) {
          acc00[c] += acc10[c];
          acc01[c] += acc11[c];
          acc10[c] = acc11[c] = 0.f;
        }
      }
    }
    float* s_h = reinterpret_cast<float*>(s_oh);
    __syncthreads();
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      s_h[tid * CT + c] = acc01[c];
      s_h[(HD_T + tid) * CT + c] = acc11[c];
    }
    __syncthreads();
    if (active) {
      float* o0 = g0 + (((size_t)n * Hl + hl) * Wl + t) * ldl;
      float* o1 = g1 + (((size_t)n * Hl + hl + 1) * Wl + t) * ldl;
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        const float left0 = tid > 0 ? s_h[(tid - 1) * CT + c] : s_carry[c];
        const float left1 = tid > 0 ? s_h[(HD_T + tid - 1) * CT + c] : s_carry[CT + c];
        o0[c] = acc00[c] + left0;
        if (hl1 != hl) o1[c] = acc10[c] + left1;
      }
    }
    __syncthreads();
    if (tid == HD_T - 1) {
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        s_carry[c] = acc01[c];
        s_carry[CT + c] = acc11[c];
      }
    }
  }
  stamp(a.stamps, 3);
  s_r1[tid] = loss * HD_LN2;
  s_r2[tid] = cnt;
  __syncthreads();
  for (int off = HD_T / 2; off > 0; off >>= 1) {
    if (tid < off) {
      s_r1[tid] += s_r1[tid + off];
      s_r2[tid] += s_r2[tid + off];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const size_t pi = (size_t)n * Hl + hl;
    a.part[2 * pi] = s_r1[0];
    a.part[2 * pi + 1] = s_r2[0];
  }
  stamp(a.stamps, 4);
}

// ---- targets -> int8 ----------------------------------------------------------------------
// The loss head reads every full-resolution target once; as int64 rows that is 16 KB per row and
// workgroup, and the head's row loop waited ~8 us per row for the next row (stamps).  Packed to
// int8 (-1 = ignored / out of range, the head's own validity test) by a streaming pass that runs
// on the side stream during the global feature extractor, a row is 2 KB and the head keeps four
// rows in flight.
__global__ __launch_bounds__(256) void ce_pack_targets_kernel(const long long* t, long long n,
                                                               int C, long long ign,
                                                               signed char* out) {
  const long long i0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 8;
  if (i0 >= n) return;
  auto cls = [&](long long v) -> uint32_t {
    return (uint32_t)(uint8_t)(signed char)((v != ign && v >= 0 && v < C) ? (int)v : -1);
  };
  if (i0 + 8 <= n && ((uintptr_t)(t + i0) & 15) == 0) {
    const longlong2* p = reinterpret_cast<const longlong2*>(t + i0);
    const longlong2 a = p[0], b = p[1], c = p[2], d = p[3];
    uint2 o;
    o.x = cls(a.x) | (cls(a.y) << 8) | (cls(b.x) << 16) | (cls(b.y) << 24);
    o.y = cls(c.x) | (cls(c.y) << 8) | (cls(d.x) << 16) | (cls(d.y) << 24);
    *reinterpret_cast<uint2*>(out + i0) = o;
  } else {
    for (long long i = i0; i < n && i < i0 + 8; ++i) out[i] = (signed char)cls(t[i]);
  }
}

int ce_pack_targets(const long long* t, long long n, int C, long long ignore_index,
                    signed char* out, hipStream_t st) {
  if (C < 1 || C > 127 || n < 0 || ((uintptr_t)out & 7)) {
    set_error("ce_pack_targets: %d classes / misaligned output", C);
    return E_INVALID;
  }
  if (n == 0) return OK;
  ProfScope ps(PK_CE, st, 9.0 * (double)n, 0.0);
  const long long blocks = (n + 2047) / 2048;
  prof_launch(ce_pack_targets_kernel, (unsigned)blocks, 256, 0, st, t, n, C, ignore_index, out);
  return check_launch("ce_pack_targets");
}

int ce_head_parts(int N, int Hl, int Wl) { return N * Hl; }

// ---- instance selection ------------------------------------------------------------------------
// Every head is instantiated for the plan dtypes x the class counts (19, exact), (2, exact) and
// the generic (8, C <= 8) and (HD_CMAX, C <= HD_CMAX); f is called with the one HdInst that
// serves (C, dtype).  A head without some instance (Dice: the two-class form is its own MODE)
// leaves it out with `if constexpr` in f.
template <typename T_, int CT_, bool EXACT_>
struct HdInst {
  using T = T_;
  static constexpr int CT = CT_;
  static constexpr bool EXACT = EXACT_;
};
template <typename T_>
struct HdType {
  using T = T_;
};
template <class F>
static void hd_dispatch_dtype(int dtype, F f) {
  if (dtype == DT_F32) f(HdType<float>{});
  else if (dtype == DT_F16) f(HdType<f16>{});
  else f(HdType<bf16>{});
}
template <class F>
static void hd_dispatch(int C, int dtype, F f) {
  hd_dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::T;
    if (C == 19) f(HdInst<T, 19, true>{});
    else if (C == 2) f(HdInst<T, 2, true>{});
    else if (C <= 8) f(HdInst<T, 8, false>{});
    else f(HdInst<T, HD_CMAX, false>{});
  });
}

// partials [P][2] -> out2 = (sum / count, count): the mean loss (NaN without a valid pixel) and
// its denominator, in fp64 and a fixed order.  The OHEM head's sums are weighted, and with thr
// given (its pass 2) nothing is written when *thr is bit-equal to thresh: pass 1's result stands.
__global__ __launch_bounds__(256) void ce_head_finalize_kernel(const float* part, int P,
                                                               const float* thr, float thresh,
                                                               float* out) {
  if (thr && __float_as_uint(*thr) == __float_as_uint(thresh)) return;
  __shared__ double r1[256], r2[256];
  double s1 = 0.0, s2 = 0.0;
  for (int p = threadIdx.x; p < P; p += 256) {
    s1 += part[2 * p];
    s2 += part[2 * p + 1];
  }
  r1[threadIdx.x] = s1;
  r2[threadIdx.x] = s2;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (threadIdx.x < off) {
      r1[threadIdx.x] += r1[threadIdx.x + off];
      r2[threadIdx.x] += r2[threadIdx.x + off];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = r2[0] > 0 ? (float)(r1[0] / r2[0]) : NAN;
    out[1] = (float)r2[0];
  }
}

bool ce_head2_form(int C, int ldl, int dtype) {
  return dtype != DT_F32 && (C == 19 || C == 2) && ldl == (C + 7) / 8 * 8;
}
bool ce_head_reads_tgt8(int C, int ldl, int W, int dtype) {
  return ce_head2_form(C, ldl, dtype) && W <= HD_TMAX && W % 8 == 0;
}

int ce_head(const CeHeadArgs& a, float* out2, int dtype, hipStream_t st) {
  if (a.C < 1 || a.C > HD_CMAX) {
    set_error("ce_head: %d classes (max %d)", a.C, HD_CMAX);
    return E_UNSUPPORTED;
  }
  dim3 grid(a.Hl, a.N);
  {
    ProfScope ps(PK_CE, st, (dtype == DT_F32 ? 4.0 : 2.0) * a.N * a.Hl * a.Wl * a.C +
                                8.0 * a.N * a.H * a.W + 2.0 * 4.0 * a.N * a.Hl * a.Wl * a.C,
                 0.0);
    // (16-bit plans: the walked-exponential kernel; round 3's one-hot-select kernel for these
    // shapes measured 211 vs 158-164 us and was retired as a switch in r05)
    if (ce_head2_form(a.C, a.ldl, dtype)) {
      CeHeadArgs as = a;
      as.stamps = stamp_region();
      hd_dispatch(a.C, dtype, [&](auto i) {
        using I = decltype(i);
        if constexpr (I::EXACT && !std::is_same<typename I::T, float>::value)
          prof_launch((ce_head2_kernel<typename I::T, I::CT>), grid, HD_T, 0, st, as);
      });
    } else {
      hd_dispatch(a.C, dtype, [&](auto i) {
        using I = decltype(i);
        prof_launch((ce_head_kernel<typename I::T, I::CT, I::EXACT>), grid, HD_T, 0, st, a);
      });
    }
    int rc = check_launch("ce_head");
    if (rc) return rc;
  }
  prof_launch(ce_head_finalize_kernel, 1, 256, 0, st, a.part, ce_head_parts(a.N, a.Hl, a.Wl),
              (const float*)nullptr, 0.f, out2);
  return check_launch("ce_head_finalize");
}

template <typename T>
__global__ __launch_bounds__(256) void ce_head_scale_kernel(const float* g_raw, T* g, int M, int C,
                                                            int ld, const float* gout,
                                                            const float* out2, float weight) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M * ld) return;
  const int c = i % ld;
  const float s = gout[0] * weight / out2[1];  // (weight 1: the single-output head, bit for bit)
  // own-row plane + the spill of the row above (fixed order)
  st1(g + i, c < C ? (g_raw[i] + g_raw[(size_t)M * ld + i]) * s : 0.f);
}

int ce_head_scale(const float* g_raw, void* g, long long M, int C, int ld, const float* gout,
                  const float* out2, int dtype, hipStream_t st, float weight) {
  const int total = (int)(M * ld);
  hd_dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::T;
    prof_launch(ce_head_scale_kernel<T>, cdiv(total, 256), 256, 0, st, g_raw, (T*)g, (int)M, C, ld,
                gout, out2, weight);
  });
  return check_launch("ce_head_scale");
}

// the criterion over (out, aux_out): main + aux_weight * aux, and the two unweighted terms
__global__ void aux_loss_combine_kernel(const float* main, const float* aux, float aux_weight,
                                        float* out3) {
  if (threadIdx.x == 0) {
    const float m = main[0], a = aux[0];
    out3[0] = fmaf(aux_weight, a, m);
    out3[1] = m;
    out3[2] = a;
  }
}

int aux_loss_combine(const float* main, const float* aux, float aux_weight, float* out3,
                     hipStream_t st) {
  prof_launch(aux_loss_combine_kernel, 1, 64, 0, st, main, aux, aux_weight, out3);
  return check_launch("aux_loss_combine");
}

// ---- Dice / Focal+Dice head (utils/loss.py:12-100) -------------------------------------------
// The work layout of head_tile.hpp.  Per pixel p = softmax(z), p1 = p[1], t = float(target)
// (targets outside [0, C) count as 0):
//   sums      I = sum p1 t, S = sum p1, T = sum t, F = sum alpha (1 - pt)^gamma ce
//   loss      wd (1 - (2 I + s) / U) + wf F / npix,  U = S + T + s
//   gradient  dz_c = (a t + b) p1 ([c == 1] - p_c) + f dfocal/dce (p_c - [c == t]),
//             a = -2 wd / U, b = wd (2 I + s) / U^2, f = wf / npix.
// a and b need the global sums, but dz is linear in (a, b, f):
//   MODE 0 (C == 2, one pass): with two classes dz_0 = -dz_1, so the pass accumulates the three
//     coefficient planes of channel 1 only, interleaved per low-res cell as (Ga, Gb, Gf) =
//     sum w (t q, q, dfocal/dce (p1 - [t == 1])), q = p1 p0; dice_head_scale combines them with
//     (a, b, f) from the device-resident sums.
//   MODE 1 / MODE 2 (3 <= C <= HD_CMAX, two passes): three planes x C classes x 4 taps do not fit
//     the register file, so pass 1 forms only the sums and pass 2, after the finalize, reads
//     (a, b) from the device sums and accumulates the one combined plane a Ga + b Gb + f Gf.
// Probabilities are evaluated per pixel (v_exp_f32 / v_rcp_f32 / v_log_f32, 1 ulp) for every plan
// dtype; 1 - pt is the sum of the other classes' probabilities (no cancellation at pt -> 1).
__device__ __forceinline__ float hd_pow(float x, float g) {  // x in [0, 1]
  if (x > 0.f) return __builtin_amdgcn_exp2f(g * __builtin_amdgcn_logf(x));
  return g == 0.f ? 1.f : 0.f;
}

struct DiceCoef {
  float a, b, f;
};
__device__ __forceinline__ DiceCoef dice_coef(const double* stats, float smooth, float wd, float wf,
                                              double npix) {
  const double U = stats[1] + stats[2] + (double)smooth;
  DiceCoef k;
  k.a = (float)(-2.0 * wd / U);
  k.b = (float)(wd * (2.0 * stats[0] + smooth) / (U * U));
  k.f = (float)((double)wf / npix);
  return k;
}

template <typename T, int CT, bool EXACT, int MODE>
__global__ __launch_bounds__(HD_T) void dice_head_kernel(DiceHeadArgs a) {
  constexpr int SL = (CT % 2 == 0) ? CT + 1 : CT;  // odd LDS stride per column
  constexpr int NA = MODE == 0 ? 3 : (MODE == 1 ? 1 : CT);  // accumulated scalars per tap
  static_assert(MODE != 0 || CT == 2, "the one-pass form is the two-class form");
  static_assert(NA <= SL, "the neighbour hand-off reuses the logit rows' LDS");
  __shared__ float s_L[2 * (HD_T + 1) * SL];
  __shared__ float s_carry[2 * NA];
  __shared__ __attribute__((aligned(8))) signed char s_t[2 * HD_TMAX];
  __shared__ float s_r[4][HD_T];
  const HeadTile tl(a.Hl, a.Wl, a.H, a.W);
  const int tid = tl.tid, ldl = a.ldl, gld = a.gld;
  const int Cm = EXACT ? CT : a.C;
  const T* lg = (const T*)a.logits + tl.image(ldl);
  float* g1 = tl.spill_plane(a.planes, a.N, gld);
  const bool focal = a.focal != 0;
  DiceCoef kf{0.f, 0.f, 0.f};
  if (MODE == 2) kf = dice_coef(a.stats, a.smooth, a.wd, a.wf, (double)a.N * tl.H * tl.W);
  float sI = 0.f, sS = 0.f, sT = 0.f, sF = 0.f;
  hd_carry_zero<NA>(s_carry, tid);
  if (MODE != 1) tl.zero_spill_row0(g1, gld);
  for (int cb = 0; cb < tl.Wl; cb += HD_T) {
    hd_stage_rows_f32<T, CT, SL>(s_L, lg, tl, cb, Cm, ldl);
    const HeadCols cl(tl, cb);
    f32x2 a0[NA], a1[NA];
#pragma unroll
    for (int c = 0; c < NA; ++c) a0[c] = a1[c] = f32x2{0.f, 0.f};
    HdTargetRows<HdClampZero, true> tr(tl, a.target, a.tgt8, s_t, HdClampZero{}, Cm,
                                       tl.W <= HD_TMAX);
    tr.start(tl.h_lo, tl.h_hi);
    const float* L0 = &s_L[tid * SL];
    const float* L1 = &s_L[((HD_T + 1) + tid) * SL];
    for (int h = tl.h_lo; h < tl.h_hi; ++h) {
      tr.commit(h, tl.h_hi);
      if (cl.active) {
        const Lerp lh = ac_lerp(h, tl.Hl, tl.H, tl.sh);
        float v0[CT], dv[CT];  // row-interpolated logits of column t, and (column t+1) - v0
#pragma unroll
        for (int c = 0; c < CT; ++c) {
          v0[c] = fmaf(lh.l1, L1[c], lh.l0 * L0[c]);
          dv[c] = fmaf(lh.l1, L1[SL + c], lh.l0 * L0[SL + c]) - v0[c];
        }
        for (int w = cl.w_lo; w < cl.w_hi; ++w) {
          const Lerp lw = ac_lerp(w, tl.Wl, tl.W, tl.sw);
          const int ti = tr.get(w);
          const float tf = (float)ti;
          float e[CT];
          float mx = -INFINITY;
#pragma unroll
          for (int c = 0; c < CT; ++c) {
            e[c] = fmaf(lw.l1, dv[c], v0[c]);
            if (c < Cm) mx = fmaxf(mx, e[c]);
          }
          float se = 0.f, lt = 0.f, et = 0.f, so = 0.f;  // so: sum of the non-target exponentials
#pragma unroll
          for (int c = 0; c < CT; ++c) {
            const float x = c < Cm ? __builtin_amdgcn_exp2f(e[c] - mx) : 0.f;
            if (c == ti) lt = e[c], et = x;
            else so += x;
            se += x;
            e[c] = x;
          }
          const float inv = __builtin_amdgcn_rcpf(se);
          const float p1 = e[1] * inv;
          float dfdce = 0.f;
          if (focal) {
            const float ce = (mx - lt + __builtin_amdgcn_logf(se)) * HD_LN2;
            const float pt = et * inv, om = so * inv;
            const float pg = hd_pow(om, a.gamma);
            if (MODE != 2) sF = fmaf(a.alpha * pg, ce, sF);
            if (MODE != 1) dfdce = a.alpha * (pg + ce * a.gamma * hd_pow(om, a.gamma - 1.f) * pt);
          }
          if (MODE != 2) {
            sI = fmaf(p1, tf, sI);
            sS += p1;
            sT += tf;
          }
          if (MODE != 1) {
            const f32x2 k0 = {lh.l0 * lw.l0, lh.l0 * lw.l1};
            const f32x2 k1 = {lh.l1 * lw.l0, lh.l1 * lw.l1};
            if (MODE == 0) {
              const float q = p1 * (e[0] * inv);
              const float gv[3] = {tf * q, q, dfdce * (p1 - (ti == 1 ? 1.f : 0.f))};
#pragma unroll
              for (int j = 0; j < 3; ++j) {
                const f32x2 gg = {gv[j], gv[j]};
                a0[j] = __builtin_elementwise_fma(k0, gg, a0[j]);
                a1[j] = __builtin_elementwise_fma(k1, gg, a1[j]);
              }
            } else {
              const float cp = fmaf(kf.a, tf, kf.b) * p1, cf = kf.f * dfdce;
#pragma unroll
              for (int c = 0; c < NA; ++c) {
                const float pc = e[c] * inv;
                const float gc = cp * ((c == 1 ? 1.f : 0.f) - pc) + cf * (pc - (c == ti ? 1.f : 0.f));
                const f32x2 gg = {gc, gc};
                a0[c] = __builtin_elementwise_fma(k0, gg, a0[c]);
                a1[c] = __builtin_elementwise_fma(k1, gg, a1[c]);
              }
            }
          }
        }
      }
    }
    if (MODE == 1) continue;  // the sums pass writes no plane (uniform: no barrier is skipped)
    hd_tile_epilogue<NA>(a0, a1, tl, cl, s_L, (HD_T + 1) * SL, SL, s_carry, a.planes, g1, gld,
                         MODE == 0 ? 3 : Cm);
  }
  if (MODE == 2) return;
  s_r[0][tid] = sI;
  s_r[1][tid] = sS;
  s_r[2][tid] = sT;
  s_r[3][tid] = sF;
  hd_block_reduce<4, 0>(s_r, nullptr, tid);
  if (tid < 4) a.part[4 * ((size_t)tl.n * tl.Hl + tl.hl) + tid] = s_r[tid][0];
}

// partials [P][4] -> stats (I, S, T, F) in fp64, fixed order, and the loss
__global__ __launch_bounds__(256) void dice_head_finalize_kernel(const float* part, int P,
                                                                 float smooth, float wd, float wf,
                                                                 double npix, double* stats,
                                                                 float* loss) {
  __shared__ double r[4][256];
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int p = threadIdx.x; p < P; p += 256)
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] += part[4 * (size_t)p + k];
#pragma unroll
  for (int k = 0; k < 4; ++k) r[k][threadIdx.x] = s[k];
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (threadIdx.x < off)
#pragma unroll
      for (int k = 0; k < 4; ++k) r[k][threadIdx.x] += r[k][threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double I = r[0][0], S = r[1][0], Tt = r[2][0], F = r[3][0];
#pragma unroll
    for (int k = 0; k < 4; ++k) stats[k] = r[k][0];
    const double dice = (2.0 * I + smooth) / (S + Tt + smooth);
    loss[0] = (float)((double)wd * (1.0 - dice) + (double)wf * F / npix);
  }
}

long long dice_head_ws_bytes(int N, int Hl, int Wl, int C, int ldl) {
  const long long M = (long long)N * Hl * Wl;
  const long long planes = 2 * M * (C == 2 ? 3 : ldl) * 4;
  const long long part = (long long)N * Hl * 4 * 4;
  return (planes + 255) / 256 * 256 + part;
}

// MODE 0 is the <2, true> instance and only that; MODE 1 / 2 have no <2, true>
template <int MODE>
static void dice_head_launch(const DiceHeadArgs& a, int dtype, dim3 grid, hipStream_t st) {
  hd_dispatch(a.C, dtype, [&](auto i) {
    using I = decltype(i);
    if constexpr ((I::CT == 2) == (MODE == 0))
      prof_launch((dice_head_kernel<typename I::T, I::CT, I::EXACT, MODE>), grid, HD_T, 0, st, a);
  });
}

int dice_head(const DiceHeadArgs& a0, void* head_ws, float* loss, double* stats, int dtype,
              hipStream_t st) {
  if (a0.C < 2 || a0.C > HD_CMAX) {
    set_error("dice_head: %d classes (2 .. %d)", a0.C, HD_CMAX);
    return E_UNSUPPORTED;
  }
  DiceHeadArgs a = a0;
  const long long M = (long long)a.N * a.Hl * a.Wl;
  a.gld = a.C == 2 ? 3 : a.ldl;
  a.planes = (float*)head_ws;
  a.part = (float*)((char*)head_ws + ((2 * M * a.gld * 4 + 255) / 256 * 256));
  a.stats = stats;
  const dim3 grid(a.Hl, a.N);
  const int P = a.N * a.Hl;
  const double npix = (double)a.N * a.H * a.W;
  const double lb = (dtype == DT_F32 ? 4.0 : 2.0) * M * a.C, tb = (a.tgt8 ? 1.0 : 8.0) * npix;
  if (a.C == 2) {
    ProfScope ps(PK_CE, st, lb + tb + 2.0 * 4.0 * M * 3, 0.0);
    dice_head_launch<0>(a, dtype, grid, st);
    if (int rc = check_launch("dice_head")) return rc;
    prof_launch(dice_head_finalize_kernel, 1, 256, 0, st, a.part, P, a.smooth, a.wd, a.wf, npix,
                stats, loss);
    return check_launch("dice_head_finalize");
  }
  ProfScope ps(PK_CE, st, 2.0 * (lb + tb) + 2.0 * 4.0 * M * a.C, 0.0);
  dice_head_launch<1>(a, dtype, grid, st);
  if (int rc = check_launch("dice_head (sums)")) return rc;
  prof_launch(dice_head_finalize_kernel, 1, 256, 0, st, a.part, P, a.smooth, a.wd, a.wf, npix,
              stats, loss);
  if (int rc = check_launch("dice_head_finalize")) return rc;
  dice_head_launch<2>(a, dtype, grid, st);
  return check_launch("dice_head (gradient)");
}

// g[m][c] = gout * (a Ga + b Gb + f Gf) (two classes: channel 1, channel 0 its negative) or
// gout * the combined plane (general C); own-row plane + the spill of the row above, fixed order;
// gout is taken times `weight` (1: the single-output head, bit for bit; the aux head: aux_weight
// -- the general-C plane already holds a, b, f, so the factor cannot ride in wd / wf)
template <typename T>
__global__ __launch_bounds__(256) void dice_head_scale_kernel(const float* planes, T* g, int M,
                                                              int C, int ld, const float* gout,
                                                              const double* stats, float smooth,
                                                              float wd, float wf, double npix,
                                                              float weight) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M * ld) return;
  const int c = i % ld, m = i / ld;
  const float go = gout[0] * weight;
  float v = 0.f;
  if (C == 2) {
    if (c < 2) {
      const DiceCoef k = dice_coef(stats, smooth, wd, wf, npix);
      const float* o = planes + (size_t)m * 3;
      const float* s = planes + ((size_t)M + m) * 3;
      v = k.a * (o[0] + s[0]) + k.b * (o[1] + s[1]) + k.f * (o[2] + s[2]);
      v = (c == 1 ? v : -v) * go;
    }
  } else if (c < C) {
    v = (planes[i] + planes[(size_t)M * ld + i]) * go;
  }
  st1(g + i, v);
}

int dice_head_scale(const void* head_ws, void* g, long long M, int C, int ld, const float* gout,
                    const double* stats, float smooth, float wd, float wf, double npix, int dtype,
                    hipStream_t st, float weight) {
  const int total = (int)(M * ld);
  const float* pl = (const float*)head_ws;
  hd_dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::T;
    prof_launch(dice_head_scale_kernel<T>, cdiv(total, 256), 256, 0, st, pl, (T*)g, (int)M, C, ld,
                gout, stats, smooth, wd, wf, npix, weight);
  });
  return check_launch("dice_head_scale");
}

// ---- OHEM head (utils/loss.py:127-206, the criterion of train.py:189-191) ----------------------
// nn.CrossEntropyLoss(weight, ignore_index) over the KEPT pixels of the upsampled logits, a pixel
// being kept when it is labelled and the softmax probability of its label is <= the threshold of
// utils/loss.py:159-170.  The work layout of head_tile.hpp.  Probabilities are evaluated per
// pixel (v_exp_f32 / v_rcp_f32) for every plan dtype, so one error bound holds for all of them.
//   PASS 1: prob[pixel] = p_label (2.0: ignored / out of range) as an fp32 plane, the two integer
//     counters ohem_threshold_dev reads (#labelled, #(prob <= thresh)), and -- assuming the
//     threshold will be `thresh`, the common case in training -- the loss partials (sum w nll,
//     sum w) and g_raw = sum w[t] (softmax - onehot) folded onto the four low-res taps.
//   ohem_threshold_dev on the plane: *thr = thresh, inf or the k-th smallest probability.
//   PASS 2: returns at once when *thr is bit-equal to thresh; otherwise recomputes the partials
//     and g_raw over prob[pixel] <= *thr.  The keep decision is always the comparison of the
//     STORED fp32 value the select saw, never a re-evaluation, so mask and threshold agree.
// The gradient has no atomics (the counters are integer adds: exact in any order): two runs give
// identical bits.
template <typename T, int CT, bool EXACT, int PASS>
__global__ __launch_bounds__(HD_T) void ohem_head_kernel(OhemHeadArgs a) {
  constexpr int SL = (CT % 2 == 0) ? CT + 1 : CT;  // odd LDS stride per column
  constexpr int CP = (CT + 1) / 2;
  float thr = a.thresh;
  if (PASS == 2) {
    thr = *a.thr;
    if (__float_as_uint(thr) == __float_as_uint(a.thresh)) return;  // pass 1's result stands
  }
  __shared__ float s_L[2 * (HD_T + 1) * SL];
  __shared__ float s_carry[2 * CT];
  __shared__ float s_w[CT];
  __shared__ __attribute__((aligned(8))) signed char s_t[2 * HD_TMAX];
  __shared__ float s_r[2][HD_T];
  __shared__ unsigned s_c[2][HD_T];
  const HeadTile tl(a.Hl, a.Wl, a.H, a.W);
  const int tid = tl.tid, ldl = a.ldl;
  const int Cm = EXACT ? CT : a.C;
  const T* lg = (const T*)a.logits + tl.image(ldl);
  float* g1 = tl.spill_plane(a.g_raw, a.N, ldl);
  float* prob = a.prob + (size_t)tl.n * tl.H * tl.W;
  float loss = 0.f, wsum = 0.f;
  unsigned nlab = 0u, nle = 0u;
  hd_carry_zero<CT>(s_carry, tid);
  if (tid < CT) s_w[tid] = (a.weight && tid < Cm) ? a.weight[tid] : 1.f;
  tl.zero_spill_row0(g1, ldl);
  for (int cb = 0; cb < tl.Wl; cb += HD_T) {
    hd_stage_rows_f32<T, CT, SL>(s_L, lg, tl, cb, Cm, ldl);
    const HeadCols cl(tl, cb);
    f32x2 a0[CT], a1[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) a0[c] = a1[c] = f32x2{0.f, 0.f};
    // PASS 1 stages the target rows; PASS 2 reads the targets of kept pixels only
    HdTargetRows<HdIgnoreAware, true> tr(tl, a.target, a.tgt8, s_t, HdIgnoreAware{a.ignore_index},
                                         Cm, PASS == 1 && tl.W <= HD_TMAX);
    tr.start(tl.h_lo, tl.h_hi);
    const float* L0 = &s_L[tid * SL];
    const float* L1 = &s_L[((HD_T + 1) + tid) * SL];
    for (int h = tl.h_lo; h < tl.h_hi; ++h) {
      tr.commit(h, tl.h_hi);
      if (cl.active) {
        const Lerp lh = ac_lerp(h, tl.Hl, tl.H, tl.sh);
        f32x2 v0[CP], dv[CP];
        hd_lerp_rows_pk<CT, SL>(L0, L1, lh, v0, dv);
        float* prow = prob + (size_t)h * tl.W;
        for (int w = cl.w_lo; w < cl.w_hi; ++w) {
          int ti;
          float pv = 2.f;
          if (PASS == 1) {
            ti = tr.get(w);
            if (ti < 0) {  // ignored: sorts after every probability, never kept
              prow[w] = 2.f;
              continue;
            }
          } else {
            pv = prow[w];
            if (!(pv <= thr && pv < 1.5f)) continue;  // not kept (2.0: ignored, also under inf)
            ti = tr.t8 ? (int)tr.tgt8[(size_t)h * tl.W + w] : (int)tr.trow[w];
            ti = min(max(ti, 0), Cm - 1);  // (a kept pixel is a labelled one: already in range)
          }
          const Lerp lw = ac_lerp(w, tl.Wl, tl.W, tl.sw);
          const f32x2 w1 = {lw.l1, lw.l1};
          f32x2 e[CP];
#pragma unroll
          for (int p = 0; p < CP; ++p) e[p] = __builtin_elementwise_fma(w1, dv[p], v0[p]);
          float mx = -INFINITY;
#pragma unroll
          for (int p = 0; p < CP; ++p) {
            if (2 * p < Cm) mx = fmaxf(mx, e[p].x);
            if (2 * p + 1 < Cm) mx = fmaxf(mx, e[p].y);
          }
          // the target's logit, re-interpolated from the staged rows with the same operations
          float lt;
          {
            const float v0t = fmaf(lh.l1, L1[ti], lh.l0 * L0[ti]);
            const float v1t = fmaf(lh.l1, L1[SL + ti], lh.l0 * L0[SL + ti]);
            lt = fmaf(lw.l1, v1t - v0t, v0t);
          }
          float se = 0.f;
#pragma unroll
          for (int p = 0; p < CP; ++p) {
            e[p].x = 2 * p < Cm ? __builtin_amdgcn_exp2f(e[p].x - mx) : 0.f;
            e[p].y = 2 * p + 1 < Cm ? __builtin_amdgcn_exp2f(e[p].y - mx) : 0.f;
            se += e[p].x + e[p].y;
          }
          const float inv = __builtin_amdgcn_rcpf(se);  // v_rcp_f32 (1 ulp)
          if (PASS == 1) {
            pv = __builtin_amdgcn_exp2f(lt - mx) * inv;
            prow[w] = pv;
            nlab += 1u;
            if (!(pv <= thr)) continue;  // the comparison of the value just stored
            nle += 1u;
          }
          const float wt = s_w[ti];
          loss = fmaf(wt, (mx - lt + __builtin_amdgcn_logf(se)) * HD_LN2, loss);
          wsum += wt;
          hd_tap_accum_pk<CT>(a0, a1, e, inv, wt, ti, true, lh, lw);
        }
      }
    }
    hd_tile_epilogue<CT>(a0, a1, tl, cl, s_L, (HD_T + 1) * SL, SL, s_carry, a.g_raw, g1, ldl, Cm);
  }
  s_r[0][tid] = loss;
  s_r[1][tid] = wsum;
  s_c[0][tid] = nlab;
  s_c[1][tid] = nle;
  hd_block_reduce<2, 2>(s_r, s_c, tid);
  if (tid == 0) {
    const size_t pi = (size_t)tl.n * tl.Hl + tl.hl;
    a.part[2 * pi] = s_r[0][0];
    a.part[2 * pi + 1] = s_r[1][0];
    if (PASS == 1) {
      if (s_c[0][0]) atomicAdd(&a.counts[0], (unsigned long long)s_c[0][0]);
      if (s_c[1][0]) atomicAdd(&a.counts[1], (unsigned long long)s_c[1][0]);
    }
  }
}

// the counters are zeroed inside the run (the library replays its runs as captured graphs)
__global__ void ohem_head_zero_kernel(unsigned long long* counts) {
  if (threadIdx.x < 2) counts[threadIdx.x] = 0ull;
}

template <int PASS>
static void ohem_head_launch(const OhemHeadArgs& a, int dtype, dim3 grid, hipStream_t st) {
  hd_dispatch(a.C, dtype, [&](auto i) {
    using I = decltype(i);
    prof_launch((ohem_head_kernel<typename I::T, I::CT, I::EXACT, PASS>), grid, HD_T, 0, st, a);
  });
}

bool ohem_head_ok(int C) { return C >= 1 && C <= HD_CMAX; }

int ohem_head(const OhemHeadArgs& a, long long min_kept, unsigned* work, float* out2, int dtype,
              hipStream_t st) {
  if (!ohem_head_ok(a.C)) {
    set_error("ohem_head: %d classes (max %d)", a.C, HD_CMAX);
    return E_UNSUPPORTED;
  }
  if (min_kept < 0 || !a.prob || !a.thr || !a.counts || !work) {
    set_error("ohem_head: min_kept=%lld / null buffer", min_kept);
    return E_INVALID;
  }
  const dim3 grid(a.Hl, a.N);
  const int P = ce_head_parts(a.N, a.Hl, a.Wl);
  const double npix = (double)a.N * a.H * a.W, M = (double)a.N * a.Hl * a.Wl;
  {
    ProfScope ps(PK_CE, st, (dtype == DT_F32 ? 4.0 : 2.0) * M * a.C + (a.tgt8 ? 1.0 : 8.0) * npix +
                                4.0 * npix + 2.0 * 4.0 * M * a.C, 0.0);
    prof_launch(ohem_head_zero_kernel, 1, 64, 0, st, a.counts);
    ohem_head_launch<1>(a, dtype, grid, st);
    if (int rc = check_launch("ohem_head (pass 1)")) return rc;
    prof_launch(ce_head_finalize_kernel, 1, 256, 0, st, a.part, P, (const float*)nullptr,
                a.thresh, out2);
    if (int rc = check_launch("ohem_head_finalize")) return rc;
  }
  if (int rc = ohem_threshold_dev(a.prob, (long long)npix, a.counts, min_kept, a.thresh, work,
                                  const_cast<float*>(a.thr), st))
    return rc;
  ProfScope ps(PK_CE, st, 4.0 * npix, 0.0);
  ohem_head_launch<2>(a, dtype, grid, st);
  if (int rc = check_launch("ohem_head (pass 2)")) return rc;
  prof_launch(ce_head_finalize_kernel, 1, 256, 0, st, a.part, P, a.thr, a.thresh, out2);
  return check_launch("ohem_head_finalize (pass 2)");
}

}  // namespace fscnn
