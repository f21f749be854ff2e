// Fused validation head: the final F.interpolate(bilinear, align_corners=True) of the logits
// (models/fast_scnn.py:40), the criterion's loss and the SegmentationMetric counters
// (Trainer.validation, train.py:370-439) in one pass over the LOW-resolution logits and the
// targets.  Nothing of full resolution is written: the outputs are one partial record per
// workgroup (reduced in a fixed order in fp64 by eval_head_finalize_kernel) and the 2 + 3C
// integer counters.
//
// Work layout (up_argmax's, interp.hip): a tile is EH_R output rows x EH_COLS output columns of
// one image; the workgroup stages the low-res rows / columns the tile interpolates from in LDS,
// class-major [row][C + 1][WP] in fp32 (plane C: each cell's maximum over the classes); a thread
// owns 4 consecutive columns of each of the EH_R rows and walks the classes outermost.  At most
// EH_MAXWG workgroups walk the tiles, so the loss sums and the counters stay on chip across a
// workgroup's tiles: one partial record and one round of global integer adds per workgroup.  Every
// logit is formed exactly as up_nchw / up_argmax form it (ac_lerp weights, lerp2 W-then-H,
// round_as<T>), so the argmax is the label predict() writes and the softmax is that of the logits
// model(x) stores.
//
// Softmax reference: a bilinear tap is a convex combination, so no logit of a thread's pixels
// exceeds M = the largest staged logit of the cells those pixels touch.  The class walk sums
// 2^(z log2e - M log2e) against that fixed M -- one fma, one v_exp_f32 and one add per class and
// pixel, nothing to rescale -- next to the running maximum (strict >, the lowest class wins ties)
// and its class.  A pixel whose own maximum lies more than EH_SPREAD below M (neighbouring cells
// that far apart: its sum could lose bits towards the fp32 underflow) is summed again against
// its own maximum.  The target's logit and class 1's (Dice) are re-interpolated from the staged
// rows after the walk with the same operations, hence the same bits.  Dice sums leave the target
// class out of the walk's sum (so), so 1 - pt = so / se has no cancellation at pt -> 1.
//
// Targets are read once, as int64, before the staging (their latency overlaps it) and kept as one
// byte per pixel: class | labeled (t >= 0) | in range (0 <= t < C) | valid for the CE sum.
#include "kernels.hpp"

namespace fscnn {

constexpr int EH_T = 256;
constexpr int EH_COLS = 4 * EH_T;
constexpr int EH_R = 4;       // output rows per workgroup
constexpr int EH_MAXR = 3;    // staged source rows per workgroup (host-checked)
constexpr int EH_CMAX = 32;   // classes (5 bits of the target byte; the Dice head's bound)
constexpr int EH_MAXWG = 1024;  // 4 workgroups per CU: all resident at once
constexpr float EH_LOG2E = 1.4426950408889634f;
constexpr float EH_LN2 = 0.6931471805599453f;
constexpr float EH_SPREAD = 60.f;
constexpr unsigned EH_LAB = 32u, EH_INR = 64u, EH_VAL = 128u;

__device__ __forceinline__ float eh_pow(float x, float g) {  // x in [0, 1]
  if (x > 0.f) return __builtin_amdgcn_exp2f(g * __builtin_amdgcn_logf(x));
  return g == 0.f ? 1.f : 0.f;
}

template <typename T, bool DICE, bool COUNT>
__global__ __launch_bounds__(EH_T, 4) void eval_head_kernel(EvalHeadArgs a, int WP, int HOFF) {
  extern __shared__ float eh_rows[];  // [rows][C + 1][WP], then s_hist at float offset HOFF
  // (prediction, target) pair counts [C][C + 1]; column C: labeled targets outside [0, C)
  unsigned* s_hist = reinterpret_cast<unsigned*>(eh_rows + HOFF);
  __shared__ unsigned s_cnt[2 + 3 * EH_CMAX];
  __shared__ float s_red[4][EH_T];
  const int tid = threadIdx.x;
  const int C = a.C, H = a.H, W = a.W, Hl = a.Hl, Wl = a.Wl;
  const float sh = ac_scale(Hl, H), sw = ac_scale(Wl, W);
  if (COUNT) {
    for (int j = tid; j < C * (C + 1); j += EH_T) s_hist[j] = 0u;
  }
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  // a workgroup walks tiles blockIdx.x, blockIdx.x + gridDim.x, ...: its sums and counters stay
  // on chip across them (one partial record and one round of global integer adds per workgroup)
  const int gx = cdiv(W, EH_COLS), gy = cdiv(H, EH_R);
  for (int item = blockIdx.x; item < gx * gy * a.N; item += gridDim.x) {
    const int bx = item % gx, by = (item / gx) % gy, n = item / (gx * gy);
    const int ho0 = by * EH_R;
    const int ho1 = min(ho0 + EH_R, H) - 1;
    const int wb0 = bx * EH_COLS, wb1 = min(wb0 + EH_COLS, W) - 1;
    const int wo0 = wb0 + tid * 4;

    // ---- targets: 4 per row and thread, packed to one byte each ------------------------------
    unsigned tp[EH_R];
    {
      const long long* tg = a.target + ((size_t)n * H + ho0) * W;
      const bool vec = a.tvec && wo0 + 4 <= W;
#pragma unroll
      for (int q = 0; q < EH_R; ++q) {
        long long t[4] = {-1, -1, -1, -1};
        if (ho0 + q <= ho1) {
          const long long* p = tg + (size_t)q * W + wo0;
          if (vec) {
            const longlong2 u = reinterpret_cast<const longlong2*>(p)[0];
            const longlong2 v = reinterpret_cast<const longlong2*>(p)[1];
            t[0] = u.x; t[1] = u.y; t[2] = v.x; t[3] = v.y;
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (wo0 + j < W) t[j] = p[j];
          }
        }
        unsigned w = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bool inr = t[j] >= 0 && t[j] < C;
          unsigned b = inr ? (unsigned)t[j] | EH_INR : 0u;
          if (t[j] >= 0) b |= EH_LAB;
          if (inr && t[j] != a.ignore_index) b |= EH_VAL;
          w |= b << (8 * j);
        }
        tp[q] = w;
      }
    }

    // ---- stage the low-res rows lo .. lo + nrows - 1, columns cl0 .. cl0 + ncols - 1 ---------
    __syncthreads();  // the previous tile's staged rows are no longer read (s_hist is zero)
    const int lo = ac_lerp(ho0, Hl, H, sh).i0;
    const int nrows = ac_lerp(ho1, Hl, H, sh).i1 - lo + 1;  // <= EH_MAXR (host-checked)
    const int cl0 = ac_lerp(wb0, Wl, W, sw).i0;
    const int ncols = ac_lerp(wb1, Wl, W, sw).i1 - cl0 + 1;  // <= WP (host-checked)
    const int CWP = (C + 1) * WP, CN = C * ncols;
    {
      const T* xb = (const T*)a.logits + (((size_t)n * Hl + lo) * Wl + cl0) * a.ldl;
      const int ne = nrows * CN;
      for (int e0 = tid; e0 < ne; e0 += 4 * EH_T) {  // 4 loads in flight per thread
        float v[4];
        int li[4];  // LDS index, -1 past the end
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int e = e0 + u * EH_T, ec = e < ne ? e : e0;
          const int r = ec / CN;
          const int rem = ec - r * CN;
          const int wi = rem / C, c = rem - wi * C;
          v[u] = ld1(xb + ((size_t)r * Wl + wi) * a.ldl + c);
          li[u] = e < ne ? r * CWP + c * WP + wi : -1;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (li[u] >= 0) eh_rows[li[u]] = v[u];
      }
    }
    __syncthreads();
    for (int i = tid; i < nrows * ncols; i += EH_T) {  // plane C: the cells' maxima
      const int r = i / ncols, wi = i - r * ncols;
      float* cell = eh_rows + r * CWP + wi;
      float m = cell[0];
      for (int c = 1; c < C; ++c) m = fmaxf(m, cell[c * WP]);
      cell[C * WP] = m;
    }
    __syncthreads();

    // ---- the class walk -------------------------------------------------------------------------
    // (columns / rows past the image are computed on clamped coordinates and dropped at the end)
    int wi0[4], wi1[4];
    float wl1[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const Lerp l = ac_lerp(min(wo0 + j, W - 1), Wl, W, sw);
      wi0[j] = l.i0 - cl0;
      wi1[j] = l.i1 - cl0;
      wl1[j] = l.l1;
    }
    int hd0[EH_R], hd1[EH_R];
    float hl0[EH_R], hl1[EH_R];
#pragma unroll
    for (int q = 0; q < EH_R; ++q) {
      const Lerp l = ac_lerp(min(ho0 + q, ho1), Hl, H, sh);
      hd0[q] = l.i0 - lo;
      hd1[q] = l.i1 - lo;
      hl0[q] = l.l0;
      hl1[q] = l.l1;
    }
    float M = -INFINITY;  // bound of every logit of this thread's pixels
    for (int r = 0; r < nrows; ++r)
      for (int wi = wi0[0]; wi <= wi1[3]; ++wi) M = fmaxf(M, eh_rows[r * CWP + C * WP + wi]);
    const float K = -(M * EH_LOG2E);
    // one logit of pixel (q, j), as the walk forms it
    auto logit = [&](int q, int j, int c) -> float {
      const float* r0 = eh_rows + hd0[q] * CWP + c * WP;
      const float* r1 = eh_rows + hd1[q] * CWP + c * WP;
      const float l0 = 1.0f - wl1[j];
      const float x0 = lerp2(l0, r0[wi0[j]], wl1[j], r0[wi1[j]]);
      const float x1 = lerp2(l0, r1[wi0[j]], wl1[j], r1[wi1[j]]);
      return round_as<T>(lerp2(hl0[q], x0, hl1[q], x1));
    };
    float best[EH_R][4], acc[EH_R][4];
    int arg[EH_R][4];
#pragma unroll
    for (int q = 0; q < EH_R; ++q)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        best[q][j] = -INFINITY;
        acc[q][j] = 0.f;
        arg[q][j] = 0;
      }
#pragma unroll 1
    for (int c = 0; c < C; ++c) {
      float wr[EH_MAXR][4];
#pragma unroll
      for (int r = 0; r < EH_MAXR; ++r) {
        const float* row = eh_rows + min(r, nrows - 1) * CWP + c * WP;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          wr[r][j] = lerp2(1.0f - wl1[j], row[wi0[j]], wl1[j], row[wi1[j]]);  // l0 = 1 - l1
      }
#pragma unroll
      for (int q = 0; q < EH_R; ++q) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float x0 = wr[0][j], x1 = wr[0][j];
#pragma unroll
          for (int r = 1; r < EH_MAXR; ++r) {  // register selects, no dynamic indexing
            x0 = hd0[q] == r ? wr[r][j] : x0;
            x1 = hd1[q] == r ? wr[r][j] : x1;
          }
          const float o = round_as<T>(lerp2(hl0[q], x0, hl1[q], x1));  // the logit up_nchw stores
          const float e = __builtin_amdgcn_exp2f(fmaf(o, EH_LOG2E, K));
          if (DICE) acc[q][j] += (int)((tp[q] >> (8 * j)) & 31u) == c ? 0.f : e;
          else acc[q][j] += e;
          const bool gt = o > best[q][j];
          best[q][j] = gt ? o : best[q][j];
          if (COUNT) arg[q][j] = gt ? c : arg[q][j];
        }
      }
    }

    // ---- per pixel: the criterion's terms and the counters ------------------------------------
    // counters: a labeled pixel adds one to its (prediction, target) pair; runs of equal pairs
    // along the thread's pixels (label maps are piecewise constant) go out as one LDS add
    unsigned run_key = 0, run_len = 0;
    auto flush = [&]() {
      if (run_len) atomicAdd(&s_hist[run_key], run_len);
    };
#pragma unroll
    for (int q = 0; q < EH_R; ++q) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (ho0 + q > ho1 || wo0 + j >= W) continue;
        const unsigned tb = (tp[q] >> (8 * j)) & 255u;
        const int tc = (int)(tb & 31u);
        if (DICE || (tb & EH_VAL)) {
          float sum = acc[q][j], k = K;
          if (M - best[q][j] > EH_SPREAD) {  // far below the bound: against the pixel's own maximum
            k = -(best[q][j] * EH_LOG2E);
            sum = 0.f;
            for (int c = 0; c < C; ++c)
              if (!DICE || c != tc) sum += __builtin_amdgcn_exp2f(fmaf(logit(q, j, c), EH_LOG2E, k));
          }
          const float lt = logit(q, j, tc);
          if (DICE) {  // targets outside [0, C) count as t = 0 (class bits 0)
            const float se = sum + __builtin_amdgcn_exp2f(fmaf(lt, EH_LOG2E, k));
            const float l2 = __builtin_amdgcn_logf(se) - k;  // log2 of sum_c e^z
            const float p1 = __builtin_amdgcn_exp2f(fmaf(logit(q, j, 1), EH_LOG2E, -l2));
            const float tf = (float)tc;
            s0 = fmaf(p1, tf, s0);
            s1 += p1;
            s2 += tf;
            if (a.focal) {
              const float ce = fmaf(-lt, EH_LOG2E, l2) * EH_LN2;
              const float om = sum * __builtin_amdgcn_rcpf(se);  // 1 - pt
              s3 = fmaf(a.alpha * eh_pow(om, a.gamma), ce, s3);
            }
          } else {
            const float l2 = __builtin_amdgcn_logf(sum) - k;
            s0 += fmaf(-lt, EH_LOG2E, l2) * EH_LN2;
            s1 += 1.f;
          }
        }
        if (COUNT && (tb & EH_LAB)) {
          const unsigned key = (unsigned)(arg[q][j] * (C + 1) + ((tb & EH_INR) ? tc : C));
          if (key == run_key) {
            ++run_len;
          } else {
            flush();
            run_key = key;
            run_len = 1;
          }
        }
      }
    }
    if (COUNT) flush();
  }  // tiles
  s_red[0][tid] = s0;
  s_red[1][tid] = s1;
  s_red[2][tid] = s2;
  s_red[3][tid] = s3;
  __syncthreads();
  for (int off = EH_T / 2; off > 0; off >>= 1) {
    if (tid < off) {
#pragma unroll
      for (int k = 0; k < 4; ++k) s_red[k][tid] += s_red[k][tid + off];
    }
    __syncthreads();
  }
  if (tid < 4) a.part[4 * (size_t)blockIdx.x + tid] = s_red[tid][0];
  if (COUNT) {
    // seg_metric_kernel's counters (misc.hip) from the pair counts: inter[c] = #(p = t = c),
    // area_pred[c] = #(p = c, t >= 0), area_lab[c] = #(t = c); correct and labeled: their sums
    for (int j = tid; j < 3 * C; j += EH_T) {
      const int c = j % C, kind = j / C;
      unsigned v = 0;
      if (kind == 0) v = s_hist[c * (C + 1) + c];
      else if (kind == 1) for (int t = 0; t <= C; ++t) v += s_hist[c * (C + 1) + t];
      else for (int p = 0; p < C; ++p) v += s_hist[p * (C + 1) + c];
      s_cnt[2 + j] = v;
    }
    __syncthreads();
    if (tid < 2) {
      unsigned v = 0;
      for (int c = 0; c < C; ++c) v += s_cnt[2 + tid * C + c];
      s_cnt[tid] = v;
    }
    __syncthreads();
    for (int j = tid; j < 2 + 3 * C; j += EH_T)  // integer adds: exact and order independent
      if (s_cnt[j]) atomicAdd(&a.counts[j], (unsigned long long)s_cnt[j]);
  }
}

// partial records [P][4] -> the loss, in fp64 and a fixed order (ce_head_finalize_kernel's and
// dice_head_finalize_kernel's formulas): CE = sum / count (NaN without a valid pixel, like the
// mean over no element), Dice = wd (1 - (2 I + s) / (S + T + s)) + wf F / npix.
// loss = (accumulate ? loss : 0) + weight * value: the aux pass adds aux_weight * its loss.
__global__ __launch_bounds__(256) void eval_head_finalize_kernel(const float* part, int P, int dice,
                                                                 float smooth, float wd, float wf,
                                                                 double npix, float weight,
                                                                 int accumulate, float* loss) {
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
    float v;
    if (dice) {
      const double I = r[0][0], S = r[1][0], Tt = r[2][0], F = r[3][0];
      const double d = (2.0 * I + smooth) / (S + Tt + smooth);
      v = (float)((double)wd * (1.0 - d) + (double)wf * F / npix);
    } else {
      v = r[1][0] > 0 ? (float)(r[0][0] / r[1][0]) : NAN;
    }
    loss[0] = accumulate ? fmaf(weight, v, loss[0]) : weight * v;
  }
}

namespace {

struct EhGeom {
  int rows, wp, gx, gy;
};
EhGeom eh_geom(int Hl, int Wl, int H, int W) {
  const float sh = ac_scale(Hl, H), sw = ac_scale(Wl, W);
  EhGeom g{0, 0, cdiv(W, EH_COLS), cdiv(H, EH_R)};
  for (int h0 = 0; h0 < H; h0 += EH_R) {
    const int h1 = std::min(h0 + EH_R, H) - 1;
    g.rows = std::max(g.rows, ac_lerp(h1, Hl, H, sh).i1 - ac_lerp(h0, Hl, H, sh).i0 + 1);
  }
  for (int w0 = 0; w0 < W; w0 += EH_COLS) {
    const int w1 = std::min(w0 + EH_COLS, W) - 1;
    g.wp = std::max(g.wp, ac_lerp(w1, Wl, W, sw).i1 - ac_lerp(w0, Wl, W, sw).i0 + 1);
  }
  g.wp |= 1;  // odd plane stride: the staging stores walk c
  return g;
}

template <typename T>
void eh_launch(const EvalHeadArgs& a, dim3 g, size_t lds, int wp, int hoff, hipStream_t st) {
  if (a.dice) {
    if (a.counts) prof_launch((eval_head_kernel<T, true, true>), g, EH_T, lds, st, a, wp, hoff);
    else prof_launch((eval_head_kernel<T, true, false>), g, EH_T, lds, st, a, wp, hoff);
  } else {
    if (a.counts) prof_launch((eval_head_kernel<T, false, true>), g, EH_T, lds, st, a, wp, hoff);
    else prof_launch((eval_head_kernel<T, false, false>), g, EH_T, lds, st, a, wp, hoff);
  }
}

}  // namespace

// workgroups (= partial records): one per tile up to EH_MAXWG, which then walk the tiles
int eval_head_parts(int N, int H, int W) {
  const long long tiles = (long long)N * cdiv(H, EH_R) * cdiv(W, EH_COLS);
  return (int)std::min<long long>(tiles, EH_MAXWG);
}

bool eval_head_ok(int N, int C, int Hl, int Wl, int H, int W, int dice) {
  if (N < 1 || C < (dice ? 2 : 1) || C > EH_CMAX || Hl < 1 || Wl < 1 || H < 1 || W < 1)
    return false;
  const EhGeom g = eh_geom(Hl, Wl, H, W);
  return g.rows <= EH_MAXR && ((size_t)g.rows * g.wp + C) * (C + 1) * sizeof(float) <= 64 * 1024 &&
         (long long)N * g.gx * g.gy < (1LL << 31);
}

int eval_head(const EvalHeadArgs& a0, int dtype, hipStream_t st) {
  if (!eval_head_ok(a0.N, a0.C, a0.Hl, a0.Wl, a0.H, a0.W, a0.dice)) {
    set_error("eval_head: unsupported geometry (C=%d Hl=%d Wl=%d H=%d W=%d)", a0.C, a0.Hl, a0.Wl,
              a0.H, a0.W);
    return E_UNSUPPORTED;
  }
  EvalHeadArgs a = a0;
  a.tvec = a.W % 2 == 0 && ((uintptr_t)a.target & 15) == 0;
  const EhGeom g = eh_geom(a.Hl, a.Wl, a.H, a.W);
  const int hoff = g.rows * (a.C + 1) * g.wp;  // floats: the staged rows, then the pair counts
  const size_t lds = ((size_t)hoff + (size_t)a.C * (a.C + 1)) * sizeof(float);
  const dim3 grid((unsigned)eval_head_parts(a.N, a.H, a.W));
  {
    ProfScope ps(PK_CE, st,
                 (dtype == DT_F32 ? 4.0 : 2.0) * a.N * a.Hl * a.Wl * a.C + 8.0 * a.N * a.H * a.W,
                 0.0);
    if (dtype == DT_F32) eh_launch<float>(a, grid, lds, g.wp, hoff, st);
    else if (dtype == DT_F16) eh_launch<f16>(a, grid, lds, g.wp, hoff, st);
    else eh_launch<bf16>(a, grid, lds, g.wp, hoff, st);
    if (int rc = check_launch("eval_head")) return rc;
  }
  prof_launch(eval_head_finalize_kernel, 1, 256, 0, st, a.part, eval_head_parts(a.N, a.H, a.W),
              a.dice, a.smooth, a.wd, a.wf, (double)a.N * a.H * a.W, a.weight, a.accumulate, a.loss);
  return check_launch("eval_head_finalize");
}

}  // namespace fscnn
