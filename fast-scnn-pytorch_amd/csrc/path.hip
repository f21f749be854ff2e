// Steering tail of the deployment pipeline: row table -> centreline -> weighted polynomial fit ->
// waypoints -> preview point -> EMA -> wheel PWM, one workgroup per frame, one launch
// (kuruma/vision/path_planning.py:316-525, kuruma/control/visual_controller.py:72-207, 236-308;
// the law: include/fastscnn.h).
//
// The fit never forms the normal equations.  The column-scaled weighted Vandermonde matrix of
// these views has condition number 3e4 .. 1e6 (1e6-weight anchor, degrees 1 .. 3); measured on the
// CPU against an 80-bit Householder solve, np.polyfit sits 2e-11 .. 4e-9 cm away on the waypoints,
// an fp64 normal-equations solve 1e-4 .. 6e-4 cm, and a row-streaming Givens QR in fp64 without
// column scaling 3e-11 .. 1.1e-9 cm from np.polyfit.  So every thread folds the weighted rows
// [y^d .. y 1 | x] of its bird's-eye rows (y = tid, tid + 256, ...) into a private upper triangle
// [R | Q^T b] in registers by Givens rotations; two triangles are combined by appending the rows of
// one to the other, down the wave with __shfl_down and across the four waves through LDS; the
// anchor row goes in last.  No matrix is stored anywhere, there is no workspace and no atomic.
// A thread without a selected row holds an all-zero triangle: the append skips a zero entry, so
// hypot(0, 0) is never divided by.
#include "kernels.hpp"

#include "../../include/fastscnn.h"

#include <climits>
#include <cmath>

namespace fscnn {

constexpr int PP_T = 256;
constexpr int PP_WAVES = PP_T / 64;

// [R | c]: r[j][k] for j <= k <= NC is the upper triangle and the rotated right-hand side (column
// NC); entries below the diagonal are never touched.  Every index is a compile-time constant after
// unrolling, so the triangle lives in registers.
template <int NC>
struct PpTri {
  double r[NC][NC + 1];
};

// Append one row v[0 .. NC] (v[NC] = right-hand side) to the triangle; v is consumed.
template <int NC>
__device__ __forceinline__ void pp_append(PpTri<NC>& t, double (&v)[NC + 1]) {
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    const double b = v[j];
    if (b != 0.0) {  // (a zero entry needs no rotation; with a == 0 too there is none to make)
      const double a = t.r[j][j];
      const double h = hypot(a, b);
      const double c = a / h, s = b / h;
      t.r[j][j] = h;
#pragma unroll
      for (int k = j + 1; k <= NC; ++k) {
        const double u = t.r[j][k], w = v[k];
        t.r[j][k] = c * u + s * w;
        v[k] = c * w - s * u;
      }
    }
  }
}

// Append row j of a triangle held as a flat [NC][NC + 1] array.
template <int NC, typename F>
__device__ __forceinline__ void pp_merge(PpTri<NC>& t, F at) {
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    double v[NC + 1];
#pragma unroll
    for (int k = 0; k <= NC; ++k) v[k] = k >= j ? at(j, k) : 0.0;
    pp_append<NC>(t, v);
  }
}

__device__ __forceinline__ int pp_floordiv(int a, int b) {  // b > 0; Python's //
  const int q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}

// the weighted row [y^d .. y 1 | x] * w
template <int NC>
__device__ __forceinline__ void pp_row(double x, double y, double w, double (&v)[NC + 1]) {
  double pw = w;
#pragma unroll
  for (int j = NC - 1; j >= 0; --j) {
    v[j] = pw;
    pw *= y;
  }
  v[NC] = x * w;
}

// np.linspace(min_y, max_y, K)[i] and np.poly1d(coef)(y): every operation rounded on its own
// (hipcc would contract i * step + start and x * y + c into fused multiply-adds otherwise).
__device__ __forceinline__ double pp_way_y(const fscnn_path_params& p, double step, int i) {
#pragma clang fp contract(off)
  const int K = p.num_waypoints;
  if (K > 1 && i == K - 1) return p.max_y;
  return (double)i * step + p.min_y;
}
template <int NC>
__device__ __forceinline__ double pp_horner(const double* coef, double y) {
#pragma clang fp contract(off)
  double x = 0.0;
#pragma unroll
  for (int j = 0; j < NC; ++j) x = x * y + coef[j];
  return x;
}
__device__ __forceinline__ double pp_dist(double dx, double dy) {
#pragma clang fp contract(off)
  return sqrt(dx * dx + dy * dy);
}
__device__ __forceinline__ double pp_clip(double v, double lo, double hi) {  // np.clip
  v = v < lo ? lo : v;
  return v > hi ? hi : v;
}

// (value, index) minimum, the lower index on equal values
__device__ __forceinline__ void pp_take_min(double& v, int& i, double ov, int oi) {
  if (ov < v || (ov == v && oi < i)) {
    v = ov;
    i = oi;
  }
}

template <int NC>
__global__ __launch_bounds__(PP_T) void path_plan_kernel(const int* __restrict__ rows, int Hb,
                                                         fscnn_path_params p, double* ema,
                                                         double* __restrict__ out) {
  __shared__ double s_tri[PP_WAVES][NC * (NC + 1)];
  __shared__ int s_cnt[PP_WAVES];
  __shared__ double s_coef[4];
  __shared__ int s_status;
  __shared__ double s_len[PP_WAVES], s_best[PP_WAVES], s_miny[PP_WAVES];
  __shared__ int s_besti[PP_WAVES], s_minyi[PP_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = blockIdx.x;
  const int K = p.num_waypoints;
  const int* R = rows + (size_t)n * Hb * 4;
  double* o = out + (size_t)n * (FSCNN_PATH_REC + 2 * K);

  // ---- 1. every thread folds its selected rows into its triangle -------------------------------
  PpTri<NC> t;
#pragma unroll
  for (int j = 0; j < NC; ++j)
#pragma unroll
    for (int k = 0; k <= NC; ++k) t.r[j][k] = 0.0;
  int cnt = 0;
  for (int y = tid; y < Hb; y += PP_T) {
    const int* r = R + 4 * y;
    int px = 0;
    bool sel;
    if (p.fast) {
      const int k = p.scan_from_bottom ? Hb - 1 - y : y;
      const int c = r[2];
      sel = k % p.skip_rows == 0 && c >= p.min_width && c > 0;
      if (sel) px = pp_floordiv(r[3], c);
    } else {
      const int a = r[0], b = r[1];
      sel = b > a && b - a >= p.min_width;
      px = (a + b) >> 1;
    }
    if (sel) {
      const double wx = p.min_x + (double)px / p.pixels_per_unit;
      const double wy = p.min_y + (double)y / p.pixels_per_unit;
      double v[NC + 1];
      pp_row<NC>(wx, wy, 1.0, v);
      pp_append<NC>(t, v);
      ++cnt;
    }
  }

  // ---- 2. combine: down the wave by shuffles, across the waves through LDS ---------------------
  // (a lane whose partner is past the wave gets its own triangle back; its result is not used)
  for (int off = 32; off >= 1; off >>= 1) {
    PpTri<NC> u;
#pragma unroll
    for (int j = 0; j < NC; ++j)
#pragma unroll
      for (int k = j; k <= NC; ++k) u.r[j][k] = __shfl_down(t.r[j][k], off);
    cnt += __shfl_down(cnt, off);
    pp_merge<NC>(t, [&](int j, int k) { return u.r[j][k]; });
  }
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < NC; ++j)
#pragma unroll
      for (int k = j; k <= NC; ++k) s_tri[wave][j * (NC + 1) + k] = t.r[j][k];
    s_cnt[wave] = cnt;
  }
  __syncthreads();

  // ---- 3. one thread: the other waves, the anchor, the rank test, back substitution ------------
  if (tid == 0) {
    for (int w = 1; w < PP_WAVES; ++w) {
      const double* s = s_tri[w];
      pp_merge<NC>(t, [&](int j, int k) { return s[j * (NC + 1) + k]; });
      cnt += s_cnt[w];
    }
    const int nfit = cnt + (p.force_bottom_center ? 1 : 0);
    int status = 0;
    double coef[4] = {NAN, NAN, NAN, NAN};
    if (cnt == 0) {
      status = FSCNN_PATH_NO_CENTERLINE;
    } else if (nfit < NC) {
      status = FSCNN_PATH_TOO_FEW;
    } else {
      if (p.force_bottom_center) {
        double v[NC + 1];
        pp_row<NC>(p.anchor_x, p.anchor_y, 1e6, v);
        pp_append<NC>(t, v);
      }
      double dmin = t.r[0][0], dmax = t.r[0][0];
#pragma unroll
      for (int j = 1; j < NC; ++j) {
        dmin = t.r[j][j] < dmin ? t.r[j][j] : dmin;
        dmax = t.r[j][j] > dmax ? t.r[j][j] : dmax;
      }
      if (!(dmin >= (double)nfit * 0x1p-52 * dmax) || !(dmin > 0.0)) {  // (a NaN fails too)
        status = FSCNN_PATH_RANK_DEFICIENT;
      } else {
#pragma unroll
        for (int j = NC - 1; j >= 0; --j) {
          double acc = t.r[j][NC];
#pragma unroll
          for (int k = j + 1; k < NC; ++k) acc -= t.r[j][k] * coef[k];
          coef[j] = acc / t.r[j][j];
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) s_coef[j] = coef[j];
    s_status = status;
    s_cnt[0] = cnt;
  }
  __syncthreads();

  // ---- 4. waypoints, one per thread; segment lengths and the two searches as reductions --------
  const bool ok = s_status == 0;
  double coef[NC];
#pragma unroll
  for (int j = 0; j < NC; ++j) coef[j] = s_coef[j];
  const double step = K > 1 ? (p.max_y - p.min_y) / (double)(K - 1) : 0.0;
  double seg = 0.0, best = INFINITY, miny = INFINITY;
  int besti = INT_MAX, minyi = INT_MAX;
  if (tid < K) {
    if (ok) {
      const double yi = pp_way_y(p, step, tid), xi = pp_horner<NC>(coef, yi);
      o[FSCNN_PATH_REC + 2 * tid] = xi;
      o[FSCNN_PATH_REC + 2 * tid + 1] = yi;
      if (tid > 0) {
        const double yp = pp_way_y(p, step, tid - 1), xp = pp_horner<NC>(coef, yp);
        seg = pp_dist(xi - xp, yi - yp);
      }
      if (yi < p.car_y) {
        const double d = fabs(pp_dist(xi - p.car_x, yi - p.car_y) - p.preview_distance);
        if (d < INFINITY) {  // (the reference's `diff < inf`: an infinite or NaN one never wins)
          best = d;
          besti = tid;
        }
      }
      if (yi == yi) {
        miny = yi;
        minyi = tid;
      }
    } else {
      o[FSCNN_PATH_REC + 2 * tid] = NAN;
      o[FSCNN_PATH_REC + 2 * tid + 1] = NAN;
    }
  }
  for (int off = 32; off >= 1; off >>= 1) {
    seg += __shfl_down(seg, off);
    pp_take_min(best, besti, __shfl_down(best, off), __shfl_down(besti, off));
    pp_take_min(miny, minyi, __shfl_down(miny, off), __shfl_down(minyi, off));
  }
  if (lane == 0) {
    s_len[wave] = seg;
    s_best[wave] = best;
    s_besti[wave] = besti;
    s_miny[wave] = miny;
    s_minyi[wave] = minyi;
  }
  __syncthreads();
  if (tid != 0) return;

  // ---- 5. one thread: the controller and the record ---------------------------------------------
  for (int w = 1; w < PP_WAVES; ++w) {
    seg += s_len[w];
    pp_take_min(best, besti, s_best[w], s_besti[w]);
    pp_take_min(miny, minyi, s_miny[w], s_minyi[w]);
  }
  int status = s_status;
  double cx = NAN, cy = NAN, raw = 0.0;
  if (ok) {
    int ci = besti;
    if (ci == INT_MAX) {
      status |= FSCNN_PATH_NONE_AHEAD;
      ci = minyi == INT_MAX ? 0 : minyi;
    }
    cy = pp_way_y(p, step, ci);
    cx = pp_horner<NC>(coef, cy);
    raw = cx - p.car_x;
  }
  double e = raw;
  if (ema) {
#pragma clang fp contract(off)
    double* st = ema + 2 * (size_t)n;
    if (st[1] != 0.0) e = p.ema_alpha * raw + (1.0 - p.ema_alpha) * st[0];
    st[0] = e;
    st[1] = 1.0;
  }
  double steering, dynamic, left, right;
  {
#pragma clang fp contract(off)
    steering = p.steering_gain * e;
    dynamic = pp_clip(p.base_pwm / (1.0 + p.curvature_damping * fabs(e)), p.min_pwm, p.max_pwm);
    left = pp_clip(dynamic + steering, -1000.0, 1000.0);
    right = pp_clip(dynamic - steering, -1000.0, 1000.0);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) o[FSCNN_PATH_COEF + j] = s_coef[j];
  o[FSCNN_PATH_NPOINTS] = (double)s_cnt[0];
  o[FSCNN_PATH_STATUS] = (double)status;
  o[FSCNN_PATH_LENGTH] = ok ? seg : 0.0;
  o[FSCNN_PATH_CONTROL_X] = cx;
  o[FSCNN_PATH_CONTROL_Y] = cy;
  o[FSCNN_PATH_RAW_ERROR] = raw;
  o[FSCNN_PATH_ERROR] = e;
  o[FSCNN_PATH_STEERING] = steering;
  o[FSCNN_PATH_DYNAMIC] = dynamic;
  o[FSCNN_PATH_PWM_LEFT] = left;
  o[FSCNN_PATH_PWM_RIGHT] = right;
  o[FSCNN_PATH_NWAY] = ok ? (double)K : 0.0;
}

bool path_plan_ok(int N, int Hb, int degree, int K) {
  return N >= 1 && N <= 65535 && Hb >= 1 && Hb <= 65535 && degree >= 1 && degree <= 3 && K >= 1 &&
         K <= PP_T;
}

int path_plan(const int* rows, int N, int Hb, const fscnn_path_params& p, double* ema_state,
              double* out, hipStream_t st) {
  if (!rows || !out) {
    set_error("path_plan: null rows or out");
    return E_INVALID;
  }
  if (!path_plan_ok(N, Hb, p.degree, p.num_waypoints)) {
    set_error("path_plan: unsupported (N=%d Hb=%d degree=%d waypoints=%d; N and Hb 1 .. 65535, "
              "degree 1 .. 3, waypoints 1 .. %d)", N, Hb, p.degree, p.num_waypoints, PP_T);
    return E_UNSUPPORTED;
  }
  const double vals[] = {p.min_x, p.min_y, p.max_y, p.pixels_per_unit, p.anchor_x, p.anchor_y,
                         p.car_x, p.car_y, p.steering_gain, p.base_pwm, p.curvature_damping,
                         p.preview_distance, p.max_pwm, p.min_pwm, p.ema_alpha};
  static const char* const names[] = {"min_x", "min_y", "max_y", "pixels_per_unit", "anchor_x",
                                      "anchor_y", "car_x", "car_y", "steering_gain", "base_pwm",
                                      "curvature_damping", "preview_distance", "max_pwm",
                                      "min_pwm", "ema_alpha"};
  for (size_t i = 0; i < sizeof(vals) / sizeof(vals[0]); ++i)
    if (!std::isfinite(vals[i])) {
      set_error("path_plan: %s is not finite", names[i]);
      return E_INVALID;
    }
  if (p.pixels_per_unit == 0.0 || p.skip_rows < 1 || p.min_width < 0) {
    set_error("path_plan: pixels_per_unit %g, skip_rows %d, min_width %d (non-zero, >= 1, >= 0)",
              p.pixels_per_unit, p.skip_rows, p.min_width);
    return E_INVALID;
  }
  const dim3 grid((unsigned)N);
  if (p.degree == 1)
    prof_launch(path_plan_kernel<2>, grid, PP_T, 0, st, rows, Hb, p, ema_state, out);
  else if (p.degree == 2)
    prof_launch(path_plan_kernel<3>, grid, PP_T, 0, st, rows, Hb, p, ema_state, out);
  else
    prof_launch(path_plan_kernel<4>, grid, PP_T, 0, st, rows, Hb, p, ema_state, out);
  return check_launch("path_plan");
}

}  // namespace fscnn
