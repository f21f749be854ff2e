// GPU train / val augmentation: CitySegmentation._sync_transform / _val_sync_transform
// (data_loader/cityscapes.py:93-150, the same code in tusimple.py:168-208) for a whole batch in
// one launch, with PIL's own integer arithmetic, so the pixels are the ones the reference's
// DataLoader workers produce:
//   mirror -> img.resize(BILINEAR) / mask.resize(NEAREST) -> zero pad -> crop -> GaussianBlur
//   -> ToTensor + Normalize / _class_to_index.
// The host (sync_tables.cpp) restates what PIL precomputes per resize: for every crop column
// and row the first source index, the tap count and the 22-bit fixed-point weights, and the
// mask's nearest source index.  A workgroup owns a 16 x 64 tile of one sample's crop:
//   1. horizontal pass  : source rows [row0, row1) the tile's vertical taps read, at the tile's
//                         columns (+ 3 halo columns each side when the sample is blurred),
//                         rounded to bytes in LDS (Resample.c ImagingResampleHorizontal_8bpc);
//   2. vertical pass    : on those bytes, to the (16+6) x (64+6) pre-blur tile in LDS;
//   3. blur             : 3 row passes then 3 column passes of BoxBlur.c's radius-<1 line filter
//                         out = (v*ww + (left + right)*fw + 2^23) >> 24, neighbours clamped at
//                         the CROP's edges (PIL blurs the cropped image); each pass invalidates
//                         one more ring of the halo, 3 rings per direction are there;
//   4. store            : (v/255 - mean)/std in normalize_u8_kernel's operation order, 4 pixels
//                         per thread (vector stores where the address allows), the remapped
//                         labels and optionally the uint8 crop.
// Integer arithmetic only in 1-3; no atomics; deterministic.
#include "../../include/fastscnn.h"
#include "kernels.hpp"

#include <algorithm>
#include <climits>

namespace fscnn {

constexpr int ST_TH = 16, ST_TW = 64, ST_HALO = 3;
constexpr int ST_PH = ST_TH + 2 * ST_HALO, ST_PW = ST_TW + 2 * ST_HALO;
constexpr int ST_TILE_BYTES = ST_PH * ST_PW * 3;
constexpr int ST_PRECISION_BITS = 22;
constexpr int ST_MAX_LDS = 48 * 1024;  // dynamic part (source rows after the horizontal pass)

struct SyncArgs {
  const fscnn_sync_desc* desc;
  const int* tab;
  int crop;
  const long long* lut;
  int lut_size, lut_offset;
  float mean[3], sd[3];
  void* x;
  long long* target;
  uint8_t* u8;
  int max_rows;
};

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

template <typename TO>
__global__ __launch_bounds__(256) void sync_transform_kernel(SyncArgs a) {
  extern __shared__ uint8_t s_h[];  // [nrows][pw][3]
  __shared__ uint8_t s_a[ST_TILE_BYTES], s_b[ST_TILE_BYTES];
  __shared__ int s_y0[ST_PH], s_y1[ST_PH];

  const fscnn_sync_desc d = a.desc[blockIdx.z];
  const int tid = threadIdx.x, crop = a.crop;
  const int h = d.blur ? ST_HALO : 0;
  const int pw = ST_TW + 2 * h, ph = ST_TH + 2 * h;
  const int vx0 = (int)blockIdx.x * ST_TW - h, vy0 = (int)blockIdx.y * ST_TH - h;
  const int* xb = a.tab + d.off_xb;
  const int* xk = a.tab + d.off_xk;
  const int* yb = a.tab + d.off_yb;
  const int* yk = a.tab + d.off_yk;

  // source rows the tile's vertical taps read
  if (tid < ph) {
    const int vy = vy0 + tid;
    int lo = INT_MAX, hi = 0;
    if (vy >= 0 && vy < crop && yb[2 * vy + 1] > 0) {
      lo = yb[2 * vy];
      hi = lo + yb[2 * vy + 1];
    }
    s_y0[tid] = lo;
    s_y1[tid] = hi;
  }
  __syncthreads();
  int row0 = INT_MAX, row1 = 0;
  for (int j = 0; j < ph; ++j) {
    row0 = min(row0, s_y0[j]);
    row1 = max(row1, s_y1[j]);
  }
  int nrows = row1 > row0 ? row1 - row0 : 0;
  if (nrows == 0) row0 = 0;
  nrows = min(nrows, a.max_rows);  // (the host sized max_rows from the same tables)

  // 1. horizontal pass, source -> bytes
  for (int it = tid; it < nrows * pw; it += 256) {
    const int r = it / pw, i = it - r * pw;
    const int vx = vx0 + i;
    int acc[3] = {0, 0, 0};
    if (vx >= 0 && vx < crop) {
      const int xmin = xb[2 * vx], cnt = xb[2 * vx + 1];
      const int* k = xk + (size_t)vx * d.kx;
      const uint8_t* srow = d.image + (size_t)(row0 + r) * d.W * 3;
      for (int t = 0; t < cnt; ++t) {
        const int sx = d.flip ? d.W - 1 - (xmin + t) : xmin + t;
        const uint8_t* p = srow + (size_t)sx * 3;
        const int kv = k[t];
        acc[0] += (int)p[0] * kv;
        acc[1] += (int)p[1] * kv;
        acc[2] += (int)p[2] * kv;
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
      s_h[it * 3 + c] =
          (uint8_t)clip8((acc[c] + (1 << (ST_PRECISION_BITS - 1))) >> ST_PRECISION_BITS);
  }
  __syncthreads();

  // 2. vertical pass on the bytes -> pre-blur tile
  for (int it = tid; it < ph * pw; it += 256) {
    const int j = it / pw, i = it - j * pw;
    const int vx = vx0 + i, vy = vy0 + j;
    int acc[3] = {0, 0, 0};
    if (vx >= 0 && vx < crop && vy >= 0 && vy < crop) {
      const int ymin = yb[2 * vy], cnt = yb[2 * vy + 1];
      const int* k = yk + (size_t)vy * d.ky;
      for (int t = 0; t < cnt; ++t) {
        const int rr = ymin + t - row0;
        if (rr < 0 || rr >= nrows) continue;
        const uint8_t* p = s_h + (rr * pw + i) * 3;
        const int kv = k[t];
        acc[0] += (int)p[0] * kv;
        acc[1] += (int)p[1] * kv;
        acc[2] += (int)p[2] * kv;
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
      s_a[it * 3 + c] =
          (uint8_t)clip8((acc[c] + (1 << (ST_PRECISION_BITS - 1))) >> ST_PRECISION_BITS);
  }
  __syncthreads();

  // 3. blur: rows x3 (a -> b -> a -> b), columns x3 (b -> a -> b -> a)
  if (d.blur) {
    const uint32_t ww = d.ww, fw = d.fw;
    for (int pass = 0; pass < 6; ++pass) {
      const uint8_t* src = (pass & 1) ? s_b : s_a;
      uint8_t* dst = (pass & 1) ? s_a : s_b;
      for (int it = tid; it < ph * pw; it += 256) {
        const int j = it / pw, i = it - j * pw;
        const int vx = vx0 + i, vy = vy0 + j;
        int li = it, ri = it;  // neighbours: clamped at the crop's edge (and the buffer's)
        if (pass < 3) {
          if (vx > 0 && i > 0) li = it - 1;
          if (vx < crop - 1 && i < pw - 1) ri = it + 1;
        } else {
          if (vy > 0 && j > 0) li = it - pw;
          if (vy < crop - 1 && j < ph - 1) ri = it + pw;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const uint32_t v = src[it * 3 + c];
          const uint32_t far = (uint32_t)src[li * 3 + c] + (uint32_t)src[ri * 3 + c];
          dst[it * 3 + c] = (uint8_t)((v * ww + far * fw + (1u << 23)) >> 24);
        }
      }
      __syncthreads();
    }
  }

  // 4. store: thread = 4 consecutive pixels of one tile row
  const int row = tid >> 4, col0 = (tid & 15) * 4;
  const int y = (int)blockIdx.y * ST_TH + row, x = (int)blockIdx.x * ST_TW + col0;
  if (y >= crop || x >= crop) return;
  const int n = blockIdx.z;
  const int npx = min(4, crop - x);
  const size_t plane = (size_t)crop * crop;
  const size_t poff = (size_t)n * plane + (size_t)y * crop + x;  // pixel offset in [N][crop][crop]
  const uint8_t* px = s_a + ((row + h) * pw + col0 + h) * 3;

  TO* xo = (TO*)a.x;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = ((float)px[(e < npx ? e : 0) * 3 + c] / 255.f - a.mean[c]) / a.sd[c];
    const size_t xoff = ((size_t)n * 3 + c) * plane + (size_t)y * crop + x;
    TO* dst = xo + xoff;
    if (npx == 4 && (xoff & 3) == 0) {
      st4v(dst, v);
    } else {
      for (int e = 0; e < npx; ++e) st1(dst + e, v[e]);
    }
  }

  // labels: nearest gather -> lookup table (pad -> id 0, ids outside the table -> -1)
  const int* nxt = a.tab + d.off_nx;
  const int ny = a.tab[d.off_ny + y];
  long long lab[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    int id = 0;
    if (e < npx) {
      const int nx = nxt[x + e];
      if (nx >= 0 && ny >= 0) id = d.mask[(size_t)ny * d.W + (d.flip ? d.W - 1 - nx : nx)];
    }
    const int k = id + a.lut_offset;
    lab[e] = (k >= 0 && k < a.lut_size) ? a.lut[k] : -1;
  }
  long long* tdst = a.target + poff;
  if (npx == 4 && (poff & 1) == 0) {
    reinterpret_cast<longlong2*>(tdst)[0] = make_longlong2(lab[0], lab[1]);
    reinterpret_cast<longlong2*>(tdst)[1] = make_longlong2(lab[2], lab[3]);
  } else {
    for (int e = 0; e < npx; ++e) tdst[e] = lab[e];
  }

  if (a.u8) {
    uint8_t* udst = a.u8 + poff * 3;
    if (npx == 4 && (poff & 3) == 0) {
      uint32_t w[3];
#pragma unroll
      for (int q = 0; q < 3; ++q)
        w[q] = (uint32_t)px[4 * q] | ((uint32_t)px[4 * q + 1] << 8) |
               ((uint32_t)px[4 * q + 2] << 16) | ((uint32_t)px[4 * q + 3] << 24);
      uint32_t* u32 = reinterpret_cast<uint32_t*>(udst);
      u32[0] = w[0]; u32[1] = w[1]; u32[2] = w[2];
    } else {
      for (int e = 0; e < npx * 3; ++e) udst[e] = px[e];
    }
  }
}

// Range-check every table entry of the host copy (the kernel reads the same bytes) and size the
// LDS rows: max over samples and tile rows of the source-row span the tile's vertical taps read.
static int sync_validate(const uint8_t* hblob, long long blob_bytes, int N, int crop, int& max_rows) {
  const long long nint = blob_bytes / 4;
  if ((uintptr_t)hblob % 8 || blob_bytes < (long long)N * (long long)sizeof(fscnn_sync_desc)) {
    set_error("sync_transform: blob of %lld bytes for %d descriptors", blob_bytes, N);
    return E_INVALID;
  }
  const fscnn_sync_desc* desc = reinterpret_cast<const fscnn_sync_desc*>(hblob);
  const int* tab = reinterpret_cast<const int*>(hblob);
  max_rows = 1;
  for (int n = 0; n < N; ++n) {
    const fscnn_sync_desc& d = desc[n];
    auto in_blob = [&](int off, long long len) { return off >= 0 && off + len <= nint; };
    if (!d.image || !d.mask || d.H < 1 || d.W < 1 || d.kx < 1 || d.ky < 1 || d.ow < 1 ||
        d.oh < 1 || d.x1 < 0 || d.y1 < 0 ||
        (long long)d.H * d.W * 3 >= (1LL << 31) ||
        !in_blob(d.off_xb, 2LL * crop) || !in_blob(d.off_yb, 2LL * crop) ||
        !in_blob(d.off_xk, (long long)crop * d.kx) || !in_blob(d.off_yk, (long long)crop * d.ky) ||
        !in_blob(d.off_nx, crop) || !in_blob(d.off_ny, crop)) {
      set_error("sync_transform: sample %d: bad descriptor (H=%d W=%d kx=%d ky=%d)", n, d.H, d.W,
                d.kx, d.ky);
      return E_INVALID;
    }
    if (d.blur && ((unsigned long long)d.ww + 2ull * d.fw > (1ull << 24))) {
      set_error("sync_transform: sample %d: blur weights %u %u", n, d.ww, d.fw);
      return E_INVALID;
    }
    const int* xb = tab + d.off_xb;
    const int* yb = tab + d.off_yb;
    for (int j = 0; j < crop; ++j) {
      const int x0 = xb[2 * j], xc = xb[2 * j + 1], y0 = yb[2 * j], yc = yb[2 * j + 1];
      const int nx = tab[d.off_nx + j], ny = tab[d.off_ny + j];
      if (x0 < 0 || xc < 0 || xc > d.kx || (long long)x0 + xc > d.W || y0 < 0 || yc < 0 ||
          yc > d.ky || (long long)y0 + yc > d.H || nx < -1 || nx >= d.W || ny < -1 || ny >= d.H) {
        set_error("sync_transform: sample %d: table entry %d out of range", n, j);
        return E_INVALID;
      }
    }
    const int h = d.blur ? ST_HALO : 0;
    for (int t0 = 0; t0 < crop; t0 += ST_TH) {
      int lo = INT_MAX, hi = 0;
      for (int vy = std::max(t0 - h, 0); vy < std::min(t0 + ST_TH + h, crop); ++vy)
        if (yb[2 * vy + 1] > 0) {
          lo = std::min(lo, yb[2 * vy]);
          hi = std::max(hi, yb[2 * vy] + yb[2 * vy + 1]);
        }
      if (hi > lo) max_rows = std::max(max_rows, hi - lo);
    }
  }
  return OK;
}

int sync_transform(const void* hblob, const void* dblob, long long blob_bytes, int N, int crop,
                   const long long* lut, int lut_size, int lut_offset, const float* mean,
                   const float* sd, void* x, int out_dtype, long long* target, uint8_t* crop_u8,
                   hipStream_t st) {
  if (N < 1 || N > 65535 || crop < 1 || crop > 32768 || lut_size < 1 ||
      (long long)N * crop * crop * 3 >= (1LL << 40) || (uintptr_t)x % 16 || (uintptr_t)target % 16 ||
      (uintptr_t)crop_u8 % 4 || (uintptr_t)dblob % 8) {
    set_error("sync_transform: N=%d crop=%d lut_size=%d (x / target 16-B, crop_u8 4-B aligned)", N,
              crop, lut_size);
    return E_INVALID;
  }
  int max_rows = 1;
  if (int rc = sync_validate((const uint8_t*)hblob, blob_bytes, N, crop, max_rows)) return rc;
  const size_t lds = ((size_t)max_rows * ST_PW * 3 + 15) & ~(size_t)15;
  if (lds > ST_MAX_LDS) {
    set_error("sync_transform: a tile reads %d source rows (%zu B of LDS > %d)", max_rows, lds,
              ST_MAX_LDS);
    return E_INVALID;
  }
  SyncArgs a;
  a.desc = reinterpret_cast<const fscnn_sync_desc*>(dblob);
  a.tab = reinterpret_cast<const int*>(dblob);
  a.crop = crop;
  a.lut = lut;
  a.lut_size = lut_size;
  a.lut_offset = lut_offset;
  for (int c = 0; c < 3; ++c) {
    a.mean[c] = mean[c];
    a.sd[c] = sd[c];
  }
  a.x = x;
  a.target = target;
  a.u8 = crop_u8;
  a.max_rows = max_rows;
  const dim3 grid((unsigned)cdiv(crop, ST_TW), (unsigned)cdiv(crop, ST_TH), (unsigned)N);
  if (out_dtype == DT_F32) prof_launch(sync_transform_kernel<float>, grid, 256, lds, st, a);
  else prof_launch(sync_transform_kernel<bf16>, grid, 256, lds, st, a);
  return check_launch("sync_transform");
}

}  // namespace fscnn
