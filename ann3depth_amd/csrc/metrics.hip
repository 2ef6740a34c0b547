// metrics.hip — held-out depth error metrics of Eigen et al. 2014 (section 4, Table 1) on the test split: per image, the
// sums every metric of the table is built from (include/a3d.h, A3D_METRIC_*), accumulated in fp64.
//
// Compiled with -ffp-contract=off (see Makefile): the prediction sampled at a target pixel must be bit-identical to what
// a3d_resize_bilinear_tf1 writes for that pixel (resample.hip, resize_rows), and the per-pixel terms are the separate
// correctly-rounded fp32 operations the test's numpy reference performs.
//
// Two launches.  metrics_part_kernel: grid (parts, n); workgroup (part, b) walks a contiguous range of image b's target
// pixels, four per thread and round (16-byte / 4-byte vector loads where the image's base allows), and leaves its 11 sums
// in ws[(b * parts + part) * 11 + col].  metrics_rows_kernel: one thread per (image, column) adds the parts in part order
// into rows[b * 11 + col].  The launch boundary makes the partials visible; every sum is taken in a fixed order, so the
// result is the same bits on every run.
#include <algorithm>
#include <cmath>

#include "a3d_internal.h"

namespace a3d {

namespace {

constexpr int kCols = A3D_METRIC_COLS;
constexpr int kThreads = 256;
constexpr int kPixelsPerPart = 4096;      // 480 x 640 targets: 75 workgroups per image; 55 x 74: one
constexpr int kMaxParts = 1024;

struct MetricsArgs {
  const float* pred;
  const void* target;
  double* ws;
  int ph, pw, th, tw, npix, chunk, parts, u8;
  float sy, sx;                           // legacy ResizeBilinear scales in / out (resize_one in resample.hip)
  float min_depth, max_depth, clamp_lo, clamp_hi;
};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// The prediction at target pixel (oy, ox): the legacy align_corners=False mapping with resize_rows' operations, or the
// pixel itself when the grids agree.
__device__ __forceinline__ float sample_pred(const MetricsArgs& a, const float* p, int oy, int ox) {
  if (a.ph == a.th && a.pw == a.tw) return p[oy * a.pw + ox];
  const float fy = __fmul_rn((float)oy, a.sy);
  const int y0 = (int)fy, y1 = min(y0 + 1, a.ph - 1);
  const float ly = __fsub_rn(fy, (float)y0);
  const float fx = __fmul_rn((float)ox, a.sx);
  const int x0 = (int)fx, x1 = min(x0 + 1, a.pw - 1);
  const float lx = __fsub_rn(fx, (float)x0);
  const float tl = p[y0 * a.pw + x0], tr = p[y0 * a.pw + x1];
  const float bl = p[y1 * a.pw + x0], br = p[y1 * a.pw + x1];
  const float top = __fadd_rn(tl, __fmul_rn(__fsub_rn(tr, tl), lx));
  const float bot = __fadd_rn(bl, __fmul_rn(__fsub_rn(br, bl), lx));
  return __fadd_rn(top, __fmul_rn(__fsub_rn(bot, top), ly));
}

__device__ __forceinline__ void accumulate(const MetricsArgs& a, float p, float t, double (&s)[kCols]) {
  if (!(isfinite(t) && t > a.min_depth && t <= a.max_depth)) return;
  if (!isfinite(p)) {
    s[A3D_METRIC_NONFINITE] += 1.0;
    return;
  }
  const float q = fminf(fmaxf(p, a.clamp_lo), a.clamp_hi);
  const float diff = __fsub_rn(q, t);
  const float sq = __fmul_rn(diff, diff);
  const float d = __fsub_rn(logf(q), logf(t));
  const float l10 = fabsf(__fsub_rn(log10f(q), log10f(t)));
  const float ratio = fmaxf(__fdiv_rn(q, t), __fdiv_rn(t, q));
  s[A3D_METRIC_N] += 1.0;
  s[A3D_METRIC_ABS_REL] += (double)__fdiv_rn(fabsf(diff), t);
  s[A3D_METRIC_SQ_REL] += (double)__fdiv_rn(sq, t);
  s[A3D_METRIC_SQ] += (double)sq;
  s[A3D_METRIC_LOG] += (double)d;
  s[A3D_METRIC_LOG_SQ] += (double)__fmul_rn(d, d);
  s[A3D_METRIC_LOG10] += (double)l10;
  s[A3D_METRIC_DELTA1] += ratio < 1.25f ? 1.0 : 0.0;
  s[A3D_METRIC_DELTA2] += ratio < 1.5625f ? 1.0 : 0.0;
  s[A3D_METRIC_DELTA3] += ratio < 1.953125f ? 1.0 : 0.0;
}

template <int U8>
__global__ __launch_bounds__(kThreads) void metrics_part_kernel(const MetricsArgs a) {
  __shared__ float lut[256];
  __shared__ double red[kThreads / 64][kCols];
  if constexpr (U8 != 0) {
    // the float the converter stored plus the loader's 0.5, as resize_kernel's table (fill_u8_lut, resample.hip)
    lut[threadIdx.x] = __fadd_rn(__fsub_rn(__fdiv_rn((float)threadIdx.x, 255.f), 0.5f), 0.5f);
    __syncthreads();
  }
  const int part = blockIdx.x, b = blockIdx.y;
  const int lo = part * a.chunk, hi = min(a.npix, lo + a.chunk);
  const float* p = a.pred + (size_t)b * a.ph * a.pw;
  const size_t base = (size_t)b * a.npix;
  // whole aligned groups of four when every image starts on a 16-byte (float) / 4-byte (uint8) boundary (chunk is a
  // multiple of 4); a uniform choice per launch
  const bool vec = (a.npix & 3) == 0 &&
                   ((reinterpret_cast<uintptr_t>(a.target) & (U8 ? 3u : 15u)) == 0);
  double s[kCols];
#pragma unroll
  for (int c = 0; c < kCols; ++c) s[c] = 0.0;
  for (int i0 = lo + 4 * threadIdx.x; i0 < hi; i0 += 4 * kThreads) {
    float t[4];
    if (U8) {
      const uint8_t* tg = static_cast<const uint8_t*>(a.target) + base + i0;
      if (vec) {
        const uchar4 k = *reinterpret_cast<const uchar4*>(tg);
        t[0] = lut[k.x]; t[1] = lut[k.y]; t[2] = lut[k.z]; t[3] = lut[k.w];
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) t[u] = i0 + u < hi ? lut[tg[u]] : 0.f;
      }
    } else {
      const float* tg = static_cast<const float*>(a.target) + base + i0;
      if (vec) {
        const float4 v = *reinterpret_cast<const float4*>(tg);
        t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w;
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) t[u] = i0 + u < hi ? tg[u] : 0.f;
      }
    }
    int oy = i0 / a.tw, ox = i0 - oy * a.tw;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (i0 + u < hi) accumulate(a, sample_pred(a, p, oy, ox), t[u], s);
      if (++ox == a.tw) { ox = 0; ++oy; }
    }
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int c = 0; c < kCols; ++c) {
    const double v = wave_sum_f64(s[c]);
    if (lane == 0) red[wave][c] = v;
  }
  __syncthreads();
  if (threadIdx.x < kCols) {
    const int c = threadIdx.x;
    a.ws[((size_t)b * a.parts + part) * kCols + c] = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
  }
}

__global__ __launch_bounds__(kThreads) void metrics_rows_kernel(const double* __restrict__ ws, double* __restrict__ rows,
                                                                int n, int parts) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n * kCols) return;
  const int b = i / kCols, c = i - b * kCols;
  const double* src = ws + (size_t)b * parts * kCols + c;
  double acc = 0.0;
  for (int q = 0; q < parts; ++q) acc += src[(size_t)q * kCols];
  rows[i] = acc;
}

int parts_for(int npix) { return std::min(kMaxParts, std::max(1, (npix + kPixelsPerPart - 1) / kPixelsPerPart)); }

bool shape_ok(int n, int th, int tw) {
  return n > 0 && n <= 65535 && th > 0 && tw > 0 && (int64_t)th * tw <= (int64_t)INT32_MAX - 4 * kThreads;   // (grid y)
}

}  // namespace

extern "C" {

size_t a3d_depth_metrics_ws_bytes(int n, int th, int tw) {
  if (!shape_ok(n, th, tw)) return 0;
  return (size_t)n * parts_for(th * tw) * kCols * sizeof(double);
}

int a3d_depth_metrics(int n, int ph, int pw, const float* pred, int th, int tw, const void* target, int target_u8,
                      float min_depth, float max_depth, float clamp_lo, float clamp_hi, double* rows, void* ws,
                      size_t ws_bytes, void* stream) {
  A3D_CHECK_ARG(shape_ok(n, th, tw) && ph > 0 && pw > 0 && (int64_t)ph * pw <= INT32_MAX && pred && target && rows,
                "depth_metrics: bad arguments");
  A3D_CHECK_ARG(!std::isnan(min_depth) && !std::isnan(max_depth) && !std::isnan(clamp_lo) && !std::isnan(clamp_hi) &&
                    clamp_lo <= clamp_hi,
                "depth_metrics: bad depth range or clamp");
  const size_t need = a3d_depth_metrics_ws_bytes(n, th, tw);
  if (!ws || ws_bytes < need)
    return set_error(A3D_EWORKSPACE, "depth_metrics: need %zu workspace bytes, got %zu", need, ws ? ws_bytes : (size_t)0);
  MetricsArgs a;
  a.pred = pred; a.target = target; a.ws = static_cast<double*>(ws);
  a.ph = ph; a.pw = pw; a.th = th; a.tw = tw; a.npix = th * tw;
  a.parts = parts_for(a.npix);
  a.chunk = ((a.npix + a.parts - 1) / a.parts + 3) & ~3;
  a.u8 = target_u8 ? 1 : 0;
  a.sy = (float)ph / (float)th; a.sx = (float)pw / (float)tw;
  a.min_depth = min_depth; a.max_depth = max_depth; a.clamp_lo = clamp_lo; a.clamp_hi = clamp_hi;
  hipStream_t st = static_cast<hipStream_t>(stream);
  clear_stale_error();
  if (a.u8)
    hipLaunchKernelGGL(metrics_part_kernel<1>, dim3(a.parts, n), dim3(kThreads), 0, st, a);
  else
    hipLaunchKernelGGL(metrics_part_kernel<0>, dim3(a.parts, n), dim3(kThreads), 0, st, a);
  int rc = check_launch("depth_metrics");
  if (rc != A3D_OK) return rc;
  hipLaunchKernelGGL(metrics_rows_kernel, dim3((n * kCols + kThreads - 1) / kThreads), dim3(kThreads), 0, st,
                     static_cast<const double*>(ws), rows, n, a.parts);
  return check_launch("depth_metrics_rows");
}

}  // extern "C"

}  // namespace a3d
