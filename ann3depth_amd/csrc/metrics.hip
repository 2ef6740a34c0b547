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
//
// The walk, the target decode, the validity test and the sampler are metrics_common.h's, shared with align.hip.
// a3da_depth_metrics_aligned (include/a3d_align.h) is the same kernel body with a per-image affine map of the prediction.
#include <algorithm>
#include <cmath>

#include "../../include/a3d_align.h"
#include "metrics_common.h"

namespace a3d {

namespace {

using namespace pixels;

constexpr int kCols = A3D_METRIC_COLS;

struct MetricsArgs : PixelArgs {           // out: double [n][parts][kCols]
  float clamp_lo, clamp_hi;
  const float* coef;                      // [n, 2] (s, b) of a3da_depth_metrics_aligned; not read by the plain entry
};

// ALIGNED: the sampled prediction p becomes fl(fl(s p) + b) (include/a3d_align.h) before the finiteness test and the clamp.
template <int ALIGNED>
__device__ __forceinline__ void accumulate(const MetricsArgs& a, float p, float t, float cs, float cb, double (&s)[kCols]) {
  if (!target_valid(a, t)) return;
  if (ALIGNED) p = __fadd_rn(__fmul_rn(cs, p), cb);
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

template <int U8, int ALIGNED>
__global__ __launch_bounds__(kThreads) void metrics_part_kernel(const MetricsArgs a) {
  __shared__ float lut[256];
  __shared__ double red[kThreads / 64][kCols];
  if constexpr (U8 != 0) {
    fill_u8_lut(lut);
    __syncthreads();
  }
  const int part = blockIdx.x, b = blockIdx.y;
  float cs = 1.f, cb = 0.f;
  if constexpr (ALIGNED != 0) { cs = a.coef[2 * b]; cb = a.coef[2 * b + 1]; }
  double s[kCols];
#pragma unroll
  for (int c = 0; c < kCols; ++c) s[c] = 0.0;
  const int lo = part * a.chunk, hi = min(a.npix, lo + a.chunk);
  const float* p = a.pred + (size_t)b * a.ph * a.pw;
  const size_t base = (size_t)b * a.npix;
  const bool vec = vector_targets<U8>(a);
  for (int i0 = lo + 4 * threadIdx.x; i0 < hi; i0 += 4 * kThreads) {
    float t[4];
    load_targets4<U8>(a, lut, base, i0, hi, vec, t);
    int oy = i0 / a.tw, ox = i0 - oy * a.tw;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (i0 + u < hi) accumulate<ALIGNED>(a, sample_pred(a, p, oy, ox), t[u], cs, cb, s);
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
    static_cast<double*>(a.out)[((size_t)b * a.parts + part) * kCols + c] = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
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

// Both entry points: coef NULL is the plain a3d_depth_metrics.
int depth_metrics(const char* what, int n, int ph, int pw, const float* pred, int th, int tw, const void* target, int target_u8,
                  float min_depth, float max_depth, float clamp_lo, float clamp_hi, const float* coef, double* rows, void* ws,
                  size_t ws_bytes, void* stream) {
  A3D_CHECK_ARG(shape_ok(n, th, tw) && pred_shape_ok(ph, pw) && pred && target && rows, "%s: bad arguments", what);
  A3D_CHECK_ARG(!std::isnan(min_depth) && !std::isnan(max_depth) && !std::isnan(clamp_lo) && !std::isnan(clamp_hi) &&
                    clamp_lo <= clamp_hi,
                "%s: bad depth range or clamp", what);
  const size_t need = a3d_depth_metrics_ws_bytes(n, th, tw);
  if (!ws || ws_bytes < need)
    return set_error(A3D_EWORKSPACE, "%s: need %zu workspace bytes, got %zu", what, need, ws ? ws_bytes : (size_t)0);
  MetricsArgs a;
  fill_pixel_args(a, ph, pw, pred, th, tw, target, target_u8, min_depth, max_depth);
  a.out = ws; a.coef = coef;
  a.clamp_lo = clamp_lo; a.clamp_hi = clamp_hi;
  hipStream_t st = static_cast<hipStream_t>(stream);
  clear_stale_error();
  const dim3 grid(a.parts, n), block(kThreads);
  if (coef) {
    if (a.u8)
      hipLaunchKernelGGL((metrics_part_kernel<1, 1>), grid, block, 0, st, a);
    else
      hipLaunchKernelGGL((metrics_part_kernel<0, 1>), grid, block, 0, st, a);
  } else {
    if (a.u8)
      hipLaunchKernelGGL((metrics_part_kernel<1, 0>), grid, block, 0, st, a);
    else
      hipLaunchKernelGGL((metrics_part_kernel<0, 0>), grid, block, 0, st, a);
  }
  int rc = check_launch(what);
  if (rc != A3D_OK) return rc;
  hipLaunchKernelGGL(metrics_rows_kernel, dim3((n * kCols + kThreads - 1) / kThreads), dim3(kThreads), 0, st,
                     static_cast<const double*>(ws), rows, n, a.parts);
  return check_launch("depth_metrics_rows");
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
  return depth_metrics("depth_metrics", n, ph, pw, pred, th, tw, target, target_u8, min_depth, max_depth, clamp_lo, clamp_hi,
                       nullptr, rows, ws, ws_bytes, stream);
}

int a3da_depth_metrics_aligned(int n, int ph, int pw, const float* pred, int th, int tw, const void* target, int target_u8,
                               float min_depth, float max_depth, float clamp_lo, float clamp_hi, const float* coef,
                               double* rows, void* ws, size_t ws_bytes, void* stream) {
  A3D_CHECK_ARG(coef, "depth_metrics_aligned: NULL coef");
  return depth_metrics("depth_metrics_aligned", n, ph, pw, pred, th, tw, target, target_u8, min_depth, max_depth, clamp_lo,
                       clamp_hi, coef, rows, ws, ws_bytes, stream);
}

}  // extern "C"

}  // namespace a3d
