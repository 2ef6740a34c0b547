// align.hip — per-image scale-and-shift alignment of a prediction to a target (include/a3d_align.h): the coefficients of
// median scaling, least-squares scale and least-squares scale and shift over the pixels a3d_depth_metrics sums over, and
// the affine map applied to a tensor.  a3da_depth_metrics_aligned is metrics.hip's: one kernel body with the plain entry.
//
// Compiled with -ffp-contract=off (see Makefile): the sampled prediction is metrics.hip's bit for bit (metrics_common.h),
// and fl(fl(s x) + b) is two roundings.
//
// Least squares, two launches.  sums_part_kernel: grid (parts, n), the walk of metrics_part_kernel; workgroup (part, b)
// leaves S_p, S_t, S_pp, S_pt and m in ws[(b * parts + part) * 5 + col], each a float64 sum in a fixed order.
// sums_solve_kernel: one thread per image adds the parts in part order and solves.
//
// Median, seven launches (the first clears the workspace): an exact radix selection on the 32-bit ordered key, digits of 11 / 11 / 10 bits from
// the top.  Per pass, hist_part_kernel (grid (parts, n), the same walk, p sampled again) counts in LDS the keys whose higher
// digits are the ones chosen so far, by this pass's digit, 2048 bins for t and 2048 for p, and adds its non-empty bins to
// the image's histogram of this pass in the workspace; select_kernel, one workgroup of two wavefronts per image, wavefront
// q for quantity q (0: t, 1: p), prefix-scans the bins (32 per lane, then across the lanes), finds the bin holding the
// rank, and leaves the digits so far and the rank inside that bin for the next pass.  The third select has the whole key of
// both medians and writes coef, count and status.  Only integer atomics, whose sums do not depend on their order.
#include <cmath>

#include "../../include/a3d_align.h"
#include "metrics_common.h"

namespace a3d {

namespace {

using namespace pixels;

constexpr int kSums = 5;                  // S_p, S_t, S_pp, S_pt, m
constexpr int kBins = 2048;
constexpr int kPasses = 3;
constexpr int kStateInts = 4;             // per (image, quantity): digits chosen so far, rank inside them, m, unused

using SumsArgs = PixelArgs;               // out: double [n][parts][kSums]

struct HistArgs : PixelArgs {             // out: this pass's histograms, int [n][2][kBins]
  const unsigned* state;                  // [n][2][kStateInts]
  int match_shift, digit_shift, digit_mask;   // a key counts iff pass 0 or key >> match_shift == the digits chosen so far
};

// The walk of metrics_part_kernel: workgroup (blockIdx.x = part, blockIdx.y = image) of kThreads threads takes its contiguous
// range of the image's target pixels, four per thread and round, and calls f(sampled prediction, target) on the pixels of
// the fitted set, in ascending order.
template <int U8, typename F>
__device__ __forceinline__ void for_each_fitted_pixel(const PixelArgs& a, const float* lut, F&& f) {
  const int part = blockIdx.x, b = blockIdx.y;
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
      if (i0 + u < hi && target_valid(a, t[u])) {
        const float v = sample_pred(a, p, oy, ox);
        if (isfinite(v)) f(v, t[u]);
      }
      if (++ox == a.tw) { ox = 0; ++oy; }
    }
  }
}

// Ascending keys are ascending floats, -0 before +0.
__device__ __forceinline__ unsigned order_key(float x) {
  const unsigned u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u ^ 0x80000000u);
}

__device__ __forceinline__ float key_value(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

template <int U8>
__global__ __launch_bounds__(kThreads) void sums_part_kernel(const SumsArgs a) {
  __shared__ float lut[256];
  __shared__ double red[kThreads / 64][kSums];
  if constexpr (U8 != 0) {
    fill_u8_lut(lut);
    __syncthreads();
  }
  const int part = blockIdx.x, b = blockIdx.y;
  double s[kSums];
#pragma unroll
  for (int c = 0; c < kSums; ++c) s[c] = 0.0;
  for_each_fitted_pixel<U8>(a, lut, [&](float p, float t) {
    const double dp = (double)p, dt = (double)t;
    s[0] += dp;
    s[1] += dt;
    s[2] += dp * dp;                      // exact: 48 significant bits
    s[3] += dp * dt;
    s[4] += 1.0;
  });
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int c = 0; c < kSums; ++c) {
    const double v = wave_sum_f64(s[c]);
    if (lane == 0) red[wave][c] = v;
  }
  __syncthreads();
  if (threadIdx.x < kSums) {
    const int c = threadIdx.x;
    static_cast<double*>(a.out)[((size_t)b * a.parts + part) * kSums + c] = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
  }
}

__device__ __forceinline__ void write_result(float* coef, int* count, int* status, int b, bool ok, float s, float sh, int m) {
  coef[2 * b] = ok ? s : 1.f;
  coef[2 * b + 1] = ok ? sh : 0.f;
  count[b] = m;
  status[b] = ok ? 0 : 1;
}

__global__ __launch_bounds__(kThreads) void sums_solve_kernel(const double* __restrict__ ws, int n, int parts, int affine,
                                                              float* __restrict__ coef, int* __restrict__ count,
                                                              int* __restrict__ status) {
  const int b = blockIdx.x * kThreads + threadIdx.x;
  if (b >= n) return;
  const double* src = ws + (size_t)b * parts * kSums;
  double S[kSums];
#pragma unroll
  for (int c = 0; c < kSums; ++c) S[c] = 0.0;
  for (int q = 0; q < parts; ++q) {
#pragma unroll
    for (int c = 0; c < kSums; ++c) S[c] += src[(size_t)q * kSums + c];
  }
  const double sp = S[0], st = S[1], spp = S[2], spt = S[3], m = S[4];
  float s, sh = 0.f;
  bool ok;
  if (affine) {
    const double den = spp - sp * sp / m;
    const double sd = (spt - sp * st / m) / den;
    s = (float)sd;
    sh = (float)((st - sd * sp) / m);
    ok = m >= 2.0 && den > 0.0 && isfinite(s) && isfinite(sh);
  } else {
    s = (float)(spt / spp);
    ok = m >= 1.0 && spp > 0.0 && isfinite(s) && s > 0.f;
  }
  write_result(coef, count, status, b, ok, s, sh, (int)m);
}

// The three passes' histograms and the selection's state start from zero: a launch of the library's own on the caller's
// stream, like every other step.
__global__ __launch_bounds__(kThreads) void clear_kernel(int* __restrict__ p, size_t words) {
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < words; i += (size_t)gridDim.x * kThreads) p[i] = 0;
}

template <int U8, int FIRST>
__global__ __launch_bounds__(kThreads) void hist_part_kernel(const HistArgs a) {
  __shared__ float lut[256];
  __shared__ int bins[2][kBins];
  if constexpr (U8 != 0) fill_u8_lut(lut);
  for (int i = threadIdx.x; i < 2 * kBins; i += kThreads) (&bins[0][0])[i] = 0;
  __syncthreads();
  const int b = blockIdx.y;
  unsigned want_t = 0, want_p = 0;
  if constexpr (FIRST == 0) {
    want_t = a.state[(size_t)(2 * b) * kStateInts];
    want_p = a.state[(size_t)(2 * b + 1) * kStateInts];
  }
  for_each_fitted_pixel<U8>(a, lut, [&](float p, float t) {
    const unsigned kt = order_key(t), kp = order_key(p);
    if (FIRST || (kt >> a.match_shift) == want_t) atomicAdd(&bins[0][(kt >> a.digit_shift) & a.digit_mask], 1);
    if (FIRST || (kp >> a.match_shift) == want_p) atomicAdd(&bins[1][(kp >> a.digit_shift) & a.digit_mask], 1);
  });
  __syncthreads();
  int* dst = static_cast<int*>(a.out) + (size_t)b * 2 * kBins;
  for (int i = threadIdx.x; i < 2 * kBins; i += kThreads) {
    const int c = (&bins[0][0])[i];
    if (c != 0) atomicAdd(dst + i, c);
  }
}

// blockDim 128: wavefront q of workgroup b selects in hist[b][q].  pass 0 starts from rank (m - 1) / 2 with m the
// histogram's total; the last pass (digit_bits = 10) completes both keys and writes the image's result.
__global__ __launch_bounds__(128) void select_kernel(const int* __restrict__ hist, unsigned* __restrict__ state, int pass,
                                                     int digit_bits, float* __restrict__ coef, int* __restrict__ count,
                                                     int* __restrict__ status) {
  __shared__ unsigned key[2];
  __shared__ int total_m[2];
  const int b = blockIdx.x, q = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int* h = hist + ((size_t)b * 2 + q) * kBins + lane * (kBins / 64);
  unsigned* st = state + ((size_t)b * 2 + q) * kStateInts;
  int c[kBins / 64];
  int sum = 0;
#pragma unroll
  for (int j = 0; j < kBins / 64; j += 4) {
    const int4 v = *reinterpret_cast<const int4*>(h + j);
    c[j] = v.x; c[j + 1] = v.y; c[j + 2] = v.z; c[j + 3] = v.w;
    sum += (v.x + v.y) + (v.z + v.w);
  }
  int incl = sum;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int up = __shfl_up(incl, off, 64);
    if (lane >= off) incl += up;
  }
  const int total = __shfl(incl, 63, 64);
  unsigned digits = 0;
  int rank, m;
  if (pass == 0) {
    m = total;
    rank = m > 0 ? (m - 1) / 2 : 0;
  } else {
    digits = st[0];
    rank = (int)st[1];
    m = (int)st[2];
  }
  const int excl = incl - sum;
  const bool mine = rank >= excl && rank < incl;      // at most one lane: the bins are disjoint ranges of ranks
  int running = excl, bin = 0, before = 0;
  bool found = false;
#pragma unroll
  for (int j = 0; j < kBins / 64; ++j) {
    if (!found && rank < running + c[j]) {
      bin = lane * (kBins / 64) + j;
      before = running;
      found = true;
    }
    running += c[j];
  }
  const unsigned chosen = (digits << digit_bits) | (unsigned)bin;
  if (mine) {
    st[0] = chosen;
    st[1] = (unsigned)(rank - before);
    st[2] = (unsigned)m;
    key[q] = chosen;
  }
  if (total == 0 && lane == 0) {                      // nothing to select from: a state the next pass can read
    st[0] = 0; st[1] = 0; st[2] = (unsigned)m;
    key[q] = 0;
  }
  if (lane == 0) total_m[q] = m;
  if (pass != kPasses - 1) return;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int mm = total_m[0];
    const float mt = key_value(key[0]), mp = key_value(key[1]);
    const float s = __fdiv_rn(mt, mp);
    const bool ok = mm >= 1 && mp > 0.f && isfinite(s) && s > 0.f;
    write_result(coef, count, status, b, ok, s, 0.f, mm);
  }
}

__global__ __launch_bounds__(kThreads) void affine_apply_kernel(size_t per_image, const float* x, const float* __restrict__ coef,
                                                                float* y, int vec) {
  const int b = blockIdx.y;
  const float s = coef[2 * b], sh = coef[2 * b + 1];
  const float* xi = x + (size_t)b * per_image;
  float* yi = y + (size_t)b * per_image;
  const size_t stride = (size_t)gridDim.x * kThreads;
  if (vec) {
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < per_image / 4; i += stride) {
      float4 v = reinterpret_cast<const float4*>(xi)[i];
      v.x = __fadd_rn(__fmul_rn(s, v.x), sh); v.y = __fadd_rn(__fmul_rn(s, v.y), sh);
      v.z = __fadd_rn(__fmul_rn(s, v.z), sh); v.w = __fadd_rn(__fmul_rn(s, v.w), sh);
      reinterpret_cast<float4*>(yi)[i] = v;
    }
  } else {
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < per_image; i += stride)
      yi[i] = __fadd_rn(__fmul_rn(s, xi[i]), sh);
  }
}

bool mode_ok(int mode) { return mode == A3DA_MEDIAN || mode == A3DA_SCALE || mode == A3DA_AFFINE; }

size_t hist_ints(int n) { return (size_t)kPasses * n * 2 * kBins; }

}  // namespace

extern "C" {

size_t a3da_depth_align_ws_bytes(int n, int th, int tw, int mode) {
  if (!shape_ok(n, th, tw) || !mode_ok(mode)) return 0;
  if (mode == A3DA_MEDIAN) return (hist_ints(n) + (size_t)n * 2 * kStateInts) * sizeof(int);
  return (size_t)n * parts_for(th * tw) * kSums * sizeof(double);
}

int a3da_depth_align(int n, int ph, int pw, const float* pred, int th, int tw, const void* target, int target_u8,
                     float min_depth, float max_depth, int mode, float* coef, int* count, int* status, void* ws,
                     size_t ws_bytes, void* stream) {
  A3D_CHECK_ARG(pred && target && coef && count && status, "depth_align: NULL pointer");
  A3D_CHECK_ARG(shape_ok(n, th, tw) && pred_shape_ok(ph, pw), "depth_align: bad shape (n %d, prediction %d x %d, target %d x %d)",
                n, ph, pw, th, tw);
  A3D_CHECK_ARG(!std::isnan(min_depth) && !std::isnan(max_depth), "depth_align: min_depth or max_depth is NaN");
  A3D_CHECK_ARG(mode_ok(mode), "depth_align: unknown mode %d (A3DA_MEDIAN, A3DA_SCALE, A3DA_AFFINE)", mode);
  const size_t need = a3da_depth_align_ws_bytes(n, th, tw, mode);
  if (!ws || ws_bytes < need)
    return set_error(A3D_EWORKSPACE, "depth_align: need %zu workspace bytes, got %zu", need, ws ? ws_bytes : (size_t)0);
  hipStream_t st = static_cast<hipStream_t>(stream);
  clear_stale_error();
  if (mode != A3DA_MEDIAN) {
    SumsArgs a;
    fill_pixel_args(a, ph, pw, pred, th, tw, target, target_u8, min_depth, max_depth);
    a.out = ws;
    if (a.u8)
      hipLaunchKernelGGL(sums_part_kernel<1>, dim3(a.parts, n), dim3(kThreads), 0, st, a);
    else
      hipLaunchKernelGGL(sums_part_kernel<0>, dim3(a.parts, n), dim3(kThreads), 0, st, a);
    int rc = check_launch("depth_align_sums");
    if (rc != A3D_OK) return rc;
    hipLaunchKernelGGL(sums_solve_kernel, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, st,
                       static_cast<const double*>(ws), n, a.parts, mode == A3DA_AFFINE ? 1 : 0, coef, count, status);
    return check_launch("depth_align_solve");
  }
  HistArgs a;
  fill_pixel_args(a, ph, pw, pred, th, tw, target, target_u8, min_depth, max_depth);
  int* hist = static_cast<int*>(ws);
  unsigned* state = reinterpret_cast<unsigned*>(hist + hist_ints(n));
  a.state = state;
  const size_t words = need / sizeof(int);
  hipLaunchKernelGGL(clear_kernel, dim3(grid_for(words, kThreads, 1024)), dim3(kThreads), 0, st, hist, words);
  int rc0 = check_launch("depth_align_clear");
  if (rc0 != A3D_OK) return rc0;
  static const int kDigitShift[kPasses] = {21, 10, 0}, kDigitBits[kPasses] = {11, 11, 10};
  for (int pass = 0; pass < kPasses; ++pass) {
    a.out = hist + (size_t)pass * n * 2 * kBins;
    a.digit_shift = kDigitShift[pass];
    a.digit_mask = (1 << kDigitBits[pass]) - 1;
    a.match_shift = pass == 0 ? 0 : kDigitShift[pass - 1];
    const dim3 grid(a.parts, n), block(kThreads);
    if (pass == 0) {
      if (a.u8)
        hipLaunchKernelGGL((hist_part_kernel<1, 1>), grid, block, 0, st, a);
      else
        hipLaunchKernelGGL((hist_part_kernel<0, 1>), grid, block, 0, st, a);
    } else {
      if (a.u8)
        hipLaunchKernelGGL((hist_part_kernel<1, 0>), grid, block, 0, st, a);
      else
        hipLaunchKernelGGL((hist_part_kernel<0, 0>), grid, block, 0, st, a);
    }
    int rc = check_launch("depth_align_hist");
    if (rc != A3D_OK) return rc;
    hipLaunchKernelGGL(select_kernel, dim3(n), dim3(128), 0, st, static_cast<const int*>(a.out), state, pass, kDigitBits[pass],
                       coef, count, status);
    rc = check_launch("depth_align_select");
    if (rc != A3D_OK) return rc;
  }
  return A3D_OK;
}

int a3da_affine_apply(int n, int per_image, const float* x, const float* coef, float* y, void* stream) {
  A3D_CHECK_ARG(x && coef && y, "affine_apply: NULL pointer");
  A3D_CHECK_ARG(n > 0 && n <= 65535 && per_image > 0, "affine_apply: bad shape (n %d, %d values per image)", n, per_image);
  const int vec = (per_image & 3) == 0 && aligned16(x) && aligned16(y);
  const size_t work = vec ? (size_t)per_image / 4 : (size_t)per_image;
  clear_stale_error();
  hipLaunchKernelGGL(affine_apply_kernel, dim3(grid_for(work, kThreads, 1024), n), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), (size_t)per_image, x, coef, y, vec);
  return check_launch("affine_apply");
}

}  // extern "C"

}  // namespace a3d
