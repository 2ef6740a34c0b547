// slic.hip — DCNF on SLIC superpixels (include/a3d_slic.h; NON-REFERENCE, --segmentation slic): the segmentation itself
// (grid labels, centre update, assignment among the 3 x 3 clusters around a pixel's home cell) and the label-driven forms
// of what reads a superpixel's pixels: mean, colour histogram, pair similarities, pooling of a feature map and its
// transpose.
//
// A superpixel's pixels lie in its clipped 3sp x 3sp window, so the reductions are one block per (image, superpixel) that
// scans the window; a label is compared, never indexed with, except in the pooling's backward, which checks it against the
// pixel's candidates first.  All of it is bound by HBM or by launch latency and tiny next to the unary conv stack: the
// kernels are written for clarity.  Floats are summed in the one order the header states (tree_sum_256), integers by LDS
// atomics; there is no float atomic, so every run gives the same bits.  Built with -ffp-contract=off; the operations are
// spelled with the __f*_rn intrinsics all the same.
#include <cmath>

#include "a3d_internal.h"
#include "../../include/a3d_slic.h"
#include "crf_common.h"
#include "pool_lanes.h"

namespace a3d {
namespace {

constexpr int kMaxSp = A3DS_MAX_SP;
constexpr int kMaxCells = A3DS_MAX_CELLS;
constexpr int kMaxSuperpixels = A3DS_MAX_SUPERPIXELS;

__device__ inline float add(float a, float b) { return __fadd_rn(a, b); }
__device__ inline int add(int a, int b) { return a + b; }

// "The sum of a block" of the header: p[t] = p[t] + p[t + k] for t < k, k = 128 .. 1; every lane of the 256 calls this
// with its partial sum already in p[threadIdx.x].  p[0] holds the sum once it returns.
template <typename T>
__device__ inline void tree_sum_256(T* p) {
  for (int k = 128; k > 0; k >>= 1) {
    __syncthreads();
    if ((int)threadIdx.x < k) p[threadIdx.x] = add(p[threadIdx.x], p[threadIdx.x + k]);
  }
  __syncthreads();
}

// The clipped window of superpixel (R, C): rows [y0, y1), columns [x0, x1).
struct Window {
  int y0, y1, x0, x1;
  __device__ Window(int R, int C, int H, int W, int sp)
      : y0(max((R - 1) * sp, 0)), y1(min((R + 2) * sp, H)), x0(max((C - 1) * sp, 0)), x1(min((C + 2) * sp, W)) {}
  __device__ int width() const { return x1 - x0; }
  __device__ int pixels() const { return (y1 - y0) * (x1 - x0); }
};

__global__ __launch_bounds__(256) void grid_labels_kernel(int32_t* __restrict__ labels, int H, int W, int sp, size_t total) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  const int xx = (int)(g % W), yy = (int)((g / W) % H);
  labels[g] = (yy / sp) * (W / sp) + xx / sp;
}

// One block per (image, superpixel): count and channel sums of the window's pixels labelled s.  COORDS = false
// (a3ds_label_mean): out [n,S,c] gets the means, NaN for an empty superpixel.  COORDS = true (a3ds_slic_update, c = 3): out
// [n,S,5] gets (ybar, xbar, means), and is left alone for an empty superpixel.
template <bool COORDS>
__global__ __launch_bounds__(256) void label_reduce_kernel(const float* __restrict__ x, const int32_t* __restrict__ labels,
                                                           float* __restrict__ out, int32_t* __restrict__ count, int H,
                                                           int W, int c, int sp) {
  __shared__ float fsum[4][256];
  __shared__ int isum[3][256];
  const int cols = W / sp, S = (H / sp) * cols;
  const int b = blockIdx.x / S, s = blockIdx.x % S;
  const Window win(s / cols, s % cols, H, W, sp);
  const int ww = win.width(), npix = win.pixels(), tid = threadIdx.x;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  int cnt = 0, sy = 0, sx = 0;
  for (int q = tid; q < npix; q += 256) {
    const int yy = win.y0 + q / ww, xx = win.x0 + q % ww;
    const size_t pix = ((size_t)b * H + yy) * W + xx;
    if (labels[pix] != s) continue;
    ++cnt, sy += yy, sx += xx;
    for (int ch = 0; ch < c; ++ch) acc[ch] = __fadd_rn(acc[ch], x[pix * c + ch]);
  }
  isum[0][tid] = cnt, isum[1][tid] = sy, isum[2][tid] = sx;
  for (int ch = 0; ch < 4; ++ch) fsum[ch][tid] = acc[ch];
  tree_sum_256(isum[0]);
  if (COORDS) tree_sum_256(isum[1]), tree_sum_256(isum[2]);
  for (int ch = 0; ch < c; ++ch) tree_sum_256(fsum[ch]);
  if (tid != 0) return;
  const size_t o = (size_t)b * S + s;
  const int total = isum[0][0];
  count[o] = total;
  const float div = (float)total;
  if (COORDS) {
    if (total == 0) return;
    out[o * 5] = __fdiv_rn((float)isum[1][0], div);
    out[o * 5 + 1] = __fdiv_rn((float)isum[2][0], div);
    for (int ch = 0; ch < 3; ++ch) out[o * 5 + 2 + ch] = __fdiv_rn(fsum[ch][0], div);
  } else {
    for (int ch = 0; ch < c; ++ch) out[o * c + ch] = total ? __fdiv_rn(fsum[ch][0], div) : __builtin_nanf("");
  }
}

__global__ __launch_bounds__(256) void label_hist_kernel(const float* __restrict__ x, const int32_t* __restrict__ labels,
                                                         float* __restrict__ hist, int H, int W, int sp) {
  __shared__ int bins[256];
  const int cols = W / sp, S = (H / sp) * cols;
  const int b = blockIdx.x / S, s = blockIdx.x % S;
  const Window win(s / cols, s % cols, H, W, sp);
  const int ww = win.width(), npix = win.pixels();
  bins[threadIdx.x] = 0;
  __syncthreads();
  for (int q = threadIdx.x; q < npix; q += 256) {
    const size_t pix = ((size_t)b * H + win.y0 + q / ww) * W + win.x0 + q % ww;
    if (labels[pix] == s) atomicAdd(&bins[colour_bin(x + pix * 3)], 1);
  }
  __syncthreads();
  hist[((size_t)b * S + s) * 256 + threadIdx.x] = (float)bins[threadIdx.x];
}

// One lane per pixel: the nearest of its candidates' centres, in ascending superpixel index; the anchor keeps its home.
__global__ __launch_bounds__(256) void slic_assign_kernel(const float* __restrict__ x, const float* __restrict__ centres,
                                                          int32_t* __restrict__ labels, int H, int W, int sp, float wgt,
                                                          size_t total) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  const int rows = H / sp, cols = W / sp;
  const int xx = (int)(g % W), yy = (int)((g / W) % H);
  const size_t b = g / ((size_t)W * H);
  const int R = yy / sp, C = xx / sp;
  int best = R * cols + C;
  if (yy != R * sp + sp / 2 || xx != C * sp + sp / 2) {
    const float p0 = x[g * 3], p1 = x[g * 3 + 1], p2 = x[g * 3 + 2];
    bool found = false;
    float best_d = 0.f;
    for (int Rk = max(R - 1, 0); Rk <= min(R + 1, rows - 1); ++Rk)
      for (int Ck = max(C - 1, 0); Ck <= min(C + 1, cols - 1); ++Ck) {
        const int k = Rk * cols + Ck;
        const float* ce = centres + (b * rows * cols + k) * 5;
        const float d0 = __fsub_rn(p0, ce[2]), d1 = __fsub_rn(p1, ce[3]), d2 = __fsub_rn(p2, ce[4]);
        const float col = __fadd_rn(__fadd_rn(__fmul_rn(d0, d0), __fmul_rn(d1, d1)), __fmul_rn(d2, d2));
        const float dy = __fsub_rn((float)yy, ce[0]), dx = __fsub_rn((float)xx, ce[1]);
        const float d = __fadd_rn(col, __fmul_rn(wgt, __fadd_rn(__fmul_rn(dy, dy), __fmul_rn(dx, dx))));
        if (d == d && (!found || d < best_d)) found = true, best_d = d, best = k;
      }
  }
  labels[g] = best;
}

// One block per (image, pair); lane t holds bin t of the two frequency histograms.
__global__ __launch_bounds__(256) void label_pair_similarity_kernel(const float* __restrict__ mean3, const float* __restrict__ hist,
                                                                    const int32_t* __restrict__ count,
                                                                    const int32_t* __restrict__ left,
                                                                    const int32_t* __restrict__ right,
                                                                    const float* __restrict__ dw, const float* __restrict__ db,
                                                                    float* __restrict__ sims, float* __restrict__ r, int S,
                                                                    int npairs, float gamma) {
  __shared__ float part[256];
  const int q = blockIdx.x % npairs, b = blockIdx.x / npairs;
  const int pl = left[q], pr = right[q];
  const size_t o = (size_t)b * npairs + q;
  if (pl < 0 || pl >= S || pr < 0 || pr >= S) {       // the whole block: nothing is indexed with a bad superpixel
    if (threadIdx.x == 0) sims[2 * o] = sims[2 * o + 1] = r[o] = __builtin_nanf("");
    return;
  }
  const size_t l = (size_t)b * S + pl, rr = (size_t)b * S + pr;
  const float f = __fsub_rn(__fdiv_rn(hist[l * 256 + threadIdx.x], (float)count[l]),
                            __fdiv_rn(hist[rr * 256 + threadIdx.x], (float)count[rr]));
  part[threadIdx.x] = __fmul_rn(f, f);
  tree_sum_256(part);
  if (threadIdx.x != 0) return;
  const float e0 = __fsub_rn(mean3[l * 3], mean3[rr * 3]), e1 = __fsub_rn(mean3[l * 3 + 1], mean3[rr * 3 + 1]),
              e2 = __fsub_rn(mean3[l * 3 + 2], mean3[rr * 3 + 2]);
  const float sc = __fadd_rn(__fadd_rn(__fmul_rn(e0, e0), __fmul_rn(e1, e1)), __fmul_rn(e2, e2));
  const float s0 = expf(__fmul_rn(-gamma, sqrtf(sc))), s1 = expf(__fmul_rn(-gamma, sqrtf(part[0])));
  sims[2 * o] = s0;
  sims[2 * o + 1] = s1;
  r[o] = __fadd_rn(__fadd_rn(__fmul_rn(s0, dw[0]), __fmul_rn(s1, dw[1])), db[0]);
}

// One block of 256 per (image, superpixel) and per 256 * VEC channels (gridDim.y): all 256 lanes scan the window, however
// few the channels leave busy afterwards.  cnt(s, ., .) over the h w <= kMaxCells cells is formed in LDS from the window's
// pixels, with the first and last cell that got one; every lane's float sum then runs over that range in ascending order.
template <int VEC>
__global__ __launch_bounds__(256) void label_pool_fwd_kernel(const float* __restrict__ feat, float* __restrict__ pooled,
                                                             const int32_t* __restrict__ ymap, const int32_t* __restrict__ xmap,
                                                             const int32_t* __restrict__ labels,
                                                             const int32_t* __restrict__ count, int h, int w, int C, int ld,
                                                             int ldp, int H, int W, int sp) {
  __shared__ int s_cnt[kMaxCells], s_lo, s_hi;
  const int cols = W / sp, S = (H / sp) * cols, cells = h * w;
  const int b = blockIdx.x / S, s = blockIdx.x % S;
  const Window win(s / cols, s % cols, H, W, sp);
  const int ww = win.width(), npix = win.pixels(), tid = threadIdx.x, nt = blockDim.x;
  for (int i = tid; i < cells; i += nt) s_cnt[i] = 0;
  if (tid == 0) s_lo = cells, s_hi = -1;
  __syncthreads();
  for (int q = tid; q < npix; q += nt) {
    const int yy = win.y0 + q / ww, xx = win.x0 + q % ww;
    if (labels[((size_t)b * H + yy) * W + xx] != s) continue;
    const int i = ymap[yy], j = xmap[xx];
    if (i < 0 || i >= h || j < 0 || j >= w) continue;
    const int cell = i * w + j;
    atomicAdd(&s_cnt[cell], 1);
    atomicMin(&s_lo, cell);
    atomicMax(&s_hi, cell);
  }
  __syncthreads();
  const int g = blockIdx.y * nt + tid;
  if (g >= C / VEC) return;
  const int c = g * VEC;
  const int cs = count[(size_t)b * S + s];
  const float* fb = feat + (size_t)b * cells * ld + c;
  float acc[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
  if (cs > 0) {
    for (int cell = s_lo; cell <= s_hi; ++cell) {
      const int k0 = s_cnt[cell];
      if (k0 == 0) continue;
      const float wgt = (float)k0;
      float v[VEC];
      load<VEC>(fb + (size_t)cell * ld, v);
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc[k] = __fadd_rn(acc[k], __fmul_rn(wgt, v[k]));
    }
    const float div = (float)cs;
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = __fdiv_rn(acc[k], div);
  }
  store<VEC>(pooled + ((size_t)b * S + s) * ldp + c, acc);
}

// One block of 256 per (image, cell) and per 256 * VEC channels: a gather over the superpixels in ascending order.  The
// pixels of cell (i, j) are the rows with ymap[y] == i crossed with the columns with xmap[x] == j: of every 256 image rows the
// block lists those that match (one lane a row), then its lanes share the pixels of the listed rows.  Nothing is assumed of
// the tables.  A label is an index into the S <= kMaxSuperpixels counts only after it passed the label contract.  Every
// branch around a barrier depends on launch arguments and LDS counts alone, the same in every lane.
template <int VEC>
__global__ __launch_bounds__(256) void label_pool_bwd_kernel(const float* __restrict__ dpooled, float* __restrict__ dfeat,
                                                             const int32_t* __restrict__ ymap, const int32_t* __restrict__ xmap,
                                                             const int32_t* __restrict__ labels,
                                                             const int32_t* __restrict__ count, int h, int w, int C, int ld,
                                                             int ldp, int H, int W, int sp) {
  __shared__ int s_cnt[kMaxSuperpixels], s_rows[256], s_nrows, s_lo, s_hi;
  const int rows = H / sp, cols = W / sp, S = rows * cols;
  const int b = blockIdx.x / (h * w), cell = blockIdx.x % (h * w);
  const int i = cell / w, j = cell % w;
  const int tid = threadIdx.x, nt = 256;
  for (int s = tid; s < S; s += nt) s_cnt[s] = 0;
  if (tid == 0) s_lo = S, s_hi = -1;
  for (int y0 = 0; y0 < H; y0 += nt) {
    if (tid == 0) s_nrows = 0;
    __syncthreads();
    if (y0 + tid < H && ymap[y0 + tid] == i) s_rows[atomicAdd(&s_nrows, 1)] = y0 + tid;
    __syncthreads();
    const int npix = s_nrows * W;                  // at most 256 rows of at most 768 * 64 columns
    for (int q = tid; q < npix; q += nt) {
      const int yy = s_rows[q / W], xx = q % W;
      if (xmap[xx] != j) continue;
      const int l = labels[((size_t)b * H + yy) * W + xx];
      if (l < 0 || l >= S) continue;
      if (abs(l / cols - yy / sp) > 1 || abs(l % cols - xx / sp) > 1) continue;
      atomicAdd(&s_cnt[l], 1);
      atomicMin(&s_lo, l);
      atomicMax(&s_hi, l);
    }
    __syncthreads();
  }
  const int g = blockIdx.y * nt + tid;
  if (g >= C / VEC) return;
  const int c = g * VEC;
  const float* db = dpooled + (size_t)b * S * ldp + c;
  float acc[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
  for (int s = s_lo; s <= s_hi; ++s) {
    const int k0 = s_cnt[s];
    if (k0 == 0) continue;
    const int cs = count[(size_t)b * S + s];
    if (cs <= 0) continue;
    const float wgt = (float)k0, div = (float)cs;
    float v[VEC];
    load<VEC>(db + (size_t)s * ldp, v);
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = __fadd_rn(acc[k], __fdiv_rn(__fmul_rn(wgt, v[k]), div));
  }
  store<VEC>(dfeat + ((size_t)b * h * w + cell) * ld + c, acc);
}

// What every entry point over an image batch refuses.
int image_args(const char* who, int n, int H, int W, int sp) {
  A3D_CHECK_ARG(n > 0 && H > 0 && W > 0 && sp > 0, "%s: n, H, W, sp must be positive", who);
  A3D_CHECK_ARG(sp <= kMaxSp, "%s: superpixel edge %d above A3DS_MAX_SP = %d", who, sp, kMaxSp);
  A3D_CHECK_ARG(H % sp == 0 && W % sp == 0, "%s: H = %d, W = %d are not multiples of sp = %d", who, H, W, sp);
  A3D_CHECK_ARG((long long)n * H * W <= 0x7fffffffLL, "%s: more than 2^31 - 1 pixels", who);
  return A3D_OK;
}

// ... and those that form coordinate means in float32.
int coord_args(const char* who, int n, int H, int W, int sp) {
  const int rc = image_args(who, n, H, W, sp);
  if (rc != A3D_OK) return rc;
  A3D_CHECK_ARG(9LL * sp * sp * std::max(H, W) < (1LL << 24),
                "%s: 9 sp^2 max(H, W) = %lld reaches 2^24: the coordinate sums would not be exact", who,
                9LL * sp * sp * std::max(H, W));
  return A3D_OK;
}

int compactness_arg(const char* who, float compactness) {
  A3D_CHECK_ARG(std::isfinite(compactness) && compactness >= 0.f, "%s: compactness %g is negative or not finite", who,
                (double)compactness);
  return A3D_OK;
}

int launch_update(int n, int H, int W, const float* x, int sp, const int32_t* labels, float* centres, int32_t* count,
                  hipStream_t st) {
  clear_stale_error();
  hipLaunchKernelGGL(label_reduce_kernel<true>, dim3(n * (H / sp) * (W / sp)), dim3(256), 0, st, x, labels, centres, count, H,
                     W, 3, sp);
  return check_launch("slic_update");
}

int launch_assign(int n, int H, int W, const float* x, int sp, const float* centres, float compactness, int32_t* labels,
                  hipStream_t st) {
  const float q = compactness / (float)sp;
  const size_t total = (size_t)n * H * W;
  clear_stale_error();
  hipLaunchKernelGGL(slic_assign_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x, centres, labels, H, W, sp,
                     q * q, total);
  return check_launch("slic_assign");
}

int pool_args(const char* who, int n, int h, int w, int C, const void* a, const void* b, int ld, int ldp, int H, int W, int sp,
              const int32_t* ymap, const int32_t* xmap, const int32_t* labels, const int32_t* count) {
  A3D_CHECK_ARG(a && b && ymap && xmap && labels && count, "%s: NULL pointer", who);
  A3D_CHECK_ARG(h > 0 && w > 0 && C > 0, "%s: h, w, C must be positive", who);
  const int rc = image_args(who, n, H, W, sp);
  if (rc != A3D_OK) return rc;
  A3D_CHECK_ARG(ld >= C && ldp >= C, "%s: strides ld = %d, ldp = %d below C = %d", who, ld, ldp, C);
  A3D_CHECK_ARG((long long)h * w <= kMaxCells, "%s: %lld cells above A3DS_MAX_CELLS = %d", who, (long long)h * w, kMaxCells);
  A3D_CHECK_ARG((long long)(H / sp) * (W / sp) <= kMaxSuperpixels, "%s: %lld superpixels above A3DS_MAX_SUPERPIXELS = %d", who,
                (long long)(H / sp) * (W / sp), kMaxSuperpixels);
  A3D_CHECK_ARG((long long)n * h * w <= 0x7fffffffLL, "%s: more than 2^31 - 1 cells", who);
  A3D_CHECK_ARG(C <= (1 << 22), "%s: C = %d above 2^22", who, C);
  return A3D_OK;
}

}  // namespace
}  // namespace a3d

using namespace a3d;

extern "C" {

int a3ds_label_mean(int n, int H, int W, int c, const float* x, int sp, const int32_t* labels, float* mean, int32_t* count,
                    void* stream) {
  A3D_CHECK_ARG(x && labels && mean && count, "label_mean: NULL pointer");
  A3D_CHECK_ARG(c >= 1 && c <= 4, "label_mean: c = %d outside 1 .. 4", c);
  const int rc = image_args("label_mean", n, H, W, sp);
  if (rc != A3D_OK) return rc;
  clear_stale_error();
  hipLaunchKernelGGL(label_reduce_kernel<false>, dim3(n * (H / sp) * (W / sp)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     x, labels, mean, count, H, W, c, sp);
  return check_launch("label_mean");
}

int a3ds_label_hist(int n, int H, int W, const float* x, int sp, const int32_t* labels, float* hist, void* stream) {
  A3D_CHECK_ARG(x && labels && hist, "label_hist: NULL pointer");
  const int rc = image_args("label_hist", n, H, W, sp);
  if (rc != A3D_OK) return rc;
  clear_stale_error();
  hipLaunchKernelGGL(label_hist_kernel, dim3(n * (H / sp) * (W / sp)), dim3(256), 0, static_cast<hipStream_t>(stream), x,
                     labels, hist, H, W, sp);
  return check_launch("label_hist");
}

int a3ds_slic_update(int n, int H, int W, const float* x, int sp, const int32_t* labels, float* centres, int32_t* count,
                     void* stream) {
  A3D_CHECK_ARG(x && labels && centres && count, "slic_update: NULL pointer");
  const int rc = coord_args("slic_update", n, H, W, sp);
  if (rc != A3D_OK) return rc;
  return launch_update(n, H, W, x, sp, labels, centres, count, static_cast<hipStream_t>(stream));
}

int a3ds_slic_assign(int n, int H, int W, const float* x, int sp, const float* centres, float compactness, int32_t* labels,
                     void* stream) {
  A3D_CHECK_ARG(x && centres && labels, "slic_assign: NULL pointer");
  int rc = coord_args("slic_assign", n, H, W, sp);
  if (rc == A3D_OK) rc = compactness_arg("slic_assign", compactness);
  if (rc != A3D_OK) return rc;
  return launch_assign(n, H, W, x, sp, centres, compactness, labels, static_cast<hipStream_t>(stream));
}

int a3ds_slic_segment(int n, int H, int W, const float* x, int sp, int iters, float compactness, int32_t* labels,
                      float* centres, int32_t* count, void* stream) {
  A3D_CHECK_ARG(x && labels && centres && count, "slic_segment: NULL pointer");
  A3D_CHECK_ARG(iters >= 0, "slic_segment: iters = %d is negative", iters);
  int rc = coord_args("slic_segment", n, H, W, sp);
  if (rc == A3D_OK) rc = compactness_arg("slic_segment", compactness);
  if (rc != A3D_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t total = (size_t)n * H * W;
  clear_stale_error();
  hipLaunchKernelGGL(grid_labels_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, labels, H, W, sp, total);
  rc = check_launch("slic_segment");
  if (rc == A3D_OK) rc = launch_update(n, H, W, x, sp, labels, centres, count, st);
  for (int it = 0; it < iters && rc == A3D_OK; ++it) {
    rc = launch_assign(n, H, W, x, sp, centres, compactness, labels, st);
    if (rc == A3D_OK) rc = launch_update(n, H, W, x, sp, labels, centres, count, st);
  }
  return rc;
}

int a3ds_pair_similarity(int n, int S, const float* mean3, const float* hist, const int32_t* count, const int32_t* left,
                         const int32_t* right, int npairs, const float* dense_w, const float* dense_b, float gamma,
                         float* sims, float* r, void* stream) {
  A3D_CHECK_ARG(mean3 && hist && count && left && right && dense_w && dense_b && sims && r, "label pair_similarity: NULL pointer");
  A3D_CHECK_ARG(n > 0 && S > 0 && npairs > 0, "label pair_similarity: n, S, npairs must be positive");
  A3D_CHECK_ARG((long long)n * npairs <= 0x7fffffffLL && (long long)n * S <= 0x7fffffffLL,
                "label pair_similarity: more than 2^31 - 1 (image, pair)s or superpixels");
  clear_stale_error();
  hipLaunchKernelGGL(label_pair_similarity_kernel, dim3(n * npairs), dim3(256), 0, static_cast<hipStream_t>(stream), mean3,
                     hist, count, left, right, dense_w, dense_b, sims, r, S, npairs, gamma);
  return check_launch("label pair_similarity");
}

int a3ds_label_pool_fwd(int n, int h, int w, int C, const float* feat, int ld, int H, int W, int sp, const int32_t* ymap,
                        const int32_t* xmap, const int32_t* labels, const int32_t* count, float* pooled, int ldp,
                        void* stream) {
  const int rc = pool_args("label_pool_fwd", n, h, w, C, feat, pooled, ld, ldp, H, W, sp, ymap, xmap, labels, count);
  if (rc != A3D_OK) return rc;
  const bool vec = vec4_ok(C, ld, ldp, feat, pooled);
  const int groups = vec ? C / 4 : C;
  const dim3 grid(n * (H / sp) * (W / sp), (groups + 255) / 256);
  clear_stale_error();
  hipLaunchKernelGGL(vec ? label_pool_fwd_kernel<4> : label_pool_fwd_kernel<1>, grid, dim3(256), 0,
                     static_cast<hipStream_t>(stream), feat, pooled, ymap, xmap, labels, count, h, w, C, ld, ldp, H, W, sp);
  return check_launch("label_pool_fwd");
}

int a3ds_label_pool_bwd(int n, int h, int w, int C, const float* dpooled, int ldp, int H, int W, int sp, const int32_t* ymap,
                        const int32_t* xmap, const int32_t* labels, const int32_t* count, float* dfeat, int ld,
                        void* stream) {
  const int rc = pool_args("label_pool_bwd", n, h, w, C, dpooled, dfeat, ld, ldp, H, W, sp, ymap, xmap, labels, count);
  if (rc != A3D_OK) return rc;
  const bool vec = vec4_ok(C, ld, ldp, dpooled, dfeat);
  const int groups = vec ? C / 4 : C;
  const dim3 grid(n * h * w, (groups + 255) / 256);
  clear_stale_error();
  hipLaunchKernelGGL(vec ? label_pool_bwd_kernel<4> : label_pool_bwd_kernel<1>, grid, dim3(256), 0,
                     static_cast<hipStream_t>(stream), dpooled, dfeat, ymap, xmap, labels, count, h, w, C, ld, ldp, H, W, sp);
  return check_launch("label_pool_bwd");
}

}  // extern "C"
