// resample.hip — legacy bilinear resize, the affine warp fused into it (train-time augmentation), their validity-aware
// forms for depth maps with holes, and patch extraction.  Compiled with -ffp-contract=off (see Makefile): the oracle does
// these computations as separate fp32 operations, and without FMA contraction the kernels are bit-exact against the numpy
// restatement (HIP's __f*_rn intrinsics are plain operators on ROCm 7.2 and do not prevent contraction by themselves).
#include <algorithm>

#include "a3d_internal.h"
#include "../../include/a3d_valid.h"

namespace a3d {

// ------------------------------------------------------------------ ResizeBilinear (legacy, align_corners=False)
// One block per output row of one tensor (blockIdx.y selects the tensor of a pair: the step resizes the image and its
// depth map, src/models.py:282-283, in ONE launch): the row's source lines and vertical weight are scalars, a thread walks
// the row's (pixel, channel) elements with 32-bit arithmetic.  Same separate fp32 operations as before: bit-exact.
struct ResizeOne { const float* x; float* y; int h, w, c, oh, ow; float sy, sx; int u8; };
// what every kernel of this family takes: one or two tensors of n images each; the warp's table; the range of a valid depth
struct ResampleArgs { ResizeOne t[2]; int n; const float* table; float lo, hi; };
// pixel value k -> the float the converter stored, plus the loader's 0.5: fl(fl(fl(k / 255) - 0.5) + 0.5), in the
// separate correctly-rounded fp32 operations numpy performed (tools/data_tf_converter.py:36-37, src/data.py:84-85)
__device__ __forceinline__ void fill_u8_lut(float (&lut)[256]) {
  lut[threadIdx.x] = __fadd_rn(__fsub_rn(__fdiv_rn((float)threadIdx.x, 255.f), 0.5f), 0.5f);
  __syncthreads();
}
// VALID (NON-REFERENCE, include/a3d_valid.h: a3dx_resize_bilinear_tf1_valid / a3dx_warp_bilinear_pair_valid): the tensor is a depth map with
// holes.  A tap counts when its weight can be non-zero (tl always, tr iff lx > 0, bl iff ly > 0, br iff both); the output is
// NaN unless every counting tap t is finite with lo < t <= hi and all four taps are finite.  No depth is invented.
__device__ __forceinline__ bool taps_valid(float tl, float tr, float bl, float br, float lx, float ly, float lo, float hi) {
  auto ok = [&](float t) { return isfinite(t) && t > lo && t <= hi; };
  const bool px = lx > 0.f, py = ly > 0.f;
  return ok(tl) && (px ? ok(tr) : isfinite(tr)) && (py ? ok(bl) : isfinite(bl)) && (px && py ? ok(br) : isfinite(br));
}
template <typename SRC, bool VALID = false>
__device__ __forceinline__ void resize_rows(const ResizeOne& r, int n, const float* lut, float lo = 0.f, float hi = 0.f) {
  const int rows = n * r.oh;
  const SRC* src = reinterpret_cast<const SRC*>(r.x);
  for (int row = blockIdx.x; row < rows; row += gridDim.x) {
    const int b = row / r.oh, oy = row - b * r.oh;
    const float fy = __fmul_rn((float)oy, r.sy);
    const int y0 = (int)fy, y1 = min(y0 + 1, r.h - 1);
    const float ly = __fsub_rn(fy, (float)y0);
    const SRC* l0 = src + ((size_t)b * r.h + y0) * r.w * r.c;
    const SRC* l1 = src + ((size_t)b * r.h + y1) * r.w * r.c;
    float* out = r.y + (size_t)row * r.ow * r.c;
    const int ne = r.ow * r.c;
    auto tap = [&](const SRC* line, int i) -> float {
      if constexpr (sizeof(SRC) == 1) return lut[line[i]];
      else return line[i];
    };
    for (int e = threadIdx.x; e < ne; e += 256) {
      const int ox = e / r.c, ch = e - ox * r.c;
      const float fx = __fmul_rn((float)ox, r.sx);
      const int x0 = (int)fx, x1 = min(x0 + 1, r.w - 1);
      const float lx = __fsub_rn(fx, (float)x0);
      const float tl = tap(l0, x0 * r.c + ch), tr = tap(l0, x1 * r.c + ch);
      const float bl = tap(l1, x0 * r.c + ch), br = tap(l1, x1 * r.c + ch);
      const float top = __fadd_rn(tl, __fmul_rn(__fsub_rn(tr, tl), lx));
      const float bot = __fadd_rn(bl, __fmul_rn(__fsub_rn(br, bl), lx));
      float y = __fadd_rn(top, __fmul_rn(__fsub_rn(bot, top), ly));
      if constexpr (VALID) {
        if (!taps_valid(tl, tr, bl, br, lx, ly, lo, hi)) y = __builtin_nanf("");
      }
      out[e] = y;
    }
  }
}
// VALID: tensor 1 (blockIdx.y == 1, always present then) is resized validity-aware; tensor 0 exactly as without
template <bool VALID>
__global__ __launch_bounds__(256) void resize_kernel(const ResampleArgs p) {
  const ResizeOne& r = p.t[blockIdx.y];
  __shared__ float lut[256];
  if constexpr (VALID) {
    if (r.u8) fill_u8_lut(lut);
    if (blockIdx.y != 0) {
      if (r.u8) resize_rows<uint8_t, true>(r, p.n, lut, p.lo, p.hi);
      else resize_rows<float, true>(r, p.n, nullptr, p.lo, p.hi);
      return;
    }
  }
  if (r.u8) {
    if constexpr (!VALID) fill_u8_lut(lut);
    resize_rows<uint8_t>(r, p.n, lut);
  } else {
    resize_rows<float>(r, p.n, nullptr);
  }
}

// ------------------------------------------------------------------ affine warp + resize (train-time augmentation)
// The resize above with an affine map of source space between the output grid and the taps (include/a3d.h,
// a3d_warp_bilinear_pair).  A rotated output row crosses many source lines, so the output is cut into kWarpTH x kWarpTW
// pixel tiles, one block per tile: a tile's taps fall in a compact source patch.  A 32-lane half wave walks the
// (pixel, channel) elements of one tile row, which are contiguous in the output.  Coordinates are clamped before they
// become indices (fmaxf sends a NaN to 0): no read leaves the image whatever the table holds.
constexpr int kWarpTW = 32, kWarpTH = 256 / kWarpTW, kWarpBlocks = 4096;
template <typename SRC, bool VALID = false>
__device__ __forceinline__ void warp_tiles(const ResizeOne& r, int n, bool second, const float* __restrict__ table,
                                           const float* lut, float lo = 0.f, float hi = 0.f) {
  const int tiles_x = (r.ow + kWarpTW - 1) / kWarpTW, tiles_y = (r.oh + kWarpTH - 1) / kWarpTH;
  const int per_image = tiles_x * tiles_y, tiles = n * per_image;
  const int line = r.w * r.c;
  const float xmax = (float)(r.w - 1), ymax = (float)(r.h - 1);
  const int ry = threadIdx.x / kWarpTW, lane = threadIdx.x % kWarpTW;
  auto tap = [&](const SRC* p, int i) -> float {
    if constexpr (sizeof(SRC) == 1) return lut[p[i]];
    else return p[i];
  };
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int b = t / per_image, q = t - b * per_image, ty = q / tiles_x, tx = q - ty * tiles_x;
    const float* m = table + b * A3D_WARP_STRIDE;
    const float m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[3], m11 = m[4], m12 = m[5];
    const float g0 = m[6], g1 = m[7], g2 = m[8], g3 = m[9], gd = m[10];
    const int oy = ty * kWarpTH + ry, ox0 = tx * kWarpTW;
    if (oy >= r.oh) continue;
    const SRC* img = reinterpret_cast<const SRC*>(r.x) + (size_t)b * r.h * line;
    float* out = r.y + (((size_t)b * r.oh + oy) * r.ow + ox0) * r.c;
    const int ne = min(kWarpTW, r.ow - ox0) * r.c;
    const float v = __fmul_rn((float)oy, r.sy);
    const float a01 = __fmul_rn(m01, v), a11 = __fmul_rn(m11, v);
    for (int e = lane; e < ne; e += kWarpTW) {
      const int px = e / r.c, ch = e - px * r.c;
      const float u = __fmul_rn((float)(ox0 + px), r.sx);
      float fx = __fadd_rn(__fadd_rn(__fmul_rn(m00, u), a01), m02);
      float fy = __fadd_rn(__fadd_rn(__fmul_rn(m10, u), a11), m12);
      fx = fminf(fmaxf(fx, 0.f), xmax);
      fy = fminf(fmaxf(fy, 0.f), ymax);
      const int x0 = (int)fx, x1 = min(x0 + 1, r.w - 1), y0 = (int)fy, y1 = min(y0 + 1, r.h - 1);
      const float lx = __fsub_rn(fx, (float)x0), ly = __fsub_rn(fy, (float)y0);
      const int o0 = y0 * line + ch, o1 = y1 * line + ch, c0 = x0 * r.c, c1 = x1 * r.c;
      const float tl = tap(img, o0 + c0), tr = tap(img, o0 + c1);
      const float bl = tap(img, o1 + c0), br = tap(img, o1 + c1);
      const float top = __fadd_rn(tl, __fmul_rn(__fsub_rn(tr, tl), lx));
      const float bot = __fadd_rn(bl, __fmul_rn(__fsub_rn(br, bl), lx));
      const float gain = second ? gd : ch == 0 ? g0 : ch == 1 ? g1 : ch == 2 ? g2 : g3;
      float y = __fmul_rn(__fadd_rn(top, __fmul_rn(__fsub_rn(bot, top), ly)), gain);
      if constexpr (VALID) {       // on the stored values, before the gain
        if (!taps_valid(tl, tr, bl, br, lx, ly, lo, hi)) y = __builtin_nanf("");
      }
      out[e] = y;
    }
  }
}
template <bool VALID>
__global__ __launch_bounds__(256) void warp_kernel(const ResampleArgs p) {
  const ResizeOne& r = p.t[blockIdx.y];
  __shared__ float lut[256];
  if constexpr (VALID) {
    if (r.u8) fill_u8_lut(lut);
    if (blockIdx.y != 0) {
      if (r.u8) warp_tiles<uint8_t, true>(r, p.n, true, p.table, lut, p.lo, p.hi);
      else warp_tiles<float, true>(r, p.n, true, p.table, nullptr, p.lo, p.hi);
      return;
    }
  }
  if (r.u8) {
    if constexpr (!VALID) fill_u8_lut(lut);
    warp_tiles<uint8_t>(r, p.n, blockIdx.y != 0, p.table, lut);
  } else {
    warp_tiles<float>(r, p.n, blockIdx.y != 0, p.table, nullptr);
  }
}

// The host side of all six entry points.  A second tensor with x == nullptr is absent: one tensor, grid y = 1.  `warp`
// takes the table and the tile grid, `valid` requires the second tensor, the depth map, and a range for it.
static ResizeOne resize_one(int h, int w, int c, const void* x, int u8, int oh, int ow, float* y) {
  ResizeOne r;
  r.u8 = u8 ? 1 : 0;
  r.x = static_cast<const float*>(x); r.y = y; r.h = h; r.w = w; r.c = c; r.oh = oh; r.ow = ow;
  r.sy = (float)h / (float)oh; r.sx = (float)w / (float)ow;
  return r;
}
static ResampleArgs resample_args(int n, int h, int w, int c0, const void* x0, int u8_0, int oh0, int ow0, float* y0, int c1,
                                  const void* x1, int u8_1, int oh1, int ow1, float* y1, const float* table = nullptr,
                                  float lo = 0.f, float hi = 0.f) {
  ResampleArgs p;
  p.t[0] = resize_one(h, w, c0, x0, u8_0, oh0, ow0, y0);
  p.t[1] = resize_one(h, w, c1, x1, u8_1, oh1, ow1, y1);
  p.n = n; p.table = table; p.lo = lo; p.hi = hi;
  return p;
}
static int launch_resample(ResampleArgs p, const char* who, bool warp, bool valid, void* stream) {
  const ResizeOne &a = p.t[0], &b = p.t[1];
  const bool two = b.x != nullptr, b_ok = b.c > 0 && b.oh > 0 && b.ow > 0 && b.y;
  A3D_CHECK_ARG(p.n > 0 && a.h > 0 && a.w > 0 && a.c > 0 && a.oh > 0 && a.ow > 0 && a.x && a.y, "%s: bad arguments", who);
  A3D_CHECK_ARG(!warp || a.c <= 4, "%s: the table holds 4 channel gains, the first tensor has %d channels", who, a.c);
  A3D_CHECK_ARG(valid || !two || b_ok, "%s: bad second tensor", who);
  A3D_CHECK_ARG(!valid || (two && b_ok), "%s: the second tensor, the depth map, is required", who);
  A3D_CHECK_ARG(!warp || p.table, "%s: no table", who);
  A3D_CHECK_ARG(!valid || p.lo <= p.hi, "%s: thresholds %g, %g (NaN, or min_depth > max_depth)", who, (double)p.lo, (double)p.hi);
  if (!two) p.t[1] = p.t[0];
  const long long lim = 0x7fffffffLL;         // the kernels' index arithmetic is 32-bit
  // resize: output rows (n oh) and the elements of one source or output line are ints; image bases are 64-bit
  A3D_CHECK_ARG((long long)p.n * std::max(a.oh, b.oh) <= lim && (long long)a.w * a.c <= lim && (long long)b.w * b.c <= lim &&
                    (long long)a.ow * a.c <= lim && (long long)b.ow * b.c <= lim,
                "%s: image too large", who);
  long long blocks = std::min((long long)p.n * std::max(a.oh, b.oh), 16384LL);       // resize: a block per output row
  if (warp) {
    A3D_CHECK_ARG((long long)a.h * a.w * std::max(a.c, b.c) <= lim && (long long)p.n * A3D_WARP_STRIDE <= lim,
                  "%s: image too large", who);
    auto tiles = [&](const ResizeOne& r) {
      return (long long)p.n * ((r.oh + kWarpTH - 1) / kWarpTH) * ((r.ow + kWarpTW - 1) / kWarpTW);
    };
    blocks = std::max(tiles(a), tiles(b));
    A3D_CHECK_ARG(blocks <= lim, "%s: output too large", who);
    blocks = std::min(blocks, (long long)kWarpBlocks);
  }
  void (*kernel)(const ResampleArgs) = warp ? (valid ? warp_kernel<true> : warp_kernel<false>)
                                            : (valid ? resize_kernel<true> : resize_kernel<false>);
  clear_stale_error();
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks, two ? 2 : 1), dim3(256), 0, static_cast<hipStream_t>(stream), p);
  return check_launch(who);
}

}  // namespace a3d

using namespace a3d;

extern "C" {

int a3d_resize_bilinear_tf1(int n, int h, int w, int c, const float* x, int oh, int ow, float* y, void* stream) {
  return launch_resample(resample_args(n, h, w, c, x, 0, oh, ow, y, 0, nullptr, 0, 0, 0, nullptr), "resize", false, false, stream);
}

int a3d_resize_bilinear_tf1_pair(int n, int h, int w, int c0, const float* x0, int oh0, int ow0, float* y0, int c1,
                                 const float* x1, int oh1, int ow1, float* y1, void* stream) {
  // both tensors are required here, under one message
  A3D_CHECK_ARG(n > 0 && h > 0 && w > 0 && c0 > 0 && c1 > 0 && oh0 > 0 && ow0 > 0 && oh1 > 0 && ow1 > 0 && x0 && y0 && x1 && y1,
                "resize_pair: bad arguments");
  return launch_resample(resample_args(n, h, w, c0, x0, 0, oh0, ow0, y0, c1, x1, 0, oh1, ow1, y1), "resize_pair", false, false,
                         stream);
}

int a3d_resize_bilinear_tf1_ex(int n, int h, int w, int c0, const void* x0, int u8_0, int oh0, int ow0, float* y0, int c1,
                               const void* x1, int u8_1, int oh1, int ow1, float* y1, void* stream) {
  return launch_resample(resample_args(n, h, w, c0, x0, u8_0, oh0, ow0, y0, c1, x1, u8_1, oh1, ow1, y1), "resize_ex", false,
                         false, stream);
}

int a3d_warp_bilinear_pair(int n, int h, int w, int c0, const void* x0, int u8_0, int oh0, int ow0, float* y0, int c1,
                           const void* x1, int u8_1, int oh1, int ow1, float* y1, const float* table, void* stream) {
  return launch_resample(resample_args(n, h, w, c0, x0, u8_0, oh0, ow0, y0, c1, x1, u8_1, oh1, ow1, y1, table), "warp_pair",
                         true, false, stream);
}

int a3dx_resize_bilinear_tf1_valid(int n, int h, int w, int c0, const void* x0, int u8_0, int oh0, int ow0, float* y0, int c1,
                                  const void* x1, int u8_1, int oh1, int ow1, float* y1, float min_depth, float max_depth,
                                  void* stream) {
  return launch_resample(resample_args(n, h, w, c0, x0, u8_0, oh0, ow0, y0, c1, x1, u8_1, oh1, ow1, y1, nullptr, min_depth,
                                       max_depth), "resize_valid", false, true, stream);
}

int a3dx_warp_bilinear_pair_valid(int n, int h, int w, int c0, const void* x0, int u8_0, int oh0, int ow0, float* y0, int c1,
                                 const void* x1, int u8_1, int oh1, int ow1, float* y1, const float* table, float min_depth,
                                 float max_depth, void* stream) {
  return launch_resample(resample_args(n, h, w, c0, x0, u8_0, oh0, ow0, y0, c1, x1, u8_1, oh1, ow1, y1, table, min_depth,
                                       max_depth), "warp_pair_valid", true, true, stream);
}

}  // extern "C"

namespace a3d {
// ------------------------------------------------------------------ extract_image_patches (SAME, zero fill)
__global__ __launch_bounds__(256) void patches_kernel(const float* __restrict__ x, float* __restrict__ y, int n, int h,
                                                      int w, int c, int k, int stride, int ph, int pw, int pad_t,
                                                      int pad_l) {
  const size_t total = (size_t)n * ph * pw * k * k * c;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int ch = (int)(i % c);
    size_t t = i / c;
    const int j = (int)(t % k);
    t /= k;
    const int ii = (int)(t % k);
    t /= k;
    const int pc = (int)(t % pw);
    t /= pw;
    const int pr = (int)(t % ph);
    const int b = (int)(t / ph);
    const int sy = pr * stride - pad_t + ii, sx = pc * stride - pad_l + j;
    float v = 0.f;
    if ((unsigned)sy < (unsigned)h && (unsigned)sx < (unsigned)w) v = x[(((size_t)b * h + sy) * w + sx) * c + ch];
    y[i] = v;
  }
}
}  // namespace a3d

extern "C" {

int a3d_extract_patches(int n, int h, int w, int c, const float* x, int k, int stride, float* y, void* stream) {
  A3D_CHECK_ARG(n > 0 && h > 0 && w > 0 && c > 0 && k > 0 && stride > 0 && x && y, "patches: bad arguments");
  const int ph = (h + stride - 1) / stride, pw = (w + stride - 1) / stride;
  const int pad_h = std::max((ph - 1) * stride + k - h, 0), pad_w = std::max((pw - 1) * stride + k - w, 0);
  const size_t total = (size_t)n * ph * pw * k * k * c;
  clear_stale_error();
  hipLaunchKernelGGL(patches_kernel, dim3(grid_for(total, 256, 16384)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), x, y, n, h, w, c, k, stride, ph, pw, pad_h / 2, pad_w / 2);
  return check_launch("patches");
}

}  // extern "C"
