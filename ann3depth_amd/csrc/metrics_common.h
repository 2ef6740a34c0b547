// metrics_common.h — the pixel rule metrics.hip (a3d_depth_metrics) and align.hip (include/a3d_align.h) share, written
// once: how a launch over grid (parts, n) divides an image's target pixels, how a target is decoded (16-byte / 4-byte vector
// loads where the image's base allows, the uint8 look-up table of converter-written records), when a target is valid, and
// the prediction sampled at a target pixel.  Both files are compiled with -ffp-contract=off (see Makefile): the sampled
// prediction is bit for bit what a3d_resize_bilinear_tf1 writes for that pixel (resample.hip, resize_rows).
#pragma once
#include <algorithm>

#include "a3d_internal.h"

namespace a3d {
namespace pixels {

constexpr int kThreads = 256;
constexpr int kPixelsPerPart = 4096;      // 480 x 640 targets: 75 workgroups per image; 55 x 74: one
constexpr int kMaxParts = 1024;

struct PixelArgs {
  const float* pred;
  const void* target;
  void* out;                              // where the launch leaves its partial results (the caller's workspace)
  int ph, pw, th, tw, npix, chunk, parts, u8;
  float sy, sx;                           // legacy ResizeBilinear scales in / out (resize_one in resample.hip)
  float min_depth, max_depth;
};

inline int parts_for(int npix) { return std::min(kMaxParts, std::max(1, (npix + kPixelsPerPart - 1) / kPixelsPerPart)); }

inline bool shape_ok(int n, int th, int tw) {
  return n > 0 && n <= 65535 && th > 0 && tw > 0 && (int64_t)th * tw <= (int64_t)INT32_MAX - 4 * kThreads;   // (grid y)
}

inline bool pred_shape_ok(int ph, int pw) { return ph > 0 && pw > 0 && (int64_t)ph * pw <= INT32_MAX; }

inline void fill_pixel_args(PixelArgs& a, int ph, int pw, const float* pred, int th, int tw, const void* target, int target_u8,
                            float min_depth, float max_depth) {
  a.pred = pred; a.target = target;
  a.ph = ph; a.pw = pw; a.th = th; a.tw = tw; a.npix = th * tw;
  a.parts = parts_for(a.npix);
  a.chunk = ((a.npix + a.parts - 1) / a.parts + 3) & ~3;
  a.u8 = target_u8 ? 1 : 0;
  a.sy = (float)ph / (float)th; a.sx = (float)pw / (float)tw;
  a.min_depth = min_depth; a.max_depth = max_depth;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// The prediction at target pixel (oy, ox): the legacy align_corners=False mapping with resize_rows' operations, or the
// pixel itself when the grids agree.
__device__ __forceinline__ float sample_pred(const PixelArgs& a, const float* p, int oy, int ox) {
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

__device__ __forceinline__ bool target_valid(const PixelArgs& a, float t) {
  return isfinite(t) && t > a.min_depth && t <= a.max_depth;
}

// lut [256] in LDS: the float the converter stored plus the loader's 0.5, as resize_kernel's table (fill_u8_lut,
// resample.hip).  Called by all kThreads threads of a workgroup; the caller synchronises.
__device__ __forceinline__ void fill_u8_lut(float* lut) {
  lut[threadIdx.x] = __fadd_rn(__fsub_rn(__fdiv_rn((float)threadIdx.x, 255.f), 0.5f), 0.5f);
}

// Whether a launch reads whole aligned groups of four targets: every image starts on a 16-byte (float) / 4-byte (uint8)
// boundary (chunk is a multiple of 4); a uniform choice per launch.
template <int U8>
__device__ __forceinline__ bool vector_targets(const PixelArgs& a) {
  return (a.npix & 3) == 0 && ((reinterpret_cast<uintptr_t>(a.target) & (U8 ? 3u : 15u)) == 0);
}

// The targets of pixels i0 .. i0 + 3 of the image whose first target is element `base`; 0 (not valid) from pixel hi on.
template <int U8>
__device__ __forceinline__ void load_targets4(const PixelArgs& a, const float* lut, size_t base, int i0, int hi, bool vec,
                                              float (&t)[4]) {
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
}

}  // namespace pixels
}  // namespace a3d
