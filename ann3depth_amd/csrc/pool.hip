// pool.hip — max pool 2x2/2 VALID (+concat), its gradients (+ReluGrad) and their entry points a3d_maxpool2x2_*.  The
// scalar kernels are written once for an element type T, float32 or bf16: values are compared as float (the maximum of
// bf16 values is exact in either type), first maximum in scan order, -0.0 and +0.0 tie.  Compiled with -ffp-contract=off
// like pointwise.hip (see Makefile), although nothing here could contract.
#include "a3d_internal.h"

namespace a3d {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// pixel index -> (b, p, q) of a [n][rows][cols] grid: an output pixel of the forward, a 2x2 cell of the input grid of a gradient
struct PoolCell { int b, p, q; };
__device__ __forceinline__ PoolCell pool_cell(size_t t, int rows, int cols) {
  PoolCell k;
  k.q = (int)(t % cols);
  t /= cols;
  k.p = (int)(t % rows);
  k.b = (int)(t / rows);
  return k;
}
// a cell cut by VALID flooring (odd last row or column): zeros, where the cell has pixels at all
template <typename D>
__device__ __forceinline__ void pool_zero_cut(D* dx, size_t base, size_t ld, int h, int w, int p, int q) {
  const D zero = (D)0.f;
  const bool has_r = 2 * p + 1 < h, has_c = 2 * q + 1 < w;
  dx[base] = zero;
  if (has_c) dx[base + ld] = zero;
  if (has_r) dx[base + (size_t)w * ld] = zero;
  if (has_r && has_c) dx[base + (size_t)w * ld + ld] = zero;
}

// ------------------------------------------------------------------ forward
// one thread per output element; pixel strides ldx of x and ldy of y; channel c of y is extra[pixel] when extra is given
template <typename T>
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const T* __restrict__ x, T* __restrict__ y,
                                                          const float* __restrict__ extra, int n, int h, int w, int c,
                                                          int ho, int wo, int ldx, int ldy) {
  const int cout = c + (extra ? 1 : 0);
  const size_t total = (size_t)n * ho * wo * cout;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int ch = (int)(i % cout);
    const size_t pix = i / cout;
    T v;
    if (ch < c) {
      const PoolCell k = pool_cell(pix, ho, wo);
      const T* s = x + (((size_t)k.b * h + 2 * k.p) * w + 2 * k.q) * ldx + ch;
      const float m = fmaxf(fmaxf((float)s[0], (float)s[ldx]), fmaxf((float)s[(size_t)w * ldx], (float)s[(size_t)w * ldx + ldx]));
      v = (T)m;
    } else {
      v = (T)extra[pix];
    }
    y[pix * ldy + ch] = v;
  }
}

// ------------------------------------------------------------------ gradient, recomputing the maximum from x
// one thread per 2x2 cell of the INPUT grid (ceil(h/2) x ceil(w/2)); x and dx share the pixel stride ldx
template <typename T>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                                                          T* __restrict__ dx, int n, int h, int w, int c, int ho, int wo,
                                                          int ldx, int lddy, int relu_mask) {
  const int hc = (h + 1) / 2, wc = (w + 1) / 2;
  const size_t total = (size_t)n * hc * wc * c;
  const T zero = (T)0.f;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int ch = (int)(i % c);
    const PoolCell k = pool_cell(i / c, hc, wc);
    const size_t base = (((size_t)k.b * h + 2 * k.p) * w + 2 * k.q) * ldx + ch;
    const size_t ld = (size_t)ldx;      // x and dx share the pixel stride
    if (k.p < ho && k.q < wo) {
      const float v0 = (float)x[base], v1 = (float)x[base + ld], v2 = (float)x[base + (size_t)w * ld],
                  v3 = (float)x[base + (size_t)w * ld + ld];
      int arg = 0;
      float best = v0;
      if (v1 > best) { best = v1; arg = 1; }
      if (v2 > best) { best = v2; arg = 2; }
      if (v3 > best) { best = v3; arg = 3; }
      T g = dy[(((size_t)k.b * ho + k.p) * wo + k.q) * lddy + ch];
      if (relu_mask && !(best > 0.f)) g = zero;
      dx[base] = arg == 0 ? g : zero;
      dx[base + ld] = arg == 1 ? g : zero;
      dx[base + (size_t)w * ld] = arg == 2 ? g : zero;
      dx[base + (size_t)w * ld + ld] = arg == 3 ? g : zero;
    } else {
      pool_zero_cut(dx, base, ld, h, w, k.p, k.q);
    }
  }
}

// ------------------------------------------------------------------ gradient from the recorded argmax
// the same from the argmax position and the pooled value that a3d_conv2d_pool_fwd left; dx is dense float32 (with bf16
// y and dy it is what the 3-channel layers' filter gradient takes)
template <typename T>
__global__ __launch_bounds__(256) void maxpool_bwd_idx_kernel(const uint8_t* __restrict__ argmax, const T* __restrict__ y,
                                                              const T* __restrict__ dy, float* __restrict__ dx, int n, int h,
                                                              int w, int c, int ho, int wo, int ldy, int lddy, int relu_mask) {
  const int hc = (h + 1) / 2, wc = (w + 1) / 2;
  const size_t total = (size_t)n * hc * wc * c;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int ch = (int)(i % c);
    const PoolCell k = pool_cell(i / c, hc, wc);
    const size_t base = (((size_t)k.b * h + 2 * k.p) * w + 2 * k.q) * c + ch;
    if (k.p < ho && k.q < wo) {
      const size_t win = ((size_t)k.b * ho + k.p) * wo + k.q;
      const int arg = argmax[win * c + ch];
      float g = (float)dy[win * lddy + ch];
      if (relu_mask && !((float)y[win * ldy + ch] > 0.f)) g = 0.f;
      dx[base] = arg == 0 ? g : 0.f;
      dx[base + c] = arg == 1 ? g : 0.f;
      dx[base + (size_t)w * c] = arg == 2 ? g : 0.f;
      dx[base + (size_t)w * c + c] = arg == 3 ? g : 0.f;
    } else {
      pool_zero_cut(dx, base, (size_t)c, h, w, k.p, k.q);
    }
  }
}

// four channels per thread, 16-byte accesses (c, ldy, lddy multiples of 4; 16-byte aligned tensors)
__global__ __launch_bounds__(256) void maxpool_bwd_idx_vec4_kernel(const uint8_t* __restrict__ argmax,
                                                                   const float* __restrict__ y, const float* __restrict__ dy,
                                                                   float* __restrict__ dx, int n, int h, int w, int c, int ho,
                                                                   int wo, int ldy, int lddy, int relu_mask) {
  const int hc = (h + 1) / 2, wc = (w + 1) / 2, c4 = c / 4;
  const uint32_t total = (uint32_t)n * hc * wc * c4;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const uint32_t ch = (i % c4) * 4;
    uint32_t t = i / c4;
    const uint32_t q = t % wc;
    t /= wc;
    const uint32_t p = t % hc, b = t / hc;
    const size_t base = (((size_t)b * h + 2 * p) * w + 2 * q) * c + ch;
    const bool has_r = 2 * p + 1 < (uint32_t)h, has_c = 2 * q + 1 < (uint32_t)w;
    f32x4 o0 = zero, o1 = zero, o2 = zero, o3 = zero;
    if (p < (uint32_t)ho && q < (uint32_t)wo) {
      const size_t win = ((size_t)b * ho + p) * wo + q;
      const uint32_t a4 = *reinterpret_cast<const uint32_t*>(argmax + win * c + ch);
      const f32x4 g4 = *reinterpret_cast<const f32x4*>(dy + win * lddy + ch);
      const f32x4 y4 = *reinterpret_cast<const f32x4*>(y + win * ldy + ch);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t arg = (a4 >> (8 * j)) & 0xffu;
        const float g = (relu_mask && !(y4[j] > 0.f)) ? 0.f : g4[j];
        o0[j] = arg == 0 ? g : 0.f; o1[j] = arg == 1 ? g : 0.f; o2[j] = arg == 2 ? g : 0.f; o3[j] = arg == 3 ? g : 0.f;
      }
    }
    *reinterpret_cast<f32x4*>(dx + base) = o0;
    if (has_c) *reinterpret_cast<f32x4*>(dx + base + c) = o1;
    if (has_r) *reinterpret_cast<f32x4*>(dx + base + (size_t)w * c) = o2;
    if (has_r && has_c) *reinterpret_cast<f32x4*>(dx + base + (size_t)w * c + c) = o3;
  }
}

// The same with a bf16 dx (config 5: the conv stack's activation gradients are bf16 tensors), eight channels per thread:
// 8 argmax bytes, 16 bytes of pooled values and of dy in, four 16-byte pieces of dx out.
__global__ __launch_bounds__(256) void maxpool_bwd_idx_bf16s_kernel(const uint8_t* __restrict__ argmax,
                                                                    const __bf16* __restrict__ y, const __bf16* __restrict__ dy,
                                                                    __bf16* __restrict__ dx, int n, int h, int w, int c, int ho,
                                                                    int wo, int ldy, int lddy, int relu_mask) {
  const int hc = (h + 1) / 2, wc = (w + 1) / 2, c8 = c / 8;
  const size_t total = (size_t)n * hc * wc * c8;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int ch = (int)(i % c8) * 8;
    size_t t = i / c8;
    const int q = (int)(t % wc);
    t /= wc;
    const int p = (int)(t % hc);
    const int b = (int)(t / hc);
    const size_t base = (((size_t)b * h + 2 * p) * w + 2 * q) * c + ch;
    const bool has_r = 2 * p + 1 < h, has_c = 2 * q + 1 < w;
    u32x4 o[4] = {u32x4{0, 0, 0, 0}, u32x4{0, 0, 0, 0}, u32x4{0, 0, 0, 0}, u32x4{0, 0, 0, 0}};
    if (p < ho && q < wo) {
      const size_t win = ((size_t)b * ho + p) * wo + q;
      const uint2 a8 = *reinterpret_cast<const uint2*>(argmax + win * c + ch);
      const u32x4 yv = *reinterpret_cast<const u32x4*>(y + win * ldy + ch);
      const u32x4 gv = *reinterpret_cast<const u32x4*>(dy + win * lddy + ch);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const uint32_t sh = (e & 1) ? 0xffff0000u : 0x0000ffffu;
        const uint32_t yb = (e & 1) ? (yv[e >> 1] & 0xffff0000u) : (yv[e >> 1] << 16);
        uint32_t g = gv[e >> 1] & sh;                                   // the gradient's 16 bits, in place
        if (relu_mask && !(__uint_as_float(yb) > 0.f)) g = 0u;
        const uint32_t arg = ((e < 4 ? a8.x : a8.y) >> (8 * (e & 3))) & 0xffu;
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (arg == (uint32_t)k) o[k][e >> 1] |= g;
      }
    }
    *reinterpret_cast<u32x4*>(dx + base) = o[0];
    if (has_c) *reinterpret_cast<u32x4*>(dx + base + c) = o[1];
    if (has_r) *reinterpret_cast<u32x4*>(dx + base + (size_t)w * c) = o[2];
    if (has_r && has_c) *reinterpret_cast<u32x4*>(dx + base + (size_t)w * c + c) = o[3];
  }
}

// What every entry point below does around its kernel: the argument check (`ok` is the caller's part of it), one thread
// per channel group of `cw` channels — of each output pixel (forward) or of each 2x2 cell of the input grid — and the launch.
template <typename... P, typename... A>
static int launch_pool(const char* who, bool ok, bool fwd, int n, int h, int w, int cw, void (*kernel)(P...), void* stream,
                       A... args) {
  A3D_CHECK_ARG(ok && n > 0 && h >= 2 && w >= 2 && cw > 0, "%s: bad arguments", who);
  const size_t total = fwd ? (size_t)n * (h / 2) * (w / 2) * cw : (size_t)n * ((h + 1) / 2) * ((w + 1) / 2) * cw;
  clear_stale_error();
  hipLaunchKernelGGL(kernel, dim3(grid_for(total)), dim3(256), 0, static_cast<hipStream_t>(stream), args...);
  return check_launch(who);
}

}  // namespace a3d

using namespace a3d;

extern "C" {

int a3d_maxpool2x2_fwd(int n, int h, int w, int c, const float* x, float* y, int ldy, const float* extra,
                       void* stream) {
  const int cout = c + (extra ? 1 : 0);
  const bool ok = n > 0 && h >= 2 && w >= 2 && c > 0 && x && y;
  A3D_CHECK_ARG(!ok || ldy >= cout, "maxpool_fwd: ldy %d too small", ldy);
  return launch_pool("maxpool_fwd", ok, true, n, h, w, cout, maxpool_fwd_kernel<float>, stream, x, y, extra, n, h, w, c,
                     h / 2, w / 2, c, ldy);
}

int a3d_maxpool2x2_fwd_bf16(int n, int h, int w, int c, const void* x, int ldx, void* y, int ldy, const float* extra,
                            void* stream) {
  const int cout = c + (extra ? 1 : 0);
  return launch_pool("maxpool_fwd_bf16", c > 0 && x && y && ldx >= c && ldy >= cout, true, n, h, w, cout,
                     maxpool_fwd_kernel<__bf16>, stream, static_cast<const __bf16*>(x), static_cast<__bf16*>(y), extra, n, h,
                     w, c, h / 2, w / 2, ldx, ldy);
}

int a3d_maxpool2x2_bwd(int n, int h, int w, int c, const float* x, const float* dy, int lddy, float* dx,
                       int relu_mask, void* stream) {
  return launch_pool("maxpool_bwd", x && dy && dx && lddy >= c, false, n, h, w, c, maxpool_bwd_kernel<float>, stream, x, dy,
                     dx, n, h, w, c, h / 2, w / 2, c, lddy, relu_mask);
}

int a3d_maxpool2x2_bwd_bf16(int n, int h, int w, int c, const void* x, int ldx, const void* dy, int lddy, void* dx,
                            int relu_mask, void* stream) {
  return launch_pool("maxpool_bwd_bf16", x && dy && dx && lddy >= c && ldx >= c, false, n, h, w, c,
                     maxpool_bwd_kernel<__bf16>, stream, static_cast<const __bf16*>(x), static_cast<const __bf16*>(dy),
                     static_cast<__bf16*>(dx), n, h, w, c, h / 2, w / 2, ldx, lddy, relu_mask);
}

int a3d_maxpool2x2_bwd_idx(int n, int h, int w, int c, const uint8_t* argmax, const float* y, int ldy, const float* dy,
                           int lddy, float* dx, int relu_mask, void* stream) {
  A3D_CHECK_ARG(n > 0 && h >= 2 && w >= 2 && c > 0 && argmax && y && dy && dx && ldy >= c && lddy >= c,
                "maxpool_bwd_idx: bad arguments");
  const size_t total = (size_t)n * ((h + 1) / 2) * ((w + 1) / 2) * c;
  const uintptr_t al = reinterpret_cast<uintptr_t>(argmax) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(dy) |
                       reinterpret_cast<uintptr_t>(dx);
  const bool vec4 = c % 4 == 0 && ldy % 4 == 0 && lddy % 4 == 0 && (al & 15) == 0 && total / 4 < (1u << 31);
  return launch_pool(vec4 ? "maxpool_bwd_idx_vec4" : "maxpool_bwd_idx", true, false, n, h, w, vec4 ? c / 4 : c,
                     vec4 ? maxpool_bwd_idx_vec4_kernel : maxpool_bwd_idx_kernel<float>, stream, argmax, y, dy, dx, n, h, w, c,
                     h / 2, w / 2, ldy, lddy, relu_mask);
}

int a3d_maxpool2x2_bwd_idx_bf16(int n, int h, int w, int c, const uint8_t* argmax, const void* y, int ldy, const void* dy,
                                int lddy, float* dx, int relu_mask, void* stream) {
  return launch_pool("maxpool_bwd_idx_bf16", argmax && y && dy && dx && ldy >= c && lddy >= c, false, n, h, w, c,
                     maxpool_bwd_idx_kernel<__bf16>, stream, argmax, static_cast<const __bf16*>(y),
                     static_cast<const __bf16*>(dy), dx, n, h, w, c, h / 2, w / 2, ldy, lddy, relu_mask);
}

int a3d_maxpool2x2_bwd_idx_bf16s(int n, int h, int w, int c, const uint8_t* argmax, const void* y, int ldy, const void* dy,
                                 int lddy, void* dx, int relu_mask, void* stream) {
  A3D_CHECK_ARG(n > 0 && h >= 2 && w >= 2 && c > 0 && argmax && y && dy && dx && ldy >= c && lddy >= c,
                "maxpool_bwd_idx_bf16s: bad arguments");
  const uintptr_t al = reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(dx);
  A3D_CHECK_ARG(c % 8 == 0 && ldy % 8 == 0 && lddy % 8 == 0 && (al & 15) == 0 && (reinterpret_cast<uintptr_t>(argmax) & 7) == 0,
                "maxpool_bwd_idx_bf16s: channels and pixel strides in whole 16-byte pieces");
  return launch_pool("maxpool_bwd_idx_bf16s", true, false, n, h, w, c / 8, maxpool_bwd_idx_bf16s_kernel, stream, argmax,
                     static_cast<const __bf16*>(y), static_cast<const __bf16*>(dy), static_cast<__bf16*>(dx), n, h, w, c, h / 2,
                     w / 2, ldy, lddy, relu_mask);
}

}  // extern "C"
