// optim_rules.h — the optimizer rules, each written once: the per-element arithmetic (momentum_one, adam_one, the frozen Adam's
// adam_frozen_* with its register-piece form for the dense filter-gradient epilogues of dense.hip and optim.hip) and the walk of a
// flat parameter group that applies it (the *_body functions).  The __global__ kernels around the walks differ only in where the
// gradient's scale comes from: a launch argument (pointwise.hip: ApplyAdam; crf.hip: gradient descent; optim.hip: momentum) or
// the control block a gradient-norm launch left on the device (clip.hip, include/a3d_clip.h).  Everything is __forceinline__: a
// kernel that passes its own argument through compiles to what it was with the body written in place.  Every file that
// includes this is compiled with -ffp-contract=off: each operation rounds to fp32 on its own.
#pragma once
#include "a3d_internal.h"

namespace a3d {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// the gradient as a rule sees it: a scale of exactly 1 multiplies nothing
__device__ __forceinline__ float scaled(float g, float gscale) { return gscale != 1.f ? __fmul_rn(g, gscale) : g; }

// ------------------------------------------------------------------ SGD with momentum (TF 1.3 ApplyMomentum, no Nesterov)
__device__ __forceinline__ void momentum_one(float& var, float& accum, float g, float lr, float mu) {
  accum = __fadd_rn(__fmul_rn(accum, mu), g);
  var = __fsub_rn(var, __fmul_rn(lr, accum));
}

// adam_body's shape: 16-byte vectors grid-strided, the count % 4 tail by block 0.  var, accum and g are hundreds of MB read
// once and written once: non-temporal, so that they do not push a GEMM's operands out of the L2 (optim.hip).
__device__ __forceinline__ void momentum_body(float* __restrict__ var, float* __restrict__ accum, const float* __restrict__ g,
                                              size_t count, float lr, float mu, float gscale) {
  const size_t nvec = count / 4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (size_t)gridDim.x * 256) {
    f32x4 w4 = __builtin_nontemporal_load(reinterpret_cast<f32x4*>(var) + i);
    f32x4 a4 = __builtin_nontemporal_load(reinterpret_cast<f32x4*>(accum) + i);
    const f32x4 g4 = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g) + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float wj = w4[j], aj = a4[j];
      momentum_one(wj, aj, scaled(g4[j], gscale), lr, mu);
      w4[j] = wj; a4[j] = aj;
    }
    __builtin_nontemporal_store(w4, reinterpret_cast<f32x4*>(var) + i);
    __builtin_nontemporal_store(a4, reinterpret_cast<f32x4*>(accum) + i);
  }
  if (blockIdx.x == 0) {
    const size_t i = nvec * 4 + threadIdx.x;
    if (i < count) momentum_one(var[i], accum[i], scaled(g[i], gscale), lr, mu);
  }
}

// ------------------------------------------------------------------ ApplyAdam (TF 1.3 formula)
__device__ __forceinline__ void adam_one(float& var, float& m, float& v, float g, float omb1, float omb2, float alpha,
                                         float eps) {
  m = __fadd_rn(m, __fmul_rn(__fsub_rn(g, m), omb1));
  v = __fadd_rn(v, __fmul_rn(__fsub_rn(__fmul_rn(g, g), v), omb2));
  // v_sqrt_f32 is 1-ulp, not correctly rounded, and hipcc emits it bare; the f64 square root rounded to f32 is
  // correctly rounded (53 >= 2*24+2 bits), which is what the numpy/Eigen reference computes.
  const float sq = (float)sqrt((double)v);
  var = __fsub_rn(var, __fdiv_rn(__fmul_rn(m, alpha), __fadd_rn(sq, eps)));
}

// what a3d_adam_apply_tf1_flag reports: the update CHANGED this value into a non-finite one (a NaN that stays a NaN, an
// infinity that stays that infinity: nothing the other ranks' copies lack)
__device__ __forceinline__ bool turned_non_finite(float before, float after) {
  return !isfinite(after) && !(after == before || (isnan(after) && isnan(before)));
}

__device__ __forceinline__ void adam_body(float* __restrict__ var, float* __restrict__ m, float* __restrict__ v,
                                          const float* __restrict__ g, size_t count, float omb1, float omb2, float alpha,
                                          float eps, float gscale, unsigned int* __restrict__ poisoned) {
  const size_t nvec = count / 4;
  bool bad = false;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (size_t)gridDim.x * 256) {
    f32x4 w4 = reinterpret_cast<f32x4*>(var)[i], m4 = reinterpret_cast<f32x4*>(m)[i];
    f32x4 v4 = reinterpret_cast<f32x4*>(v)[i], g4 = reinterpret_cast<const f32x4*>(g)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float gj = scaled(g4[j], gscale);
      float wj = w4[j], mj = m4[j], vj = v4[j];
      adam_one(wj, mj, vj, gj, omb1, omb2, alpha, eps);
      bad |= turned_non_finite(w4[j], wj) || turned_non_finite(v4[j], vj);
      w4[j] = wj; m4[j] = mj; v4[j] = vj;
    }
    reinterpret_cast<f32x4*>(var)[i] = w4;
    reinterpret_cast<f32x4*>(m)[i] = m4;
    reinterpret_cast<f32x4*>(v)[i] = v4;
  }
  if (blockIdx.x == 0) {
    const size_t i = nvec * 4 + threadIdx.x;
    if (i < count) {
      float gj = scaled(g[i], gscale);
      const float w0 = var[i], v0 = v[i];
      adam_one(var[i], m[i], v[i], gj, omb1, omb2, alpha, eps);
      bad |= turned_non_finite(w0, var[i]) || turned_non_finite(v0, v[i]);
    }
  }
  if (poisoned && bad) atomicOr(poisoned, 1u);
}

// ApplyAdam specialised for alpha == 0 and 1-beta2 == 0 — what the reference's AdamOptimizer(rate, 0.9, 1) always is
// (src/models.py:309).  Then v += (g*g - v)*0 and var -= (m*0)/(sqrt(v)+eps) leave v and var bit-identical unless a
// non-finite value poisons them (inf*0 = NaN), so only m needs the full read-modify-write: 3 HBM streams instead of
// 7.  Poisoned elements get exactly the NaNs the general formula would produce.  (Assumes v holds no +-inf from a
// foreign checkpoint; v is only ever written by these two bodies, which never produce one.)
// The element rule, in two parts: the new m ...
__device__ __forceinline__ float adam_frozen_m(float m, float g, float omb1) {
  return __fadd_rn(m, __fmul_rn(__fsub_rn(g, m), omb1));
}
// ... and the poison stores: v = NaN where g*g is not finite, var = NaN where that holds or the new m is not finite.  Returns
// whether a store changed something (turned_non_finite; the flag of adam_frozen_body).  A caller that drops the result
// reads neither var nor v.
__device__ __forceinline__ bool adam_frozen_poison(float& var, float& v, float g, float mn) {
  const bool g_poison = !isfinite(__fmul_rn(g, g));
  if (!g_poison && isfinite(mn)) return false;
  const bool changed = !isnan(var) || (g_poison && !isnan(v));
  const float qnan = __builtin_nanf("");
  if (g_poison) v = qnan;
  var = qnan;
  return changed;
}
__device__ __forceinline__ bool adam_frozen_one(float& var, float& m, float& v, float g, float omb1) {
  m = adam_frozen_m(m, g, omb1);
  return adam_frozen_poison(var, v, g, m);
}

// The rule on a piece of CW adjacent elements held in registers (the dense filter-gradient kernels: g, mo, mn are anything
// indexable).  The poison test is one sum per piece, returned — a non-finite term makes it non-finite — and the per-element
// work (adam_frozen_piece_poison) happens only behind !isfinite of it.  The caller stores mn: how is the kernel's business.
template <int CW, class G, class M, class O>
__device__ __forceinline__ float adam_frozen_piece(const G& g, const M& mo, O& mn, float omb1, float gscale) {
  float chk = 0.f;
#pragma unroll
  for (int j = 0; j < CW; ++j) {
    const float gj = scaled(g[j], gscale);
    mn[j] = adam_frozen_m(mo[j], gj, omb1);
    chk += __fmul_rn(gj, gj) + fabsf(mn[j]);
  }
  return chk;
}
template <int CW, class G, class O>
__device__ __forceinline__ void adam_frozen_piece_poison(float* __restrict__ var, float* __restrict__ v, const G& g, const O& mn,
                                                         float gscale) {
#pragma unroll
  for (int j = 0; j < CW; ++j) adam_frozen_poison(var[j], v[j], scaled(g[j], gscale), mn[j]);
}

__device__ __forceinline__ void adam_frozen_body(float* __restrict__ var, float* __restrict__ m, float* __restrict__ v,
                                                 const float* __restrict__ g, size_t count, float omb1, float gscale,
                                                 unsigned int* __restrict__ poisoned) {
  const size_t nvec = count / 4;
  bool bad = false;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (size_t)gridDim.x * 256) {
    f32x4 m4 = reinterpret_cast<f32x4*>(m)[i], g4 = reinterpret_cast<const f32x4*>(g)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float gj = scaled(g4[j], gscale);
      m4[j] = adam_frozen_m(m4[j], gj, omb1);
      bad |= adam_frozen_poison(var[4 * i + j], v[4 * i + j], gj, m4[j]);      // rare
    }
    reinterpret_cast<f32x4*>(m)[i] = m4;
  }
  if (blockIdx.x == 0) {
    const size_t i = nvec * 4 + threadIdx.x;
    if (i < count) bad |= adam_frozen_one(var[i], m[i], v[i], scaled(g[i], gscale), omb1);
  }
  if (poisoned && bad) atomicOr(poisoned, 1u);      // rare: a non-finite gradient reached this slice
}

// ------------------------------------------------------------------ gradient descent (tf.train.GradientDescentOptimizer)
__device__ __forceinline__ void sgd_body(float* __restrict__ var, const float* __restrict__ g, size_t count, float lr) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256)
    var[i] = __fsub_rn(var[i], __fmul_rn(lr, g[i]));
}

// projected gradient descent: sgd_body's step, then no lower than `floor`.  The comparison keeps a NaN a NaN.
__device__ __forceinline__ void sgd_floor_body(float* __restrict__ var, const float* __restrict__ g, size_t count, float lr,
                                               float floor) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) {
    const float v = __fsub_rn(var[i], __fmul_rn(lr, g[i]));
    var[i] = v < floor ? floor : v;
  }
}

// ------------------------------------------------------------------ host side, shared by an entry point and its _ctl form
// the grids the rules have always been launched on
inline unsigned rule_grid_vec(size_t count) { return grid_for(count / 4 + 1, 256, 4096); }                    // momentum, Adam
inline unsigned rule_grid_scalar(size_t count) { return (unsigned)std::min<size_t>((count + 255) / 256, 4096); }   // gradient descent

// ApplyAdam's host scalars: alpha, and whether the launch is the frozen kernel's (alpha == 0 and 1 - beta2 == 0)
struct AdamHost { float alpha; bool frozen; };
inline AdamHost adam_host(float lr, float beta2, float beta1_power, float beta2_power) {
  const float alpha = lr * sqrtf(1.f - beta2_power) / (1.f - beta1_power);
  return {alpha, alpha == 0.f && 1.f - beta2 == 0.f};
}

}  // namespace a3d
