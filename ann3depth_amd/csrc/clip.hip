// clip.hip — gradient clipping by global norm, per optimizer group (include/a3d_clip.h, NON-REFERENCE, --clip-norm): one launch
// that reduces a flat gradient to S = sum g^2 in float64 and leaves n, scale and skip in a 32-byte control block on the device,
// and the four optimizer rules (optim_rules.h: the bodies the existing kernels run) launched with that block in place of the
// host's grad_scale.  The reduction is loss_common.h's: per-thread accumulators -> wave_sum -> ((w0 + w1) + w2) + w3 -> one
// 8-byte agent-scope store per block -> the block whose ticket came last adds the partials in a fixed order.  No floating-point
// atomics, no block waits for another, no trip count depends on a value: the same bits on every run.
// This file is compiled with -ffp-contract=off (see Makefile), like optim.hip.
#include <math.h>

#include "a3d_internal.h"
#include "loss_common.h"
#include "optim_rules.h"
#include "../../include/a3d_clip.h"

using namespace a3d;

namespace a3d {

struct ClipCtl {      // include/a3d_clip.h: the control block
  double sumsq;
  float norm, scale;
  unsigned skip, skipped;
  unsigned reserved[2];
};
static_assert(sizeof(ClipCtl) == A3DN_CTL_BYTES, "the control block is 32 bytes");

constexpr int kClipUnroll = 4;                                   // 16-byte loads a thread keeps in flight, one accumulator each
constexpr size_t kClipBlockVecs = 256 * kClipUnroll;             // vectors of one sweep of a block
static_assert(kClipBlockVecs * 4 == A3DN_BLOCK_ELEMS, "the header states the block's capacity");
static_assert(A3DN_MAX_BLOCKS == 4 * 256, "the last block folds four partials per thread");

// workspace: [0] the ticket (8 bytes), then one float64 per block
inline unsigned clip_grid(size_t count) {
  return (unsigned)std::min<size_t>(std::max<size_t>((count / 4 + kClipBlockVecs - 1) / kClipBlockVecs, 1), A3DN_MAX_BLOCKS);
}

// g is read with ordinary loads.  -DA3D_CLIP_NT is the diagnostic build it was measured against, never shipped:
// the same kernel with the non-temporal bit on every load of g
#ifdef A3D_CLIP_NT
#define A3D_CLIP_LOAD(p) __builtin_nontemporal_load(p)
#else
#define A3D_CLIP_LOAD(p) (*(p))
#endif

__device__ __forceinline__ double sumsq4(double acc, f32x4 q) {
#pragma unroll
  for (int j = 0; j < 4; ++j) acc += (double)q[j] * (double)q[j];      // the product is exact (48 bits); the sum rounds
  return acc;
}

__global__ __launch_bounds__(256) void grad_norm_kernel(const float* __restrict__ g, size_t count, float gs, float clip,
                                                        ClipCtl* __restrict__ ctl, unsigned* __restrict__ ticket,
                                                        double* __restrict__ partials) {
  __shared__ double red[4];
  const size_t nvec = count / 4;
  const size_t per = (nvec + gridDim.x - 1) / gridDim.x;
  const size_t lo = std::min(nvec, per * blockIdx.x), hi = std::min(nvec, lo + per);
  const f32x4* __restrict__ g4 = reinterpret_cast<const f32x4*>(g);
  double acc[kClipUnroll];
#pragma unroll
  for (int u = 0; u < kClipUnroll; ++u) acc[u] = 0.0;
  for (size_t i = lo + threadIdx.x; i < hi; i += kClipBlockVecs) {
    f32x4 q[kClipUnroll];
#pragma unroll
    for (int u = 0; u < kClipUnroll; ++u) q[u] = i + 256 * u < hi ? A3D_CLIP_LOAD(g4 + i + 256 * u) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < kClipUnroll; ++u) acc[u] = sumsq4(acc[u], q[u]);
  }
  double s = ((acc[0] + acc[1]) + acc[2]) + acc[3];
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0)      // the count % 4 tail, behind the last block's vectors
    for (size_t i = nvec * 4; i < count; ++i) s += (double)g[i] * (double)g[i];
  block_put(red, wave_sum(s));
  __syncthreads();
  if (threadIdx.x == 0)
    __hip_atomic_store(&partials[blockIdx.x], block_sum64(red), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (!arrive_of(ticket, gridDim.x)) return;

  // the last block to arrive: thread t takes the partials of blocks 4t .. 4t + 3 in ascending order (agent-scope loads,
  // past this CU's L1), then the same two levels as above
  double p[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned b = 4 * threadIdx.x + k;
    p[k] = b < gridDim.x ? __hip_atomic_load(&partials[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
  }
  block_put(red, wave_sum(((p[0] + p[1]) + p[2]) + p[3]));
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double S = block_sum64(red);
  const double n = fabs((double)gs) * sqrt(S);
  const bool skip = !isfinite(S);
  ctl->sumsq = S;
  ctl->norm = (float)n;
  ctl->scale = skip ? 0.f : n > (double)clip ? (float)((double)gs * (double)clip / n) : gs;
  ctl->skip = skip ? 1u : 0u;
  if (skip) ctl->skipped += 1u;      // one lane of one block per launch, launches stream-ordered: no atomic needed
}

// ------------------------------------------------------------------ the four rules under a control block
// skip and scale are uniform: every thread reads the same two words, written by an earlier launch of the same stream
__global__ __launch_bounds__(256) void momentum_ctl_kernel(float* __restrict__ var, float* __restrict__ accum,
                                                           const float* __restrict__ g, size_t count, float lr, float mu,
                                                           const ClipCtl* __restrict__ ctl) {
  if (ctl->skip != 0u) return;
  momentum_body(var, accum, g, count, lr, mu, ctl->scale);
}

__global__ __launch_bounds__(256) void adam_ctl_kernel(float* __restrict__ var, float* __restrict__ m, float* __restrict__ v,
                                                       const float* __restrict__ g, size_t count, float omb1, float omb2,
                                                       float alpha, float eps, const ClipCtl* __restrict__ ctl,
                                                       unsigned int* __restrict__ poisoned) {
  if (ctl->skip != 0u) return;
  adam_body(var, m, v, g, count, omb1, omb2, alpha, eps, ctl->scale, poisoned);
}

__global__ __launch_bounds__(256) void adam_frozen_ctl_kernel(float* __restrict__ var, float* __restrict__ m,
                                                              float* __restrict__ v, const float* __restrict__ g,
                                                              size_t count, float omb1, const ClipCtl* __restrict__ ctl,
                                                              unsigned int* __restrict__ poisoned) {
  if (ctl->skip != 0u) return;
  adam_frozen_body(var, m, v, g, count, omb1, ctl->scale, poisoned);
}

__global__ __launch_bounds__(256) void sgd_ctl_kernel(float* __restrict__ var, const float* __restrict__ g, size_t count,
                                                      float lr, const ClipCtl* __restrict__ ctl) {
  if (ctl->skip != 0u) return;
  sgd_body(var, g, count, __fmul_rn(lr, ctl->scale));
}

__global__ __launch_bounds__(256) void sgd_floor_ctl_kernel(float* __restrict__ var, const float* __restrict__ g, size_t count,
                                                            float lr, float floor, const ClipCtl* __restrict__ ctl) {
  if (ctl->skip != 0u) return;
  sgd_floor_body(var, g, count, __fmul_rn(lr, ctl->scale), floor);
}

inline bool on_grid(const void* p, uintptr_t grid) { return (reinterpret_cast<uintptr_t>(p) & (grid - 1)) == 0; }

}  // namespace a3d

// the control block of a *_ctl entry point: there, and on the 8-byte grid
#define A3DN_CHECK_CTL(who)                                                                         \
  do {                                                                                              \
    A3D_CHECK_ARG(ctl != nullptr, who ": no control block");                                        \
    A3D_CHECK_ARG(on_grid(ctl, 8), who ": the control block must be 8-byte aligned");               \
  } while (0)

extern "C" {

size_t a3dn_grad_norm_ws_bytes(size_t count) { return up256(8 + sizeof(double) * clip_grid(count)); }

int a3dn_grad_norm_scale(size_t count, const float* g, float grad_scale, float clip_norm, void* ctl, void* ws, size_t ws_bytes,
                         void* stream) {
  A3D_CHECK_ARG(g && ctl && ws, "grad_norm_scale: bad arguments: a NULL pointer");
  A3D_CHECK_ARG(count > 0, "grad_norm_scale: bad arguments: no elements");
  A3D_CHECK_ARG(on_grid(g, 16), "grad_norm_scale: the gradient must be 16-byte aligned");
  A3D_CHECK_ARG(on_grid(ctl, 8) && on_grid(ws, 8), "grad_norm_scale: the control block and the workspace must be 8-byte aligned");
  A3D_CHECK_ARG(isfinite(grad_scale) && grad_scale != 0.f, "grad_norm_scale: grad_scale %g must be finite and not 0",
                (double)grad_scale);
  A3D_CHECK_ARG(clip_norm > 0.f, "grad_norm_scale: clip_norm %g must be > 0 (+inf: measure and skip only)", (double)clip_norm);
  const size_t need = a3dn_grad_norm_ws_bytes(count);
  if (ws_bytes < need) return set_error(A3D_EWORKSPACE, "grad_norm_scale: need %zu workspace bytes, got %zu", need, ws_bytes);
  clear_stale_error();
  hipLaunchKernelGGL(grad_norm_kernel, dim3(clip_grid(count)), dim3(256), 0, static_cast<hipStream_t>(stream), g, count,
                     grad_scale, clip_norm, static_cast<ClipCtl*>(ctl), static_cast<unsigned*>(ws),
                     reinterpret_cast<double*>(static_cast<char*>(ws) + 8));
  return check_launch("grad_norm_scale");
}

int a3dn_momentum_apply_ctl(size_t count, float* var, float* accum, const float* g, float lr, float momentum, const void* ctl,
                            void* stream) {
  A3D_CHECK_ARG(count > 0 && var && accum && g, "momentum_apply_ctl: bad arguments");
  A3D_CHECK_ARG(((reinterpret_cast<uintptr_t>(var) | reinterpret_cast<uintptr_t>(accum) | reinterpret_cast<uintptr_t>(g)) & 15) == 0,
                "momentum_apply_ctl: buffers must be 16-byte aligned");
  A3DN_CHECK_CTL("momentum_apply_ctl");
  clear_stale_error();
  hipLaunchKernelGGL(momentum_ctl_kernel, dim3(rule_grid_vec(count)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     var, accum, g, count, lr, momentum, static_cast<const ClipCtl*>(ctl));
  return check_launch("momentum_apply_ctl");
}

int a3dn_adam_apply_tf1_ctl(size_t count, float* var, float* m, float* v, const float* g, float lr, float beta1, float beta2,
                            float eps, float beta1_power, float beta2_power, const void* ctl, unsigned int* poisoned,
                            void* stream) {
  A3D_CHECK_ARG(count > 0 && var && m && v && g, "adam_ctl: bad arguments");
  A3D_CHECK_ARG(((reinterpret_cast<uintptr_t>(var) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v) |
                  reinterpret_cast<uintptr_t>(g)) & 15) == 0, "adam_ctl: buffers must be 16-byte aligned");
  A3DN_CHECK_CTL("adam_ctl");
  const AdamHost h = adam_host(lr, beta2, beta1_power, beta2_power);
  clear_stale_error();
  if (h.frozen) {
    hipLaunchKernelGGL(adam_frozen_ctl_kernel, dim3(rule_grid_vec(count)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       var, m, v, g, count, 1.f - beta1, static_cast<const ClipCtl*>(ctl), poisoned);
    return check_launch("adam_frozen_ctl");
  }
  hipLaunchKernelGGL(adam_ctl_kernel, dim3(rule_grid_vec(count)), dim3(256), 0, static_cast<hipStream_t>(stream), var, m, v, g,
                     count, 1.f - beta1, 1.f - beta2, h.alpha, eps, static_cast<const ClipCtl*>(ctl), poisoned);
  return check_launch("adam_ctl");
}

int a3dn_sgd_apply_ctl(size_t count, float* var, const float* g, float lr, const void* ctl, void* stream) {
  A3D_CHECK_ARG(count > 0 && var && g, "sgd_ctl: bad arguments");
  A3DN_CHECK_CTL("sgd_ctl");
  clear_stale_error();
  hipLaunchKernelGGL(sgd_ctl_kernel, dim3(rule_grid_scalar(count)), dim3(256), 0, static_cast<hipStream_t>(stream), var, g,
                     count, lr, static_cast<const ClipCtl*>(ctl));
  return check_launch("sgd_ctl");
}

int a3dn_sgd_apply_floor_ctl(size_t count, float* var, const float* g, float lr, float floor, const void* ctl, void* stream) {
  A3D_CHECK_ARG(count > 0 && var && g, "sgd_floor_ctl: bad arguments");
  A3DN_CHECK_CTL("sgd_floor_ctl");
  clear_stale_error();
  hipLaunchKernelGGL(sgd_floor_ctl_kernel, dim3(rule_grid_scalar(count)), dim3(256), 0, static_cast<hipStream_t>(stream), var,
                     g, count, lr, floor, static_cast<const ClipCtl*>(ctl));
  return check_launch("sgd_floor_ctl");
}

}  // extern "C"
