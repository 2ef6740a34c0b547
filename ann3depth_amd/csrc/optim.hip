// optim.hip — SGD with momentum (include/a3d_optim.h, NON-REFERENCE, --optimizer momentum): TensorFlow 1.3's ApplyMomentum
// without Nesterov, as a streaming kernel over a flat parameter group and fused into the dense layers' filter gradient.
//   g' = grad_scale == 1 ? g : g * grad_scale;   accum' = accum * momentum + g';   var' = var - lr * accum'
// This file is compiled with -ffp-contract=off (see Makefile): every operation rounds to fp32 on its own, so the kernels are
// bit-exact against the numpy restatement (tests/momentum_ref.py) and the fused launch against the two-call form.
// var, accum and g are hundreds of MB read once and written once: their accesses are non-temporal (igemm.h, kAuxStream),
// so that they do not push the operands a GEMM of the other stream re-reads out of the L2.
#include "a3d_internal.h"
#include "dense_dw.h"
#include "igemm.h"
#include "optim_rules.h"
#include "../../include/a3d_optim.h"

using namespace a3d;

namespace a3d {

// momentum_one and the walk of a flat group (momentum_body): optim_rules.h, shared with the launch that takes its scale from a
// gradient-norm control block (clip.hip)
__global__ __launch_bounds__(256) void momentum_kernel(float* __restrict__ var, float* __restrict__ accum,
                                                       const float* __restrict__ g, size_t count, float lr, float mu,
                                                       float gscale) {
  momentum_body(var, accum, g, count, lr, mu, gscale);
}

// dense_dw_kernel's contraction (dense_dw.h) at CW = 2, with the momentum rule in its epilogue: a wave owns 32 weight rows x 64
// columns, lane li takes dz[m][n0 + 2 li .. + 1] with one 8-byte load and feeds two fp32 MFMA 32x32x2 (the batch is the contraction
// axis, in ascending order: dense_dw_launch's sum, bit for bit), and register v of the two accumulators is two adjacent columns of
// row row_of(v).  The wave's accum AND var tiles (2 x 16 registers of two floats) are requested before the contraction starts, so
// their HBM latency passes under the operand loads (x and dz: L2-resident) and the MFMAs.  No LDS.  Rows of an odd n are
// 4-byte aligned only: the two-float type is aligned(4), and the lanes across the last column take the scalar path.
// GEMM_ORDER: the batch rows in the order of the implicit-GEMM route, which is what a3d_dense_bwd_filter runs below k n = 2^16:
// the two-call form's bits there too.
template <bool GEMM_ORDER>
__global__ __launch_bounds__(256) void dense_dw_momentum_kernel(const float* __restrict__ x, const float* __restrict__ dz,
                                                                float* __restrict__ var_w, float* __restrict__ acc_w,
                                                                float* __restrict__ var_b, float* __restrict__ acc_b,
                                                                int M, int K, int N, float lr, float mu, float gscale) {
  constexpr int CW = 2;
  typedef VecOf<CW>::type vec;
  const DwTile<CW> t(N);

  // BiasAddGrad and its step: the blocks of the first row group, one column per thread
  if (blockIdx.y == 0 && t.tid < 32 * CW && t.n0 + t.tid < N && acc_b != nullptr) {
    const int col = t.n0 + t.tid;
    momentum_one(var_b[col], acc_b[col], scaled(colsum_rows(dz, M, N, col), gscale), lr, mu);
  }
  if (t.k0 >= K) return;      // wave-uniform

  // Branch-free: a lane without a whole piece in row_of(v) reads the piece at element 0 instead and never uses it (sixteen
  // conditional loads ahead of the loop made the register allocator spill the accumulators).  A 1 x 1 matrix has no piece.
  vec aold[16], wold[16];
#pragma unroll
  for (int v = 0; v < 16; ++v) aold[v] = wold[v] = vec{0.f, 0.f};
  if ((size_t)K * N >= 2) {      // uniform
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int row = t.row_of(v);
      const size_t o = (row < K && t.cfull) ? (size_t)row * N + t.col0 : 0;
      aold[v] = __builtin_nontemporal_load(reinterpret_cast<const vec*>(acc_w + o));
      wold[v] = __builtin_nontemporal_load(reinterpret_cast<const vec*>(var_w + o));
    }
  }

  f32x16 acc[CW];
  dw_contract<CW, GEMM_ORDER>(t, x, dz, M, K, N, acc);

  // epilogue: register v of the two accumulators = two adjacent columns of row row_of(v)
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int row = t.row_of(v);
    if (row >= K) continue;
    const size_t o = (size_t)row * N + t.col0;
    if (t.cfull) {
      vec an = aold[v], wn = wold[v];
#pragma unroll
      for (int j = 0; j < CW; ++j) {
        float wj = wn[j], aj = an[j];
        momentum_one(wj, aj, scaled(acc[j][v], gscale), lr, mu);
        wn[j] = wj; an[j] = aj;
      }
      __builtin_nontemporal_store(an, reinterpret_cast<vec*>(acc_w + o));
      __builtin_nontemporal_store(wn, reinterpret_cast<vec*>(var_w + o));
    } else {
#pragma unroll
      for (int j = 0; j < CW; ++j)
        if (t.col0 + j < N) momentum_one(var_w[o + j], acc_w[o + j], scaled(acc[j][v], gscale), lr, mu);
    }
  }
}

}  // namespace a3d

extern "C" {

int a3do_momentum_apply(size_t count, float* var, float* accum, const float* g, float lr, float momentum, float grad_scale,
                        void* stream) {
  A3D_CHECK_ARG(count > 0 && var && accum && g, "momentum_apply: bad arguments");
  A3D_CHECK_ARG(((reinterpret_cast<uintptr_t>(var) | reinterpret_cast<uintptr_t>(accum) | reinterpret_cast<uintptr_t>(g)) & 15) == 0,
                "momentum_apply: buffers must be 16-byte aligned");
  clear_stale_error();
  hipLaunchKernelGGL(momentum_kernel, dim3(rule_grid_vec(count)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     var, accum, g, count, lr, momentum, grad_scale);
  return check_launch("momentum_apply");
}

int a3do_dense_bwd_filter_momentum(int m, int k, int n, const float* x, const float* dz, float* var_w, float* accum_w,
                                   float* var_b, float* accum_b, float lr, float momentum, float grad_scale, void* stream) {
  A3D_CHECK_ARG(m > 0 && k > 0 && n > 0 && x && dz && var_w && accum_w, "dense_bwd_filter_momentum: bad arguments");
  A3D_CHECK_ARG((var_b && accum_b) || (!var_b && !accum_b), "dense_bwd_filter_momentum: the bias and its accumulator come as a pair");
  A3D_CHECK_ARG(dense_dw_applicable(m, k, n),
                "dense_bwd_filter_momentum: batches of at most 64 rows only; otherwise call a3d_dense_bwd_filter and "
                "a3do_momentum_apply");
  A3D_CHECK_ARG(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(dz) | reinterpret_cast<uintptr_t>(var_w) |
                  reinterpret_cast<uintptr_t>(accum_w) | reinterpret_cast<uintptr_t>(var_b) | reinterpret_cast<uintptr_t>(accum_b)) & 3) == 0,
                "dense_bwd_filter_momentum: tensors must be 4-byte aligned");
  clear_stale_error();
  const dim3 grid((n + 63) / 64, (k + 127) / 128);
  // a3d_dense_bwd_filter's own dispatch: the dense kernel from k n = 2^16 on, the implicit-GEMM route below
  if ((long)k * n >= (1L << 16))
    hipLaunchKernelGGL(dense_dw_momentum_kernel<false>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), x, dz, var_w, accum_w,
                       var_b, accum_b, m, k, n, lr, momentum, grad_scale);
  else
    hipLaunchKernelGGL(dense_dw_momentum_kernel<true>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), x, dz, var_w, accum_w,
                       var_b, accum_b, m, k, n, lr, momentum, grad_scale);
  return check_launch("dense_dw_momentum");
}

}  // extern "C"
