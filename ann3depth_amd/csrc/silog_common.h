// silog_common.h — what the scale-invariant log loss kernels of pointwise.hip (plain and masked) and of gradloss.hip (with the
// gradient-matching term) share: the logarithm with tf.where's NaN rule, the wavefront sums, the number of parts per sample and
// the reference's folded constant.  Both files are compiled with -ffp-contract=off; the bits of d = masked_log(o) - masked_log(t)
// and the order of the sums are the same in every kernel that includes this.
#pragma once
#include "a3d_internal.h"

namespace a3d {

constexpr int kSilogParts = A3D_SILOG_PARTS;
static const float kSilogC = (float)(0.5 / (74 * 55));   // src/models.py:269, folded constant

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

__device__ __forceinline__ float masked_log(float v) {
  float l = logf(__fadd_rn(v, 1e-8f));
  return isnan(l) ? 0.f : l;     // tf.where(tf.is_nan(log), 0, log): -inf is kept
}

}  // namespace a3d
