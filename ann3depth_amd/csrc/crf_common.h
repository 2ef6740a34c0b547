// crf_common.h — what the dense CRF kernels of crf.hip and the banded ones of crf_band.hip share: the wavefront sum, the
// mean of a batch's losses and the likelihoods' constant; and the colour histogram's bin, which slic.hip uses as well.  All
// three files are compiled with -ffp-contract=off.
#pragma once
#include "a3d_internal.h"

namespace a3d {

constexpr float kHalfLogPi = 0.57236494292470009f;

// xor butterfly, offsets 32 .. 1: every lane ends with the same sum
__device__ __forceinline__ float wave_sum_f(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// color_histogram's bin of one RGB pixel (src/models.py:95-100): 256 bins of r*2^24 + g*2^16 + b*2^8 over [0, 2^24), a
// value outside (or NaN) clamped into the end bins.  superpixel_hist_kernel (crf.hip) and label_hist_kernel (slic.hip).
__device__ __forceinline__ int colour_bin(const float* __restrict__ px) {
  const float v = __fadd_rn(__fadd_rn(__fmul_rn(px[0], 16777216.f), __fmul_rn(px[1], 65536.f)), __fmul_rn(px[2], 256.f));
  const float scaled = __fdiv_rn(v, 16777216.f);
  const int idx = (int)floorf(__fmul_rn(256.f, scaled));
  return min(max(idx, 0), 255);
}

// out[0] = the mean of v[0 .. n): one wavefront, lane i adds v[i], v[i + 64], ... in order, then the butterfly.  Internal
// linkage: each file that includes this launches its own copy.
static __global__ __launch_bounds__(64) void mean_kernel(const float* __restrict__ v, int n, float* __restrict__ out) {
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 64) s += v[i];
  s = wave_sum_f(s);
  if (threadIdx.x == 0) out[0] = s / (float)n;
}

}  // namespace a3d
