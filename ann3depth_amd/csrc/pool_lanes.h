// pool_lanes.h — how the lanes of the pooling kernels (sppool.hip, slic.hip) move their channels: 16 bytes per lane where
// C, the strides and the base pointers allow, one float otherwise.
#pragma once
#include "a3d_internal.h"

namespace a3d {

template <int VEC>
__device__ inline void load(const float* p, float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  } else {
    v[0] = *p;
  }
}

template <int VEC>
__device__ inline void store(float* p, const float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    *p = v[0];
  }
}

inline bool vec4_ok(int C, int ld, int ldp, const void* a, const void* b) {
  return C % 4 == 0 && ld % 4 == 0 && ldp % 4 == 0 && aligned16(a) && aligned16(b);
}

}  // namespace a3d
