// sppool.hip — superpixel pooling of a feature map and its transpose (include/a3d_fcsp.h; NON-REFERENCE, --unary fcsp):
// what stands between the last conv map of DCNF's fully convolutional unary and its dense head.
//
// Both kernels move each byte once and are bound by HBM; the lanes run along the channels (innermost in memory), 16 bytes
// per lane where C, the strides and the base pointers allow, one float otherwise.  A superpixel window touches only a few
// cells per axis, so what a block needs of the tables is a handful of integer counts: they are formed once per block in
// LDS, by integer arithmetic only, and every lane's float sum then runs over them in the order the header states.  Built
// with -ffp-contract=off; the operations are spelled with the __f*_rn intrinsics all the same.
#include "a3d_internal.h"
#include "../../include/a3d_fcsp.h"
#include "pool_lanes.h"

namespace a3d {
namespace {

constexpr int kMaxSp = A3DF_MAX_SP;
constexpr int kChunk = 64;      // superpixel rows / columns whose counts the backward holds at a time

// One block per (image, superpixel) and per blockDim.x * VEC channels (gridDim.y).  Per axis the block reduces the
// window's sp table entries to the ascending list of its distinct in-range cells and their counts; arbitrary tables
// (entries out of range, not monotone) cost nothing extra.
template <int VEC>
__global__ __launch_bounds__(256) void superpixel_pool_fwd_kernel(const float* __restrict__ feat, float* __restrict__ pooled,
                                                                  const int32_t* __restrict__ ymap,
                                                                  const int32_t* __restrict__ xmap, int h, int w, int C,
                                                                  int ld, int ldp, int SR, int SC, int sp) {
  __shared__ int s_val[2][kMaxSp], s_first[2][kMaxSp], s_idx[2][kMaxSp], s_cnt[2][kMaxSp], s_n[2];
  const int S = SR * SC;
  const int b = blockIdx.x / S, s = blockIdx.x % S;
  const int R = s / SC, Cc = s % SC;
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int t = tid; t < 2 * sp; t += nt) {
    const int axis = t >= sp, k = t - axis * sp;
    const int v = axis ? xmap[Cc * sp + k] : ymap[R * sp + k];
    s_val[axis][k] = (v >= 0 && v < (axis ? w : h)) ? v : -1;
  }
  if (tid < 2) s_n[tid] = 0;
  __syncthreads();
  for (int t = tid; t < 2 * sp; t += nt) {
    const int axis = t >= sp, k = t - axis * sp;
    const int v = s_val[axis][k];
    int first = v >= 0;
    for (int q = 0; q < k; ++q) first &= s_val[axis][q] != v;
    s_first[axis][k] = first;
  }
  __syncthreads();
  for (int t = tid; t < 2 * sp; t += nt) {
    const int axis = t >= sp, k = t - axis * sp;
    if (!s_first[axis][k]) continue;
    const int v = s_val[axis][k];
    int rank = 0, count = 0;
    for (int q = 0; q < sp; ++q) {
      const int u = s_val[axis][q];
      count += u == v;
      rank += s_first[axis][q] && u < v;
    }
    s_idx[axis][rank] = v;
    s_cnt[axis][rank] = count;
    atomicAdd(&s_n[axis], 1);
  }
  __syncthreads();
  const int g = blockIdx.y * nt + tid;
  if (g >= C / VEC) return;
  const int c = g * VEC;
  const int ny = s_n[0], nx = s_n[1];
  const float* fb = feat + (size_t)b * h * w * ld + c;
  float acc[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
  for (int a = 0; a < ny; ++a) {
    const float* row = fb + (size_t)s_idx[0][a] * w * ld;
    const int cy = s_cnt[0][a];
    for (int e = 0; e < nx; ++e) {
      const float wgt = (float)(cy * s_cnt[1][e]);
      float v[VEC];
      load<VEC>(row + (size_t)s_idx[1][e] * ld, v);
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc[k] = __fadd_rn(acc[k], __fmul_rn(wgt, v[k]));
    }
  }
  const float div = (float)(sp * sp);
#pragma unroll
  for (int k = 0; k < VEC; ++k) acc[k] = __fdiv_rn(acc[k], div);
  store<VEC>(pooled + ((size_t)b * S + s) * ldp + c, acc);
}

// counts[q] = #{ p in [q sp, (q + 1) sp) : map[p] == target } for q < nq <= kChunk: integer LDS atomics, so the same
// numbers in any order.  The leading barrier lets the lanes that still read the previous contents finish.
__device__ inline void count_chunk(int* counts, const int32_t* __restrict__ map, int nq, int sp, int target) {
  __syncthreads();
  for (int q = threadIdx.x; q < nq; q += blockDim.x) counts[q] = 0;
  __syncthreads();
  for (int p = threadIdx.x; p < nq * sp; p += blockDim.x)
    if (map[p] == target) atomicAdd(&counts[p / sp], 1);
  __syncthreads();
}

// One block per (image, cell) and per blockDim.x * VEC channels: a gather over the superpixels in ascending order.  The
// counts of the cell's row in kChunk superpixel rows, and of its column in kChunk superpixel columns, stand in LDS; with
// at most kChunk superpixels per axis (48 = 6 x 8 in the model) each is formed once.  Every branch around a barrier
// depends on LDS counts and launch arguments alone, the same in every lane.
template <int VEC>
__global__ __launch_bounds__(256) void superpixel_pool_bwd_kernel(const float* __restrict__ dpooled, float* __restrict__ dfeat,
                                                                  const int32_t* __restrict__ ymap,
                                                                  const int32_t* __restrict__ xmap, int h, int w, int C,
                                                                  int ld, int ldp, int SR, int SC, int sp) {
  __shared__ int s_cy[kChunk], s_cx[kChunk];
  const int S = SR * SC;
  const int b = blockIdx.x / (h * w), cell = blockIdx.x % (h * w);
  const int i = cell / w, j = cell % w;
  const int g = blockIdx.y * blockDim.x + threadIdx.x;
  const bool active = g < C / VEC;
  const int c = g * VEC;
  const float* db = dpooled + (size_t)b * S * ldp + c;
  float acc[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
  int cx_base = -1;
  for (int R0 = 0; R0 < SR; R0 += kChunk) {
    const int nr = min(kChunk, SR - R0);
    count_chunk(s_cy, ymap + (size_t)R0 * sp, nr, sp, i);
    for (int r = 0; r < nr; ++r) {
      const int cy = s_cy[r];
      if (cy == 0) continue;
      for (int C0 = 0; C0 < SC; C0 += kChunk) {
        const int nc = min(kChunk, SC - C0);
        if (cx_base != C0) {
          count_chunk(s_cx, xmap + (size_t)C0 * sp, nc, sp, j);
          cx_base = C0;
        }
        if (!active) continue;
        const float* row = db + ((size_t)(R0 + r) * SC + C0) * ldp;
        for (int e = 0; e < nc; ++e) {
          const int cx = s_cx[e];
          if (cx == 0) continue;
          const float wgt = (float)(cy * cx);
          float v[VEC];
          load<VEC>(row + (size_t)e * ldp, v);
#pragma unroll
          for (int k = 0; k < VEC; ++k) acc[k] = __fadd_rn(acc[k], __fmul_rn(wgt, v[k]));
        }
      }
    }
  }
  if (!active) return;
  const float div = (float)(sp * sp);
#pragma unroll
  for (int k = 0; k < VEC; ++k) acc[k] = __fdiv_rn(acc[k], div);
  store<VEC>(dfeat + ((size_t)b * h * w + cell) * ld + c, acc);
}

// What both entry points refuse.  The (image, superpixel) and (image, cell) blocks have to fit gridDim.x, the channel
// passes gridDim.y.
int pool_args(const char* who, int n, int h, int w, int C, const void* a, const void* b, int ld, int ldp, int H, int W, int sp,
              const int32_t* ymap, const int32_t* xmap) {
  A3D_CHECK_ARG(a && b && ymap && xmap, "%s: NULL pointer", who);
  A3D_CHECK_ARG(n > 0 && h > 0 && w > 0 && C > 0 && H > 0 && W > 0 && sp > 0, "%s: n, h, w, C, H, W, sp must be positive", who);
  A3D_CHECK_ARG(sp <= kMaxSp, "%s: superpixel edge %d above A3DF_MAX_SP = %d", who, sp, kMaxSp);
  A3D_CHECK_ARG(H % sp == 0 && W % sp == 0, "%s: H = %d, W = %d are not multiples of sp = %d", who, H, W, sp);
  A3D_CHECK_ARG(ld >= C && ldp >= C, "%s: strides ld = %d, ldp = %d below C = %d", who, ld, ldp, C);
  const long long cells = (long long)n * h * w, sps = (long long)n * (H / sp) * (W / sp);
  A3D_CHECK_ARG(cells <= 0x7fffffffLL && sps <= 0x7fffffffLL && (long long)h * w <= 0x7fffffffLL,
                "%s: more than 2^31 - 1 cells or superpixels", who);
  A3D_CHECK_ARG(C <= (1 << 22), "%s: C = %d above 2^22", who, C);
  return A3D_OK;
}

}  // namespace
}  // namespace a3d

using namespace a3d;

extern "C" {

int a3df_superpixel_pool_fwd(int n, int h, int w, int C, const float* feat, int ld, int H, int W, int sp,
                             const int32_t* ymap, const int32_t* xmap, float* pooled, int ldp, void* stream) {
  int rc = pool_args("superpixel_pool_fwd", n, h, w, C, feat, pooled, ld, ldp, H, W, sp, ymap, xmap);
  if (rc != A3D_OK) return rc;
  const bool vec = vec4_ok(C, ld, ldp, feat, pooled);
  const int groups = vec ? C / 4 : C;
  const int threads = std::min(256, (groups + 63) / 64 * 64);
  const dim3 grid(n * (H / sp) * (W / sp), (groups + threads - 1) / threads);
  clear_stale_error();
  hipLaunchKernelGGL(vec ? superpixel_pool_fwd_kernel<4> : superpixel_pool_fwd_kernel<1>, grid, dim3(threads), 0,
                     static_cast<hipStream_t>(stream), feat, pooled, ymap, xmap, h, w, C, ld, ldp, H / sp, W / sp, sp);
  return check_launch("superpixel_pool_fwd");
}

int a3df_superpixel_pool_bwd(int n, int h, int w, int C, const float* dpooled, int ldp, int H, int W, int sp,
                             const int32_t* ymap, const int32_t* xmap, float* dfeat, int ld, void* stream) {
  int rc = pool_args("superpixel_pool_bwd", n, h, w, C, dpooled, dfeat, ld, ldp, H, W, sp, ymap, xmap);
  if (rc != A3D_OK) return rc;
  const bool vec = vec4_ok(C, ld, ldp, dpooled, dfeat);
  const int groups = vec ? C / 4 : C;
  const int threads = std::min(256, (groups + 63) / 64 * 64);
  const dim3 grid(n * h * w, (groups + threads - 1) / threads);
  clear_stale_error();
  hipLaunchKernelGGL(vec ? superpixel_pool_bwd_kernel<4> : superpixel_pool_bwd_kernel<1>, grid, dim3(threads), 0,
                     static_cast<hipStream_t>(stream), dpooled, dfeat, ymap, xmap, h, w, C, ld, ldp, H / sp, W / sp, sp);
  return check_launch("superpixel_pool_bwd");
}

}  // extern "C"
