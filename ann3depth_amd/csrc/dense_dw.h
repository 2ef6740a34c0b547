// dense_dw.h — the walks the small-batch filter-gradient kernels share (dense.hip: dense_dw_kernel and the Adam rows / stream
// kernels; optim.hip: dense_dw_momentum_kernel): the BiasAddGrad column sum, and the register-resident contraction
// dw[k][n] = sum_m x[m][k] * dz[m][n] of the two kernels that take their operands straight from global memory.  A kernel is a
// prefetch of its own, dw_contract, and an epilogue that feeds its own rule (optim_rules.h).  Everything is __forceinline__, and
// every file that includes this is compiled with -ffp-contract=off.
#pragma once
#include "a3d_internal.h"
#include "igemm.h"

namespace a3d {

// BiasAddGrad of one column: eight loads in flight, added in row order
__device__ __forceinline__ float colsum_rows(const float* __restrict__ dz, int M, int N, int col) {
  float s = 0.f;
  for (int m0 = 0; m0 < M; m0 += 8) {
    float t[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) t[i] = m0 + i < M ? dz[(size_t)(m0 + i) * N + col] : 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (m0 + i < M) s += t[i];
  }
  return s;
}

// CW adjacent floats of a row, one access; rows of any length are 4-byte aligned only
template <int CW>
struct VecOf { typedef float type __attribute__((ext_vector_type(CW), aligned(4))); };

// A block is four waves, and a wave owns 32 weight rows x 32*CW columns.  Lane li takes dz[m][col0 .. col0 + CW-1] with ONE
// 4*CW-byte load and feeds the CW values to CW MFMAs, so accumulator j holds the columns n0 + CW li + j: the CW accumulators of a
// lane are ADJACENT columns of one row, register v of them the row row_of(v), and a wave-instruction of the epilogue moves two
// row segments of 128*CW bytes — for a slot's read (issued before the contraction starts, so its HBM latency passes under the
// operand loads and the MFMAs) as for the write.  No LDS.
template <int CW>
struct DwTile {
  int tid, li, lh, n0, k0, col0;
  bool cfull;             // the lane's CW columns all exist (only the last lanes of the last column group may lack some)
  __device__ __forceinline__ explicit DwTile(int N) {
    tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    li = lane & 31, lh = lane >> 5;
    n0 = blockIdx.x * 32 * CW, k0 = (blockIdx.y * 4 + wave) * 32;      // k0 is wave-uniform
    col0 = n0 + CW * li;
    cfull = col0 + CW - 1 < N;
  }
  __device__ __forceinline__ int row_of(int v) const { return k0 + (v & 3) + 8 * (v >> 2) + 4 * lh; }
};

// fp32 MFMA 32x32x2 with the batch as the contraction axis: D[k][n] += A[k][m] * B[m][n], A = x^T, B = dz:
//   A[i = weight row k0+li][kk = batch row 2t+lh] = x[2t+lh][k0+li];  B_j[kk][li] = dz[2t+lh][col0 + j]
// The sum runs over m in ascending order, one fmaf per term — the order of the BiasAddGrad sum too.  Eight instructions' operands
// are loaded, then multiplied.  GEMM_ORDER: the batch rows reach the matrix cores in the order of the implicit-GEMM route
// (igemm.h: a lane half holds four consecutive rows of a chunk of eight, instruction j of the chunk multiplies rows 8u + j and
// 8u + 4 + j).  Rows past the batch are zeros in both.
template <int CW, bool GEMM_ORDER>
__device__ __forceinline__ void dw_contract(const DwTile<CW>& t, const float* __restrict__ x, const float* __restrict__ dz, int M,
                                            int K, int N, f32x16 (&acc)[CW]) {
  typedef typename VecOf<CW>::type vec;
#pragma unroll
  for (int j = 0; j < CW; ++j)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[j][v] = 0.f;
  const int krow = t.k0 + t.li;
  const bool kok = krow < K;
  const int T = GEMM_ORDER ? (M + 7) / 8 * 4 : (M + 1) / 2;       // instructions: two batch rows each
  for (int t0 = 0; t0 < T; t0 += 8) {
    float a[8];
    vec bq[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int m = GEMM_ORDER ? 8 * ((t0 + u) >> 2) + 4 * t.lh + ((t0 + u) & 3) : 2 * (t0 + u) + t.lh;
      const bool mok = m < M;
      a[u] = (mok && kok) ? x[(size_t)m * K + krow] : 0.f;
#pragma unroll
      for (int j = 0; j < CW; ++j) bq[u][j] = 0.f;
      if (mok) {
        if (t.cfull) {
          bq[u] = *reinterpret_cast<const vec*>(dz + (size_t)m * N + t.col0);
        } else {
#pragma unroll
          for (int j = 0; j < CW; ++j)
            if (t.col0 + j < N) bq[u][j] = dz[(size_t)m * N + t.col0 + j];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int j = 0; j < CW; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], bq[u][j], acc[j], 0, 0, 0);
  }
}

}  // namespace a3d
