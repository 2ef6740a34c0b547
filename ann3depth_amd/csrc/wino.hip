// wino.hip — A3D_PREC_F32_WINOGRAD: the stride-1 3x3 convolutions as Winograd F(2x2,3x3) in fp32 (Lavin & Gray 2015).
// Four stages.  The filter transform U = G g G^T runs once per weight change (a3d_conv2d_*_prepare_filter) or into the
// workspace on each call; per call the input transform V = B^T d B of every 4x4 window (2x2 outputs each), sixteen products
// M[xi] = V[xi] [T x C] . U[xi] [C x N] as ONE launch of the fp32 forward GEMM body (blockIdx.y = xi), and the output transform
// Y = A^T M A with the epilogue (bias + activation, or the ReLU mask of bwd-data).  bwd-data is the same pipeline on dz with
// padding 2 - pad and the filter's taps flipped and its channels swapped.  V, U and M are padded to whole 16-byte pieces of
// channels (zeros), so the GEMM always gathers and stores vectors.  Every sum has a fixed order: no atomics.
#include "a3d_internal.h"
#include "igemm.h"
#include "igemm_cfgs.h"

namespace a3d {

typedef float f4 __attribute__((ext_vector_type(4)));

// ---- filter transform: g [3][3][rows][cols] (forward) or its flipped transpose (bwd-data) -> U [16][Rp][Cp] ----
// bwd-data: U'[xi][k][c] from g'[r][s][k][c] = w[2-r][2-s][c][k]
__global__ __launch_bounds__(256) void wino_filter_kernel(const float* w, float* U, int c, int k, int Rp, int Cp, int bwd) {
  const int total = Rp * Cp;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int col = i % Cp, row = i / Cp;
    const int rows = bwd ? k : c, cols = bwd ? c : k;
    float g[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        float v = 0.f;
        if (row < rows && col < cols)
          v = bwd ? w[((size_t)((2 - r) * 3 + (2 - s)) * c + col) * k + row] : w[((size_t)(r * 3 + s) * c + row) * k + col];
        g[r][s] = v;
      }
    float t[4][3];
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      const float a = g[0][s] + g[2][s];
      t[0][s] = g[0][s];
      t[1][s] = (a + g[1][s]) * 0.5f;
      t[2][s] = (a - g[1][s]) * 0.5f;
      t[3][s] = g[2][s];
    }
#pragma unroll
    for (int a4 = 0; a4 < 4; ++a4) {
      const float a = t[a4][0] + t[a4][2];
      const float u[4] = {t[a4][0], (a + t[a4][1]) * 0.5f, (a - t[a4][1]) * 0.5f, t[a4][2]};
#pragma unroll
      for (int b4 = 0; b4 < 4; ++b4) U[(size_t)(a4 * 4 + b4) * total + i] = u[b4];
    }
  }
}

// ---- input transform: x [n][h][w][ld] -> V [16][T][Cp]; one thread per (tile, 4 channels) ----
// VEC: 16-byte loads (c % 4 == 0, ld % 4 == 0, x on the 16-byte grid); otherwise float by float, channels >= c zero
template <bool VEC>
__global__ __launch_bounds__(256) void wino_input_kernel(const float* __restrict__ x, float* __restrict__ V, int h, int w, int c, int ld,
                                                         int th, int tw, int pad_t, int pad_l, int Cp, size_t T) {
  const int cqn = Cp / 4;
  const size_t total = T * (size_t)cqn;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int cq = (int)(i % cqn);
    const size_t t = i / cqn;
    const int tj = (int)(t % tw), ti = (int)((t / tw) % th);
    const size_t img = t / ((size_t)tw * th);
    const int y0 = 2 * ti - pad_t, x0 = 2 * tj - pad_l;
    f4 d[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        f4 v = f4(0.f);
        const int yy = y0 + a, xx = x0 + b;
        if (yy >= 0 && yy < h && xx >= 0 && xx < w) {
          const float* src = x + ((img * h + yy) * w + xx) * (size_t)ld + cq * 4;
          if (VEC) {
            v = *reinterpret_cast<const f4*>(src);
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (cq * 4 + e < c) v[e] = src[e];
          }
        }
        d[a][b] = v;
      }
    // B^T d: rows
    f4 r[4][4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      r[0][b] = d[0][b] - d[2][b];
      r[1][b] = d[1][b] + d[2][b];
      r[2][b] = d[2][b] - d[1][b];
      r[3][b] = d[1][b] - d[3][b];
    }
    // (B^T d) B: columns
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const f4 v[4] = {r[a][0] - r[a][2], r[a][1] + r[a][2], r[a][2] - r[a][1], r[a][1] - r[a][3]};
#pragma unroll
      for (int b = 0; b < 4; ++b) *reinterpret_cast<f4*>(V + ((size_t)(a * 4 + b) * T + t) * Cp + cq * 4) = v[b];
    }
  }
}

// ---- output transform: M [16][T][Np] -> out [n][oh][ow][ld]; one thread per (tile, 4 columns) ----
// Forward: + bias, activation.  bwd-data: *= (mask > 0), mask laid out as out.  Tile rows / columns beyond oh / ow and
// columns >= ncols are never written.  VEC: 16-byte stores (ncols % 4 == 0, ld % 4 == 0, out and mask on the 16-byte grid).
template <bool VEC>
__global__ __launch_bounds__(256) void wino_output_kernel(const float* __restrict__ M, float* __restrict__ out, const float* __restrict__ bias,
                                                          const float* __restrict__ mask, int act, int oh, int ow, int ncols, int ld,
                                                          int th, int tw, int Np, size_t T) {
  const int cqn = Np / 4;
  const size_t total = T * (size_t)cqn;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int cq = (int)(i % cqn);
    const size_t t = i / cqn;
    const int tj = (int)(t % tw), ti = (int)((t / tw) % th);
    const size_t img = t / ((size_t)tw * th);
    f4 m[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) m[a][b] = *reinterpret_cast<const f4*>(M + ((size_t)(a * 4 + b) * T + t) * Np + cq * 4);
    f4 r[2][4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      r[0][b] = (m[0][b] + m[1][b]) + m[2][b];
      r[1][b] = (m[1][b] - m[2][b]) - m[3][b];
    }
    f4 bv = f4(0.f);
    if (bias) {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (cq * 4 + e < ncols) bv[e] = bias[cq * 4 + e];
    }
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const f4 y2[2] = {(r[a][0] + r[a][1]) + r[a][2], (r[a][1] - r[a][2]) - r[a][3]};
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int oy = 2 * ti + a, ox = 2 * tj + b;
        if (oy >= oh || ox >= ow) continue;
        const size_t o = ((img * oh + oy) * ow + ox) * (size_t)ld + cq * 4;
        f4 v = y2[b] + bv;
        if (act == EPI_RELU) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
        } else if (act == EPI_SIGMOID) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = 1.f / (1.f + expf(-v[e]));
        }
        if (VEC) {
          if (mask) {
            const f4 y = *reinterpret_cast<const f4*>(mask + o);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = apply_act_grad(v[e], y[e], EPI_RELU, 1.f);
          }
          *reinterpret_cast<f4*>(out + o) = v;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (cq * 4 + e < ncols) out[o + e] = mask ? apply_act_grad(v[e], mask[o + e], EPI_RELU, 1.f) : v[e];
        }
      }
    }
  }
}

// ---- the sixteen products: igemm_body on problem blockIdx.y of sixteen that differ in their three base addresses ----
constexpr int kBM = 128, kBN = 128, kWavesM = 4, kNWaves = 8, kBK = 32;
__global__ __launch_bounds__(64 * kNWaves, 2 * kNWaves / 4) void wino_gemm_kernel(const IgemmParams p, const size_t batch_a,
                                                                                   const size_t batch_b, const size_t batch_c) {
  IgemmParams q = p;
  q.A = p.A + (size_t)blockIdx.y * batch_a;
  q.B = p.B + (size_t)blockIdx.y * batch_b;
  q.C = p.C + (size_t)blockIdx.y * batch_c;
  igemm_body<MODE_FWD, kBM, kBN, kWavesM, kNWaves, kBK, 4, 4>(q, gridDim.x, blockIdx.x);
}

WinoGeom wino_geom(const a3d_conv_desc* d, bool bwd) {
  WinoGeom g{};
  g.oh = bwd ? d->h : d->ho;
  g.ow = bwd ? d->w : d->wo;
  g.th = (g.oh + 1) / 2;
  g.tw = (g.ow + 1) / 2;
  g.T = (size_t)d->n * g.th * g.tw;
  g.K = bwd ? d->k : d->c;
  g.N = bwd ? d->c : d->k;
  g.Kp = (g.K + 3) / 4 * 4;
  g.Np = (g.N + 3) / 4 * 4;
  auto up = [](size_t b) { return (b + 255) / 256 * 256; };
  g.v_bytes = up((size_t)16 * g.T * g.Kp * 4);
  g.m_bytes = up((size_t)16 * g.T * g.Np * 4);
  g.u_bytes = up((size_t)16 * g.Kp * g.Np * 4);
  return g;
}

bool wino_applicable(const a3d_conv_desc* d) {
  if (d->precision != A3D_PREC_F32_WINOGRAD || d->storage || d->r != 3 || d->s != 3 || d->stride != 1 || d->pad_t > 1 || d->pad_l > 1)
    return false;
  // the GEMM's rows are addressed from their tile's first one, a row table entry is a 31-bit byte offset
  for (bool bwd : {false, true}) {
    const WinoGeom g = wino_geom(d, bwd);
    if ((double)g.T * std::max(g.Kp, g.Np) * 4.0 >= 2147483647.0 || g.T >= ((size_t)1 << 30)) return false;
  }
  return true;
}

int wino_filter(const a3d_conv_desc* d, bool bwd, const float* w, float* U, hipStream_t st) {
  const WinoGeom g = wino_geom(d, bwd);
  clear_stale_error();
  hipLaunchKernelGGL(wino_filter_kernel, dim3(grid_for((size_t)g.Kp * g.Np)), dim3(256), 0, st, w, U, d->c, d->k, g.Kp, g.Np, bwd ? 1 : 0);
  return check_launch("wino_filter");
}

int wino_input(const a3d_conv_desc* d, bool bwd, const float* src, float* V, hipStream_t st) {
  const WinoGeom g = wino_geom(d, bwd);
  const int h = bwd ? d->ho : d->h, w = bwd ? d->wo : d->w, ld = bwd ? d->ldy : d->ldx;
  const int pad_t = bwd ? 2 - d->pad_t : d->pad_t, pad_l = bwd ? 2 - d->pad_l : d->pad_l;
  const bool vec = g.K % 4 == 0 && ld % 4 == 0 && aligned16(src);
  const dim3 grid(grid_for(g.T * (size_t)(g.Kp / 4), 256, 1u << 20)), block(256);
  clear_stale_error();
  if (vec) hipLaunchKernelGGL(wino_input_kernel<true>, grid, block, 0, st, src, V, h, w, g.K, ld, g.th, g.tw, pad_t, pad_l, g.Kp, g.T);
  else hipLaunchKernelGGL(wino_input_kernel<false>, grid, block, 0, st, src, V, h, w, g.K, ld, g.th, g.tw, pad_t, pad_l, g.Kp, g.T);
  return check_launch("wino_input");
}

int wino_output(const a3d_conv_desc* d, bool bwd, const float* M, float* out, const float* bias, const float* mask, int act,
                hipStream_t st) {
  const WinoGeom g = wino_geom(d, bwd);
  const int ld = bwd ? d->ldx : d->ldy;
  const bool vec = g.N % 4 == 0 && ld % 4 == 0 && aligned16(out) && aligned16(mask);
  const dim3 grid(grid_for(g.T * (size_t)(g.Np / 4), 256, 1u << 20)), block(256);
  clear_stale_error();
  if (vec) hipLaunchKernelGGL(wino_output_kernel<true>, grid, block, 0, st, M, out, bias, mask, act, g.oh, g.ow, g.N, ld, g.th, g.tw, g.Np, g.T);
  else hipLaunchKernelGGL(wino_output_kernel<false>, grid, block, 0, st, M, out, bias, mask, act, g.oh, g.ow, g.N, ld, g.th, g.tw, g.Np, g.T);
  return check_launch("wino_output");
}

a3d_timing_record wino_record(int mode, const WinoGeom& g) {
  return timing_record(mode, A3D_PREC_F32, kBM, kBN, kWavesM, kNWaves, kBK, 4, 4, 0, (int)(16 * g.T), g.N, g.K);
}

int wino_gemm(IgemmParams& p, const WinoGeom& g, hipStream_t st) {
  using Cfg = IgemmCfg<MODE_FWD, kBM, kBN, kWavesM, kNWaves, kBK, 4, 4>;
  // the raised LDS limit is a per-DEVICE attribute of the kernel: one flag per device (a benign race at worst sets it twice)
  static bool attr_done[64] = {};
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev < 0 || dev >= 64 || !attr_done[dev]) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(wino_gemm_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)Cfg::LDS_BYTES);
    if (e != hipSuccess) return set_error(A3D_ELAUNCH, "hipFuncSetAttribute: %s", hipGetErrorString(e));
    if (dev >= 0 && dev < 64) attr_done[dev] = true;
  }
  p.splitk = 1;
  p.ktiles_per_split = (p.K + kBK - 1) / kBK;
  p.tiles_m = (p.M + kBM - 1) / kBM;
  p.tiles_n = (p.N + kBN - 1) / kBN;
  p.slab = (size_t)p.M * p.N;
  clear_stale_error();
  hipLaunchKernelGGL(wino_gemm_kernel, dim3((unsigned)(p.tiles_m * p.tiles_n), 16), dim3(Cfg::NT), Cfg::LDS_BYTES, st, p,
                     g.T * (size_t)g.Kp, (size_t)g.Kp * g.Np, g.T * (size_t)g.Np);
  return check_launch("wino_gemm");
}

// ==== the filter gradient (include/a3d_wino_grad.h): dg = G^T [ sum over tiles (B^T d B) (.) (A dY A^T) ] G ====
// V = B^T d B is the forward's input transform (wino_input, bwd = false).  Z = A dY A^T expands each 2x2 tile of dz to 4x4 with
// adds alone; the sixteen sums over tiles M[xi] [C x K] = V[xi]^T [C x T] . Z[xi] [T x K] are sixteen filter-gradient GEMMs of a
// 1x1 convolution over T one-pixel images, ONE launch of the fp32 bwd-filter body (blockIdx.y = xi) whose T axis is split the
// classic way into raw slabs [xi][split][Cp][Kp]; the final transform adds a (c, k)'s splits in ascending order and applies
// G^T . G.  The bias gradient is the column sum of plane xi = (1,1) of Z (the sum of a tile's four dz), which the body sums from
// the tiles it stages.  No atomics, no fix-up: every sum has a fixed order.

// ---- dz transform: dz [n][ho][wo][ld] -> Z [16][T][Kp]; one thread per (tile, 4 channels) ----
// Positions beyond ho / wo read as zero; VEC as wino_input_kernel's, otherwise float by float with channels >= k zero
template <bool VEC>
__global__ __launch_bounds__(256) void wino_dz_kernel(const float* __restrict__ dz, float* __restrict__ Z, int ho, int wo, int k, int ld,
                                                      int th, int tw, int Kp, size_t T) {
  const int cqn = Kp / 4;
  const size_t total = T * (size_t)cqn;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int cq = (int)(i % cqn);
    const size_t t = i / cqn;
    const int tj = (int)(t % tw), ti = (int)((t / tw) % th);
    const size_t img = t / ((size_t)tw * th);
    f4 y[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        f4 v = f4(0.f);
        const int yy = 2 * ti + a, xx = 2 * tj + b;
        if (yy < ho && xx < wo) {
          const float* src = dz + ((img * ho + yy) * wo + xx) * (size_t)ld + cq * 4;
          if (VEC) {
            v = *reinterpret_cast<const f4*>(src);
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (cq * 4 + e < k) v[e] = src[e];
          }
        }
        y[a][b] = v;
      }
    // A dY: rows (A = [[1,0],[1,1],[1,-1],[0,-1]])
    const f4 r[4][2] = {{y[0][0], y[0][1]}, {y[0][0] + y[1][0], y[0][1] + y[1][1]}, {y[0][0] - y[1][0], y[0][1] - y[1][1]},
                        {-y[1][0], -y[1][1]}};
    // (A dY) A^T: columns
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const f4 z[4] = {r[a][0], r[a][0] + r[a][1], r[a][0] - r[a][1], -r[a][1]};
#pragma unroll
      for (int b = 0; b < 4; ++b) *reinterpret_cast<f4*>(Z + ((size_t)(a * 4 + b) * T + t) * Kp + cq * 4) = z[b];
    }
  }
}

// ---- final transform: slabs [16][splits][Cp][Kp] -> dw [3][3][c][k] = G^T M G, M = the splits added in ascending order; one
//      thread per (input channel, filter), which also adds the [splits][Kp] bias partials of its filter into db when it is the
//      first channel's.  Columns >= k and rows >= c of the slabs are never read, nothing but dw and db is written ----
__global__ __launch_bounds__(256) void wino_dw_kernel(const float* __restrict__ slabs, const float* __restrict__ bparts, float* __restrict__ dw,
                                                      float* __restrict__ db, int c, int k, int Cp, int Kp, int splits) {
  const size_t total = (size_t)c * k, plane = (size_t)Cp * Kp;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int col = (int)(i % k), row = (int)(i / k);
    const size_t at = (size_t)row * Kp + col;
    // split by split, the sixteen loads of a split in flight together: a thread's chain of 16 x splits dependent loads was
    // the cost of this kernel (13.6 / 21.5 us for conv2d_3 / conv2d_2's 28 / 31 MB at 3 / 5 splits)
    float m[4][4];
#pragma unroll
    for (int xi = 0; xi < 16; ++xi) m[xi / 4][xi % 4] = slabs[(size_t)xi * splits * plane + at];
    for (int z = 1; z < splits; ++z) {
      float v[16];
#pragma unroll
      for (int xi = 0; xi < 16; ++xi) v[xi] = slabs[((size_t)xi * splits + z) * plane + at];
#pragma unroll
      for (int xi = 0; xi < 16; ++xi) m[xi / 4][xi % 4] += v[xi];
    }
    // G^T M: rows (G^T = [[1,1/2,1/2,0],[0,1/2,-1/2,0],[0,1/2,1/2,1]])
    float t[3][4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const float hs = (m[1][b] + m[2][b]) * 0.5f;
      t[0][b] = m[0][b] + hs;
      t[1][b] = (m[1][b] - m[2][b]) * 0.5f;
      t[2][b] = hs + m[3][b];
    }
    // (G^T M) G: columns
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float hs = (t[a][1] + t[a][2]) * 0.5f;
      const float g[3] = {t[a][0] + hs, (t[a][1] - t[a][2]) * 0.5f, hs + t[a][3]};
#pragma unroll
      for (int b = 0; b < 3; ++b) dw[((size_t)(a * 3 + b) * c + row) * k + col] = g[b];
    }
    if (db && row == 0) {
      float s = bparts[col];
      for (int z = 1; z < splits; ++z) s += bparts[(size_t)z * Kp + col];
      db[col] = s;
    }
  }
}

// ---- the sixteen sums over tiles: the bwd-filter body on problem blockIdx.y; the bias partials belong to plane (1,1) ----
constexpr int kBiasPlane = 1 * 4 + 1;
__global__ __launch_bounds__(64 * kNWaves, 2 * kNWaves / 4) void wino_grad_gemm_kernel(const IgemmParams p, const size_t batch_a,
                                                                                        const size_t batch_b, const size_t batch_c) {
  IgemmParams q = p;
  q.A = p.A + (size_t)blockIdx.y * batch_a;
  q.B = p.B + (size_t)blockIdx.y * batch_b;
  q.C = p.C + (size_t)blockIdx.y * batch_c;
  if (blockIdx.y != kBiasPlane) q.dbias = nullptr;
  igemm_body<MODE_BWD_F, kBM, kBN, kWavesM, kNWaves, kBK, 4, 4>(q, gridDim.x, blockIdx.x);
}

// How many ways the T axis of the sixteen products is split: a pure function of (C, K, T), asked by the workspace query and by
// the launch.  The launch stays within one round of the chip's 512 slots for blocks of eight waves (two on each of 256 CUs) and
// a split keeps at least kMinKTiles k-tiles on average (a shorter K loop is all prologue).  Among those counts the one with the
// least work on the busiest CU wins — a CU holds ceil(blocks / 256) blocks of 1 / s of a tile's K loop each, and a block that
// has its CU to itself runs at nearly twice the rate of two that share one — the smaller count on a tie (fewer slabs).  Measured
// at B = 8, 16, 32 for conv2d_2 and conv2d_3 (profiles/wino_grad_split_sweep.txt): the rule's pick is the fastest count or
// within 4 us (3 %) of it in all six.
constexpr int kBlockSlots = 512, kCUs = 256, kMinKTiles = 5;
int wino_grad_splits(int C, int K, size_t T) {
  const long blocks1 = 16L * ((C + kBM - 1) / kBM) * ((K + kBN - 1) / kBN);
  const long nk = (long)((T + kBK - 1) / kBK);
  const long smax = std::max(1L, std::min(kBlockSlots / blocks1, nk / kMinKTiles));
  long s = 1, load = (blocks1 + kCUs - 1) / kCUs;      // the busiest CU's work is load / s
  for (long t = 2; t <= smax; ++t) {
    const long l = (blocks1 * t + kCUs - 1) / kCUs;
    if (l * s < load * t) { s = t; load = l; }
  }
  const int forced = tune_int("A3D_WINO_GRAD_SPLIT", 0);      // tuning processes only (A3D_TUNING=1): the sweep behind the rule
  if (forced > 0) s = std::min((long)forced, nk);
  const long per = (nk + s - 1) / s;
  return (int)((nk + per - 1) / per);
}

WinoGradGeom wino_grad_geom(const a3d_conv_desc* d) {
  const WinoGeom w = wino_geom(d, false);
  WinoGradGeom g{};
  g.T = w.T; g.Cp = w.Kp; g.Kp = w.Np;
  g.splits = wino_grad_splits(d->c, d->k, w.T);
  auto up = [](size_t b) { return (b + 255) / 256 * 256; };
  g.v_bytes = w.v_bytes;
  g.z_bytes = w.m_bytes;
  g.slab_bytes = up((size_t)16 * g.splits * g.Cp * g.Kp * 4);
  g.bias_bytes = up((size_t)g.splits * g.Kp * 4);
  return g;
}

bool wino_grad_applicable(const a3d_conv_desc* d) {
  if (d->precision != A3D_PREC_F32 && d->precision != A3D_PREC_F32_WINOGRAD) return false;
  a3d_conv_desc e = *d;
  e.precision = A3D_PREC_F32_WINOGRAD;
  return wino_applicable(&e);
}

int wino_dz(const a3d_conv_desc* d, const float* dz, float* Z, hipStream_t st) {
  const WinoGeom g = wino_geom(d, false);
  const bool vec = d->k % 4 == 0 && d->ldy % 4 == 0 && aligned16(dz);
  const dim3 grid(grid_for(g.T * (size_t)(g.Np / 4), 256, 1u << 20)), block(256);
  clear_stale_error();
  if (vec) hipLaunchKernelGGL(wino_dz_kernel<true>, grid, block, 0, st, dz, Z, d->ho, d->wo, d->k, d->ldy, g.th, g.tw, g.Np, g.T);
  else hipLaunchKernelGGL(wino_dz_kernel<false>, grid, block, 0, st, dz, Z, d->ho, d->wo, d->k, d->ldy, g.th, g.tw, g.Np, g.T);
  return check_launch("wino_dz");
}

int wino_dw(const a3d_conv_desc* d, const WinoGradGeom& g, const float* slabs, const float* bparts, float* dw, float* db, hipStream_t st) {
  clear_stale_error();
  hipLaunchKernelGGL(wino_dw_kernel, dim3(grid_for((size_t)d->c * d->k, 256, 1u << 20)), dim3(256), 0, st, slabs, bparts, dw, db, d->c, d->k,
                     g.Cp, g.Kp, g.splits);
  return check_launch("wino_dw");
}

// m = C, n = K, k = 16 T: the FLOPs executed
a3d_timing_record wino_grad_record(const a3d_conv_desc* d, const WinoGradGeom& g) {
  a3d_timing_record r = timing_record(MODE_BWD_F, A3D_PREC_F32, kBM, kBN, kWavesM, kNWaves, kBK, 4, 4, 0, d->c, d->k, (int)(16 * g.T));
  r.splitk = g.splits;
  return r;
}

int wino_grad_gemm(IgemmParams& p, const WinoGradGeom& g, hipStream_t st) {
  using Cfg = IgemmCfg<MODE_BWD_F, kBM, kBN, kWavesM, kNWaves, kBK, 4, 4>;
  static bool attr_done[64] = {};      // per device, as wino_gemm's
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev < 0 || dev >= 64 || !attr_done[dev]) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(wino_grad_gemm_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)Cfg::LDS_BYTES);
    if (e != hipSuccess) return set_error(A3D_ELAUNCH, "hipFuncSetAttribute: %s", hipGetErrorString(e));
    if (dev >= 0 && dev < 64) attr_done[dev] = true;
  }
  const int nk = (p.K + kBK - 1) / kBK;
  p.splitk = g.splits;
  p.ktiles_per_split = (nk + g.splits - 1) / g.splits;
  p.tiles_m = (p.M + kBM - 1) / kBM;
  p.tiles_n = (p.N + kBN - 1) / kBN;
  p.slab = (size_t)p.M * p.N;
  clear_stale_error();
  hipLaunchKernelGGL(wino_grad_gemm_kernel, dim3((unsigned)(p.tiles_m * p.tiles_n * p.splitk), 16), dim3(Cfg::NT), Cfg::LDS_BYTES, st, p,
                     g.T * (size_t)g.Cp, g.T * (size_t)g.Kp, (size_t)g.splits * g.Cp * g.Kp);
  return check_launch("wino_grad_gemm");
}

}  // namespace a3d
