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

}  // namespace a3d
