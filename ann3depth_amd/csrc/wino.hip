// wino.hip — A3D_PREC_F32_WINOGRAD: the stride-1 3x3 convolutions as Winograd F(2x2,3x3) in fp32 (Lavin & Gray 2015).
// Four stages.  The filter transform U = G g G^T runs once per weight change (a3d_conv2d_*_prepare_filter) or into the
// workspace on each call; per call the input transform V = B^T d B of every 4x4 window (2x2 outputs each), sixteen products
// M[xi] = V[xi] [T x C] . U[xi] [C x N] as ONE launch of the fp32 forward GEMM body (blockIdx.y = xi), and the output transform
// Y = A^T M A with the epilogue (bias + activation, or the ReLU mask of bwd-data).  bwd-data is the same pipeline on dz with
// padding 2 - pad and the filter's taps flipped and its channels swapped.  V, U and M are padded to whole 16-byte pieces of
// channels (zeros), so the GEMM always gathers and stores vectors.  Every sum has a fixed order: no atomics.
// Below them the filter gradient through the same identity (include/a3d_wino_grad.h) and, last, both gradients of a layer as one
// chain of three launches (include/a3d_wino_bwd.h).  The per-item bodies are device functions, so that the chain's kernels run
// the very statements of the kernels they merge.
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

// the 4x4 window of image `img` whose first pixel is (y0, x0), channels cq*4 .. cq*4+3; positions outside h x w read as zero
template <bool VEC>
__device__ __forceinline__ void wino_load_window(const float* __restrict__ x, f4 (&d)[4][4], size_t img, int y0, int x0, int h, int w, int c,
                                                 int ld, int cq) {
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
}

// B^T d B of one window into its sixteen planes of V
__device__ __forceinline__ void wino_input_store(const f4 (&d)[4][4], float* __restrict__ V, size_t T, size_t t, int Cp, int cq) {
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
    f4 d[4][4];
    wino_load_window<VEC>(x, d, img, 2 * ti - pad_t, 2 * tj - pad_l, h, w, c, ld, cq);
    wino_input_store(d, V, T, t, Cp, cq);
  }
}

// ---- output transform: M [16][T][Np] -> out [n][oh][ow][ld]; one thread per (tile, 4 columns) ----
// Forward: + bias, activation.  bwd-data: *= (mask > 0), mask laid out as out.  Tile rows / columns beyond oh / ow and
// columns >= ncols are never written.  VEC: 16-byte stores (ncols % 4 == 0, ld % 4 == 0, out and mask on the 16-byte grid).
// A^T M of one tile's sixteen planes: the rows of the output transform
__device__ __forceinline__ void wino_output_rows(const float* __restrict__ M, f4 (&r)[2][4], size_t T, size_t t, int Np, int cq) {
  f4 m[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) m[a][b] = *reinterpret_cast<const f4*>(M + ((size_t)(a * 4 + b) * T + t) * Np + cq * 4);
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    r[0][b] = (m[0][b] + m[1][b]) + m[2][b];
    r[1][b] = (m[1][b] - m[2][b]) - m[3][b];
  }
}

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
    f4 r[2][4];
    wino_output_rows(M, r, T, t, Np, cq);
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

// ---- the products of every route: igemm_body on plane blockIdx.y of a PlaneBatch (igemm.h) ----
template <int MODE, int BN, int WAVES_M, int NWAVES>
__global__ __launch_bounds__(64 * NWAVES, 2 * NWAVES / 4) void plane_gemm_kernel(const IgemmParams p, const PlaneBatch bt) {
  igemm_body<MODE, kBM, BN, WAVES_M, NWAVES, kBK, 4, 4>(plane_params(p, bt, blockIdx.y), gridDim.x, blockIdx.x);
}

template <int MODE, int BN, int WAVES_M, int NWAVES>
static int plane_gemm_as(const IgemmParams& p, const PlaneBatch& bt, unsigned blocks, int planes, const char* what, hipStream_t st) {
  using Cfg = IgemmCfg<MODE, kBM, BN, WAVES_M, NWAVES, kBK, 4, 4>;
  static bool attr_done[64] = {};
  const int rc = raise_lds(reinterpret_cast<const void*>(plane_gemm_kernel<MODE, BN, WAVES_M, NWAVES>), Cfg::LDS_BYTES, attr_done);
  if (rc != A3D_OK) return rc;
  clear_stale_error();
  hipLaunchKernelGGL((plane_gemm_kernel<MODE, BN, WAVES_M, NWAVES>), dim3(blocks, (unsigned)planes), dim3(Cfg::NT), Cfg::LDS_BYTES, st, p, bt);
  return check_launch(what);
}

int plane_gemm(int mode, int bn, const IgemmParams& p, const PlaneBatch& bt, unsigned blocks, int planes, const char* what, hipStream_t st) {
  if (mode == MODE_BWD_F) return plane_gemm_as<MODE_BWD_F, kBN, kWavesM, kNWaves>(p, bt, blocks, planes, what, st);
  if (bn == 96) return plane_gemm_as<MODE_FWD, 96, 4, 4>(p, bt, blocks, planes, what, st);
  return plane_gemm_as<MODE_FWD, kBN, kWavesM, kNWaves>(p, bt, blocks, planes, what, st);
}

void plane_tiles(IgemmParams& p, int splits) {
  const int nk = (p.K + kBK - 1) / kBK;
  p.splitk = splits;
  p.ktiles_per_split = (nk + splits - 1) / splits;
  p.tiles_m = (p.M + kBM - 1) / kBM;
  p.tiles_n = (p.N + kBN - 1) / kBN;
  p.slab = (size_t)p.M * p.N;
}

// How many ways the pixel axis of a route's bwd-filter products is split: a pure function of its arguments, asked by the
// workspace query and by the launch.  The launch stays within one round of the chip's 512 slots for blocks of eight waves (two on
// each of 256 CUs) and a split keeps at least kMinKTiles k-tiles on average (a shorter K loop is all prologue).  Among those
// counts the one with the least work on the busiest CU wins — a CU holds ceil(blocks / 256) blocks of 1 / s of a tile's K loop
// each, and a block that has its CU to itself runs at nearly twice the rate of two that share one.  On a tie:
//   F(2x2,3x3), sixteen planes: the SMALLER count (fewer slabs).  Measured at B = 8, 16, 32 for conv2d_2 and conv2d_3
//     (profiles/wino_grad_split_sweep.txt): the rule's pick is the fastest count or within 4 us (3 %) of it in all six.
//   F(4,5), eight planes: the LARGER count.  conv2d_1's 64 tiles tie at 4 splits (one block on every CU) and 8 (two), and two
//     short blocks on a CU hide each other's prologue and slab stores better than one long block runs alone: 62.9 / 100.7 /
//     179.6 us against 67.2 / 113.8 / 205.4 at B = 8 / 16 / 32 (profiles/wino1d_split_sweep.txt; the rule's pick is the fastest
//     count in all three).
int plane_splits(int planes, int M, int N, size_t pixels, bool larger_on_tie, const char* tuning) {
  const long blocks1 = (long)planes * ((M + kBM - 1) / kBM) * ((N + kBN - 1) / kBN);
  const long nk = (long)((pixels + kBK - 1) / kBK);
  const long smax = std::max(1L, std::min(kBlockSlots / blocks1, nk / kMinKTiles));
  long s = 1, load = (blocks1 + kCUs - 1) / kCUs;      // the busiest CU's work is load / s
  for (long t = 2; t <= smax; ++t) {
    const long l = (blocks1 * t + kCUs - 1) / kCUs;
    if (l * s < load * t || (larger_on_tie && l * s == load * t)) { s = t; load = l; }
  }
  const int forced = tune_int(tuning, 0);      // tuning processes only (A3D_TUNING=1): the sweep behind the rule
  if (forced > 0) s = std::min((long)forced, nk);
  const long per = (nk + s - 1) / s;
  return (int)((nk + per - 1) / per);
}

// ---- F(2x2,3x3): sixteen planes.  The strides between the planes of V, U and M (forward, bwd-data) and of V, Z and the raw
//      slabs (filter gradient), whose bias partials belong to plane (1,1) ----
constexpr int kWinoPlanes = 16;
static PlaneBatch wino_batch(const WinoGeom& g) { return {g.T * (size_t)g.Kp, (size_t)g.Kp * g.Np, g.T * (size_t)g.Np, 0, -1}; }
static PlaneBatch wino_grad_batch(const WinoGradGeom& g) {
  return {g.T * (size_t)g.Cp, g.T * (size_t)g.Kp, (size_t)g.splits * g.Cp * g.Kp, 0, 1 * 4 + 1};
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
  g.v_bytes = up256((size_t)16 * g.T * g.Kp * 4);
  g.m_bytes = up256((size_t)16 * g.T * g.Np * 4);
  g.u_bytes = up256((size_t)16 * g.Kp * g.Np * 4);
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

// the sixteen products M[xi] = V[xi] . U[xi]: no split
int wino_gemm(IgemmParams& p, const WinoGeom& g, hipStream_t st) {
  plane_tiles(p, 1);
  return plane_gemm(MODE_FWD, kBN, p, wino_batch(g), (unsigned)(p.tiles_m * p.tiles_n), kWinoPlanes, "wino_gemm", st);
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

// A dY A^T of one 2x2 tile into its sixteen planes of Z
__device__ __forceinline__ void wino_dz_store(const f4 (&y)[2][2], float* __restrict__ Z, size_t T, size_t t, int Kp, int cq) {
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
    wino_dz_store(y, Z, T, t, Kp, cq);
  }
}

// ---- final transform: slabs [16][splits][Cp][Kp] -> dw [3][3][c][k] = G^T M G, M = the splits added in ascending order; one
//      thread per (input channel, filter), which also adds the [splits][Kp] bias partials of its filter into db when it is the
//      first channel's.  Columns >= k and rows >= c of the slabs are never read, nothing but dw and db is written ----
__device__ __forceinline__ void wino_dw_item(size_t i, const float* __restrict__ slabs, const float* __restrict__ bparts, float* __restrict__ dw,
                                             float* __restrict__ db, int c, int k, int Cp, int Kp, int splits) {
  const size_t plane = (size_t)Cp * Kp;
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

__global__ __launch_bounds__(256) void wino_dw_kernel(const float* __restrict__ slabs, const float* __restrict__ bparts, float* __restrict__ dw,
                                                      float* __restrict__ db, int c, int k, int Cp, int Kp, int splits) {
  const size_t total = (size_t)c * k;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256)
    wino_dw_item(i, slabs, bparts, dw, db, c, k, Cp, Kp, splits);
}

int wino_grad_splits(int C, int K, size_t T) { return plane_splits(kWinoPlanes, C, K, T, false, "A3D_WINO_GRAD_SPLIT"); }

WinoGradGeom wino_grad_geom(const a3d_conv_desc* d) {
  const WinoGeom w = wino_geom(d, false);
  WinoGradGeom g{};
  g.T = w.T; g.Cp = w.Kp; g.Kp = w.Np;
  g.splits = wino_grad_splits(d->c, d->k, w.T);
  g.v_bytes = w.v_bytes;
  g.z_bytes = w.m_bytes;
  g.slab_bytes = up256((size_t)16 * g.splits * g.Cp * g.Kp * 4);
  g.bias_bytes = up256((size_t)g.splits * g.Kp * 4);
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

// the sixteen sums over tiles, the T axis in g.splits pieces
int wino_grad_gemm(IgemmParams& p, const WinoGradGeom& g, hipStream_t st) {
  plane_tiles(p, g.splits);
  return plane_gemm(MODE_BWD_F, kBN, p, wino_grad_batch(g), (unsigned)(p.tiles_m * p.tiles_n * p.splitk), kWinoPlanes, "wino_grad_gemm", st);
}

// ==== both gradients of one layer as one chain (include/a3d_wino_bwd.h): the transforms, products and finishing transforms of
//      the filter gradient above and of bwd-data, three launches in place of seven.  Every item runs the statements of the
//      kernel it comes from (the helpers above), so dw, db and dx are the bits of the two routes run one after the other ====

// ---- launch 1: V_x = B^T x B on the forward's tile grid; V_dz = B^T dz B on bwd-data's grid (padding 2 - pad) and, from the
//      same sixteen loads, Z = A dY A^T of the 2x2 tile inside that window.  With pad 0 bwd-data's grid (over h x w) is larger
//      than Z's (over ho x wo): the dz items walk the larger one and write Z where it has a tile ----
struct WinoBwdXform {
  const float *x, *dz;
  float *Vx, *Vdz, *Z;
  int h, w, c, ldx, xth, xtw, xpt, xpl, Cp;      // x [n][h][w][ldx], the forward's tiles (Z's too) and padding
  int ho, wo, k, ldy, dth, dtw, dpt, dpl, Kp;    // dz [n][ho][wo][ldy], bwd-data's tiles and padding (1 or 2)
  size_t Tx, Td, x_items;                        // tiles of the two grids; items [0, x_items) are x's
};
template <bool VEC>
__global__ __launch_bounds__(256) void wino_bwd_transform_kernel(const WinoBwdXform q) {
  const int cqx = q.Cp / 4, cqd = q.Kp / 4;
  const size_t total = q.x_items + q.Td * (size_t)cqd;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    f4 d[4][4];
    if (i < q.x_items) {
      const int cq = (int)(i % cqx);
      const size_t t = i / cqx;
      const int tj = (int)(t % q.xtw), ti = (int)((t / q.xtw) % q.xth);
      const size_t img = t / ((size_t)q.xtw * q.xth);
      wino_load_window<VEC>(q.x, d, img, 2 * ti - q.xpt, 2 * tj - q.xpl, q.h, q.w, q.c, q.ldx, cq);
      wino_input_store(d, q.Vx, q.Tx, t, q.Cp, cq);
      continue;
    }
    const size_t j = i - q.x_items;
    const int cq = (int)(j % cqd);
    const size_t t = j / cqd;
    const int tj = (int)(t % q.dtw), ti = (int)((t / q.dtw) % q.dth);
    const size_t img = t / ((size_t)q.dtw * q.dth);
    wino_load_window<VEC>(q.dz, d, img, 2 * ti - q.dpt, 2 * tj - q.dpl, q.ho, q.wo, q.k, q.ldy, cq);
    wino_input_store(d, q.Vdz, q.Td, t, q.Kp, cq);
    if (ti < q.xth && tj < q.xtw) {      // dz (2 ti + a, 2 tj + b) is window position (dpt + a, dpl + b)
      f4 y[2][2];
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const f4 lo = q.dpl == 1 ? d[1 + a][1 + b] : d[1 + a][2 + b], hi = q.dpl == 1 ? d[2 + a][1 + b] : d[2 + a][2 + b];
          y[a][b] = q.dpt == 1 ? lo : hi;
        }
      wino_dz_store(y, q.Z, q.Tx, (img * q.xth + ti) * q.xtw + tj, q.Kp, cq);
    }
  }
}

int wino_bwd_transforms(const a3d_conv_desc* d, const float* x, const float* dz, float* Vx, float* Vdz, float* Z, hipStream_t st) {
  const WinoGeom gx = wino_geom(d, false), gd = wino_geom(d, true);
  WinoBwdXform q{};
  q.x = x; q.dz = dz; q.Vx = Vx; q.Vdz = Vdz; q.Z = Z;
  q.h = d->h; q.w = d->w; q.c = d->c; q.ldx = d->ldx; q.xth = gx.th; q.xtw = gx.tw; q.xpt = d->pad_t; q.xpl = d->pad_l; q.Cp = gx.Kp;
  q.ho = d->ho; q.wo = d->wo; q.k = d->k; q.ldy = d->ldy; q.dth = gd.th; q.dtw = gd.tw; q.dpt = 2 - d->pad_t; q.dpl = 2 - d->pad_l;
  q.Kp = gd.Kp;
  q.Tx = gx.T; q.Td = gd.T; q.x_items = gx.T * (size_t)(gx.Kp / 4);
  const bool vec = d->c % 4 == 0 && d->ldx % 4 == 0 && aligned16(x) && d->k % 4 == 0 && d->ldy % 4 == 0 && aligned16(dz);
  const dim3 grid(grid_for(q.x_items + gd.T * (size_t)(gd.Kp / 4), 256, 1u << 20)), block(256);
  clear_stale_error();
  if (vec) hipLaunchKernelGGL(wino_bwd_transform_kernel<true>, grid, block, 0, st, q);
  else hipLaunchKernelGGL(wino_bwd_transform_kernel<false>, grid, block, 0, st, q);
  return check_launch("wino_bwd_transform");
}

// ---- launch 2: the two sets of sixteen products in one grid.  Blocks [0, 16 gf) are the filter gradient's (the longer K loop
//      first), the rest bwd-data's; within a set the block order is that of the set's own launch (plane-major), and a block runs
//      the body of that launch on the same parameters: same tiles, same splits, same sums ----
__global__ __launch_bounds__(64 * kNWaves, 2 * kNWaves / 4) void wino_bwd_gemm_kernel(const IgemmParams pf, const PlaneBatch bf, const uint32_t gf,
                                                                                       const IgemmParams pd, const PlaneBatch bd, const uint32_t gd) {
  if (blockIdx.x < kWinoPlanes * gf) {
    const uint32_t xi = blockIdx.x / gf;
    igemm_body<MODE_BWD_F, kBM, kBN, kWavesM, kNWaves, kBK, 4, 4>(plane_params(pf, bf, xi), gf, blockIdx.x - xi * gf);
  } else {
    const uint32_t id = blockIdx.x - kWinoPlanes * gf, xi = id / gd;
    igemm_body<MODE_FWD, kBM, kBN, kWavesM, kNWaves, kBK, 4, 4>(plane_params(pd, bd, xi), gd, id - xi * gd);
  }
}

int wino_bwd_gemm(IgemmParams& pf, const WinoGradGeom& gg, IgemmParams& pd, const WinoGeom& g, hipStream_t st) {
  constexpr size_t kLds = std::max(IgemmCfg<MODE_BWD_F, kBM, kBN, kWavesM, kNWaves, kBK, 4, 4>::LDS_BYTES,
                                   IgemmCfg<MODE_FWD, kBM, kBN, kWavesM, kNWaves, kBK, 4, 4>::LDS_BYTES);
  static bool attr_done[64] = {};
  const int rc = raise_lds(reinterpret_cast<const void*>(wino_bwd_gemm_kernel), kLds, attr_done);
  if (rc != A3D_OK) return rc;
  plane_tiles(pf, gg.splits);
  plane_tiles(pd, 1);
  const uint32_t gf = (uint32_t)(pf.tiles_m * pf.tiles_n * pf.splitk), gd = (uint32_t)(pd.tiles_m * pd.tiles_n);
  clear_stale_error();
  hipLaunchKernelGGL(wino_bwd_gemm_kernel, dim3(kWinoPlanes * (gf + gd)), dim3(64 * kNWaves), kLds, st, pf, wino_grad_batch(gg), gf, pd,
                     wino_batch(g), gd);
  return check_launch("wino_bwd_gemm");
}

// ---- launch 3: wino_dw_kernel's items (the splits added in ascending order, G^T . G, db), then the output transform's:
//      A^T M A, times (mask > 0) — or, POOL, scattered through a 2x2 max pool's recorded positions into the unpooled gradient
//      [n][h2][w2][ncols]: what a3d_maxpool2x2_bwd_idx(relu_mask = 1) writes from the pooled-size dx, which is never stored,
//      the zero last row / column of odd extents included ----
struct WinoBwdFinish {
  const float *slabs, *bparts;
  float *dw, *db;
  int c, k, Cp, Kp, splits;                                    // wino_dw_item's
  const float* M;
  float* dx;
  const float* mask;
  int oh, ow, ncols, ld, th, tw, Np;                           // bwd-data's output transform
  size_t T, dw_items;                                          // items [0, dw_items) are dw's
  const uint8_t* argmax;                                       // POOL: positions [n][oh][ow][ncols], pooled values y with
  const float* py;                                             // pixel stride pldy, unpooled extents h2 x w2
  int pldy, h2, w2;
};
template <bool VEC, bool POOL>
__global__ __launch_bounds__(256) void wino_bwd_finish_kernel(const WinoBwdFinish q) {
  const int cqn = q.Np / 4;
  const size_t total = q.dw_items + q.T * (size_t)cqn;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    if (i < q.dw_items) {
      wino_dw_item(i, q.slabs, q.bparts, q.dw, q.db, q.c, q.k, q.Cp, q.Kp, q.splits);
      continue;
    }
    const size_t j = i - q.dw_items;
    const int cq = (int)(j % cqn);
    const size_t t = j / cqn;
    const int tj = (int)(t % q.tw), ti = (int)((t / q.tw) % q.th);
    const size_t img = t / ((size_t)q.tw * q.th);
    f4 r[2][4];
    wino_output_rows(q.M, r, q.T, t, q.Np, cq);
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const f4 y2[2] = {(r[a][0] + r[a][1]) + r[a][2], (r[a][1] - r[a][2]) - r[a][3]};
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int oy = 2 * ti + a, ox = 2 * tj + b;
        if (oy >= q.oh || ox >= q.ow) continue;
        const f4 v = y2[b] + f4(0.f);      // wino_output_kernel's "+ bias" without one (-0 becomes +0 there too)
        const size_t win = (img * q.oh + oy) * q.ow + ox;
        if (!POOL) {
          const size_t o = win * (size_t)q.ld + cq * 4;
          if (VEC) {
            f4 u = v;
            if (q.mask) {
              const f4 y = *reinterpret_cast<const f4*>(q.mask + o);
#pragma unroll
              for (int e = 0; e < 4; ++e) u[e] = apply_act_grad(v[e], y[e], EPI_RELU, 1.f);
            }
            *reinterpret_cast<f4*>(q.dx + o) = u;
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (cq * 4 + e < q.ncols) q.dx[o + e] = q.mask ? apply_act_grad(v[e], q.mask[o + e], EPI_RELU, 1.f) : v[e];
          }
          continue;
        }
        // the pool's window of pooled pixel (oy, ox): rows 2 oy, 2 oy + 1, columns 2 ox, 2 ox + 1 of dx; an odd extent's last
        // row / column, which the pool dropped, is zeroed by the last pooled row / column's items
        const size_t px = (size_t)q.ncols, row = (size_t)q.w2 * px;
        const size_t base = ((img * q.h2 + 2 * oy) * q.w2 + 2 * ox) * px + cq * 4;
        const bool cut_r = oy == q.oh - 1 && (q.h2 & 1), cut_c = ox == q.ow - 1 && (q.w2 & 1);
        if (VEC) {
          const uint32_t a4 = *reinterpret_cast<const uint32_t*>(q.argmax + win * px + cq * 4);
          const f4 y4 = *reinterpret_cast<const f4*>(q.py + win * (size_t)q.pldy + cq * 4);
          const f4 zero = f4(0.f);
          f4 o[4] = {zero, zero, zero, zero};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const uint32_t arg = (a4 >> (8 * e)) & 0xffu;
            const float g = !(y4[e] > 0.f) ? 0.f : v[e];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) o[kk][e] = arg == (uint32_t)kk ? g : 0.f;
          }
          *reinterpret_cast<f4*>(q.dx + base) = o[0];
          *reinterpret_cast<f4*>(q.dx + base + px) = o[1];
          *reinterpret_cast<f4*>(q.dx + base + row) = o[2];
          *reinterpret_cast<f4*>(q.dx + base + row + px) = o[3];
          if (cut_c) {
            *reinterpret_cast<f4*>(q.dx + base + 2 * px) = zero;
            *reinterpret_cast<f4*>(q.dx + base + row + 2 * px) = zero;
          }
          if (cut_r) {
            *reinterpret_cast<f4*>(q.dx + base + 2 * row) = zero;
            *reinterpret_cast<f4*>(q.dx + base + 2 * row + px) = zero;
            if (cut_c) *reinterpret_cast<f4*>(q.dx + base + 2 * row + 2 * px) = zero;
          }
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            if (cq * 4 + e >= q.ncols) continue;
            const int arg = q.argmax[win * px + cq * 4 + e];
            const float g = !(q.py[win * (size_t)q.pldy + cq * 4 + e] > 0.f) ? 0.f : v[e];
            float* dst = q.dx + base + e;
            dst[0] = arg == 0 ? g : 0.f;
            dst[px] = arg == 1 ? g : 0.f;
            dst[row] = arg == 2 ? g : 0.f;
            dst[row + px] = arg == 3 ? g : 0.f;
            if (cut_c) dst[2 * px] = dst[row + 2 * px] = 0.f;
            if (cut_r) {
              dst[2 * row] = dst[2 * row + px] = 0.f;
              if (cut_c) dst[2 * row + 2 * px] = 0.f;
            }
          }
        }
      }
    }
  }
}

int wino_bwd_finish(const a3d_conv_desc* d, const WinoGradGeom& gg, const float* slabs, const float* bparts, float* dw, float* db,
                    const float* M, float* dx, const float* mask, const WinoBwdPool* pool, hipStream_t st) {
  const WinoGeom g = wino_geom(d, true);
  WinoBwdFinish q{};
  q.slabs = slabs; q.bparts = bparts; q.dw = dw; q.db = db; q.c = d->c; q.k = d->k; q.Cp = gg.Cp; q.Kp = gg.Kp; q.splits = gg.splits;
  q.M = M; q.dx = dx; q.mask = mask; q.oh = g.oh; q.ow = g.ow; q.ncols = g.N; q.ld = d->ldx; q.th = g.th; q.tw = g.tw; q.Np = g.Np;
  q.T = g.T; q.dw_items = (size_t)d->c * d->k;
  bool vec = g.N % 4 == 0 && aligned16(dx);
  if (pool) {
    q.argmax = pool->argmax; q.py = pool->y; q.pldy = pool->ldy; q.h2 = pool->h2; q.w2 = pool->w2;
    vec = vec && pool->ldy % 4 == 0 && aligned16(pool->y) && (reinterpret_cast<uintptr_t>(pool->argmax) & 3) == 0;
  } else {
    vec = vec && d->ldx % 4 == 0 && aligned16(mask);
  }
  const dim3 grid(grid_for(q.dw_items + g.T * (size_t)(g.Np / 4), 256, 1u << 20)), block(256);
  clear_stale_error();
  if (pool && vec) hipLaunchKernelGGL((wino_bwd_finish_kernel<true, true>), grid, block, 0, st, q);
  else if (pool) hipLaunchKernelGGL((wino_bwd_finish_kernel<false, true>), grid, block, 0, st, q);
  else if (vec) hipLaunchKernelGGL((wino_bwd_finish_kernel<true, false>), grid, block, 0, st, q);
  else hipLaunchKernelGGL((wino_bwd_finish_kernel<false, false>), grid, block, 0, st, q);
  return check_launch("wino_bwd_finish");
}

}  // namespace a3d
