// wino1d.hip — the two gradients of a stride-1 convolution with a window 5 wide through 1-D Winograd F(4,5) along the width, in
// fp32 (include/a3d_wino1d.h).  A row of 4 outputs costs 8 multiplies instead of 20 and the transformed operand is only twice the
// tensor; the window's rows stay a direct r x 1 convolution inside the product GEMM.  The stages are wino.hip's:
//   bwd-data:  U[xi][r] = G g' (taps flipped, channels swapped; once per weight change or per call), V[xi] = B^T of every 8-column
//              window of dz, eight products M[xi] = conv_{r x 1}(V[xi], U[xi]) as ONE launch of the fp32 forward GEMM body
//              (blockIdx.y = xi) dealt as stream-K shares per plane, the fix-up of the tiles two blocks share, and dx = A^T M.
//   filter:    V[xi] = B^T of x's windows, Z[xi] = A dz, eight filter-gradient GEMMs of an r x 1 convolution in one launch of the
//              bwd-filter body with the pixel axis split the classic way, and dw = G^T (splits added in ascending order); db is the
//              column sum of Z's plane of point 1 (a tile's four dz added).
// V, U, Z and M are padded to whole 16-byte pieces of channels (zeros).  Every sum has a fixed order: no atomics.
#include "a3d_internal.h"
#include "igemm.h"
#include "igemm_cfgs.h"
#include "wino1d_mats.h"

namespace a3d {

typedef float f4 __attribute__((ext_vector_type(4)));

// out = Mx in (TR: Mx^T in), each sum in ascending order of the input's index, zero entries skipped: the matrices are literals, so
// every product below is a fixed chain of multiply-adds
template <typename C, int ROWS, int COLS, const C (&Mx)[ROWS][COLS], bool TR, int J, int L, typename T>
__device__ __forceinline__ void w1_dot(const T (&in)[TR ? ROWS : COLS], T& acc) {
  if constexpr (L < (TR ? ROWS : COLS)) {
    constexpr C c = TR ? Mx[L][J] : Mx[J][L];
    if constexpr (c != C(0)) acc += c * in[L];
    w1_dot<C, ROWS, COLS, Mx, TR, J, L + 1, T>(in, acc);
  }
}
template <typename C, int ROWS, int COLS, const C (&Mx)[ROWS][COLS], bool TR, typename T, int J = 0>
__device__ __forceinline__ void w1_apply(const T (&in)[TR ? ROWS : COLS], T (&out)[TR ? COLS : ROWS]) {
  if constexpr (J < (TR ? COLS : ROWS)) {
    T acc = T(0);
    w1_dot<C, ROWS, COLS, Mx, TR, J, 0, T>(in, acc);
    out[J] = acc;
    w1_apply<C, ROWS, COLS, Mx, TR, T, J + 1>(in, out);
  }
}

// ---- filter transform (bwd-data form): w [R][5][c][k] -> U [8][R][Kp][Np], U[xi][r][k][c] = sum_s G[xi][s] w[R-1-r][4-s][c][k];
//      rows >= k and columns >= c zero ----
__global__ __launch_bounds__(256) void wino1d_filter_kernel(const float* __restrict__ w, float* __restrict__ U, int c, int k, int R, int Kp,
                                                            int Np) {
  const size_t plane = (size_t)R * Kp * Np;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < plane; i += (size_t)gridDim.x * 256) {
    const int col = (int)(i % Np), row = (int)((i / Np) % Kp), r = (int)(i / ((size_t)Np * Kp));
    float g[5], u[8];
#pragma unroll
    for (int s = 0; s < 5; ++s) g[s] = (row < k && col < c) ? w[((size_t)((R - 1 - r) * 5 + (4 - s)) * c + col) * k + row] : 0.f;
    w1_apply<float, 8, 5, kW1G, false, float>(g, u);
#pragma unroll
    for (int xi = 0; xi < 8; ++xi) U[(size_t)xi * plane + i] = u[xi];
  }
}

// ---- input transform: src [rows][W][ld] -> V [8][rows][tw][Cp], B^T of the 8-column window at column 4 t - off; positions outside
//      the row read as zero.  One thread per (row, tile, 4 channels).  VEC: 16-byte loads (c % 4 == 0, ld % 4 == 0, src on the
//      16-byte grid); otherwise float by float, channels >= c zero ----
template <bool VEC>
__global__ __launch_bounds__(256) void wino1d_input_kernel(const float* __restrict__ src, float* __restrict__ V, int W, int c, int ld, int off,
                                                           int tw, int Cp, size_t P) {
  const int cqn = Cp / 4;
  const size_t total = P * (size_t)cqn;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int cq = (int)(i % cqn);
    const size_t pix = i / cqn, row = pix / tw;
    const int x0 = 4 * (int)(pix % tw) - off;
    f4 d[8], v[8];
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      f4 t = f4(0.f);
      const int xx = x0 + b;
      if (xx >= 0 && xx < W) {
        const float* s = src + (row * W + xx) * (size_t)ld + cq * 4;
        if (VEC) {
          t = *reinterpret_cast<const f4*>(s);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (cq * 4 + e < c) t[e] = s[e];
        }
      }
      d[b] = t;
    }
    w1_apply<float, 8, 8, kW1BT, false, f4>(d, v);
#pragma unroll
    for (int xi = 0; xi < 8; ++xi) *reinterpret_cast<f4*>(V + ((size_t)xi * P + pix) * Cp + cq * 4) = v[xi];
  }
}

// ---- dz transform: dz [rows][wo][ld] -> Z [8][rows][tw][Kp] = A of the tile's 4 columns; columns >= wo read as zero ----
template <bool VEC>
__global__ __launch_bounds__(256) void wino1d_dz_kernel(const float* __restrict__ dz, float* __restrict__ Z, int wo, int k, int ld, int tw, int Kp,
                                                        size_t P) {
  const int cqn = Kp / 4;
  const size_t total = P * (size_t)cqn;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int cq = (int)(i % cqn);
    const size_t pix = i / cqn, row = pix / tw;
    const int x0 = 4 * (int)(pix % tw);
    f4 y[4], z[8];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      f4 t = f4(0.f);
      if (x0 + b < wo) {
        const float* s = dz + (row * wo + x0 + b) * (size_t)ld + cq * 4;
        if (VEC) {
          t = *reinterpret_cast<const f4*>(s);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (cq * 4 + e < k) t[e] = s[e];
        }
      }
      y[b] = t;
    }
    w1_apply<float, 4, 8, kW1AT, true, f4>(y, z);
#pragma unroll
    for (int xi = 0; xi < 8; ++xi) *reinterpret_cast<f4*>(Z + ((size_t)xi * P + pix) * Kp + cq * 4) = z[xi];
  }
}

// ---- output transform: M [8][rows][tw][Np] -> out [rows][w][ld] = A^T M, times (mask > 0) where a mask (laid out as out) is given.
//      Columns >= w of the last tile and channels >= ncols are never written.  VEC: 16-byte stores (ncols % 4 == 0, ld % 4 == 0,
//      out and mask on the 16-byte grid) ----
template <bool VEC>
__global__ __launch_bounds__(256) void wino1d_output_kernel(const float* __restrict__ M, float* __restrict__ out, const float* __restrict__ mask,
                                                            int w, int ncols, int ld, int tw, int Np, size_t P) {
  const int cqn = Np / 4;
  const size_t total = P * (size_t)cqn;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int cq = (int)(i % cqn);
    const size_t pix = i / cqn, row = pix / tw;
    const int x0 = 4 * (int)(pix % tw);
    f4 m[8], y[4];
#pragma unroll
    for (int xi = 0; xi < 8; ++xi) m[xi] = *reinterpret_cast<const f4*>(M + ((size_t)xi * P + pix) * Np + cq * 4);
    w1_apply<float, 4, 8, kW1AT, false, f4>(m, y);
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      if (x0 + b >= w) continue;
      const size_t o = (row * w + x0 + b) * (size_t)ld + cq * 4;
      f4 v = y[b];
      if (VEC) {
        if (mask) {
          const f4 a = *reinterpret_cast<const f4*>(mask + o);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = apply_act_grad(v[e], a[e], EPI_RELU, 1.f);
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

// ---- final transform of the filter gradient: slabs [8][splits][R Cp][Kp] -> dw [R][5][c][k] = G^T M, M = the splits added in
//      ascending order; one thread per (window row, input channel, filter), which also adds the [splits][Kp] bias partials of its
//      filter into db when it is the first row's first channel's.  Nothing but dw and db is written ----
__global__ __launch_bounds__(256) void wino1d_dw_kernel(const float* __restrict__ slabs, const float* __restrict__ bparts, float* __restrict__ dw,
                                                        float* __restrict__ db, int c, int k, int R, int Cp, int Kp, int splits) {
  const size_t total = (size_t)R * c * k, plane = (size_t)R * Cp * Kp;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int col = (int)(i % k), row = (int)((i / k) % c), r = (int)(i / ((size_t)k * c));
    const size_t at = ((size_t)r * Cp + row) * Kp + col;
    // in double: the eight terms of a tap are some twenty times the sum they cancel to, and a tap at the map's edge may sum a
    // handful of products only; the splits are added in double on the way
    double m[8], g[5];
#pragma unroll
    for (int xi = 0; xi < 8; ++xi) m[xi] = (double)slabs[(size_t)xi * splits * plane + at];
    for (int z = 1; z < splits; ++z) {      // a split's eight loads in flight together
      float v[8];
#pragma unroll
      for (int xi = 0; xi < 8; ++xi) v[xi] = slabs[((size_t)xi * splits + z) * plane + at];
#pragma unroll
      for (int xi = 0; xi < 8; ++xi) m[xi] += (double)v[xi];
    }
    w1_apply<double, 8, 5, kW1Gd, true, double>(m, g);
#pragma unroll
    for (int s = 0; s < 5; ++s) dw[((size_t)(r * 5 + s) * c + row) * k + col] = (float)g[s];
    if (db && r == 0 && row == 0) {
      float s = bparts[col];
      for (int z = 1; z < splits; ++z) s += bparts[(size_t)z * Kp + col];
      db[col] = s;
    }
  }
}

// ---- F(4,5): eight planes.  The strides between the planes of V, U, M and the stream-K slabs [2 * blocks][128 * bn] (bwd-data)
//      and of V, Z and the raw slabs (filter gradient), whose bias partials belong to the plane of point 1 ----
constexpr int kPlanes = 8;
static PlaneBatch wino1d_batch(const Wino1dGeom& g) {
  return {g.Pv * (size_t)g.Kp, (size_t)g.R * g.Kp * g.Np, g.Pm * (size_t)g.Np, (size_t)2 * g.blocks * 128 * g.bn, -1};
}
static PlaneBatch wino1d_grad_batch(const Wino1dGradGeom& g) {
  return {g.Px * (size_t)g.Cp, g.Pz * (size_t)g.Kp, (size_t)g.splits * g.R * g.Cp * g.Kp, 0, 1};
}

// the fix-up of the tiles that two stream-K shares of a plane of bwd-data's products meet in (blockIdx.z = plane)
template <int BN, int WAVES_M, int NWAVES>
__global__ __launch_bounds__(256) void wino1d_fixup_kernel(const IgemmParams p, const uint32_t nblk, const PlaneBatch bt) {
  igemm_fixup_body<MODE_FWD, kBM, BN, WAVES_M, NWAVES>(plane_params(p, bt, blockIdx.z), nblk, blockIdx.x, blockIdx.y);
}

// ---- work division: two pure functions, asked by the workspace queries and by the launches ----
// Blocks per plane of bwd-data's products.  The eight planes share one round of the chip's 512 block slots (two blocks on each
// of 256 CUs, for the four-wave 128 x 96 tile and the eight-wave 128 x 128 one alike), 64 blocks a plane, and a plane's (tile,
// k-tile) iterations are dealt to them as equal stream-K shares: at B = 32 conv2d_1 has 67.5 tiles of 128 rows a plane, which as
// whole tiles would put 3 blocks on the busiest CU against a mean of 2.1.  A share keeps at least kMinShare k-tiles (a shorter K
// loop is all prologue and slab traffic).  Swept at B = 8, 16, 32 (profiles/wino1d_split_sweep.txt): 64 is the fastest count or
// within 1 us of it in all three; 72 and 96, a second partial round, cost 20-30 %.
constexpr int kMinShare = 4;
int wino1d_bwd_blocks(long tiles, long nk) {
  long b = std::max(1L, std::min((long)(kBlockSlots / kPlanes), tiles * nk / kMinShare));
  const int forced = tune_int("A3D_WINO1D_BLOCKS", 0);      // tuning processes only (A3D_TUNING=1): the sweep behind the rule
  if (forced > 0) b = std::min((long)forced, std::min(tiles * nk, 128L));
  return (int)b;
}

// plane_splits for eight planes, the larger count on a tie
int wino1d_grad_splits(int M, int N, size_t pixels) { return plane_splits(kPlanes, M, N, pixels, true, "A3D_WINO1D_GRAD_SPLIT"); }

Wino1dGeom wino1d_geom(const a3d_conv_desc* d) {
  Wino1dGeom g{};
  g.R = d->r;
  g.tw = (d->w + 3) / 4;
  g.off = 4 - d->pad_l;
  g.Pv = (size_t)d->n * d->ho * g.tw;
  g.Pm = (size_t)d->n * d->h * g.tw;
  g.K = d->k; g.N = d->c;
  g.Kp = (g.K + 3) / 4 * 4;
  g.Np = (g.N + 3) / 4 * 4;
  g.bn = g.Np <= 96 ? 96 : 128;
  g.tiles_m = (int)((g.Pm + 127) / 128);
  g.tiles_n = (g.Np + g.bn - 1) / g.bn;
  g.nk = (g.R * g.Kp + kBK - 1) / kBK;
  g.blocks = wino1d_bwd_blocks((long)g.tiles_m * g.tiles_n, g.nk);
  g.v_bytes = up256((size_t)kPlanes * g.Pv * g.Kp * 4);
  g.m_bytes = up256((size_t)kPlanes * g.Pm * g.Np * 4);
  g.u_bytes = up256((size_t)kPlanes * g.R * g.Kp * g.Np * 4);
  g.sk_bytes = up256((size_t)kPlanes * 2 * g.blocks * 128 * g.bn * 4);
  return g;
}

Wino1dGradGeom wino1d_grad_geom(const a3d_conv_desc* d) {
  Wino1dGradGeom g{};
  g.R = d->r;
  g.tw = (d->wo + 3) / 4;
  g.Px = (size_t)d->n * d->h * g.tw;
  g.Pz = (size_t)d->n * d->ho * g.tw;
  g.Cp = (d->c + 3) / 4 * 4;
  g.Kp = (d->k + 3) / 4 * 4;
  g.splits = wino1d_grad_splits(g.R * g.Cp, g.Kp, g.Pz);
  g.v_bytes = up256((size_t)kPlanes * g.Px * g.Cp * 4);
  g.z_bytes = up256((size_t)kPlanes * g.Pz * g.Kp * 4);
  g.slab_bytes = up256((size_t)kPlanes * g.splits * g.R * g.Cp * g.Kp * 4);
  g.bias_bytes = up256((size_t)g.splits * g.Kp * 4);
  return g;
}

// fp32 tensors, a window 5 wide at stride 1 (pad_l <= 4 then), and planes whose rows the GEMM bodies can address: a plane is one
// tensor of the body's, its byte offsets are 31-bit
bool wino1d_applicable(const a3d_conv_desc* d) {
  if (d->precision != A3D_PREC_F32 || d->storage || d->s != 5 || d->stride != 1 || d->pad_l > 4) return false;
  const Wino1dGeom g = wino1d_geom(d);
  const Wino1dGradGeom gg = wino1d_grad_geom(d);
  const double lim = 2147483647.0;
  for (double bytes : {(double)g.Pv * g.Kp, (double)g.Pm * g.Np, (double)g.R * g.Kp * g.Np, (double)gg.Px * gg.Cp, (double)gg.Pz * gg.Kp,
                       (double)g.R * gg.Cp * gg.Kp})
    if (bytes * 4.0 >= lim) return false;
  return true;
}

int wino1d_filter(const a3d_conv_desc* d, const float* w, float* U, hipStream_t st) {
  const Wino1dGeom g = wino1d_geom(d);
  clear_stale_error();
  hipLaunchKernelGGL(wino1d_filter_kernel, dim3(grid_for((size_t)g.R * g.Kp * g.Np)), dim3(256), 0, st, w, U, d->c, d->k, g.R, g.Kp, g.Np);
  return check_launch("wino1d_filter");
}

int wino1d_input(const float* src, float* V, size_t rows, int W, int c, int ld, int off, int tw, int Cp, hipStream_t st) {
  const size_t P = rows * tw;
  const bool vec = c % 4 == 0 && ld % 4 == 0 && aligned16(src);
  const dim3 grid(grid_for(P * (size_t)(Cp / 4), 256, 1u << 20)), block(256);
  clear_stale_error();
  if (vec) hipLaunchKernelGGL(wino1d_input_kernel<true>, grid, block, 0, st, src, V, W, c, ld, off, tw, Cp, P);
  else hipLaunchKernelGGL(wino1d_input_kernel<false>, grid, block, 0, st, src, V, W, c, ld, off, tw, Cp, P);
  return check_launch("wino1d_input");
}

int wino1d_dz(const a3d_conv_desc* d, const Wino1dGradGeom& g, const float* dz, float* Z, hipStream_t st) {
  const bool vec = d->k % 4 == 0 && d->ldy % 4 == 0 && aligned16(dz);
  const dim3 grid(grid_for(g.Pz * (size_t)(g.Kp / 4), 256, 1u << 20)), block(256);
  clear_stale_error();
  if (vec) hipLaunchKernelGGL(wino1d_dz_kernel<true>, grid, block, 0, st, dz, Z, d->wo, d->k, d->ldy, g.tw, g.Kp, g.Pz);
  else hipLaunchKernelGGL(wino1d_dz_kernel<false>, grid, block, 0, st, dz, Z, d->wo, d->k, d->ldy, g.tw, g.Kp, g.Pz);
  return check_launch("wino1d_dz");
}

int wino1d_output(const a3d_conv_desc* d, const Wino1dGeom& g, const float* M, float* dx, const float* mask, hipStream_t st) {
  const bool vec = g.N % 4 == 0 && d->ldx % 4 == 0 && aligned16(dx) && aligned16(mask);
  const dim3 grid(grid_for(g.Pm * (size_t)(g.Np / 4), 256, 1u << 20)), block(256);
  clear_stale_error();
  if (vec) hipLaunchKernelGGL(wino1d_output_kernel<true>, grid, block, 0, st, M, dx, mask, d->w, g.N, d->ldx, g.tw, g.Np, g.Pm);
  else hipLaunchKernelGGL(wino1d_output_kernel<false>, grid, block, 0, st, M, dx, mask, d->w, g.N, d->ldx, g.tw, g.Np, g.Pm);
  return check_launch("wino1d_output");
}

int wino1d_dw(const a3d_conv_desc* d, const Wino1dGradGeom& g, const float* slabs, const float* bparts, float* dw, float* db, hipStream_t st) {
  clear_stale_error();
  hipLaunchKernelGGL(wino1d_dw_kernel, dim3(grid_for((size_t)g.R * d->c * d->k, 256, 1u << 20)), dim3(256), 0, st, slabs, bparts, dw, db, d->c,
                     d->k, g.R, g.Cp, g.Kp, g.splits);
  return check_launch("wino1d_dw");
}

// m = the rows of the eight planes, n = c, k = r k: the FLOPs executed, under the tile launched
a3d_timing_record wino1d_record(const Wino1dGeom& g) {
  return timing_record(MODE_BWD_D, A3D_PREC_F32, 128, g.bn, 4, g.bn == 96 ? 4 : 8, kBK, 4, 4, 0, (int)(kPlanes * g.Pm), g.N, g.R * g.K);
}
// m = r c, n = k, k = the pixels of the eight planes
a3d_timing_record wino1d_grad_record(const a3d_conv_desc* d, const Wino1dGradGeom& g) {
  a3d_timing_record r = timing_record(MODE_BWD_F, A3D_PREC_F32, kBM, kBN, kWavesM, kNWaves, kBK, 4, 4, 0, g.R * d->c, d->k, (int)(kPlanes * g.Pz));
  r.splitk = g.splits;
  return r;
}

// p: one product (wino1d_product); the eight planes' stream-K shares in one launch, then the fix-up of the tiles they share
int wino1d_gemm(IgemmParams& p, const Wino1dGeom& g, float* sk, hipStream_t st) {
  p.splitk = 1;
  p.ktiles_per_split = g.nk;
  p.tiles_m = g.tiles_m;
  p.tiles_n = g.tiles_n;
  p.slab = (size_t)p.M * p.N;
  p.streamk = 1;
  p.sk_ws = sk;
  p.div_nk = make_fastdiv((uint32_t)g.nk);
  const PlaneBatch bt = wino1d_batch(g);
  const int rc = plane_gemm(MODE_FWD, g.bn, p, bt, (unsigned)g.blocks, kPlanes, "wino1d_gemm", st);
  if (rc != A3D_OK) return rc;
  const dim3 grid((unsigned)(g.tiles_m * g.tiles_n), (128 * g.bn / 256 + 3) / 4, kPlanes);
  if (g.bn == 96) hipLaunchKernelGGL((wino1d_fixup_kernel<96, 4, 4>), grid, dim3(256), 0, st, p, (uint32_t)g.blocks, bt);
  else hipLaunchKernelGGL((wino1d_fixup_kernel<kBN, kWavesM, kNWaves>), grid, dim3(256), 0, st, p, (uint32_t)g.blocks, bt);
  return check_launch("wino1d_fixup");
}

// p: one product (wino1d_grad_product), splits and tiles filled in here
int wino1d_grad_gemm(IgemmParams& p, const Wino1dGradGeom& g, hipStream_t st) {
  plane_tiles(p, g.splits);
  return plane_gemm(MODE_BWD_F, kBN, p, wino1d_grad_batch(g), (unsigned)(p.tiles_m * p.tiles_n * p.splitk), kPlanes, "wino1d_grad_gemm", st);
}

}  // namespace a3d
