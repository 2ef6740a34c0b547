// a3d_internal.h — shared between the translation units of liba3d.so (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/a3d.h"
#include "igemm_plan.h"

namespace a3d {

int set_error(int code, const char* fmt, ...);

#define A3D_CHECK_ARG(cond, ...)                                 \
  do {                                                           \
    if (!(cond)) return ::a3d::set_error(A3D_EINVAL, __VA_ARGS__); \
  } while (0)

// hipGetLastError() is sticky across unrelated runtime calls made by the process (PyTorch probes devices, etc.):
// clear it before launching so check_launch() reports only this launch.
inline void clear_stale_error() { (void)hipGetLastError(); }

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_error(A3D_ELAUNCH, "%s: %s", what, hipGetErrorString(e));
  return A3D_OK;
}

// blocks of a grid-stride launch: one thread per unit of work, at most `cap` blocks
inline unsigned grid_for(size_t total, int per_block = 256, unsigned cap = 8192) {
  size_t g = (total + per_block - 1) / per_block;
  return (unsigned)std::min<size_t>(std::max<size_t>(g, 1), cap);
}

__host__ __device__ inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// workspace segments start on 256-byte boundaries
inline size_t up256(size_t b) { return (b + 255) / 256 * 256; }

// Raises a kernel's dynamic-LDS limit once per device.  The limit is a per-DEVICE attribute of the kernel: `done` is the
// call site's `static bool[64]`, one flag per device (a benign race at worst sets it twice)
inline int raise_lds(const void* kern, size_t bytes, bool (&done)[64]) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev < 0 || dev >= 64 || !done[dev]) {
    hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return set_error(A3D_ELAUNCH, "hipFuncSetAttribute: %s", hipGetErrorString(e));
    if (dev >= 0 && dev < 64) done[dev] = true;
  }
  return A3D_OK;
}

// ---- implicit-GEMM launch layer (igemm_launch.hip) under the front end (igemm_host.hip); the planner: igemm_plan.h, igemm_plan.cc ----
struct IgemmParams;
int launch_igemm(int mode, const GemmPlan& plan, int avec, int bvec, IgemmParams& p, void* ws, hipStream_t st);
int take_second_output(IgemmParams& p, const a3d_second_output* o);      // a3d_second_output -> the host-only fields of IgemmParams

// opt-in launch timing (a3d_timing_*)
struct TimingSlot {
  hipEvent_t start, stop;
  a3d_timing_record rec;
};
bool timing_wanted(const a3d_timing_record& r);
int timing_begin(TimingSlot& slot, hipStream_t st);
void timing_end(TimingSlot& slot, hipStream_t st);
// The record of a launch that computes an m x n x k GEMM unsplit; callers overwrite what differs (splitk, flops).
a3d_timing_record timing_record(int mode, int prec, int bm, int bn, int waves_m, int nwaves, int bk, int avec, int bvec, int lds_dma,
                                int m, int n, int k);
// Runs launch() on `st`, between two events when the timing list wants launches like `rec`; returns launch()'s code.  If
// the events cannot be had, that error is returned and launch() is not called: nothing is enqueued.
template <typename Launch>
int timed_launch(const a3d_timing_record& rec, hipStream_t st, Launch&& launch) {
  if (!timing_wanted(rec)) return launch();
  TimingSlot slot{};
  slot.rec = rec;
  int rc = timing_begin(slot, st);
  if (rc != A3D_OK) return rc;
  rc = launch();
  timing_end(slot, st);
  return rc;
}

// ---- weight-streaming dense kernels for batches of at most 64 rows (dense.hip) ----
bool dense_dw_applicable(int m, int k, int n);
bool dense_stream_applicable(int m, int k, int n);
size_t dense_stream_ws_bytes(int m, int k, int n);
int dense_fwd_stream(int m, int k, int n, const float* x, const float* w, const float* bias, float* y, int act,
                     const uint8_t* keep, float keep_scale, void* ws, size_t ws_bytes, hipStream_t st);
struct ReduceParams;
int launch_splitk_reduce(const ReduceParams& r, hipStream_t st);
int dense_dw_launch(int m, int k, int n, const float* x, const float* dz, float* dw, float* db, hipStream_t st);

// ---- BiasAddGrad of a bf16 gradient tensor beside the LDS-DMA bwd-filter (igemm_ring.hip) ----
size_t colsum_bf16_ws_bytes(int n);
bool colsum_bf16_ok(int n);
int colsum_bf16(const void* dz, int rows, int n, int ld, float* out, void* ws, int* nparts, hipStream_t st);

// ---- single-output-channel 5x5 stencil (stencil1.hip) ----
bool stencil1_applicable(const a3d_conv_desc* d);
size_t stencil1_bwdf_ws_bytes(const a3d_conv_desc* d);
int stencil1_fwd(const a3d_conv_desc* d, const float* x, const float* w, const float* bias, float* y, int act,
                 hipStream_t st);
int stencil1_bwd_filter(const a3d_conv_desc* d, const float* x, const float* dz, float* dw, float* db, void* ws,
                        hipStream_t st);
bool stencil1_bwd_both_applicable(const a3d_conv_desc* d);
size_t stencil1_bwd_both_ws_bytes(const a3d_conv_desc* d);
int stencil1_bwd_both(const a3d_conv_desc* d, const float* x, const float* dz, const float* w, float* dw, float* db,
                      void* dx, int lddx, int dx_bf16, int relu_mask, unsigned* state, void* ws, hipStream_t st);

// ---- few-channel filter gradient from LDS-staged input rows, optionally with the max pool's gradient fused (fewch.hip) ----
bool fewch_bwdf_applicable(const a3d_conv_desc* d, bool pooled);
size_t fewch_bwdf_ws_bytes(const a3d_conv_desc* d, bool pooled);
bool fewch_extents_ok(const a3d_conv_desc* d, bool pooled, int ldz, int esz, int ld_arg);
int fewch_bwd_filter(const a3d_conv_desc* d, const float* x, int src, const void* dz, int ldz, const void* pooled_act,
                     const uint8_t* argmax, int ld_arg, float* dw, float* db, void* ws, hipStream_t st);

int fewch_reduce_launch(const float* slabs, int splits, int Mp, int NP, int M, int N, float* dw, float* db, hipStream_t st);
// ... on the bf16 matrix cores (float32 image, bf16 gradient tensors: config 5; fewch16.hip)
bool fewch16_bwdf_applicable(const a3d_conv_desc* d, bool pooled);
size_t fewch16_bwdf_ws_bytes(const a3d_conv_desc* d, bool pooled);
int fewch16_bwd_filter(const a3d_conv_desc* d, const float* x, bool pooled, const void* dz, int ldz, const void* pooled_act,
                       const uint8_t* argmax, int ld_arg, float* dw, float* db, void* ws, hipStream_t st);

// ---- few-channel forward convolution straight from L2 (conv3.hip) ----
bool conv3_applicable(const a3d_conv_desc* d, unsigned x_off);      // x_off: x's address & 15
size_t conv3_ws_bytes(const a3d_conv_desc* d);
int conv3_pack(const a3d_conv_desc* d, const float* w, float* wp, hipStream_t st);
int conv3_fwd(const a3d_conv_desc* d, const float* x, const float* w, const float* bias, float* y, int act, int pool,
              int ld_out, uint8_t* argmax, void* ws, size_t ws_bytes, hipStream_t st, bool prepared = false);

// ---- the same from a 4-channel bf16 image on the bf16 matrix cores (conv3.hip, conv3b_*) ----
bool conv3b_applicable(const a3d_conv_desc* d);
size_t conv3b_filter_bytes(const a3d_conv_desc* d);
int conv3b_pack(const a3d_conv_desc* d, const float* w, void* wp, hipStream_t st);
int conv3b_fwd(const a3d_conv_desc* d, const void* x, const float* w, const float* bias, void* y, int act, int pool, int ld_out,
               uint8_t* argmax, void* ws, size_t ws_bytes, hipStream_t st, bool prepared);

// ---- what the Winograd routes below share (wino.hip).  A route supplies its transform kernels, a geometry (the planes' extents,
//      the segments of its workspace) and a surrogate descriptor of one plane's product (igemm_host.hip: plane_product, the
//      workspace layouts); its products run here, all planes in one launch of an fp32 GEMM body ----
struct PlaneBatch;                                                             // igemm.h: the strides between planes, the bias plane
constexpr int kBM = 128, kBN = 128, kWavesM = 4, kNWaves = 8, kBK = 32;        // the products' tile
constexpr int kBlockSlots = 512, kCUs = 256, kMinKTiles = 5;                   // blocks of that tile the chip holds at once; plane_splits
void plane_tiles(IgemmParams& p, int splits);                                  // the tiles of one product and the split of its K loop
// MODE_FWD (tile 128 x bn: 128 on eight waves, 96 on four) or MODE_BWD_F (bn = 128) on grid (blocks, planes); what: check_launch's name
int plane_gemm(int mode, int bn, const IgemmParams& p, const PlaneBatch& bt, unsigned blocks, int planes, const char* what, hipStream_t st);
// how many ways the pixel axis of `planes` bwd-filter products M x N is split; tuning: the variable that forces a count
int plane_splits(int planes, int M, int N, size_t pixels, bool larger_on_tie, const char* tuning);

// ---- Winograd F(2x2,3x3) route of A3D_PREC_F32_WINOGRAD (wino.hip); bwd: the bwd-data form of the descriptor ----
struct WinoGeom {
  int oh, ow, th, tw;                    // the output grid (bwd: dx's) and its 2x2 tiles
  size_t T;                              // n * th * tw
  int K, N, Kp, Np;                      // channels contracted / produced, and padded to whole 16-byte pieces
  size_t v_bytes, m_bytes, u_bytes;      // V [16][T][Kp], M [16][T][Np], U [16][Kp][Np]
  size_t sk_bytes;                       // 0: whole tiles, no stream-K slabs
};
WinoGeom wino_geom(const a3d_conv_desc* d, bool bwd);
bool wino_applicable(const a3d_conv_desc* d);
int wino_filter(const a3d_conv_desc* d, bool bwd, const float* w, float* U, hipStream_t st);
int wino_input(const a3d_conv_desc* d, bool bwd, const float* src, float* V, hipStream_t st);
int wino_output(const a3d_conv_desc* d, bool bwd, const float* M, float* out, const float* bias, const float* mask, int act,
                hipStream_t st);
a3d_timing_record wino_record(int mode, const WinoGeom& g);
int wino_gemm(IgemmParams& p, const WinoGeom& g, hipStream_t st);      // p: one product; the sixteen differ in A, B and C

// ---- the same identity for the filter gradient (include/a3d_wino_grad.h; wino.hip) ----
struct WinoGradGeom {
  size_t T;                              // 2x2 tiles of dz: the forward's
  int Cp, Kp;                            // c and k padded to whole 16-byte pieces
  int splits;                            // wino_grad_splits(c, k, T)
  size_t v_bytes, z_bytes;               // V [16][T][Cp], Z [16][T][Kp]
  size_t slab_bytes, bias_bytes;         // raw sums [16][splits][Cp][Kp], bias partials [splits][Kp]
};
int wino_grad_splits(int C, int K, size_t T);
WinoGradGeom wino_grad_geom(const a3d_conv_desc* d);
bool wino_grad_applicable(const a3d_conv_desc* d);      // precision F32 or F32_WINOGRAD: the entry point names the arithmetic
int wino_dz(const a3d_conv_desc* d, const float* dz, float* Z, hipStream_t st);
int wino_dw(const a3d_conv_desc* d, const WinoGradGeom& g, const float* slabs, const float* bparts, float* dw, float* db, hipStream_t st);
a3d_timing_record wino_grad_record(const a3d_conv_desc* d, const WinoGradGeom& g);
int wino_grad_gemm(IgemmParams& p, const WinoGradGeom& g, hipStream_t st);      // p: one product, splits and tiles filled in here

// ---- both gradients of a layer as one chain of three launches (include/a3d_wino_bwd.h; wino.hip) ----
struct WinoBwdPool {                     // a3dwb_pool
  const uint8_t* argmax;
  const float* y;
  int ldy, h2, w2;
};
// V_x (forward grid), V_dz (bwd-data's grid) and Z (forward grid) in one launch
int wino_bwd_transforms(const a3d_conv_desc* d, const float* x, const float* dz, float* Vx, float* Vdz, float* Z, hipStream_t st);
// wino_grad_gemm(pf, gg) and wino_gemm(pd, g) as one grid, the filter gradient's blocks first
int wino_bwd_gemm(IgemmParams& pf, const WinoGradGeom& gg, IgemmParams& pd, const WinoGeom& g, hipStream_t st);
// wino_dw and bwd-data's wino_output (no bias, no activation) in one launch; pool: the output scattered into the unpooled dx
int wino_bwd_finish(const a3d_conv_desc* d, const WinoGradGeom& gg, const float* slabs, const float* bparts, float* dw, float* db,
                    const float* M, float* dx, const float* mask, const WinoBwdPool* pool, hipStream_t st);

// ---- 1-D Winograd F(4,5) along the width for the gradients of stride-1 convolutions 5 wide (include/a3d_wino1d.h; wino1d.hip) ----
struct Wino1dGeom {                      // bwd-data
  int R, tw, off;                        // window height, tiles of 4 columns of dx, a window starts at column 4 t - off of dz
  size_t Pv, Pm;                         // pixels of one plane of V (n * ho * tw) and of M (n * h * tw)
  int K, N, Kp, Np;                      // channels contracted / produced, and padded to whole 16-byte pieces
  int bn, tiles_m, tiles_n, nk, blocks;  // the product's tile width (96 or 128), tiles and k-tiles of a plane, wino1d_bwd_blocks of them
  size_t v_bytes, m_bytes, u_bytes;      // V [8][Pv][Kp], M [8][Pm][Np], U [8][R][Kp][Np]
  size_t sk_bytes;                       // stream-K slabs [8][2 * blocks][128 * bn]
};
struct Wino1dGradGeom {                  // filter gradient
  int R, tw;                             // window height, tiles of 4 columns of dz
  size_t Px, Pz;                         // pixels of one plane of V (n * h * tw) and of Z (n * ho * tw)
  int Cp, Kp, splits;                    // c and k padded to whole 16-byte pieces; wino1d_grad_splits(R Cp, Kp, Pz)
  size_t v_bytes, z_bytes;               // V [8][Px][Cp], Z [8][Pz][Kp]
  size_t slab_bytes, bias_bytes;         // raw sums [8][splits][R Cp][Kp], bias partials [splits][Kp]
};
int wino1d_bwd_blocks(long tiles, long nk);
int wino1d_grad_splits(int M, int N, size_t pixels);
Wino1dGeom wino1d_geom(const a3d_conv_desc* d);
Wino1dGradGeom wino1d_grad_geom(const a3d_conv_desc* d);
bool wino1d_applicable(const a3d_conv_desc* d);
int wino1d_filter(const a3d_conv_desc* d, const float* w, float* U, hipStream_t st);
// src [rows][W][ld] of c channels -> V [8][rows][tw][Cp], windows at column 4 t - off
int wino1d_input(const float* src, float* V, size_t rows, int W, int c, int ld, int off, int tw, int Cp, hipStream_t st);
int wino1d_dz(const a3d_conv_desc* d, const Wino1dGradGeom& g, const float* dz, float* Z, hipStream_t st);
int wino1d_output(const a3d_conv_desc* d, const Wino1dGeom& g, const float* M, float* dx, const float* mask, hipStream_t st);
int wino1d_dw(const a3d_conv_desc* d, const Wino1dGradGeom& g, const float* slabs, const float* bparts, float* dw, float* db, hipStream_t st);
a3d_timing_record wino1d_record(const Wino1dGeom& g);
a3d_timing_record wino1d_grad_record(const a3d_conv_desc* d, const Wino1dGradGeom& g);
int wino1d_gemm(IgemmParams& p, const Wino1dGeom& g, float* sk, hipStream_t st);      // the eight products and their fix-up
int wino1d_grad_gemm(IgemmParams& p, const Wino1dGradGeom& g, hipStream_t st);

// ---- the routes' workspaces.  Each layout is written once, as the order in which its segments (the *_bytes of a geometry, each
//      a multiple of 256) are taken from a Carve.  A query carves from offset 0 and answers the end offset, a launch carves from
//      its workspace: the two cannot disagree.  The chain's layout is the first followed by the second ----
struct Carve {
  uintptr_t at;
  float* take(size_t bytes) {
    float* p = reinterpret_cast<float*>(at);
    at += bytes;
    return p;
  }
};
struct ProductWs { float *U, *V, *M, *sk; };           // forward, bwd-data: [U unless prepared][V][M][stream-K slabs]
struct GradWs { float *V, *Z, *slabs, *bparts; };      // filter gradient: [V][Z][raw slabs][bias partials]
template <typename Geom>      // WinoGeom, Wino1dGeom
ProductWs carve_product(Carve& c, const Geom& g, bool prepared) {
  ProductWs w{};
  if (!prepared) w.U = c.take(g.u_bytes);
  w.V = c.take(g.v_bytes);
  w.M = c.take(g.m_bytes);
  w.sk = c.take(g.sk_bytes);
  return w;
}
template <typename Geom>      // WinoGradGeom, Wino1dGradGeom
GradWs carve_grad(Carve& c, const Geom& g) {
  GradWs w{};
  w.V = c.take(g.v_bytes);
  w.Z = c.take(g.z_bytes);
  w.slabs = c.take(g.slab_bytes);
  w.bparts = c.take(g.bias_bytes);
  return w;
}

}  // namespace a3d
