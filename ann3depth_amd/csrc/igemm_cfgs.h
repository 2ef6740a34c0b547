// igemm_cfgs.h — the tile configurations of the implicit-GEMM kernels, written down once.  The launch switches
// (igemm_inst.h, igemm_ring.hip) and the host tables the planner and launch_igemm read are all generated from the three
// lists below, so a planned tile is the launched tile by construction.  Plain C++: nothing of HIP in here.
#pragma once
#include <array>

namespace a3d {

// Register-staged fp32 kernel (igemm.h): index, BM, BN, WAVES_M, NWAVES, BK, eff.
// eff: relative efficiency of the configuration, fitted (tools/fit_planner.py); 0 = only via A3D_FORCE_CFG
#define A3D_CFGS(X)                                                                                          \
  X(0, 128, 128, 2, 4, 32, 1.00f) X(1, 128, 96, 4, 4, 32, 1.00f) X(2, 128, 64, 4, 4, 32, 0.92f)             \
  X(3, 128, 32, 4, 4, 32, 0.60f) X(4, 64, 64, 2, 4, 32, 0.98f) X(5, 32, 128, 1, 4, 32, 0.90f)               \
  X(6, 64, 128, 1, 4, 32, 1.00f) /* 8-wave blocks: */ X(7, 128, 128, 4, 8, 32, 1.15f) X(8, 128, 64, 4, 8, 32, 1.05f)

// LDS-DMA staged fp32 kernel (igemm_glds.h), forward only: index, BM, BN, WAVES_M, NWAVES, twin, eff.
// twin: the register-staged configuration of the same tile, launched instead when an operand is not 16-byte vectorisable.
// Round 1: +3-5 % over the twins; since those stage through buffer loads with addresses computed a tile ahead (round 2)
// the twins are the faster ones (fine/second forward 245 vs 259 us, conv2d_1 325 vs 339 us: profiles/r02_sweep_hot.txt)
#define A3D_GLDS_CFGS(X) X(9, 128, 128, 4, 8, 7, 1.10f) X(10, 128, 64, 4, 8, 8, 1.00f)

// LDS-DMA bf16 kernel for bf16-stored operands (igemm_ring.h): index, BM, BN, WAVES_M.  Tiles 0-3 exist for all three
// modes, 5 and 6 for forward and bwd-data, and the 96-column tile 4 for bwd-data alone (conv2d_1's 96 input channels).
#define A3D_RING_CFGS_EVERY_MODE(X) X(0, 256, 128, 4) X(1, 256, 64, 8) X(2, 256, 256, 4) X(3, 128, 128, 4)
#define A3D_RING_CFGS_FWD_BWD_D(X) A3D_RING_CFGS_EVERY_MODE(X) X(5, 512, 64, 8) X(6, 64, 128, 2)
#define A3D_RING_CFGS_BWD_D_ONLY(X) X(4, 256, 96, 8)
#define A3D_RING_CFGS(X) A3D_RING_CFGS_FWD_BWD_D(X) A3D_RING_CFGS_BWD_D_ONLY(X)

struct TileCfg {
  int bm, bn, waves_m, nwaves, bk;
  float eff;
  int twin;   // LDS-DMA staged: index of the register-staged twin; -1 for a register-staged configuration
};
struct RingTile { int bm, bn, waves_m; };

#define A3D_COUNT_(...) +1
constexpr int kNumCfgs = 0 A3D_CFGS(A3D_COUNT_) A3D_GLDS_CFGS(A3D_COUNT_);
constexpr int kNumRingCfgs = 0 A3D_RING_CFGS(A3D_COUNT_);
#undef A3D_COUNT_

// the lists as arrays, each entry at its own index whatever the order it is listed in
constexpr std::array<TileCfg, kNumCfgs> make_cfg_table() {
  std::array<TileCfg, kNumCfgs> t{};
#define X(i, bm, bn, wm, nw, bk, eff) t[i] = TileCfg{bm, bn, wm, nw, bk, eff, -1};
  A3D_CFGS(X)
#undef X
#define X(i, bm, bn, wm, nw, twin, eff) t[i] = TileCfg{bm, bn, wm, nw, t[twin].bk, eff, twin};
  A3D_GLDS_CFGS(X)
#undef X
  return t;
}
constexpr std::array<RingTile, kNumRingCfgs> make_ring_table() {
  std::array<RingTile, kNumRingCfgs> t{};
#define X(i, bm, bn, wm) t[i] = RingTile{bm, bn, wm};
  A3D_RING_CFGS(X)
#undef X
  return t;
}
inline constexpr std::array<TileCfg, kNumCfgs> kCfgs = make_cfg_table();
inline constexpr std::array<RingTile, kNumRingCfgs> kRingCfgs = make_ring_table();

// the forward-only LDS-DMA kernels of round 1 (igemm_glds.h); the register-staged ones are those that run stream-K shares
// (slabs + igemm_fixup_kernel)
constexpr bool is_glds_cfg(int c) { return kCfgs[c].twin >= 0; }

}  // namespace a3d
