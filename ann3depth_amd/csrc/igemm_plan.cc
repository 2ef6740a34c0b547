// igemm_plan.cc — the tile / split-K planner of the implicit-GEMM kernels: which kernel and tile a GEMM problem runs on,
// how its K axis is split, and the workspace that takes.  Host code only; the launches are igemm_launch.hip's.
#include <algorithm>
#include <array>
#include <map>
#include <mutex>

#include "../../include/a3d.h"
#include "igemm_cfgs.h"
#include "igemm_plan.h"

namespace a3d {

static const int kSlots = 512;               // 256 CUs x 2 resident blocks
static const size_t kMaxSlabBytes = (size_t)192 << 20;

// `splitk` float32 slabs of the whole output
static size_t slab_bytes(const GemmProblem& g, int splitk) { return (size_t)splitk * g.M * g.N * 4; }

// the largest factor up to `splitk` whose slabs stay below kMaxSlabBytes
static int clamp_to_slab_cap(const GemmProblem& g, int splitk) {
  while (splitk > 1 && slab_bytes(g, splitk) > kMaxSlabBytes) --splitk;
  return splitk;
}

// Finishes a split of `nk` k-tiles into `splitk` ranges: equal ranges, the factor that many ranges actually need, and the
// slabs of that factor.
static void finish_split(GemmPlan& pl, const GemmProblem& g, int nk, int splitk) {
  const int kps = (nk + splitk - 1) / splitk;
  pl.ktiles_per_split = kps;
  pl.splitk = (nk + kps - 1) / kps;
  pl.ws_bytes = pl.splitk > 1 ? slab_bytes(g, pl.splitk) : 0;
}

// an LDS-DMA staged configuration on a problem it cannot run: those kernels are forward-only, take 16-byte operands, and
// have neither the pooling epilogue nor a bf16 output — their register-staged twins do
static bool needs_twin(int c, const GemmProblem& g) {
  return is_glds_cfg(c) && (g.mode != MODE_FWD || g.avec != 4 || g.bvec != 4 || g.plain || g.no_glds);
}

// bf16-stored operands, forward / stride-1 bwd-data: igemm_ring.h.  One block of eight waves per CU works on a 256-row tile
// (128 rows, two blocks per CU, where 256-row tiles would leave a third of the chip idle); never split (a launch that small
// stays on igemm_bf16's split-K).  A3D_RING=0 turns the kernel off, A3D_RING_CFG pins a tile (tuning processes).
static bool ring_plan(const GemmProblem& g, GemmPlan& pl) {
  static const bool off = tune_int("A3D_RING", 1) == 0;
  if (!g.ring_ok || (g.plain && g.mode != MODE_FWD)) return false;      // (plain = the forward with the 2x2 max pool fused: never split)
  if (g.mode != MODE_BWD_F && g.M <= 64 && g.N >= 1024 && g.K >= 1024) {      // (not under A3D_RING: bf16 x / dz have no other kernel)
    // a dense layer of a small batch: a weight stream.  64-row tiles of 128 columns, K split until ~512 blocks (three per
    // CU) pull on HBM; the slabs are a few MB
    pl.ring = 1 + 6;
    pl.tiles_m = 1;
    pl.tiles_n = (g.N + 127) / 128;
    const int nk = std::max(1, (g.K + 63) / 64);
    int splitk = (int)std::min<long>(std::max<long>(512 / pl.tiles_n, 1), std::max(1, nk / 4));
    if (tune_int("A3D_FORCE_SPLITK", 0) > 0) splitk = std::min(tune_int("A3D_FORCE_SPLITK", 0), nk);
    if (g.need_reduce && nk >= 2) splitk = std::max(splitk, 2);      // rows narrower than the GEMM: stored by the reduction
    finish_split(pl, g, nk, splitk);       // (not clamped to kMaxSlabBytes: at most 64 rows per slab)
    return true;
  }
  if (off && !g.plain) return false;              // (a pooled forward on bf16 inputs has no other kernel: ADVICE r4)
  if (g.need_reduce) return false;                // the tiles below are never split: igemm_bf16's split-K stores the narrower rows
  if (g.mode == MODE_BWD_F) {
    // filter gradient: few tiles (M = r s Cin rows) over a long pixel axis — 256-row tiles, split-K until every CU has one block
    if (g.M < 512 || g.N < 64 || g.K < 64 * 64) return false;      // (short pixel axes stay with igemm_bf16's finer tiles)
    int cfg = g.N <= 64 ? 1 : (g.N % 256 == 0 ? 2 : 0);
    const int forced = tune_int("A3D_RING_CFG", -1);
    if (forced >= 0 && forced <= 3) cfg = forced;
    const int bm = kRingCfgs[cfg].bm, bn = kRingCfgs[cfg].bn;
    pl.tiles_m = (g.M + bm - 1) / bm;
    pl.tiles_n = (g.N + bn - 1) / bn;
    const long tiles = (long)pl.tiles_m * pl.tiles_n;
    const int nk = std::max(1, (g.K + 63) / 64);
    int splitk = (int)std::min<long>(std::max<long>(256 / tiles, 1), std::max(1, nk / 8));
    if (tune_int("A3D_FORCE_SPLITK", 0) > 0) splitk = std::min(tune_int("A3D_FORCE_SPLITK", 0), nk);
    pl.ring = 1 + cfg;
    finish_split(pl, g, nk, clamp_to_slab_cap(g, splitk));
    return true;
  }
  int cfg;
  if (g.mode == MODE_BWD_D && g.N <= 96 && g.N > 64) cfg = 4;
  else if (g.N <= 64) cfg = (g.M + 511) / 512 >= 192 ? 5 : 1;      // 64 columns: 512-row tiles (wave tiles of 64 x 64) when they fill the chip
  else if (g.N % 256 == 0 && (long)((g.M + 255) / 256) * (g.N / 256) >= 192) cfg = 2;
  else cfg = (long)((g.M + 255) / 256) * ((g.N + 127) / 128) >= 192 ? 0 : 3;
  const int forced = tune_int("A3D_RING_CFG", -1);
  if (forced >= 0 && forced <= 6 && !(forced == 4 && g.mode != MODE_BWD_D) && !(forced == 6 && g.plain)) cfg = forced;
  const int bm = kRingCfgs[cfg].bm, bn = kRingCfgs[cfg].bn;
  const long tiles = (long)((g.M + bm - 1) / bm) * ((g.N + bn - 1) / bn);
  if (tiles < 96 && forced < 0 && !g.plain) return false;      // (a pooled forward on bf16 inputs has no other kernel)
  pl.ring = 1 + cfg;
  pl.tiles_m = (g.M + bm - 1) / bm;
  pl.tiles_n = (g.N + bn - 1) / bn;
  pl.splitk = 1;
  pl.ktiles_per_split = std::max(1, (g.K + 63) / 64);
  pl.ws_bytes = 0;
  return true;
}

// bf16 / bf16x3 kernel: BM = 128.  Staging-bound rather than MFMA-bound: the wider tile wins whenever N allows it
// (even at one block per CU for the two-plane x3 variant); split-K factors: x3 by round 1's sweep
// (profiles/r01_sweep_bf16.txt: ~600 blocks with >= 12 k-tiles each), plain bf16 by round 3's, below.
static GemmPlan plan_gemm_bf16(const GemmProblem& g, int precision) {
  GemmPlan pl{};
  pl.prec = precision;
  if (precision == A3D_PREC_BF16 && ring_plan(g, pl)) return pl;
  pl.bf16_bn = g.N <= 64 ? 64 : 128;
  if (tune_int("A3D_BF16_BN", 0) == 64 || tune_int("A3D_BF16_BN", 0) == 128) pl.bf16_bn = tune_int("A3D_BF16_BN", 0);
  pl.tiles_m = (g.M + 127) / 128;
  pl.tiles_n = (g.N + pl.bf16_bn - 1) / pl.bf16_bn;
  const int bk = precision == A3D_PREC_BF16X3 ? 32 : 64;        // Bf16Cfg::BK: the plain bf16 kernel takes k-tiles of 64
  const int nk = std::max(1, (g.K + bk - 1) / bk);
  const long tiles = (long)pl.tiles_m * pl.tiles_n;
  int splitk = (int)std::min<long>(std::max<long>(768 / tiles, 1), std::max(1, nk * (bk / 32) / 12));
  if (precision == A3D_PREC_BF16) {
    // Plain bf16 kernel, measured (profiles/r03_bf16_splitk_sweep.txt): one 128 x 128 block keeps a CU's staging path
    // nearly as busy as two do (0.87 us per k-tile alone, 1.47 us each when two share the CU), so splitting K pays only
    // until every CU has ONE block (two of the lighter 128 x 64 ones); past that it just adds a slab of the whole
    // output per factor (conv2d_2 / conv2d_3 forward and bwd-data at batch 64: 351 tiles, 53 / 71 us unsplit against
    // 72 / 85 us split in two).
    const long target = pl.bf16_bn == 128 ? 256 : 512;
    splitk = (int)std::min<long>(std::max<long>(target / tiles, 1), std::max(1, nk / 4));
  }
  if (tune_int("A3D_FORCE_SPLITK", 0) > 0) splitk = std::min(tune_int("A3D_FORCE_SPLITK", 0), std::max(1, nk));
  if (g.need_reduce && nk >= 2) splitk = std::max(splitk, 2);
  if (g.plain) splitk = 1;                      // fused pool: whole K ranges only
  finish_split(pl, g, nk, clamp_to_slab_cap(g, splitk));
  return pl;
}

// Measured winners for shapes where the cost model below loses more than 3 % to a configuration of the sweep
// (tools/sweep_hot.py --assert-auto-within 0.03; profiles/r03_sweep_hot.txt).  The model's block-slot count is that of
// the 8-wave tiles (two per CU); 4-wave 64x64 blocks sit four to a CU and want several thousand blocks when a handful
// of tiles carry a K of 10^5 — fine/second's bwd-filter: 64x64 x 128 splits 290 us, the model's pick 315-363 us.
struct TunedPlan { int mode, M, N, K, cfg, splitk; };
static const TunedPlan kTuned[] = {
    {MODE_BWD_F, 1600, 64, 130240, 4, 128},        // fine/second/conv2d bwd-filter at batch 32
};

static GemmPlan plan_gemm_search(const GemmProblem& g, int precision) {
  if (precision != A3D_PREC_F32 && g.avec == 4 && g.bvec == 4) return plan_gemm_bf16(g, precision);
  if (tune_int("A3D_FORCE_CFG", -1) < 0 && !g.plain) {
    for (const TunedPlan& t : kTuned) {
      if (t.mode != g.mode || t.M != g.M || t.N != g.N || t.K != g.K) continue;
      GemmPlan pl{};
      pl.cfg = t.cfg;
      pl.tiles_m = (g.M + kCfgs[t.cfg].bm - 1) / kCfgs[t.cfg].bm; pl.tiles_n = (g.N + kCfgs[t.cfg].bn - 1) / kCfgs[t.cfg].bn;
      finish_split(pl, g, std::max(1, (g.K + 31) / 32), t.splitk);
      if (pl.ws_bytes <= kMaxSlabBytes) return pl;      // (not clamped: past the cap the search below plans the problem)
    }
  }
  GemmPlan best{};
  double best_t = 1e300;
  const int nk = std::max(1, (g.K + 31) / 32);
  const int force_cfg = tune_int("A3D_FORCE_CFG", -1), force_split = tune_int("A3D_FORCE_SPLITK", -1);
  const int force_streamk = std::min(tune_int("A3D_FORCE_STREAMK", 0), 1024);      // tuning aid: stream-K with this many blocks (the fixup lists at most 1024 contributors per tile)
  if (force_cfg >= 0 && force_cfg < kNumCfgs) {
    // a pinned configuration still has to be one this problem can run on
    const int cfg = needs_twin(force_cfg, g) ? kCfgs[force_cfg].twin : force_cfg;
    const int bm = kCfgs[cfg].bm, bn = kCfgs[cfg].bn;
    const int nk = std::max(1, (g.K + kCfgs[cfg].bk - 1) / kCfgs[cfg].bk);
    int splitk = std::max(1, std::min(force_split > 0 ? force_split : 1, nk));
    if (g.need_reduce && nk >= 2) splitk = std::max(splitk, 2);      // a narrower output is stored by the split-K reduction
    if (g.plain) splitk = 1;                     // the fused pool takes whole K ranges
    best.cfg = cfg;
    best.tiles_m = (g.M + bm - 1) / bm; best.tiles_n = (g.N + bn - 1) / bn;
    finish_split(best, g, nk, clamp_to_slab_cap(g, splitk));
    if (force_streamk > 0 && !is_glds_cfg(cfg) && !g.plain && !g.need_reduce) {
      best.splitk = 1; best.ktiles_per_split = nk; best.streamk = force_streamk;
      best.ws_bytes = (size_t)2 * force_streamk * ((size_t)bm * bn + bn) * 4;
    }
    return best;
  }
  // Cost model calibrated on MI355X with tools/sweep_igemm.py (profiles/r01_sweep_igemm.txt): a block progresses at
  // ~96.5 GMAC/s when two share a CU and ~1.6x that when alone; split-K costs one slab write+read at ~3 TB/s.
  // Model picks are within 1.15x (mostly 1.05x) of the best measured configuration for every MSDN layer/direction.
  for (int c = 0; c < kNumCfgs; ++c) {
    if (kCfgs[c].eff <= 0.f) continue;
    if (needs_twin(c, g)) continue;
    const int bm = kCfgs[c].bm, bn = kCfgs[c].bn;
    const int tm = (g.M + bm - 1) / bm, tn = (g.N + bn - 1) / bn;
    const long tiles = (long)tm * tn;
    // split-K candidates: every small factor, coarser steps above, and the two factors that fill the chip's block
    // slots exactly once or twice (tiles * splitk just below 512 / 1024: a kernel of 486 blocks beats one of 648)
    int wants[48];
    int nw = 0;
    for (int w = 1; w <= 24; ++w) wants[nw++] = w;
    for (int w = 32; w <= 256; w *= 2) { wants[nw++] = w; if (w < 256) wants[nw++] = w + w / 2; }
    wants[nw++] = (int)std::max<long>(1, kSlots / tiles);
    wants[nw++] = (int)std::max<long>(1, 2 * kSlots / tiles);
    for (int wi = 0; wi < nw; ++wi) {
      const int want = wants[wi];
      if (want > 1 && g.plain) continue;
      if (want == 1 && g.need_reduce && nk >= 2) continue;      // (nk == 1: launch_igemm refuses the call, nothing is enqueued)
      if (want > 1 && want > nk / 2 && !(g.need_reduce && want == 2)) continue;
      if (want > 1 && slab_bytes(g, want) > kMaxSlabBytes) continue;
      GemmPlan cand{};
      cand.cfg = c; cand.tiles_m = tm; cand.tiles_n = tn;
      finish_split(cand, g, nk, want);
      const int kps = cand.ktiles_per_split, splitk = cand.splitk;
      const long blocks = tiles * splitk;
      double t_b = (double)bm * bn * kps * 32.0 / (96.5e3 * kCfgs[c].eff);                // us
      if (is_glds_cfg(c) && kps < 40) t_b *= 1.08;     // LDS-DMA pays off on long K ranges only (conv2d_2: 158 vs 146 us)
      double f;      // kernel time in units of t_b: the slowest CU decides (tools/fit_planner.py)
      if (blocks <= 256) f = 0.62;
      else if (blocks <= kSlots) f = 1.0;
      else f = std::max((double)blocks / kSlots + 0.08, 1.45);
      double t = t_b * f;
      if (splitk > 1) t += 2.5 + (double)g.M * g.N * 4.0 * (splitk + 1) / 3.0e6;
      if (t < best_t) {
        best_t = t;
        best = cand;
      }
    }
    // stream-K: equal shares of the (tile, k-tile) iterations for one or two blocks per CU — no tile quantisation, and
    // at most two partial slabs per block (register-staged kernels only; the pooling forward never splits)
    if (!is_glds_cfg(c) && !g.plain && !g.need_reduce) {
      const long iters = tiles * nk;
      for (int G = 256; G <= 512; G += 256) {
        if (force_streamk > 0 && G != 256) continue;
        const int grid = force_streamk > 0 ? force_streamk : G;
        if (iters < 4L * grid) continue;
        const long per = (iters + grid - 1) / grid;
        // blocks meeting in one tile: their slabs are added one after the other by the fixup, so few tiles with very
        // long K (bwd-filter of the 3-channel layers, dense layers) stay with classic split-K and its flat reduction
        const long meet = (nk + per - 1) / per + 1;
        if (force_streamk <= 0 && (meet > 16 || tiles < 24)) continue;
        double t = (double)bm * bn * per * 32.0 / (96.5e3 * kCfgs[c].eff) * (grid <= 256 ? 0.62 : 1.0);
        // ~1.5 slabs per block are written and read back, then the split tiles are written once more
        const double slabs = std::min<double>(1.5 * grid, 2.0 * tiles) * bm * bn * 4.0;
        // (round 3 refit: 4.5 TB/s for the slab traffic — the fixup reads eight slabs deep; at 3 TB/s the model preferred
        // split-K 2 for conv2d_1's bwd-data, measured 349 us against 334 for stream-K: profiles/r03_sweep_hot.txt)
        t += 3.0 + 0.4 * meet + (2.0 * slabs + (double)std::min<long>(tiles, grid) * bm * bn * 4.0) / 4.5e6;
        if (force_streamk > 0) t = 0;
        if (t < best_t) {
          best_t = t;
          best.cfg = c;
          best.splitk = 1;
          best.ktiles_per_split = nk;
          best.tiles_m = tm;
          best.tiles_n = tn;
          best.streamk = grid;
          best.ws_bytes = (size_t)2 * grid * ((size_t)bm * bn + bn) * 4;
        }
      }
    }
  }
  return best;
}

// The search above walks 11 tile configurations x ~50 split factors: once per distinct problem, not once per launch
// (a training step launches the same ~50 problems over and over).
GemmPlan plan_gemm(const GemmProblem& g, int precision) {
  if (tuning()) return plan_gemm_search(g, precision);
  static std::mutex mu;
  static std::map<std::array<int, 10>, GemmPlan> cache;
  const std::array<int, 10> key = {g.mode, g.M, g.N, g.K, g.avec, g.bvec, g.plain + 2 * g.need_reduce, g.no_glds, precision, g.ring_ok};
  std::lock_guard<std::mutex> lk(mu);
  auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  const GemmPlan plan = plan_gemm_search(g, precision);
  cache.emplace(key, plan);
  return plan;
}

// A launch whose operands lie off the 16-byte grid plans another GEMM than its *_ws_bytes query did (scalar gathers: another tile,
// another split): it keeps the query's promise by splitting no deeper than the bytes it was given allow.  The LDS-DMA plans
// (bf16 tensors, always on the grid) and a plan that must end in a reduction (need_reduce) are left as they are.
GemmPlan plan_within(const GemmProblem& g, GemmPlan pl, size_t avail, size_t per_split) {
  const size_t need = pl.ws_bytes + (pl.splitk > 1 ? (size_t)pl.splitk * per_split : 0);
  if (need <= avail || pl.ring) return pl;
  const int bk = pl.prec == A3D_PREC_F32 ? kCfgs[pl.cfg].bk : (pl.prec == A3D_PREC_BF16X3 ? 32 : 64);
  const int nk = std::max(1, (g.K + bk - 1) / bk);
  const size_t each = slab_bytes(g, 1) + per_split;
  const int splitk = g.plain ? 1 : (int)std::min<size_t>(avail / each, (size_t)(pl.streamk > 0 ? std::min(nk, 256) : pl.splitk));
  if (g.need_reduce && splitk < 2) return pl;
  pl.streamk = 0;
  finish_split(pl, g, nk, std::max(1, splitk));
  return pl;
}

}  // namespace a3d
