// igemm_launch.hip — the launch layer under the conv / dense front end (igemm_host.hip): dispatch of a planned GEMM
// (the plans: igemm_plan.cc), split-K reduction and second-output kernels, and the opt-in launch timing (a3d_timing_*).
#include <algorithm>
#include <cstdio>
#include <mutex>
#include <vector>

#include "a3d_internal.h"
#include "igemm.h"
#include "igemm_cfgs.h"

namespace a3d {

int launch_igemm_mode0(int cfg, int avec, int bvec, IgemmParams& p, unsigned grid, hipStream_t st);
int launch_igemm_mode1(int cfg, int avec, int bvec, IgemmParams& p, unsigned grid, hipStream_t st);
int launch_igemm_mode2(int cfg, int avec, int bvec, IgemmParams& p, unsigned grid, hipStream_t st);
int launch_igemm_bf16(int mode, int bn, bool x3, IgemmParams& p, unsigned grid, hipStream_t st);   // p.a16/b16/c16 pick the storage variant
int launch_fixup_mode0(int cfg, IgemmParams& p, unsigned tiles, unsigned nblk, hipStream_t st);
int launch_fixup_mode1(int cfg, IgemmParams& p, unsigned tiles, unsigned nblk, hipStream_t st);
int launch_fixup_mode2(int cfg, IgemmParams& p, unsigned tiles, unsigned nblk, hipStream_t st);
int launch_igemm_ring(int mode, int cfg, IgemmParams& p, unsigned grid, hipStream_t st);

#ifdef A3D_STAMPS
static unsigned long long* g_stamps = nullptr;
static unsigned g_stamp_grid = 0;
static const size_t kStampBytes = (size_t)8 << 20;
#endif

// ---- opt-in launch timing (a3d_timing_*; timed_launch: a3d_internal.h) ----
static std::mutex g_timing_mu;
static bool g_timing_on = false;
static bool g_timing_only = false;          // a3d_timing_select: bracket only launches of one kernel
static a3d_timing_record g_timing_like{};
static std::vector<TimingSlot> g_timing;

// Is this launch to be bracketed?  `r` names the kernel about to be launched.
bool timing_wanted(const a3d_timing_record& r) {
  std::lock_guard<std::mutex> lk(g_timing_mu);
  if (!g_timing_on) return false;
  if (!g_timing_only) return true;
  const a3d_timing_record& l = g_timing_like;
  return r.mode == l.mode && r.prec == l.prec && r.bm == l.bm && r.bn == l.bn && r.waves_m == l.waves_m &&
         r.nwaves == l.nwaves && r.bk == l.bk && r.avec == l.avec && r.bvec == l.bvec && r.lds_dma == l.lds_dma;
}
int timing_begin(TimingSlot& slot, hipStream_t st) {
  if (hipEventCreate(&slot.start) != hipSuccess || hipEventCreate(&slot.stop) != hipSuccess)
    return set_error(A3D_ELAUNCH, "timing: hipEventCreate failed");
  (void)hipEventRecord(slot.start, st);
  return A3D_OK;
}
void timing_end(TimingSlot& slot, hipStream_t st) {
  (void)hipEventRecord(slot.stop, st);
  std::lock_guard<std::mutex> lk(g_timing_mu);
  g_timing.push_back(slot);
}
// The record of a launch that computes an m x n x k GEMM unsplit; callers overwrite what differs (splitk, flops).
a3d_timing_record timing_record(int mode, int prec, int bm, int bn, int waves_m, int nwaves, int bk, int avec, int bvec,
                                int lds_dma, int m, int n, int k) {
  a3d_timing_record r{};
  r.mode = mode; r.prec = prec; r.bm = bm; r.bn = bn; r.waves_m = waves_m; r.nwaves = nwaves; r.bk = bk;
  r.avec = avec; r.bvec = bvec; r.lds_dma = lds_dma; r.splitk = 1; r.m = m; r.n = n; r.k = k; r.ms = 0.f;
  r.flops = 2.0 * m * n * k;
  return r;
}

// Sums the split-K slabs in slab order (deterministic) and applies the epilogue.  Slab reads are issued four at a
// time into independent registers: a thread's serial chain of `splitk` dependent loads was the cost of this kernel.
template <typename V>
__device__ __forceinline__ V slab_sum(const V* ws, size_t slab, int splitk, size_t i) {
  V s = V(0.f);
  int z = 0;
  for (; z + 8 <= splitk; z += 8) {       // eight slabs in flight, added in slab order
    V t[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) t[u] = ws[(size_t)(z + u) * slab + i];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += t[u];
  }
  if (z + 4 <= splitk) {
    const V a = ws[(size_t)z * slab + i], b = ws[(size_t)(z + 1) * slab + i];
    const V c = ws[(size_t)(z + 2) * slab + i], d = ws[(size_t)(z + 3) * slab + i];
    s += a; s += b; s += c; s += d;
    z += 4;
  }
  for (; z < splitk; ++z) s += ws[(size_t)z * slab + i];
  return s;
}

// C position (in units of V) of slab position i when the slabs' rows are padded window runs (ReduceParams::row_rlp), or
// SIZE_MAX for a pad row; nv = V's per row
__device__ __forceinline__ size_t unpadded_pos(size_t i, int nv, int rl, int rlp) {
  if (rlp == 0) return i;
  const size_t row = i / (size_t)nv, c = i - row * (size_t)nv;
  const size_t rr = row / (size_t)rlp, q = row - rr * (size_t)rlp;
  return q < (size_t)rl ? (rr * (size_t)rl + q) * (size_t)nv + c : SIZE_MAX;
}
template <typename V>
__device__ __forceinline__ void reduce_wide(const V* src, V* dst, size_t slab, size_t count, int splitk, size_t first, V* lds, int nv,
                                            int rl, int rlp);
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const ReduceParams p) {
  const size_t total = (size_t)p.M * p.N;
  unsigned nblk = gridDim.x;
  if (p.dbias_splits > 0) {      // up to 256 rows of column-sum partials: blocks of their own, sixteen threads per column
    __shared__ float lds[256];
    if (blockIdx.x >= p.dbias_block0) {
      reduce_wide<float>(p.dbias_ws, p.dbias_out, (size_t)p.N, (size_t)p.N, p.dbias_splits, (size_t)(blockIdx.x - p.dbias_block0) * 16, lds,
                         0, 0, 0);
      return;
    }
    nblk = p.dbias_block0;
  } else if (p.dbias_out) {       // N sums of `splitk` values: the grid's first threads do them on the side
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)p.N; i += (size_t)gridDim.x * 256)
      p.dbias_out[i] = slab_sum<float>(p.dbias_ws, (size_t)p.N, p.splitk, i);
  }
  if (p.vec4) {   // plain sum of 16-byte columns: bwd-filter slabs (no epilogue, contiguous output)
    typedef float f4 __attribute__((ext_vector_type(4)));
    const size_t nv = total / 4;
    const f4* ws4 = reinterpret_cast<const f4*>(p.ws);
    const size_t slab4 = p.slab / 4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += (size_t)nblk * 256) {
      const size_t o = unpadded_pos(i, p.N / 4, p.row_rl, p.row_rlp);
      if (o != SIZE_MAX) reinterpret_cast<f4*>(p.C)[o] = slab_sum<f4>(ws4, slab4, p.splitk, i);
    }
    return;
  }
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)nblk * 256) {
    float s = slab_sum<float>(p.ws, p.slab, p.splitk, i);
    const int row = (int)(i / p.N), col = (int)(i - (size_t)row * p.N);
    const size_t o = remap_row(row, p.mode == MODE_BWD_D ? p.sub_step : 1, p.sub_ph, p.sub_pw, p.outW, p.outHW, p.div_phw,
                               p.div_pw) * p.ldc + col;
    if (p.mode == MODE_FWD) {
      if (p.bias) s += p.bias[col];
      if (p.act == EPI_RELU) s = fmaxf(s, 0.f);
      else if (p.act == EPI_SIGMOID) s = 1.f / (1.f + expf(-s));
      if (p.keep) s = p.keep[i] ? s * p.mask_scale : 0.f;
    } else if (p.mode == MODE_BWD_D) {
      if (p.mask) {
        const float y = p.c16 ? (float)reinterpret_cast<const __bf16*>(p.mask)[o] : p.mask[o];
        s = apply_act_grad(s, y, p.mask_act, p.mask_scale);
      }
    }
    if (p.c_cols == 0 || col < p.c_cols) {
      if (p.c16) reinterpret_cast<__bf16*>(p.C)[o] = (__bf16)s;
      else p.C[o] = s;
    }
    if (p.C2 && col < p.cols2) {
      const size_t o2 = ((size_t)row * p.ld2 + col) * p.step2 + p.off2;
      if (p.c2_16) static_cast<__bf16*>(p.C2)[o2] = (__bf16)(p.c16 ? (float)(__bf16)s : s);
      else static_cast<float*>(p.C2)[o2] = p.c16 ? (float)(__bf16)s : s;
    }
  }
}

// the second output of a launch that had no reduction stage to write it: a copy of the finished tensor
__global__ __launch_bounds__(256) void second_output_kernel(const void* C, int c16, int M, int ldc, void* C2, int ld2, int step2, int off2,
                                                            int c2_16, int cols2) {
  const size_t total = (size_t)M * cols2;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int row = (int)(i / cols2), col = (int)(i - (size_t)row * cols2);
    const size_t o = (size_t)row * ldc + col;
    const float s = c16 ? (float)static_cast<const __bf16*>(C)[o] : static_cast<const float*>(C)[o];
    const size_t o2 = ((size_t)row * ld2 + col) * step2 + off2;
    if (c2_16) static_cast<__bf16*>(C2)[o2] = (__bf16)s;
    else static_cast<float*>(C2)[o2] = s;
  }
}

// Many slabs, few outputs (conv2d_0's bwd-filter: 128 slabs of 36 k floats, and its 96 bias sums): one thread per output
// means 35 blocks on 256 CUs, each walking 128 dependent-latency rounds — 28 us for 18 MB.  Here sixteen threads share
// an output: thread `part` adds its contiguous sixteenth of the slabs in slab order, the sixteen partial sums meet in
// LDS and are added in part order.  A fixed order, so still the same bits on every run (a different order than the
// one-thread sum above: a launch uses one or the other by shape alone, never by timing).
template <typename V>
__device__ __forceinline__ void reduce_wide(const V* src, V* dst, size_t slab, size_t count, int splitk, size_t first,
                                            V* lds, int nv, int rl, int rlp) {
  const int tid = threadIdx.x, out = tid & 15, part = tid >> 4;
  const size_t i = first + out;
  const int per = (splitk + 15) / 16, z0 = part * per, z1 = min(splitk, z0 + per);
  V s = V(0.f);
  if (i < count) {
    int z = z0;
    for (; z + 4 <= z1; z += 4) {
      const V a = src[(size_t)z * slab + i], b = src[(size_t)(z + 1) * slab + i];
      const V c = src[(size_t)(z + 2) * slab + i], d = src[(size_t)(z + 3) * slab + i];
      s += a; s += b; s += c; s += d;
    }
    for (; z < z1; ++z) s += src[(size_t)z * slab + i];
  }
  lds[part * 16 + out] = s;
  __syncthreads();
  if (part == 0 && i < count) {
    V t = lds[out];
#pragma unroll
    for (int q = 1; q < 16; ++q) t += lds[q * 16 + out];
    const size_t o = unpadded_pos(i, nv, rl, rlp);
    if (o != SIZE_MAX) dst[o] = t;
  }
}
__global__ __launch_bounds__(256) void splitk_reduce_wide_kernel(const ReduceParams p, unsigned blocks_c) {
  typedef float f4 __attribute__((ext_vector_type(4)));
  __shared__ f4 lds[256];
  if (blockIdx.x < blocks_c)
    reduce_wide<f4>(reinterpret_cast<const f4*>(p.ws), reinterpret_cast<f4*>(p.C), p.slab / 4, (size_t)p.M * p.N / 4,
                    p.splitk, (size_t)blockIdx.x * 16, lds, p.N / 4, p.row_rl, p.row_rlp);
  else
    reduce_wide<float>(p.dbias_ws, p.dbias_out, (size_t)p.N, (size_t)p.N, p.dbias_splits > 0 ? p.dbias_splits : p.splitk, (size_t)(blockIdx.x - blocks_c) * 16,
                       reinterpret_cast<float*>(lds), 0, 0, 0);
}

int launch_splitk_reduce(const ReduceParams& r, hipStream_t st) {
  const size_t total = (size_t)r.M * r.N;
  clear_stale_error();
  if (r.vec4 && r.splitk >= 16 && total / 4 <= (size_t)1 << 16) {
    const unsigned blocks_c = (unsigned)((total / 4 + 15) / 16), blocks_b = r.dbias_out ? (unsigned)((r.N + 15) / 16) : 0u;
    hipLaunchKernelGGL(splitk_reduce_wide_kernel, dim3(blocks_c + blocks_b), dim3(256), 0, st, r, blocks_c);
    return check_launch("splitk_reduce_wide");
  }
  const unsigned g = (unsigned)std::min<size_t>(((r.vec4 ? total / 4 : total) + 255) / 256, 2048);
  ReduceParams rr = r;
  rr.dbias_block0 = g;
  const unsigned gb = (r.dbias_out && r.dbias_splits > 0) ? (unsigned)((r.N + 15) / 16) : 0u;
  hipLaunchKernelGGL(splitk_reduce_kernel, dim3(g + gb), dim3(256), 0, st, rr);
  return check_launch("splitk_reduce");
}

int launch_igemm(int mode, const GemmPlan& plan, int avec, int bvec, IgemmParams& p, void* ws, hipStream_t st) {
  if (mode == MODE_BWD_D && p.stride != 1)      // strided bwd-data always arrives as stride-1 parity classes
    return set_error(A3D_EINVAL, "igemm: bwd-data launches are stride-1 problems");
  p.splitk = plan.splitk;
  p.ktiles_per_split = plan.ktiles_per_split;
  p.tiles_m = plan.tiles_m;
  p.tiles_n = plan.tiles_n;
  p.slab = (size_t)p.M * p.N;
  float* final_c = p.C;
  float* final_dbias = p.dbias;
  if (plan.splitk > 1) {
    if (!ws) return set_error(A3D_EWORKSPACE, "igemm: split-K needs a workspace");
    p.C = static_cast<float*>(ws);
    if (p.dbias) p.dbias = static_cast<float*>(ws) + (size_t)plan.splitk * p.slab;   // [splitk][N] after the C slabs
  }
  unsigned grid = (unsigned)((long)plan.tiles_m * plan.tiles_n * plan.splitk);
  if (plan.streamk > 0) {
    if (!ws) return set_error(A3D_EWORKSPACE, "igemm: stream-K needs a workspace");
    const size_t tile_elems = (size_t)kCfgs[plan.cfg].bm * kCfgs[plan.cfg].bn;
    p.streamk = 1;
    p.sk_ws = static_cast<float*>(ws);
    p.sk_bias = p.sk_ws + (size_t)2 * plan.streamk * tile_elems;
    p.div_nk = make_fastdiv((uint32_t)std::max(1, (p.K + 31) / 32));
    grid = (unsigned)plan.streamk;
  }
  int rc;
#ifdef A3D_STAMPS
  if (!g_stamps) (void)hipMalloc(&g_stamps, kStampBytes);
  (void)hipMemsetAsync(g_stamps, 0, kStampBytes, st);
  p.stamps = grid * 8ull * 16 * 8 <= kStampBytes ? g_stamps : nullptr;
  g_stamp_grid = grid;
#endif
  p.dbg = tune_int("A3D_DBG", 0);
  static const bool plan_log = tune_int("A3D_PLAN_LOG", 0) != 0;       // tuning aid: one line per launch on stderr
  if (plan_log)
    fprintf(stderr, "a3d plan: mode %d M %d N %d K %d -> %s %d (%dx%d) splitk %d streamk %d grid %u\n", mode, p.M, p.N, p.K,
            plan.ring ? "ring" : "cfg", plan.ring ? plan.ring - 1 : plan.cfg, plan.ring ? kRingCfgs[plan.ring - 1].bm : kCfgs[plan.cfg].bm,
            plan.ring ? kRingCfgs[plan.ring - 1].bn : kCfgs[plan.cfg].bn, plan.splitk, plan.streamk, grid);
  a3d_timing_record rec;
  if (plan.ring) {                                          // lds_dma 3: igemm_ring_kernel
    const RingTile& t = kRingCfgs[plan.ring - 1];
    rec = timing_record(mode, plan.prec, t.bm, t.bn, 0, 8, 64, avec, bvec, 3, p.M, p.N, p.K);
  } else if (plan.prec != A3D_PREC_F32) {
    rec = timing_record(mode, plan.prec, 128, plan.bf16_bn, 4, 8, plan.prec == A3D_PREC_BF16X3 ? 32 : 64, avec, bvec, 0, p.M, p.N, p.K);
  } else {
    const TileCfg& t = kCfgs[plan.cfg];
    rec = timing_record(mode, plan.prec, t.bm, t.bn, t.waves_m, t.nwaves, t.bk, avec, bvec,
                        is_glds_cfg(plan.cfg) && avec == 4 && bvec == 4, p.M, p.N, p.K);
  }
  rec.splitk = plan.splitk;
  // a second output / a narrower output are written by the reduction stage of a classic split-K forward or bwd-data launch
  // (or, the second output, by a copy launch behind an unsplit one): refuse the other combinations BEFORE anything is
  // enqueued — a GEMM that has already stored N columns into rows of c_cols floats cannot be taken back
  const bool reduce_vec4 = plan.splitk > 1 && mode == MODE_BWD_F && p.ldc == p.N && (p.slab % 4) == 0 && aligned16(final_c) && aligned16(ws);
  if (plan.streamk > 0) {
    A3D_CHECK_ARG(!p.out2 && !p.c_cols, "second output: not on stream-K launches");
  } else if (plan.splitk > 1) {
    if (mode == MODE_BWD_F) A3D_CHECK_ARG(!p.out2 && !p.c_cols, "a second output belongs to a forward or bwd-data launch");
  } else {
    A3D_CHECK_ARG(!p.c_cols || p.c_cols == p.N, "this launch has no reduction stage: the output cannot be narrower than the GEMM");
    A3D_CHECK_ARG(!p.out2 || (p.sub_step == 1 && !p.pool), "second output: plain forward / bwd-data launches only");
  }
  rc = timed_launch(rec, st, [&] {
    if (plan.ring) return launch_igemm_ring(mode, plan.ring - 1, p, grid, st);
    if (plan.prec != A3D_PREC_F32) return launch_igemm_bf16(mode, plan.bf16_bn, plan.prec == A3D_PREC_BF16X3, p, grid, st);
    if (mode == MODE_FWD) return launch_igemm_mode0(plan.cfg, avec, bvec, p, grid, st);
    if (mode == MODE_BWD_D) return launch_igemm_mode1(plan.cfg, avec, bvec, p, grid, st);
    return launch_igemm_mode2(plan.cfg, avec, bvec, p, grid, st);
  });
  if (rc != A3D_OK) return rc;
  if (plan.streamk > 0) {
    const unsigned tiles = (unsigned)(plan.tiles_m * plan.tiles_n);
    if (mode == MODE_FWD) return launch_fixup_mode0(plan.cfg, p, tiles, grid, st);
    if (mode == MODE_BWD_D) return launch_fixup_mode1(plan.cfg, p, tiles, grid, st);
    return launch_fixup_mode2(plan.cfg, p, tiles, grid, st);
  }
  if (plan.splitk > 1) {
    ReduceParams r{};
    r.ws = static_cast<const float*>(ws); r.C = final_c; r.bias = p.bias; r.mask = p.mask; r.keep = p.keep;
    r.mask_scale = p.mask_scale; r.M = p.M; r.N = p.N; r.ldc = p.ldc; r.splitk = plan.splitk; r.act = p.act;
    r.mode = mode; r.slab = p.slab; r.mask_act = p.mask_act; r.c16 = p.c16;
    r.vec4 = reduce_vec4;
    r.sub_step = p.sub_step; r.sub_ph = p.sub_ph; r.sub_pw = p.sub_pw; r.outW = p.outW; r.outHW = p.outHW;
    r.div_phw = p.div_phw; r.div_pw = p.div_pw;
    r.dbias_ws = final_dbias ? p.dbias : nullptr;
    r.dbias_out = final_dbias;
    if (p.dbias_parts) { r.dbias_ws = p.dbias_parts; r.dbias_out = p.dbias_parts_out; r.dbias_splits = p.dbias_parts_n; }
    if (r.vec4 && p.unpad_dst && p.unpad_rlp > 0 && p.N % 4 == 0 && aligned16(p.unpad_dst)) {
      r.C = p.unpad_dst; r.row_rl = p.unpad_rl; r.row_rlp = p.unpad_rlp;
      p.unpad_done = 1;
    }
    r.C2 = p.out2; r.ld2 = p.out2_ld; r.step2 = p.out2_step; r.off2 = p.out2_off; r.c2_16 = p.out2_bf16; r.cols2 = p.out2_cols;
    r.c_cols = p.c_cols;
    rc = launch_splitk_reduce(r, st);
    return rc;
  }
  if (p.out2) {                                       // no reduction stage wrote it: one copy launch (what the caller saved otherwise)
    const size_t total = (size_t)p.M * p.out2_cols;
    clear_stale_error();
    hipLaunchKernelGGL(second_output_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, 2048)), dim3(256), 0, st,
                       static_cast<const void*>(final_c), p.c16, p.M, p.ldc, p.out2, p.out2_ld, p.out2_step, p.out2_off, p.out2_bf16,
                       p.out2_cols);
    rc = check_launch("second_output");
  }
  return rc;
}

// a3d_second_output -> the host-only fields of IgemmParams
int take_second_output(IgemmParams& p, const a3d_second_output* o) {
  if (!o || !o->ptr) return A3D_OK;
  A3D_CHECK_ARG(o->ld > 0 && o->step > 0 && o->offset >= 0 && o->cols > 0 && o->cols <= p.N, "second output: bad geometry");
  p.out2 = o->ptr; p.out2_ld = o->ld; p.out2_step = o->step; p.out2_off = o->offset; p.out2_bf16 = o->bf16 ? 1 : 0; p.out2_cols = o->cols;
  return A3D_OK;
}

}  // namespace a3d

using namespace a3d;

extern "C" {

#ifdef A3D_STAMPS
// diagnostic build only: copies the last launch's [grid][8 waves][8] phase sums to the host; returns the grid size
int a3d_debug_stamps(unsigned long long* out, size_t cap_bytes) {
  (void)hipDeviceSynchronize();
  if (g_stamps && out) (void)hipMemcpy(out, g_stamps, std::min(cap_bytes, kStampBytes), hipMemcpyDeviceToHost);
  return (int)g_stamp_grid;
}
#endif

int a3d_timing_enable(int on) {
  std::lock_guard<std::mutex> lk(g_timing_mu);
  g_timing_on = on != 0;
  return A3D_OK;
}

int a3d_timing_select(const a3d_timing_record* like) {
  std::lock_guard<std::mutex> lk(g_timing_mu);
  g_timing_only = like != nullptr;
  if (like) g_timing_like = *like;
  return A3D_OK;
}

int a3d_timing_collect(a3d_timing_record* out, int cap) {
  std::vector<TimingSlot> slots;
  {
    std::lock_guard<std::mutex> lk(g_timing_mu);
    slots.swap(g_timing);
  }
  int n = 0;
  for (TimingSlot& s : slots) {
    (void)hipEventSynchronize(s.stop);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, s.start, s.stop);
    s.rec.ms = ms;
    if (out && n < cap) out[n++] = s.rec;
    (void)hipEventDestroy(s.start);
    (void)hipEventDestroy(s.stop);
  }
  return n;
}

}  // extern "C"
