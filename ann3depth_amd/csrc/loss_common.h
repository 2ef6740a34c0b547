// loss_common.h — the machine the loss kernels share: pointwise.hip (silog, plain and masked), gradloss.hip (silog with the
// gradient-matching term), berhu.hip (reverse Huber) and ssi.hip (scale-and-shift-invariant).  Every forward kernel there is
//   kSilogParts blocks per sample, each on a contiguous chunk (loss_part) -> per-thread accumulators -> one value per block
//   (wave_sum / wave_max, block_put into red[K][4]) -> published and handed to the block that arrives last (publish_and_arrive) ->
//   that block adds each sample's parts in part order (fold_parts), the same sum whatever the timing;
// and the silog arithmetic — masked_log, the per-sample term, the pull of the backward — is written here once, so that
// pointwise.hip and gradloss.hip give the same bits by construction.  All four files are compiled with -ffp-contract=off.
// Everything is __forceinline__: no call, no scratch.
#pragma once
#include "a3d_internal.h"

namespace a3d {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kSilogParts = A3D_SILOG_PARTS;
static const float kSilogC = (float)(0.5 / (74 * 55));   // src/models.py:269, folded constant

// ------------------------------------------------------------------ small helpers
template <typename T>      // float, or double where whole numbers past 2^24 are added
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_down(v, off, 64));
  return v;
}

__device__ __forceinline__ float masked_log(float v) {
  float l = logf(__fadd_rn(v, 1e-8f));
  return isnan(l) ? 0.f : l;     // tf.where(tf.is_nan(log), 0, log): -inf is kept
}

// pixels [i, i + 4) of a row, i a multiple of 4: one 16-byte load where the row starts on a 16-byte address and all four lie
// below hi, one by one otherwise (what lies at or past hi reads as 0 and is never used)
__device__ __forceinline__ void load4(const float* __restrict__ row, int i, int hi, bool vec, float (&v)[4]) {
  if (vec && i + 4 <= hi) {
    const f32x4 q = *reinterpret_cast<const f32x4*>(row + i);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = i + u < hi ? row[i + u] : 0.f;
  }
}

// ------------------------------------------------------------------ part bounds
// Block blockIdx.x is one of the kSilogParts parts of sample `b` and walks pixels [lo, hi) of it.  The partition fixes the
// order of every sum, so both forms are kept as they are: silog's chunk = ceil(npix / parts), lo = part * chunk (an empty
// part has hi < lo); ROUND4 (berhu): the chunk rounded up to a multiple of 4, so that every part starts where the row's
// 16-byte pieces do, and lo = min(npix, part * chunk).
struct LossPart { int b, lo, hi; };

template <bool ROUND4>
__device__ __forceinline__ LossPart loss_part(int npix) {
  LossPart p;
  p.b = blockIdx.x / kSilogParts;
  const int part = blockIdx.x % kSilogParts;
  int chunk = (npix + kSilogParts - 1) / kSilogParts;
  if constexpr (ROUND4) chunk = (chunk + 3) & ~3;
  p.lo = ROUND4 ? min(npix, part * chunk) : part * chunk;
  p.hi = min(npix, p.lo + chunk);
  return p;
}

// ------------------------------------------------------------------ block reduction
// Per-thread values become one value per wavefront by wave_sum / wave_max — all of a kernel's first, so that their shuffle
// chains overlap — and block_put leaves each in its row of the kernel's red[K][4]; after a __syncthreads() block_combine
// adds or compares a row in wave order, ((r0 + r1) + r2) + r3: the same sum whatever the timing.
__device__ __forceinline__ void block_put(float (&row)[4], float v) {
  if ((threadIdx.x & 63) == 0) row[threadIdx.x >> 6] = v;
}

template <bool MAX>
__device__ __forceinline__ float block_combine(const float (&row)[4]) {
  if constexpr (MAX) return fmaxf(fmaxf(fmaxf(row[0], row[1]), row[2]), row[3]);
  else return ((row[0] + row[1]) + row[2]) + row[3];
}

// ------------------------------------------------------------------ publish and arrive
// The hand-off of MI355X_MICROARCH.md, "inter-workgroup visibility", in its last-arriver form: ONE lane of each workgroup
// signals for ALL that workgroup's stores by an agent-scope atomic add to ONE unsharded counter, the consumer is the
// workgroup whose add came last and learns it from the value the add returned, stores and loads are all write-through /
// past the L1.  Step by step, in lane 0 of the block:
//   1. the block's K values (rows of red, combined in wave order; MAXES: the rows that are maxima, SKIP: words that are
//      not stored at all; words past the R rows are stored as 0) go to partials[K * blockIdx.x ..] as agent-scope relaxed
//      atomic stores — global_store sc1, write-through: a plain store may stay in this CU's L1 / this XCD's L2 where no
//      other CU's load finds it;
//   2. s_waitcnt vmcnt(0): the stores have left before the ticket says so.  The lane that stored is the lane that waits
//      and the lane that signals, so no other wave has anything outstanding;
//   3. atomicInc on ws[0], wrapping at nb * kSilogParts: the block that draws the last ticket knows every other block is
//      past its step 2, and the ticket is 0 again for the next call — nothing to re-initialise, and no batch size leaves a
//      sum in ws[0], so one workspace serves calls of different batch sizes.  The returned value is used, so lane 0 has
//      waited for the add before anything after it;
//   4. the flag crosses to the other waves through LDS and a barrier lane 0 joins after its add has returned.
// partials = ws + K * nb + 1: behind the ticket and the nb samples' words.
// The block for which this returns true then reads the partials with fold_parts, whose agent-scope relaxed loads (sc1) go
// past its own L1: every load of the handed-off words is such a load.  No block waits for another.
template <int K, unsigned MAXES, unsigned SKIP, int R>
__device__ __forceinline__ bool publish_and_arrive(float* __restrict__ ws, float* __restrict__ partials, int nb,
                                                   const float (&red)[R][4]) {
  static_assert(R <= K, "more rows than words");
  __shared__ unsigned last;
  if (threadIdx.x == 0) {
    const unsigned total = (unsigned)(nb * kSilogParts);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if ((SKIP >> k) & 1u) continue;
      const float(&row)[4] = red[k < R ? k : 0];
      const float v = k >= R ? 0.f : ((MAXES >> k) & 1u) ? block_combine<true>(row) : block_combine<false>(row);
      __hip_atomic_store(&partials[K * blockIdx.x + k], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    last = atomicInc(reinterpret_cast<unsigned*>(ws), total - 1u) == total - 1u;
  }
  __syncthreads();
  return last != 0u;
}

// ------------------------------------------------------------------ reading parts back
// Word `word` of the partials of sample i's parts, folded in ascending part order (agent-scope relaxed loads: see above).
// Acc = double where the parts are counts whose sum may pass 2^24 (gradloss's pairs).
template <int K, typename Acc = float, bool MAX = false>
__device__ __forceinline__ Acc fold_parts(const float* __restrict__ partials, int i, int word) {
  Acc a = 0;
#pragma unroll
  for (int q = 0; q < kSilogParts; ++q) {
    const float v = __hip_atomic_load(&partials[K * (i * kSilogParts + q) + word], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if constexpr (MAX) a = fmaxf(a, v);
    else a += (Acc)v;
  }
  return a;
}

// ------------------------------------------------------------------ the same hand-off for float64 values (ssi.hip)
// A kernel whose partial sums are float64 runs the same four steps itself: block_put / block_sum64 on a red64[K][4], lane 0
// publishes its block's words one by one (publish64 / publish32), every thread calls arrive, and the last block reads with
// fold_parts64 (and fold_parts for its float words).  A float64 word is ONE 8-byte agent-scope relaxed store or load
// (global_store_dwordx2 sc1): it lies at an even word offset of a workspace that starts on an 8-byte address, so it never
// straddles and is never seen half written.
__device__ __forceinline__ void block_put(double (&row)[4], double v) {
  if ((threadIdx.x & 63) == 0) row[threadIdx.x >> 6] = v;
}

__device__ __forceinline__ double block_sum64(const double (&row)[4]) { return ((row[0] + row[1]) + row[2]) + row[3]; }

__device__ __forceinline__ void publish64(float* __restrict__ word, double v) {
  __hip_atomic_store(reinterpret_cast<double*>(word), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void publish32(float* __restrict__ word, float v) {
  __hip_atomic_store(word, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// steps 2 to 4 of publish_and_arrive, for a block whose lane 0 has just published its words itself; called by every thread
// (arrive_of: the same for a grid of `total` blocks that is not nb * kSilogParts — clip.hip's)
__device__ __forceinline__ bool arrive_of(unsigned* __restrict__ ticket, unsigned total) {
  __shared__ unsigned last_arrived;
  if (threadIdx.x == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    last_arrived = atomicInc(ticket, total - 1u) == total - 1u;
  }
  __syncthreads();
  return last_arrived != 0u;
}

__device__ __forceinline__ bool arrive(float* __restrict__ ws, int nb) {
  return arrive_of(reinterpret_cast<unsigned*>(ws), (unsigned)(nb * kSilogParts));
}

// the float64 word at `word` (even) of the K-word partials of sample i's parts, added in ascending part order from 0.0
template <int K>
__device__ __forceinline__ double fold_parts64(const float* __restrict__ partials, int i, int word) {
  static_assert(K % 2 == 0, "float64 words lie at even offsets");
  double a = 0.0;
#pragma unroll
  for (int q = 0; q < kSilogParts; ++q)
    a += __hip_atomic_load(reinterpret_cast<const double*>(&partials[K * (i * kSilogParts + q) + word]), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
  return a;
}

// ------------------------------------------------------------------ silog arithmetic (pointwise.hip and gradloss.hip)
// the per-sample term from a2 = sum d^2 and a1 = sum d: plain with the folded constant c, masked over an > 0 pixels that count
__device__ __forceinline__ float silog_term(float a2, float a1, float c) { return a2 - c * (a1 * a1); }

__device__ __forceinline__ float silog_term_masked(float a2, float a1, float an, int npix) {
  const float cn = (float)(0.5 / (double)an), rn = (float)((double)npix / (double)an);
  return rn * (a2 - cn * (a1 * a1));
}

// the per-sample coefficients of the backward: plain 2c and 1; masked from the sample's count n (read only at a pixel that
// counts: then n >= 1)
struct SilogCoef { float two_c, rn; };

template <bool MASKED>
__device__ __forceinline__ SilogCoef silog_coef(float c, float n_word, int npix) {
  if (!MASKED) return {__fmul_rn(2.f, c), 1.f};
  const double n = (double)n_word;
  return {__fmul_rn(2.f, (float)(0.5 / n)), (float)((double)npix / n)};
}

// the pull on log(o + 1e-8) before the division by o + 1e-8: (2 d - 2c sd) / b [* rn]
template <bool MASKED>
__device__ __forceinline__ float silog_pull(float d, float sd, SilogCoef k, float inv_b) {
  const float a = __fmul_rn(__fsub_rn(__fmul_rn(2.f, d), __fmul_rn(k.two_c, sd)), inv_b);
  return MASKED ? __fmul_rn(a, k.rn) : a;
}

// ------------------------------------------------------------------ gradient write
// the bf16 copy the bf16 dense layer reads (the *_bwd_ex entry points): [b][ld16 >= npix], columns npix.. are left alone
__device__ __forceinline__ void write_grad16(__bf16* __restrict__ dout16, int ld16, int smp, size_t col, float g) {
  if (dout16) dout16[(size_t)smp * ld16 + col] = (__bf16)g;
}

__device__ __forceinline__ void write_grad(float* __restrict__ dout, __bf16* __restrict__ dout16, int ld16, int smp, size_t npix,
                                           size_t col, float g) {
  dout[(size_t)smp * npix + col] = g;
  write_grad16(dout16, ld16, smp, col, g);
}

// ------------------------------------------------------------------ host side of the entry points
// The argument check of all eight loss entry points.  npix is given as long long (gradloss: h * w); count_floats: the
// kernel keeps pixel counts in floats, exact up to 2^24; ld_bf16 is looked at only where there is a bf16 copy.
inline int loss_check(const char* who, int b, long long npix, bool pointers, bool count_floats, const void* dout_bf16 = nullptr,
                      int ld_bf16 = 0) {
  A3D_CHECK_ARG(pointers, "%s: bad arguments: a NULL pointer", who);
  A3D_CHECK_ARG(b > 0 && npix > 0, "%s: bad arguments: a batch of %d samples of %lld pixels: both must be positive", who, b, npix);
  A3D_CHECK_ARG(!count_floats || npix <= (1 << 24), "%s: %lld pixels per sample, the counts are kept in floats", who, npix);
  A3D_CHECK_ARG(!dout_bf16 || ld_bf16 >= npix, "%s: bad arguments: a bf16 pitch of %d below %lld pixels", who, ld_bf16, npix);
  return A3D_OK;
}

// one launch of 256-thread blocks: the kernel's plain instantiation, or the one that leaves out the holes of the target
template <typename... P, typename... A>
inline void launch_masked(int masked, void (*plain)(P...), void (*holes)(P...), unsigned grid, void* stream, A... args) {
  void (*kernel)(P...) = masked ? holes : plain;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), args...);
}

}  // namespace a3d
