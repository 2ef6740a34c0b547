// gradloss.hip — the scale-invariant log loss with the gradient-matching term of Eigen & Fergus 2015 (eq. 4), NON-REFERENCE
// (include/a3d_gradloss.h, --loss-gradient): sum over the horizontal and vertical neighbour pairs of (d_j - d_i)^2 beside the
// per-sample term of pointwise.hip's silog kernels, in the same two launches — both sit on the step's critical path.
// Compiled with -ffp-contract=off like pointwise.hip: every rounding the header names is a rounding of its own, and d, s2, s1
// and n come out of the same operations in the same order as there (silog_common.h), so that the silog part of the loss and,
// with grad_weight = 0, the gradient are the bits of the plain / masked kernels.
#include "a3d_internal.h"
#include "silog_common.h"
#include "../../include/a3d_gradloss.h"

namespace a3d {

constexpr int kGradK = 5;                      // s2, s1, n, sg, m per block and per sample
constexpr int kGradRound = 4 * 256;            // pixels of one round of the block's walk over its chunk (silog_fwd_kernel's)
constexpr int kGradRing = 4096;                // power of two >= kGradRound + A3DG_MAX_W
constexpr int kGradTile = 8192;                // values of d a backward block stages: at least 3 rows of A3DG_MAX_W
constexpr int kGradGrid = 4096;                // blocks of the backward launch at most (40 KB of LDS each: ~4 resident per CU); the rest by grid stride
static_assert(kGradRing >= kGradRound + A3DG_MAX_W && (kGradRing & (kGradRing - 1)) == 0, "forward window");
static_assert(kGradTile >= 3 * A3DG_MAX_W, "backward tile");

// Block (b, part) walks its chunk [lo, hi) of the sample in rounds of 1024 pixels with silog_fwd_kernel's thread-to-pixel
// mapping, and owns the pairs whose FIRST pixel lies in the chunk.  The second pixel lies up to w further on, possibly several
// chunks away: before a round the block brings d over [round start, round end + w) — what is not there yet, so one logarithm
// pair per pixel of chunk + halo — from global memory into a ring in LDS (the window is at most 1024 + w <= kGradRing values;
// a slot is overwritten only by a pixel kGradRing further on, which lies behind the round).  Then every thread takes its four
// pixels of the round from the ring: s2, s1, n exactly as silog_fwd_kernel adds them, and the pair right of and the pair below
// each pixel.  Five partials per block; stores, drain, ticket and last block as in silog_fwd_kernel.
template <bool MASKED>
__global__ __launch_bounds__(256) void gradloss_fwd_kernel(const float* __restrict__ out, const float* __restrict__ tgt,
                                                           float* __restrict__ ws, float* __restrict__ loss, int h, int w, int nb,
                                                           float c, float gw) {
  constexpr int K = kGradK;
  __shared__ float dring[kGradRing];
  __shared__ unsigned char cring[MASKED ? kGradRing : 4];      // 1: the pixel counts
  __shared__ float red[K][4];
  __shared__ unsigned last;
  const int npix = h * w;
  const int b = blockIdx.x / kSilogParts, part = blockIdx.x % kSilogParts;
  const int chunk = (npix + kSilogParts - 1) / kSilogParts;
  const int lo = part * chunk, hi = min(npix, lo + chunk);
  const float* o = out + (size_t)b * npix;
  const float* t = tgt + (size_t)b * npix;
  float* partials = ws + K * nb + 1;
  float s2 = 0.f, s1 = 0.f, cnt = 0.f, sg = 0.f, mp = 0.f;
  int fill = lo;                                // d over [round start, fill) is in the ring
  for (int r_lo = lo; r_lo < hi; r_lo += kGradRound) {
    const int r_hi = min(hi, r_lo + kGradRound);
    const int need = min(npix, r_hi + w);
    __syncthreads();                            // the round before has read what is overwritten now
    for (int j0 = fill + threadIdx.x; j0 < need; j0 += kGradRound) {
      float ov[4], tv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {             // all eight loads issued before the first logarithm
        const int j = j0 + u * 256;
        ov[u] = j < need ? o[j] : 0.f;
        tv[u] = j < need ? t[j] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = j0 + u * 256;
        if (j >= need) break;
        if constexpr (MASKED) {
          const bool ok = isfinite(tv[u]);
          cring[j & (kGradRing - 1)] = ok;
          if (!ok) continue;
        }
        dring[j & (kGradRing - 1)] = __fsub_rn(masked_log(ov[u]), masked_log(tv[u]));
      }
    }
    fill = max(fill, need);
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = r_lo + threadIdx.x + u * 256;
      if (i >= r_hi) break;
      if constexpr (MASKED) {
        if (!cring[i & (kGradRing - 1)]) continue;
        cnt += 1.f;
      }
      const float d = dring[i & (kGradRing - 1)];
      s2 += d * d;
      s1 += d;
      if (i % w < w - 1) {                      // the right neighbour, same row: i + 1 < r_hi + w and < npix
        bool ok = true;
        if constexpr (MASKED) ok = cring[(i + 1) & (kGradRing - 1)];
        if (ok) {
          const float e = __fsub_rn(dring[(i + 1) & (kGradRing - 1)], d);
          sg += e * e;
          mp += 1.f;
        }
      }
      if (i + w < npix) {                       // the pixel below
        bool ok = true;
        if constexpr (MASKED) ok = cring[(i + w) & (kGradRing - 1)];
        if (ok) {
          const float e = __fsub_rn(dring[(i + w) & (kGradRing - 1)], d);
          sg += e * e;
          mp += 1.f;
        }
      }
    }
  }
  s2 = wave_sum(s2);
  s1 = wave_sum(s1);
  sg = wave_sum(sg);
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = s2;
    red[1][threadIdx.x >> 6] = s1;
    red[3][threadIdx.x >> 6] = sg;
  }
  if constexpr (MASKED) {
    cnt = wave_sum(cnt);            // whole numbers below 2^24: exact in any order
    mp = wave_sum(mp);
    if ((threadIdx.x & 63) == 0) {
      red[2][threadIdx.x >> 6] = cnt;
      red[4][threadIdx.x >> 6] = mp;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned total = (unsigned)(nb * kSilogParts);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (!MASKED && (k == 2 || k == 4)) continue;      // n = npix and m = M: nothing to count
      __hip_atomic_store(&partials[K * blockIdx.x + k], red[k][0] + red[k][1] + red[k][2] + red[k][3], __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    last = atomicInc(reinterpret_cast<unsigned*>(ws), total - 1u) == total - 1u;
  }
  __syncthreads();
  if (!last || threadIdx.x >= 64) return;
  const double pairs = (double)h * (double)(w - 1) + (double)(h - 1) * (double)w;      // M
  float s = 0.f, sgrad = 0.f;
  double valid = 0.0;
  for (int i = threadIdx.x; i < nb; i += 64) {
    float a2 = 0.f, a1 = 0.f, an = 0.f, ag = 0.f;
    double am = 0.0;                // up to 2^25 pairs: the parts (each below 2^24) are added exactly, then rounded once
#pragma unroll
    for (int q = 0; q < kSilogParts; ++q) {
      const float* p = &partials[K * (i * kSilogParts + q)];
      a2 += __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      a1 += __hip_atomic_load(p + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      ag += __hip_atomic_load(p + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if constexpr (MASKED) {
        an += __hip_atomic_load(p + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        am += (double)__hip_atomic_load(p + 4, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    if constexpr (!MASKED) {
      an = (float)npix;
      am = pairs;
    }
    const float m = (float)am;
    ws[1 + K * i] = a2;
    ws[2 + K * i] = a1;
    ws[3 + K * i] = an;
    ws[4 + K * i] = ag;
    ws[5 + K * i] = m;
    if constexpr (MASKED) {
      valid += (double)an;
      if (an > 0.f) {
        const float cn = (float)(0.5 / (double)an), rn = (float)((double)npix / (double)an);
        s += rn * (a2 - cn * (a1 * a1));
      }
      if (m > 0.f) sgrad += (float)(pairs / (double)m) * ag;
    } else {
      s += a2 - c * (a1 * a1);
      sgrad += ag;
    }
  }
  s = wave_sum(s);
  sgrad = wave_sum(sgrad);
  if constexpr (MASKED) valid = wave_sum(valid);
  if (threadIdx.x == 0) {
    const float silog = s / (float)nb, grad = sgrad / (float)nb;
    loss[0] = gw == 0.f ? silog : silog + gw * grad;
    loss[1] = MASKED ? (float)(valid / ((double)nb * (double)npix)) : 1.f;
    loss[2] = silog;
    loss[3] = grad;
  }
}

// One work item is a band of `band` rows of one sample: the block stages d and two flags per pixel over the band and the row
// above and below it (one logarithm pair per staged pixel, (band + 2) / band per pixel of the image), then every thread
// writes the gradient of its pixels from the five-point stencil on the staged d.  Operation order: include/a3d_gradloss.h.
template <bool MASKED>
__global__ __launch_bounds__(256) void gradloss_bwd_kernel(const float* __restrict__ out, const float* __restrict__ tgt,
                                                           const float* __restrict__ ws, float* __restrict__ dout, int nb, int h,
                                                           int w, int band, float c, float inv_b, float gw,
                                                           __bf16* __restrict__ dout16, int ld16) {
  constexpr int K = kGradK;
  __shared__ float dt[kGradTile];
  __shared__ unsigned char ft[kGradTile];       // bit 0: the pixel counts; bit 1: log(o + 1e-8) is NaN
  const int npix = h * w;
  const int nbands = (h + band - 1) / band;
  const long long items = (long long)nb * nbands;
  for (long long item = blockIdx.x; item < items; item += gridDim.x) {
    const int smp = (int)(item / nbands), r0 = (int)(item % nbands) * band, r1 = min(h, r0 + band);
    const int rs = max(r0 - 1, 0), re = min(h, r1 + 1);
    const float* o = out + (size_t)smp * npix;
    const float* t = tgt + (size_t)smp * npix;
    const int base = rs * w, staged = (re - rs) * w;          // <= (band + 2) w <= kGradTile
    __syncthreads();                                           // the item before has read the tile
    for (int j = threadIdx.x; j < staged; j += 256) {
      const float ov = o[base + j], tv = t[base + j];
      unsigned char f = 1;
      if constexpr (MASKED) f = isfinite(tv) ? 1 : 0;
      float d = 0.f;
      if (f) {
        const float lo = logf(__fadd_rn(ov, 1e-8f));
        if (isnan(lo)) f |= 2;
        d = __fsub_rn(isnan(lo) ? 0.f : lo, masked_log(tv));
      }
      dt[j] = d;
      ft[j] = f;
    }
    __syncthreads();
    const float sd = ws[1 + K * smp + 1];
    float two_c = __fmul_rn(2.f, c), rn = 1.f, two_gwr = 0.f;
    if constexpr (MASKED) {
      const double n = (double)ws[1 + K * smp + 2];           // used only at a pixel that counts: then n >= 1
      two_c = __fmul_rn(2.f, (float)(0.5 / n));
      rn = (float)((double)npix / n);
    }
    if (gw != 0.f) {
      float rm = 1.f;
      if constexpr (MASKED) {
        const float m = ws[1 + K * smp + 4];
        const double pairs = (double)h * (double)(w - 1) + (double)(h - 1) * (double)w;
        rm = m > 0.f ? (float)(pairs / (double)m) : 0.f;
      }
      two_gwr = __fmul_rn(2.f, __fmul_rn(gw, rm));
    }
    const int count = (r1 - r0) * w;
    for (int idx = threadIdx.x; idx < count; idx += 256) {
      const int rr = idx / w, col = idx - rr * w, r = r0 + rr;
      const int li = (r - rs) * w + col, pi = r * w + col;
      float g = 0.f;
      if (ft[li] == 1) {                                       // counts, and its logarithm is a number
        const float d = dt[li];
        const float arg = __fadd_rn(o[pi], 1e-8f);
        float a = __fmul_rn(__fsub_rn(__fmul_rn(2.f, d), __fmul_rn(two_c, sd)), inv_b);
        if constexpr (MASKED) a = __fmul_rn(a, rn);
        if (gw != 0.f) {
          float lap = 0.f;
          if (col > 0 && (ft[li - 1] & 1)) lap = __fadd_rn(lap, __fsub_rn(d, dt[li - 1]));
          if (col < w - 1 && (ft[li + 1] & 1)) lap = __fadd_rn(lap, __fsub_rn(d, dt[li + 1]));
          if (r > 0 && (ft[li - w] & 1)) lap = __fadd_rn(lap, __fsub_rn(d, dt[li - w]));
          if (r < h - 1 && (ft[li + w] & 1)) lap = __fadd_rn(lap, __fsub_rn(d, dt[li + w]));
          a = __fadd_rn(a, __fmul_rn(__fmul_rn(two_gwr, lap), inv_b));
        }
        g = __fdiv_rn(a, arg);
      }
      dout[(size_t)smp * npix + pi] = g;
      if (dout16) dout16[(size_t)smp * ld16 + pi] = (__bf16)g;
    }
  }
}

// rows per backward work item: about 512 pixels, and band + 2 rows fit the tile
static int gradloss_band(int w) { return std::max(1, std::min(kGradTile / w - 2, (512 + w - 1) / w)); }

}  // namespace a3d
using namespace a3d;

extern "C" {

int a3dg_silog_grad_loss_fwd(int b, int h, int w, const float* out, const float* tgt, int masked, float grad_weight, float* loss,
                             float* ws, void* stream) {
  A3D_CHECK_ARG(b > 0 && h > 0 && w > 0 && out && tgt && loss && ws, "silog_grad_fwd: bad arguments");
  A3D_CHECK_ARG(w <= A3DG_MAX_W, "silog_grad_fwd: rows of %d pixels, at most A3DG_MAX_W = %d", w, A3DG_MAX_W);
  A3D_CHECK_ARG((long long)h * w <= (1 << 24), "silog_grad_fwd: %d x %d pixels per sample, the counts are kept in floats", h, w);
  A3D_CHECK_ARG(grad_weight >= 0.f, "silog_grad_fwd: grad_weight must be a number >= 0");
  hipStream_t st = static_cast<hipStream_t>(stream);
  clear_stale_error();
  if (masked)
    hipLaunchKernelGGL(gradloss_fwd_kernel<true>, dim3(b * kSilogParts), dim3(256), 0, st, out, tgt, ws, loss, h, w, b, 0.f,
                       grad_weight);
  else
    hipLaunchKernelGGL(gradloss_fwd_kernel<false>, dim3(b * kSilogParts), dim3(256), 0, st, out, tgt, ws, loss, h, w, b, kSilogC,
                       grad_weight);
  return check_launch("silog_grad_fwd");
}

int a3dg_silog_grad_loss_bwd_ex(int b, int h, int w, const float* out, const float* tgt, int masked, float grad_weight,
                                const float* ws, float* dout, void* dout_bf16, int ld_bf16, void* stream) {
  A3D_CHECK_ARG(b > 0 && h > 0 && w > 0 && out && tgt && ws && dout, "silog_grad_bwd: bad arguments");
  A3D_CHECK_ARG(w <= A3DG_MAX_W, "silog_grad_bwd: rows of %d pixels, at most A3DG_MAX_W = %d", w, A3DG_MAX_W);
  A3D_CHECK_ARG((long long)h * w <= (1 << 24), "silog_grad_bwd: %d x %d pixels per sample, the counts are kept in floats", h, w);
  A3D_CHECK_ARG(grad_weight >= 0.f, "silog_grad_bwd: grad_weight must be a number >= 0");
  A3D_CHECK_ARG(!dout_bf16 || ld_bf16 >= h * w, "silog_grad_bwd: a bf16 pitch of %d below %d pixels", ld_bf16, h * w);
  const int band = gradloss_band(w);
  const long long items = (long long)b * ((h + band - 1) / band);
  const unsigned grid = (unsigned)std::min<long long>(items, kGradGrid);
  hipStream_t st = static_cast<hipStream_t>(stream);
  clear_stale_error();
  if (masked)
    hipLaunchKernelGGL(gradloss_bwd_kernel<true>, dim3(grid), dim3(256), 0, st, out, tgt, ws, dout, b, h, w, band, 0.f,
                       1.0f / (float)b, grad_weight, static_cast<__bf16*>(dout_bf16), ld_bf16);
  else
    hipLaunchKernelGGL(gradloss_bwd_kernel<false>, dim3(grid), dim3(256), 0, st, out, tgt, ws, dout, b, h, w, band, kSilogC,
                       1.0f / (float)b, grad_weight, static_cast<__bf16*>(dout_bf16), ld_bf16);
  return check_launch("silog_grad_bwd");
}

}  // extern "C"
