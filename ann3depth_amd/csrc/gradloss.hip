// gradloss.hip — the scale-invariant log loss with the gradient-matching term of Eigen & Fergus 2015 (eq. 4), NON-REFERENCE
// (include/a3d_gradloss.h, --loss-gradient): sum over the horizontal and vertical neighbour pairs of (d_j - d_i)^2 beside the
// per-sample silog term, in the same two launches — both sit on the step's critical path.  The parts, the block reduction, the
// hand-off to the block that arrives last and the silog arithmetic are loss_common.h's, which pointwise.hip's plain and masked
// silog kernels use too: d, s2, s1 and n come out of the same operations in the same order, so that the silog part of the
// loss and, with grad_weight = 0, the gradient are the bits of those kernels.
// Compiled with -ffp-contract=off: every rounding include/a3d_gradloss.h names is a rounding of its own.
#include "a3d_internal.h"
#include "loss_common.h"
#include "../../include/a3d_gradloss.h"

namespace a3d {

constexpr int kGradK = 5;                      // s2, s1, n, sg, m per block and per sample
constexpr int kGradRound = 4 * 256;            // pixels of one round of the block's walk over its chunk (the silog kernels')
constexpr int kGradRing = 4096;                // power of two >= kGradRound + A3DG_MAX_W
constexpr int kGradTile = 8192;                // values of d a backward block stages: at least 3 rows of A3DG_MAX_W
constexpr int kGradGrid = 4096;                // blocks of the backward launch at most (40 KB of LDS each: ~4 resident per CU); the rest by grid stride
static_assert(kGradRing >= kGradRound + A3DG_MAX_W && (kGradRing & (kGradRing - 1)) == 0, "forward window");
static_assert(kGradTile >= 3 * A3DG_MAX_W, "backward tile");

// Block (b, part) walks its chunk [lo, hi) of the sample in rounds of 1024 pixels with the silog kernels' thread-to-pixel
// mapping (i0 + u * 256), and owns the pairs whose FIRST pixel lies in the chunk.  The second pixel lies up to w further on, possibly several
// chunks away: before a round the block brings d over [round start, round end + w) — what is not there yet, so one logarithm
// pair per pixel of chunk + halo — from global memory into a ring in LDS (the window is at most 1024 + w <= kGradRing values;
// a slot is overwritten only by a pixel kGradRing further on, which lies behind the round).  Then every thread takes its four
// pixels of the round from the ring: s2, s1, n exactly as the silog kernels add them, and the pair right of and the pair below
// each pixel.  Five partials per block (unmasked, n = npix and m = M are not counted and words 2 and 4 not published).
template <bool MASKED>
__global__ __launch_bounds__(256) void gradloss_fwd_kernel(const float* __restrict__ out, const float* __restrict__ tgt,
                                                           float* __restrict__ ws, float* __restrict__ loss, int h, int w, int nb,
                                                           float c, float gw) {
  constexpr int K = kGradK;
  __shared__ float dring[kGradRing];
  __shared__ unsigned char cring[MASKED ? kGradRing : 4];      // 1: the pixel counts
  __shared__ float red[K][4];
  const int npix = h * w;
  const auto [b, lo, hi] = loss_part<false>(npix);
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
  block_put(red[0], s2);
  block_put(red[1], s1);
  block_put(red[3], sg);
  if constexpr (MASKED) {
    cnt = wave_sum(cnt);            // whole numbers below 2^24: exact in any order
    mp = wave_sum(mp);
    block_put(red[2], cnt);
    block_put(red[4], mp);
  }
  __syncthreads();
  constexpr unsigned kNotCounted = MASKED ? 0u : (1u << 2) | (1u << 4);      // n = npix and m = M: nothing to count
  if (!publish_and_arrive<K, 0, kNotCounted>(ws, partials, nb, red) || threadIdx.x >= 64) return;
  const double pairs = (double)h * (double)(w - 1) + (double)(h - 1) * (double)w;      // M
  float s = 0.f, sgrad = 0.f;
  double valid = 0.0;
  for (int i = threadIdx.x; i < nb; i += 64) {
    const float a2 = fold_parts<K>(partials, i, 0), a1 = fold_parts<K>(partials, i, 1), ag = fold_parts<K>(partials, i, 3);
    // up to 2^25 pairs: the parts (each below 2^24) are added exactly in a double, then rounded once
    const float an = MASKED ? fold_parts<K>(partials, i, 2) : (float)npix;
    const double am = MASKED ? fold_parts<K, double>(partials, i, 4) : pairs;
    const float m = (float)am;
    ws[1 + K * i] = a2;
    ws[2 + K * i] = a1;
    ws[3 + K * i] = an;
    ws[4 + K * i] = ag;
    ws[5 + K * i] = m;
    if constexpr (MASKED) {
      valid += (double)an;
      if (an > 0.f) s += silog_term_masked(a2, a1, an, npix);
      if (m > 0.f) sgrad += (float)(pairs / (double)m) * ag;
    } else {
      s += silog_term(a2, a1, c);
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
    const SilogCoef coef = silog_coef<MASKED>(c, MASKED ? ws[1 + K * smp + 2] : 0.f, npix);      // used only at a pixel that counts
    float two_gwr = 0.f;
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
        float a = silog_pull<MASKED>(d, sd, coef, inv_b);
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
      write_grad(dout, dout16, ld16, smp, npix, pi, g);
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
  A3D_CHECK_ARG(w <= A3DG_MAX_W, "silog_grad_fwd: rows of %d pixels, at most A3DG_MAX_W = %d", w, A3DG_MAX_W);
  const long long npix = h > 0 && w > 0 ? (long long)h * w : 0;      // 0, which loss_check refuses, unless both are positive
  if (int rc = loss_check("silog_grad_fwd", b, npix, out && tgt && loss && ws, true)) return rc;
  A3D_CHECK_ARG(grad_weight >= 0.f, "silog_grad_fwd: grad_weight must be a number >= 0");
  clear_stale_error();
  launch_masked(masked, gradloss_fwd_kernel<false>, gradloss_fwd_kernel<true>, b * kSilogParts, stream, out, tgt, ws, loss, h, w,
                b, masked ? 0.f : kSilogC, grad_weight);
  return check_launch("silog_grad_fwd");
}

int a3dg_silog_grad_loss_bwd_ex(int b, int h, int w, const float* out, const float* tgt, int masked, float grad_weight,
                                const float* ws, float* dout, void* dout_bf16, int ld_bf16, void* stream) {
  A3D_CHECK_ARG(w <= A3DG_MAX_W, "silog_grad_bwd: rows of %d pixels, at most A3DG_MAX_W = %d", w, A3DG_MAX_W);
  const long long npix = h > 0 && w > 0 ? (long long)h * w : 0;      // 0, which loss_check refuses, unless both are positive
  if (int rc = loss_check("silog_grad_bwd", b, npix, out && tgt && ws && dout, true, dout_bf16, ld_bf16)) return rc;
  A3D_CHECK_ARG(grad_weight >= 0.f, "silog_grad_bwd: grad_weight must be a number >= 0");
  const int band = gradloss_band(w);
  const long long items = (long long)b * ((h + band - 1) / band);
  const unsigned grid = (unsigned)std::min<long long>(items, kGradGrid);
  clear_stale_error();
  launch_masked(masked, gradloss_bwd_kernel<false>, gradloss_bwd_kernel<true>, grid, stream, out, tgt, ws, dout, b, h, w, band,
                masked ? 0.f : kSilogC, 1.0f / (float)b, grad_weight, static_cast<__bf16*>(dout_bf16), ld_bf16);
  return check_launch("silog_grad_bwd");
}

}  // extern "C"
