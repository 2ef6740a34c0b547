// berhu.hip — the reverse Huber loss on linear depth, NON-REFERENCE (include/a3d_berhu.h, --loss berhu): L1 up to a threshold
// taken from each sample's own largest error, quadratic beyond it.  Three launches on the step's critical path: the
// per-sample maxima, the sums, the gradient.  The two forward launches are built from loss_common.h like the silog kernels:
// A3D_SILOG_PARTS blocks per sample (chunks rounded up to 4 pixels), the block reduction, the hand-off to the block that
// arrives last, which folds the parts in part order.  No block waits for another.
// Compiled with -ffp-contract=off: every rounding include/a3d_berhu.h names is a rounding of its own.
// The kernels stream 2 x 4 bytes per pixel (the backward writes 4 to 6 more): 16-byte accesses where the addresses allow.
// -Rpass-analysis=kernel-resource-usage (gfx950, ROCm 7.2), plain / masked:
//   berhu_max_kernel             VGPRs 28 / 37, SGPRs 32 / 36, scratch 0, LDS 52 bytes
//   berhu_sum_kernel             VGPRs 36 / 40, SGPRs 38 / 42, scratch 0, LDS 36 bytes
//   berhu_bwd_kernel, 16 bytes   VGPRs 28 / 40, SGPRs 58 / 58, scratch 0, LDS 0
//   berhu_bwd_kernel, 4 bytes    VGPRs 20 / 28, SGPRs 44 / 45, scratch 0, LDS 0
// all at 8 waves per SIMD.
#include "a3d_internal.h"
#include "loss_common.h"
#include "../../include/a3d_berhu.h"

namespace a3d {

constexpr int kBerhuK = 3;                      // per sample: c, n, poison; per block: max / count / poison, then S / nq
constexpr int kBerhuRound = 4 * 256;            // pixels of one round of a block's walk over its chunk

// First forward launch: block (b, part) leaves the largest |o - t| of its chunk's counting pixels, their number and whether
// one of them is not finite; the last block writes c, n and the poison flag of every sample to ws[1 + 3 b ..].
template <bool MASKED>
__global__ __launch_bounds__(256) void berhu_max_kernel(const float* __restrict__ out, const float* __restrict__ tgt,
                                                        float* __restrict__ ws, int npix, int nb, float fraction) {
  constexpr int K = kBerhuK;
  __shared__ float red[3][4];
  const auto [b, lo, hi] = loss_part<true>(npix);
  const float* o = out + (size_t)b * npix;
  const float* t = tgt + (size_t)b * npix;
  const bool ovec = aligned16(o), tvec = aligned16(t);
  float* partials = ws + K * nb + 1;
  float mx = 0.f, cnt = 0.f, bad = 0.f;
  for (int i0 = lo + 4 * threadIdx.x; i0 < hi; i0 += kBerhuRound) {
    float ov[4], tv[4];
    load4(o, i0, hi, ovec, ov);
    load4(t, i0, hi, tvec, tv);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (i0 + u >= hi) break;
      if constexpr (MASKED) {
        if (!isfinite(tv[u])) continue;
        cnt += 1.f;
      }
      const float a = fabsf(__fsub_rn(ov[u], tv[u]));
      if (isfinite(a)) mx = fmaxf(mx, a);
      else bad = 1.f;
    }
  }
  mx = wave_max(mx);
  bad = wave_max(bad);
  if constexpr (MASKED) cnt = wave_sum(cnt);            // whole numbers below 2^24: exact in any order; unmasked: zeros
  block_put(red[0], mx);
  block_put(red[1], cnt);
  block_put(red[2], bad);
  __syncthreads();
  constexpr unsigned kMaxes = (1u << 0) | (1u << 2);
  if (!publish_and_arrive<K, kMaxes, 0>(ws, partials, nb, red) || threadIdx.x >= 64) return;
  for (int i = threadIdx.x; i < nb; i += 64) {
    const float m = fold_parts<K, float, true>(partials, i, 0), poison = fold_parts<K, float, true>(partials, i, 2);
    const float n = MASKED ? fold_parts<K>(partials, i, 1) : (float)npix;
    ws[1 + K * i] = poison != 0.f ? __builtin_nanf("") : __fmul_rn(fraction, m);
    ws[2 + K * i] = n;
    ws[3 + K * i] = poison;
  }
}

// Second forward launch: S and nq of every chunk against the sample's c; the last block adds the parts in part order and the
// samples in ascending order (every lane of its first wavefront walks the same sequence).  A poisoned sample's c is NaN: every
// comparison with it fails, its pixels are quadratic and their rho NaN, so per, loss[0] and loss[2] are NaN by arithmetic.
template <bool MASKED>
__global__ __launch_bounds__(256) void berhu_sum_kernel(const float* __restrict__ out, const float* __restrict__ tgt,
                                                        float* __restrict__ ws, float* __restrict__ loss, int npix, int nb) {
  constexpr int K = kBerhuK;
  __shared__ float red[2][4];                           // S and nq; the third word of a block's partials is stored as 0
  const auto [b, lo, hi] = loss_part<true>(npix);
  const float* o = out + (size_t)b * npix;
  const float* t = tgt + (size_t)b * npix;
  const bool ovec = aligned16(o), tvec = aligned16(t);
  float* partials = ws + K * nb + 1;
  const float c = ws[1 + K * b];
  const float cc = __fmul_rn(c, c), c2 = __fmul_rn(2.f, c);
  float s = 0.f, nq = 0.f;
  for (int i0 = lo + 4 * threadIdx.x; i0 < hi; i0 += kBerhuRound) {
    float ov[4], tv[4];
    load4(o, i0, hi, ovec, ov);
    load4(t, i0, hi, tvec, tv);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (i0 + u >= hi) break;
      if constexpr (MASKED) {
        if (!isfinite(tv[u])) continue;
      }
      const float a = fabsf(__fsub_rn(ov[u], tv[u]));
      if (a <= c || c == 0.f) {
        s = __fadd_rn(s, a);
      } else {
        s = __fadd_rn(s, __fdiv_rn(__fadd_rn(__fmul_rn(a, a), cc), c2));
        nq += 1.f;
      }
    }
  }
  s = wave_sum(s);
  nq = wave_sum(nq);                                    // whole numbers below 2^24: exact in any order
  block_put(red[0], s);
  block_put(red[1], nq);
  __syncthreads();
  if (!publish_and_arrive<K, 0, 0>(ws, partials, nb, red) || threadIdx.x >= 64) return;
  float sum_per = 0.f, sum_c = 0.f, poisoned = 0.f;
  double sum_n = 0.0, sum_q = 0.0;
  for (int base = 0; base < nb; base += 64) {
    const int i = base + threadIdx.x;
    float per = 0.f, ci = 0.f, ni = 0.f, qi = 0.f, pi = 0.f;
    if (i < nb) {
      const float as = fold_parts<K>(partials, i, 0);
      qi = fold_parts<K>(partials, i, 1);
      ci = ws[1 + K * i];
      ni = ws[2 + K * i];
      pi = ws[3 + K * i];
      if (ni > 0.f) per = __fmul_rn(MASKED ? (float)((double)npix / (double)ni) : 1.f, as);
    }
    const int live = min(64, nb - base);
    for (int j = 0; j < live; ++j) {                    // ascending sample order, the same in every lane
      sum_per += __shfl(per, j, 64);
      sum_c += __shfl(ci, j, 64);
      sum_n += (double)__shfl(ni, j, 64);
      sum_q += (double)__shfl(qi, j, 64);
      poisoned = fmaxf(poisoned, __shfl(pi, j, 64));
    }
  }
  if (threadIdx.x == 0) {
    loss[0] = sum_per / (float)nb;
    loss[1] = MASKED ? (float)(sum_n / ((double)nb * (double)npix)) : 1.f;
    loss[2] = sum_c / (float)nb;
    loss[3] = poisoned != 0.f ? __builtin_nanf("") : sum_n > 0.0 ? (float)(sum_q / sum_n) : 0.f;
  }
}

__device__ __forceinline__ float berhu_grad(float o, float t, float c, float s, bool alive, bool poisoned) {
  if (poisoned) return __builtin_nanf("");
  if (!alive) return 0.f;
  const float e = __fsub_rn(o, t);
  if (e == 0.f) return 0.f;
  if (fabsf(e) <= c || c == 0.f) return copysignf(s, e);
  return __fmul_rn(__fdiv_rn(e, c), s);
}

// One work item is four consecutive elements of the flat [b npix] tensors (VEC: all three base addresses lie on 16 bytes, so
// the group is one 16-byte access whatever npix is; a group may span the end of a row) or one element.  Operation order:
// include/a3d_berhu.h.
template <bool MASKED, bool VEC>
__global__ __launch_bounds__(256) void berhu_bwd_kernel(const float* __restrict__ out, const float* __restrict__ tgt,
                                                        const float* __restrict__ ws, float* __restrict__ dout, int nb, int npix,
                                                        float inv_b, __bf16* __restrict__ dout16, int ld16) {
  constexpr int W = VEC ? 4 : 1;
  const size_t total = (size_t)nb * npix;
  const size_t items = (total + W - 1) / W;
  for (size_t it = (size_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (size_t)gridDim.x * 256) {
    const size_t i0 = it * W;
    float ov[W], tv[W], gv[W];
    const bool whole = i0 + W <= total;
    if constexpr (VEC) {
      if (whole) {
        const f32x4 qo = *reinterpret_cast<const f32x4*>(out + i0), qt = *reinterpret_cast<const f32x4*>(tgt + i0);
        ov[0] = qo.x; ov[1] = qo.y; ov[2] = qo.z; ov[3] = qo.w;
        tv[0] = qt.x; tv[1] = qt.y; tv[2] = qt.z; tv[3] = qt.w;
      }
    }
    if (!VEC || !whole) {
#pragma unroll
      for (int u = 0; u < W; ++u) {
        ov[u] = i0 + u < total ? out[i0 + u] : 0.f;
        tv[u] = i0 + u < total ? tgt[i0 + u] : 0.f;
      }
    }
    int smp = (int)(i0 / (size_t)npix);
    int col = (int)(i0 - (size_t)smp * npix);
#pragma unroll
    for (int u = 0; u < W; ++u) {
      if (i0 + u < total) {
        const float c = ws[1 + kBerhuK * smp];
        float s = inv_b;
        if constexpr (MASKED) {
          const float n = ws[2 + kBerhuK * smp];        // used only at a pixel that counts: then n >= 1
          s = __fmul_rn(inv_b, (float)((double)npix / (double)fmaxf(n, 1.f)));
        }
        const float g = berhu_grad(ov[u], tv[u], c, s, !MASKED || isfinite(tv[u]), ws[3 + kBerhuK * smp] != 0.f);
        gv[u] = g;
        write_grad16(dout16, ld16, smp, col, g);
        if (++col == npix) {
          col = 0;
          ++smp;
        }
      }
    }
    if (VEC && whole) {
      f32x4 q;
      q.x = gv[0]; q.y = gv[W > 1 ? 1 : 0]; q.z = gv[W > 2 ? 2 : 0]; q.w = gv[W > 3 ? 3 : 0];
      *reinterpret_cast<f32x4*>(dout + i0) = q;
    } else {
#pragma unroll
      for (int u = 0; u < W; ++u)
        if (i0 + u < total) dout[i0 + u] = gv[u];
    }
  }
}

}  // namespace a3d
using namespace a3d;

extern "C" {

int a3dh_berhu_loss_fwd(int b, int npix, const float* out, const float* tgt, int masked, float fraction, float* loss, float* ws,
                        void* stream) {
  if (int rc = loss_check("berhu_fwd", b, npix, out && tgt && loss && ws, true)) return rc;
  A3D_CHECK_ARG(masked == 0 || masked == 1, "berhu_fwd: masked = %d is neither 0 nor 1", masked);
  A3D_CHECK_ARG(fraction > 0.f && fraction <= 1.f, "berhu_fwd: a threshold fraction of %g, outside (0, 1]", (double)fraction);
  clear_stale_error();
  launch_masked(masked, berhu_max_kernel<false>, berhu_max_kernel<true>, b * kSilogParts, stream, out, tgt, ws, npix, b, fraction);
  launch_masked(masked, berhu_sum_kernel<false>, berhu_sum_kernel<true>, b * kSilogParts, stream, out, tgt, ws, loss, npix, b);
  return check_launch("berhu_fwd");
}

int a3dh_berhu_loss_bwd_ex(int b, int npix, const float* out, const float* tgt, int masked, float fraction, const float* ws,
                           float* dout, void* dout_bf16, int ld_bf16, void* stream) {
  if (int rc = loss_check("berhu_bwd", b, npix, out && tgt && ws && dout, true, dout_bf16, ld_bf16)) return rc;
  A3D_CHECK_ARG(masked == 0 || masked == 1, "berhu_bwd: masked = %d is neither 0 nor 1", masked);
  A3D_CHECK_ARG(fraction > 0.f && fraction <= 1.f, "berhu_bwd: a threshold fraction of %g, outside (0, 1]", (double)fraction);
  const size_t total = (size_t)b * npix;
  const bool vec = aligned16(out) && aligned16(tgt) && aligned16(dout);
  const float inv_b = 1.0f / (float)b;
  __bf16* d16 = static_cast<__bf16*>(dout_bf16);
  clear_stale_error();
  if (vec)
    launch_masked(masked, berhu_bwd_kernel<false, true>, berhu_bwd_kernel<true, true>, grid_for((total + 3) / 4), stream, out, tgt,
                  ws, dout, b, npix, inv_b, d16, ld_bf16);
  else
    launch_masked(masked, berhu_bwd_kernel<false, false>, berhu_bwd_kernel<true, false>, grid_for(total), stream, out, tgt, ws,
                  dout, b, npix, inv_b, d16, ld_bf16);
  return check_launch("berhu_bwd");
}

}  // extern "C"
