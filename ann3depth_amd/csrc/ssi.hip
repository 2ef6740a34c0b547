// ssi.hip — the least-squares scale-and-shift-invariant loss on linear depth, NON-REFERENCE (include/a3d_ssi.h, --loss ssi):
// per sample the squared error that remains after the best scale and shift of the OUTPUT.  Three launches on the step's
// critical path: the float64 sums of the fit, the residual sum, the gradient.  The two forward launches are built from
// loss_common.h like berhu.hip's: A3D_SILOG_PARTS blocks per sample (chunks rounded up to 4 pixels), the block reduction,
// the hand-off to the block that arrives last, which folds the parts in part order — in the first launch in float64 (8-byte
// words at even offsets of ws), where that block also solves the fit.  No block waits for another.
// Compiled with -ffp-contract=off: every rounding include/a3d_ssi.h names is a rounding of its own.
// The kernels stream 2 x 4 bytes per pixel (the backward writes 4 to 6 more): 16-byte accesses where the addresses allow.
// -Rpass-analysis=kernel-resource-usage (gfx950, ROCm 7.2), plain / masked:
//   ssi_fit_kernel              VGPRs 79 / 89, SGPRs 36 / 32, scratch 0, LDS 168 bytes, 6 / 5 waves per SIMD
//   ssi_sum_kernel              VGPRs 18 / 26, SGPRs 34 / 35, scratch 0, LDS 20 bytes
//   ssi_bwd_kernel, 16 bytes    VGPRs 28 / 36, SGPRs 54 / 58, scratch 0, LDS 0
//   ssi_bwd_kernel, 4 bytes     VGPRs 19 / 28, SGPRs 43 / 44, scratch 0, LDS 0
// the last three at 8 waves per SIMD.  ssi_fit_kernel's registers are the last block's: four float64 folds of eight parts
// and the solve's divisions; at b = 32 a launch is 256 blocks of four waves on 1024 SIMDs, so occupancy does not bind.
#include "a3d_internal.h"
#include "loss_common.h"
#include "../../include/a3d_ssi.h"

namespace a3d {

constexpr int kSsiSample = 4;                   // per sample: s, t, n, flag at ws[2 + 4 i ..]
constexpr int kSsiFitK = 10;                    // per block, first launch: S_o, S_d, S_oo, S_od (float64), n, poison mark
constexpr int kSsiSumK = 1;                     // per block, second launch: S
constexpr int kSsiRound = 4 * 256;              // pixels of one round of a block's walk over its chunk
constexpr float kSsiFitted = 0.f, kSsiDegenerate = 1.f, kSsiPoisoned = 2.f;

__device__ __forceinline__ float* ssi_partials(float* ws, int nb) { return ws + 2 + kSsiSample * nb; }

// First forward launch: block (b, part) leaves the four float64 sums of its chunk's counting pixels, their number and
// whether the sample is poisoned there; the last block adds the parts, solves and writes s, t, n and the flag of every sample.
template <bool MASKED>
__global__ __launch_bounds__(256) void ssi_fit_kernel(const float* __restrict__ out, const float* __restrict__ tgt,
                                                      float* __restrict__ ws, int npix, int nb) {
  constexpr int K = kSsiFitK;
  __shared__ double red64[4][4];
  __shared__ float red[2][4];
  const auto [b, lo, hi] = loss_part<true>(npix);
  const float* o = out + (size_t)b * npix;
  const float* t = tgt + (size_t)b * npix;
  const bool ovec = aligned16(o), tvec = aligned16(t);
  float* partials = ssi_partials(ws, nb);
  double so = 0.0, sd = 0.0, soo = 0.0, sod = 0.0;
  float cnt = 0.f, bad = 0.f;
  for (int i0 = lo + 4 * threadIdx.x; i0 < hi; i0 += kSsiRound) {
    float ov[4], tv[4];
    load4(o, i0, hi, ovec, ov);
    load4(t, i0, hi, tvec, tv);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (i0 + u >= hi) break;
      if constexpr (MASKED) {
        if (!isfinite(tv[u])) continue;
        cnt += 1.f;
        if (!isfinite(ov[u])) bad = 1.f;
      } else {
        if (!isfinite(ov[u]) || !isfinite(tv[u])) bad = 1.f;
      }
      const double od = (double)ov[u], dd = (double)tv[u];
      so += od;
      sd += dd;
      soo += od * od;                                   // 24-bit factors: the float64 product is exact
      sod += od * dd;
    }
  }
  so = wave_sum(so);
  sd = wave_sum(sd);
  soo = wave_sum(soo);
  sod = wave_sum(sod);
  bad = wave_max(bad);
  if constexpr (MASKED) cnt = wave_sum(cnt);            // whole numbers below 2^24: exact in any order; unmasked: zeros
  block_put(red64[0], so);
  block_put(red64[1], sd);
  block_put(red64[2], soo);
  block_put(red64[3], sod);
  block_put(red[0], cnt);
  block_put(red[1], bad);
  __syncthreads();
  if (threadIdx.x == 0) {
    float* mine = partials + K * blockIdx.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) publish64(mine + 2 * k, block_sum64(red64[k]));
    publish32(mine + 8, block_combine<false>(red[0]));
    publish32(mine + 9, block_combine<true>(red[1]));
  }
  if (!arrive(ws, nb) || threadIdx.x >= 64) return;
  for (int i = threadIdx.x; i < nb; i += 64) {
    const double s_o = fold_parts64<K>(partials, i, 0), s_d = fold_parts64<K>(partials, i, 2);
    const double s_oo = fold_parts64<K>(partials, i, 4), s_od = fold_parts64<K>(partials, i, 6);
    const float nf = MASKED ? fold_parts<K>(partials, i, 8) : (float)npix;
    const float poison = fold_parts<K, float, true>(partials, i, 9);
    const double n = (double)nf;
    float s = 0.f, sh = 0.f, flag = kSsiDegenerate;
    if (poison != 0.f) {
      s = sh = __builtin_nanf("");
      flag = kSsiPoisoned;
    } else if (nf >= 1.f) {
      const double den = s_oo - (s_o * s_o) / n, num = s_od - (s_o * s_d) / n;
      const double s64 = num / den, t64 = (s_d - s64 * s_o) / n;
      const float sf = (float)s64, tf = (float)t64;
      if (nf >= 2.f && den > 0x1p-30 * s_oo && isfinite(sf) && isfinite(tf)) {
        s = sf;
        sh = tf;
        flag = kSsiFitted;
      } else {
        sh = (float)(s_d / n);
      }
    }
    float* mine = ws + 2 + kSsiSample * i;
    mine[0] = s;
    mine[1] = sh;
    mine[2] = nf;
    mine[3] = flag;
  }
}

// r of include/a3d_ssi.h: the residual of one pixel after the sample's scale and shift
__device__ __forceinline__ float ssi_residual(float o, float d, float s, float sh) {
  return __fsub_rn(__fadd_rn(__fmul_rn(s, o), sh), d);
}

// Second forward launch: S of every chunk under the sample's s and t; the last block adds the parts in part order and the
// samples in ascending order (every lane of its first wavefront walks the same sequence).  A poisoned sample's s and t are
// NaN and it has a counting pixel, so its S, per, and with them loss[0], loss[2] and loss[3], are NaN by arithmetic; a
// degenerate sample's s is +0.0 and its residual t - d.
template <bool MASKED>
__global__ __launch_bounds__(256) void ssi_sum_kernel(const float* __restrict__ out, const float* __restrict__ tgt,
                                                      float* __restrict__ ws, float* __restrict__ loss, int npix, int nb) {
  constexpr int K = kSsiSumK;
  __shared__ float red[1][4];
  const auto [b, lo, hi] = loss_part<true>(npix);
  const float* o = out + (size_t)b * npix;
  const float* t = tgt + (size_t)b * npix;
  const bool ovec = aligned16(o), tvec = aligned16(t);
  float* partials = ssi_partials(ws, nb);
  const float s = ws[2 + kSsiSample * b], sh = ws[3 + kSsiSample * b];
  float acc = 0.f;
  for (int i0 = lo + 4 * threadIdx.x; i0 < hi; i0 += kSsiRound) {
    float ov[4], tv[4];
    load4(o, i0, hi, ovec, ov);
    load4(t, i0, hi, tvec, tv);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (i0 + u >= hi) break;
      if constexpr (MASKED) {
        if (!isfinite(tv[u])) continue;
      }
      const float r = ssi_residual(ov[u], tv[u], s, sh);
      acc = __fadd_rn(acc, __fmul_rn(r, r));
    }
  }
  acc = wave_sum(acc);
  block_put(red[0], acc);
  __syncthreads();
  if (!publish_and_arrive<K, 0, 0>(ws, partials, nb, red) || threadIdx.x >= 64) return;
  float sum_per = 0.f, sum_s = 0.f, sum_t = 0.f;
  double sum_n = 0.0;
  for (int base = 0; base < nb; base += 64) {
    const int i = base + threadIdx.x;
    float per = 0.f, si = 0.f, ti = 0.f, ni = 0.f;
    if (i < nb) {
      const float as = fold_parts<K>(partials, i, 0);
      si = ws[2 + kSsiSample * i];
      ti = ws[3 + kSsiSample * i];
      ni = ws[4 + kSsiSample * i];
      if (ni > 0.f) per = __fmul_rn(MASKED ? (float)(0.5 * (double)npix / (double)ni) : 0.5f, as);
    }
    const int live = min(64, nb - base);
    for (int j = 0; j < live; ++j) {                    // ascending sample order, the same in every lane
      sum_per += __shfl(per, j, 64);
      sum_s += __shfl(si, j, 64);
      sum_t += __shfl(ti, j, 64);
      sum_n += (double)__shfl(ni, j, 64);
    }
  }
  if (threadIdx.x == 0) {
    loss[0] = sum_per / (float)nb;
    loss[1] = MASKED ? (float)(sum_n / ((double)nb * (double)npix)) : 1.f;
    loss[2] = sum_s / (float)nb;
    loss[3] = sum_t / (float)nb;
  }
}

// One work item is four consecutive elements of the flat [b npix] tensors (VEC: all three base addresses lie on 16 bytes, so
// the group is one 16-byte access whatever npix is; a group may span the end of a row) or one element.  Operation order:
// include/a3d_ssi.h.
template <bool MASKED, bool VEC>
__global__ __launch_bounds__(256) void ssi_bwd_kernel(const float* __restrict__ out, const float* __restrict__ tgt,
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
        const float* mine = ws + 2 + kSsiSample * smp;
        const float s = mine[0], sh = mine[1], flag = mine[3];
        float k = inv_b;
        if constexpr (MASKED) k = __fmul_rn(inv_b, (float)((double)npix / (double)fmaxf(mine[2], 1.f)));   // used where n >= 1
        float g = 0.f;
        if (flag == kSsiPoisoned) g = __builtin_nanf("");
        else if (flag == kSsiFitted && (!MASKED || isfinite(tv[u])))
          g = __fmul_rn(__fmul_rn(s, ssi_residual(ov[u], tv[u], s, sh)), k);
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

int a3di_ssi_loss_fwd(int b, int npix, const float* out, const float* tgt, int masked, float* loss, float* ws, void* stream) {
  if (int rc = loss_check("ssi_fwd", b, npix, out && tgt && loss && ws, true)) return rc;
  A3D_CHECK_ARG(masked == 0 || masked == 1, "ssi_fwd: masked = %d is neither 0 nor 1", masked);
  A3D_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "ssi_fwd: the workspace does not start on an 8-byte address");
  clear_stale_error();
  launch_masked(masked, ssi_fit_kernel<false>, ssi_fit_kernel<true>, b * kSilogParts, stream, out, tgt, ws, npix, b);
  launch_masked(masked, ssi_sum_kernel<false>, ssi_sum_kernel<true>, b * kSilogParts, stream, out, tgt, ws, loss, npix, b);
  return check_launch("ssi_fwd");
}

int a3di_ssi_loss_bwd_ex(int b, int npix, const float* out, const float* tgt, int masked, const float* ws, float* dout,
                         void* dout_bf16, int ld_bf16, void* stream) {
  if (int rc = loss_check("ssi_bwd", b, npix, out && tgt && ws && dout, true, dout_bf16, ld_bf16)) return rc;
  A3D_CHECK_ARG(masked == 0 || masked == 1, "ssi_bwd: masked = %d is neither 0 nor 1", masked);
  A3D_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "ssi_bwd: the workspace does not start on an 8-byte address");
  const size_t total = (size_t)b * npix;
  const bool vec = aligned16(out) && aligned16(tgt) && aligned16(dout);
  const float inv_b = 1.0f / (float)b;
  __bf16* d16 = static_cast<__bf16*>(dout_bf16);
  clear_stale_error();
  if (vec)
    launch_masked(masked, ssi_bwd_kernel<false, true>, ssi_bwd_kernel<true, true>, grid_for((total + 3) / 4), stream, out, tgt,
                  ws, dout, b, npix, inv_b, d16, ld_bf16);
  else
    launch_masked(masked, ssi_bwd_kernel<false, false>, ssi_bwd_kernel<true, false>, grid_for(total), stream, out, tgt, ws,
                  dout, b, npix, inv_b, d16, ld_bf16);
  return check_launch("ssi_bwd");
}

}  // extern "C"
