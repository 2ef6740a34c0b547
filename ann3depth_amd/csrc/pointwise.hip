// pointwise.hip — the HBM-bound kernels of the step that are neither pooling (pool.hip) nor resampling (resample.hip):
// scale-invariant log loss (wavefront-shuffle reductions), TF-1.3 ApplyAdam, the dropout keep mask, the casts and copies
// of bf16 storage, streams and the collective stand-in; each family's kernels are followed by its entry points.
// This file is compiled with -ffp-contract=off (see Makefile): the oracle does these computations as separate
// fp32 operations, and without FMA contraction the kernels are bit-exact against the numpy restatement (HIP's
// __f*_rn intrinsics are plain operators on ROCm 7.2 and do not prevent contraction by themselves).
#include <algorithm>

#include "a3d_internal.h"
#include "loss_common.h"
#include "optim_rules.h"
#include "../../include/a3d_valid.h"

using namespace a3d;

namespace a3d {
// ------------------------------------------------------------------ scale-invariant log loss
// The parts, the block reduction, the hand-off to the block that arrives last and the silog arithmetic: loss_common.h,
// shared with gradloss.hip and berhu.hip.
// kSilogParts blocks per sample (one sample is 4070 pixels at MSDN's size: with one block per sample 32 CUs each walked a
// chain of load latencies and logarithms — 29 us on the step's critical path; now every CU holds one short piece).  Block
// (b, part) leaves its partial sums in ws[2nb+1 + 2(b*parts+part) ..]; the block that finishes last adds each sample's
// parts in part order, writes ws[1+2b] = sum d^2, ws[2+2b] = sum d for the backward kernel, and the batch mean.
//
// MASKED (NON-REFERENCE, a3dx_silog_masked_loss_fwd): a target that is not finite is a hole and is left out of the sums;
// a third value per block and per sample, the number n of pixels that count, travels beside the two sums (K = 3 floats
// where the plain kernel has 2), and the sample's term is (npix / n) (s2 - (0.5 / n) s1^2), 0 when n = 0.  Same parts, same
// reductions, same last block: with no hole and npix = 4070 the constants are the plain kernel's and so are the bits.
template <bool MASKED>
__global__ __launch_bounds__(256) void silog_fwd_kernel(const float* __restrict__ out, const float* __restrict__ tgt,
                                                        float* __restrict__ ws, float* __restrict__ loss, int npix, int nb,
                                                        float c) {
  constexpr int K = MASKED ? 3 : 2;
  __shared__ float red[K][4];
  const auto [b, lo, hi] = loss_part<false>(npix);
  const float* o = out + (size_t)b * npix;
  const float* t = tgt + (size_t)b * npix;
  float* partials = ws + K * nb + 1;
  float s2 = 0.f, s1 = 0.f, cnt = 0.f;
  // four elements per thread and round, all eight loads issued before the first logarithm
  for (int i0 = lo + threadIdx.x; i0 < hi; i0 += 4 * 256) {
    float ov[4], tv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + u * 256;
      ov[u] = i < hi ? o[i] : 0.f;
      tv[u] = i < hi ? t[i] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (i0 + u * 256 >= hi) break;
      if constexpr (MASKED) {
        if (!isfinite(tv[u])) continue;
        cnt += 1.f;
      }
      const float d = __fsub_rn(masked_log(ov[u]), masked_log(tv[u]));
      s2 += d * d;
      s1 += d;
    }
  }
  s2 = wave_sum(s2);
  s1 = wave_sum(s1);
  block_put(red[0], s2);
  block_put(red[1], s1);
  if constexpr (MASKED) block_put(red[2], wave_sum(cnt));            // whole numbers below 2^24: exact in any order
  __syncthreads();
  if (!publish_and_arrive<K, 0, 0>(ws, partials, nb, red) || threadIdx.x >= 64) return;
  float s = 0.f;
  double valid = 0.0;
  for (int i = threadIdx.x; i < nb; i += 64) {
    const float a2 = fold_parts<K>(partials, i, 0), a1 = fold_parts<K>(partials, i, 1);
    const float an = MASKED ? fold_parts<K>(partials, i, 2) : 0.f;      // every load of the partials before the first store to ws
    ws[1 + K * i] = a2;
    ws[2 + K * i] = a1;
    if constexpr (MASKED) {
      ws[3 + K * i] = an;
      valid += (double)an;
      if (an > 0.f) s += silog_term_masked(a2, a1, an, npix);
    } else {
      s += silog_term(a2, a1, c);
    }
  }
  s = wave_sum(s);
  if constexpr (MASKED) valid = wave_sum(valid);
  if (threadIdx.x == 0) {
    loss[0] = s / (float)nb;
    if constexpr (MASKED) loss[1] = (float)(valid / ((double)nb * (double)npix));
  }
}

template <bool MASKED>
__global__ __launch_bounds__(256) void silog_bwd_kernel(const float* __restrict__ out, const float* __restrict__ tgt,
                                                        const float* __restrict__ ws, float* __restrict__ dout, int b,
                                                        int npix, float c, float inv_b, __bf16* __restrict__ dout16 = nullptr,
                                                        int ld16 = 0) {
  constexpr int K = MASKED ? 3 : 2;
  const size_t total = (size_t)b * npix;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int smp = (int)(i / npix);
    const float o = out[i];
    const float arg = __fadd_rn(o, 1e-8f);
    const float lo = logf(arg);
    float g = 0.f;
    const float t = MASKED || !isnan(lo) ? tgt[i] : 0.f;
    if (!isnan(lo) && (!MASKED || isfinite(t))) {        // a pixel that counts: its sample has n >= 1
      const float d = __fsub_rn(lo, masked_log(t));
      const float sd = ws[K * smp + 2];
      g = __fdiv_rn(silog_pull<MASKED>(d, sd, silog_coef<MASKED>(c, MASKED ? ws[K * smp + 3] : 0.f, npix), inv_b), arg);
    }
    write_grad(dout, dout16, ld16, smp, npix, i - (size_t)smp * npix, g);
  }
}

}  // namespace a3d

extern "C" {

int a3d_silog_loss_fwd(int b, int npix, const float* out, const float* tgt, float* loss, float* ws, void* stream) {
  if (int rc = loss_check("silog_fwd", b, npix, out && tgt && loss && ws, false)) return rc;
  clear_stale_error();
  hipLaunchKernelGGL(silog_fwd_kernel<false>, dim3(b * kSilogParts), dim3(256), 0, static_cast<hipStream_t>(stream), out, tgt,
                     ws, loss, npix, b, kSilogC);
  return check_launch("silog_fwd");
}

int a3d_silog_loss_bwd(int b, int npix, const float* out, const float* tgt, const float* ws, float* dout, void* stream) {
  return a3d_silog_loss_bwd_ex(b, npix, out, tgt, ws, dout, nullptr, 0, stream);
}

int a3d_silog_loss_bwd_ex(int b, int npix, const float* out, const float* tgt, const float* ws, float* dout, void* dout_bf16,
                          int ld_bf16, void* stream) {
  if (int rc = loss_check("silog_bwd", b, npix, out && tgt && ws && dout, false, dout_bf16, ld_bf16)) return rc;
  clear_stale_error();
  hipLaunchKernelGGL(silog_bwd_kernel<false>, dim3(grid_for((size_t)b * npix)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     out, tgt, ws, dout, b, npix, kSilogC, 1.0f / (float)b, static_cast<__bf16*>(dout_bf16), ld_bf16);
  return check_launch("silog_bwd");
}

int a3dx_silog_masked_loss_fwd(int b, int npix, const float* out, const float* tgt, float* loss, float* ws, void* stream) {
  if (int rc = loss_check("silog_masked_fwd", b, npix, out && tgt && loss && ws, true)) return rc;
  clear_stale_error();
  hipLaunchKernelGGL(silog_fwd_kernel<true>, dim3(b * kSilogParts), dim3(256), 0, static_cast<hipStream_t>(stream), out, tgt,
                     ws, loss, npix, b, 0.f);
  return check_launch("silog_masked_fwd");
}

int a3dx_silog_masked_loss_bwd_ex(int b, int npix, const float* out, const float* tgt, const float* ws, float* dout,
                                 void* dout_bf16, int ld_bf16, void* stream) {
  if (int rc = loss_check("silog_masked_bwd", b, npix, out && tgt && ws && dout, false, dout_bf16, ld_bf16)) return rc;
  clear_stale_error();
  hipLaunchKernelGGL(silog_bwd_kernel<true>, dim3(grid_for((size_t)b * npix)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     out, tgt, ws, dout, b, npix, 0.f, 1.0f / (float)b, static_cast<__bf16*>(dout_bf16), ld_bf16);
  return check_launch("silog_masked_bwd");
}

}  // extern "C"

namespace a3d {
// ------------------------------------------------------------------ ApplyAdam (TF 1.3 formula)
// adam_one and the two walks (adam_body; adam_frozen_body, the reference's alpha == 0, beta2 == 1 case): optim_rules.h, shared with
// the launches that take their scale from a gradient-norm control block (clip.hip)
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ var, float* __restrict__ m,
                                                   float* __restrict__ v, const float* __restrict__ g, size_t count,
                                                   float omb1, float omb2, float alpha, float eps, float gscale,
                                                   unsigned int* __restrict__ poisoned) {
  adam_body(var, m, v, g, count, omb1, omb2, alpha, eps, gscale, poisoned);
}

__global__ __launch_bounds__(256) void adam_frozen_kernel(float* __restrict__ var, float* __restrict__ m,
                                                          float* __restrict__ v, const float* __restrict__ g,
                                                          size_t count, float omb1, float gscale,
                                                          unsigned int* __restrict__ poisoned) {
  adam_frozen_body(var, m, v, g, count, omb1, gscale, poisoned);
}

}  // namespace a3d

extern "C" {

int a3d_adam_apply_tf1(size_t count, float* var, float* m, float* v, const float* g, float lr, float beta1,
                       float beta2, float eps, float beta1_power, float beta2_power, float grad_scale,
                       void* stream) {
  return a3d_adam_apply_tf1_flag(count, var, m, v, g, lr, beta1, beta2, eps, beta1_power, beta2_power, grad_scale,
                                 nullptr, stream);
}

int a3d_adam_apply_tf1_flag(size_t count, float* var, float* m, float* v, const float* g, float lr, float beta1,
                            float beta2, float eps, float beta1_power, float beta2_power, float grad_scale,
                            unsigned int* poisoned, void* stream) {
  A3D_CHECK_ARG(count > 0 && var && m && v && g, "adam: bad arguments");
  A3D_CHECK_ARG(((reinterpret_cast<uintptr_t>(var) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v) |
                  reinterpret_cast<uintptr_t>(g)) & 15) == 0, "adam: buffers must be 16-byte aligned");
  const AdamHost h = adam_host(lr, beta2, beta1_power, beta2_power);
  if (h.frozen) {
    clear_stale_error();
    hipLaunchKernelGGL(adam_frozen_kernel, dim3(rule_grid_vec(count)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), var, m, v, g, count, 1.f - beta1, grad_scale, poisoned);
    return check_launch("adam_frozen");
  }
  clear_stale_error();
  hipLaunchKernelGGL(adam_kernel, dim3(rule_grid_vec(count)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), var, m, v, g, count, 1.f - beta1, 1.f - beta2, h.alpha, eps,
                     grad_scale, poisoned);
  return check_launch("adam");
}

}  // extern "C"

namespace a3d {
// ------------------------------------------------------------------ dropout keep mask (Philox4x32-10)
// TF draws U[0,1) from its own Philox stream, which is not reproducible outside TF; this is the same generator
// family keyed by (seed, step), one counter per 4 mask bytes.  keep = floor(keep_prob + u)  (nn.dropout, TF 1.3), written
// as the comparison below: the same byte wherever the sum is below 2, and 1 instead of 2 where rate = 0 meets
// u = 1 - 2^-24 (fl(1 + u) = 2, tie to even).
__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
  const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
  const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
  const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
  c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
}

__global__ __launch_bounds__(256) void dropout_mask_kernel(uint8_t* __restrict__ keep, size_t count, uint32_t seed_lo,
                                                           uint32_t seed_hi, uint32_t step_lo, uint32_t step_hi,
                                                           float keep_prob) {
  const size_t nquad = (count + 3) / 4;
  for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < nquad; q += (size_t)gridDim.x * 256) {
    uint32_t c[4] = {(uint32_t)q, (uint32_t)(q >> 32), step_lo, step_hi};
    uint32_t k0 = seed_lo, k1 = seed_hi;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
      philox_round(c, k0, k1);
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const size_t i = q * 4 + j;
      if (i < count) {
        const float u = (float)(c[j] >> 8) * (1.0f / 16777216.0f);      // 24 random bits -> [0,1)
        keep[i] = __fadd_rn(keep_prob, u) >= 1.0f ? 1 : 0;
      }
    }
  }
}
}  // namespace a3d

extern "C" {

int a3d_dropout_keep_mask(size_t count, uint64_t seed, uint64_t step, float rate, uint8_t* keep, void* stream) {
  A3D_CHECK_ARG(count > 0 && keep && rate >= 0.f && rate < 1.f, "dropout_keep_mask: bad arguments");
  clear_stale_error();
  hipLaunchKernelGGL(dropout_mask_kernel, dim3(grid_for((count + 3) / 4)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), keep, count, (uint32_t)seed, (uint32_t)(seed >> 32),
                     (uint32_t)step, (uint32_t)(step >> 32), 1.0f - rate);
  return check_launch("dropout_mask");
}

}  // extern "C"

namespace a3d {
// ------------------------------------------------------------------ bf16 storage (BASELINE config 5)
// float32 [pixels][c_src] -> bf16 [pixels][4], missing channels zero: an 8-byte pixel, so that the window runs of a
// few-channel conv start 16 bytes apart at even strides and the bf16 kernel can gather them (igemm_host.hip)
__global__ __launch_bounds__(256) void pad_channels_bf16_kernel(const float* __restrict__ src, __bf16* __restrict__ dst,
                                                                size_t pixels, int c_src) {
  typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < pixels; i += (size_t)gridDim.x * 256) {
    bf16x4 o = {(__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f};
    for (int c = 0; c < c_src; ++c) o[c] = (__bf16)src[i * c_src + c];
    reinterpret_cast<bf16x4*>(dst)[i] = o;
  }
}

__global__ __launch_bounds__(256) void cast_bf16_kernel(const void* __restrict__ src, void* __restrict__ dst, size_t count,
                                                        int to_bf16) {
  typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
  const size_t nvec = count / 4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (size_t)gridDim.x * 256) {
    if (to_bf16) {
      const f32x4 v = reinterpret_cast<const f32x4*>(src)[i];
      const bf16x4 o = {(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
      reinterpret_cast<bf16x4*>(dst)[i] = o;
    } else {
      const bf16x4 v = reinterpret_cast<const bf16x4*>(src)[i];
      const f32x4 o = {(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
      reinterpret_cast<f32x4*>(dst)[i] = o;
    }
  }
  if (blockIdx.x == 0) {
    const size_t i = nvec * 4 + threadIdx.x;
    if (i < count) {
      if (to_bf16) reinterpret_cast<__bf16*>(dst)[i] = (__bf16) reinterpret_cast<const float*>(src)[i];
      else reinterpret_cast<float*>(dst)[i] = (float)reinterpret_cast<const __bf16*>(src)[i];
    }
  }
}
// dst[r][c] = src[r][c] for c < cols (float32 or bf16 on either side, round to nearest even), dst[r][c] = 0 for
// cols <= c < ld_dst: row pitches change (a padded bf16 copy of a matrix whose rows are not whole 16-byte pieces, and back)
template <bool S16, bool D16>
__global__ __launch_bounds__(256) void cast_rows_kernel(const void* __restrict__ src, void* __restrict__ dst, size_t rows, int cols,
                                                        int ld_src, int ld_dst) {
  const size_t total = rows * (size_t)ld_dst;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t r = i / (size_t)ld_dst;
    const int c = (int)(i - r * (size_t)ld_dst);
    float v = 0.f;
    if (c < cols) v = S16 ? (float)static_cast<const __bf16*>(src)[r * ld_src + c] : static_cast<const float*>(src)[r * ld_src + c];
    if (D16) static_cast<__bf16*>(dst)[i] = (__bf16)v;
    else static_cast<float*>(dst)[i] = v;
  }
}
// one channel of a float32 tensor into one channel of a float32 or bf16 tensor (round to nearest even)
template <typename D>
__global__ __launch_bounds__(256) void copy_channel_kernel(const float* __restrict__ src, D* __restrict__ dst, size_t npix,
                                                           int ld_src, int c_src, int ld_dst, int c_dst) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (size_t)gridDim.x * 256)
    dst[i * ld_dst + c_dst] = (D)src[i * ld_src + c_src];
}
}  // namespace a3d

extern "C" {

int a3d_pad_channels_bf16(size_t pixels, int c_src, const float* src, int c_dst, void* dst, void* stream) {
  A3D_CHECK_ARG(pixels > 0 && src && dst && c_src >= 1 && c_dst == 4 && c_src <= 4, "pad_channels_bf16: 1..4 channels to 4");
  A3D_CHECK_ARG((reinterpret_cast<uintptr_t>(dst) & 7) == 0, "pad_channels_bf16: 8-byte aligned destination");
  clear_stale_error();
  hipLaunchKernelGGL(pad_channels_bf16_kernel, dim3(grid_for(pixels, 256, 4096)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     src, static_cast<__bf16*>(dst), pixels, c_src);
  return check_launch("pad_channels_bf16");
}

int a3d_cast_bf16(size_t count, const void* src, void* dst, int to_bf16, void* stream) {
  A3D_CHECK_ARG(count > 0 && src && dst, "cast_bf16: bad arguments");
  A3D_CHECK_ARG(((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0, "cast_bf16: 16-byte aligned buffers");
  clear_stale_error();
  hipLaunchKernelGGL(cast_bf16_kernel, dim3(grid_for(count / 4 + 1, 256, 4096)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), src, dst, count, to_bf16);
  return check_launch("cast_bf16");
}

int a3d_cast_rows(size_t rows, int cols, const void* src, int ld_src, int src_bf16, void* dst, int ld_dst, int dst_bf16,
                  void* stream) {
  A3D_CHECK_ARG(rows > 0 && cols > 0 && src && dst && ld_src >= cols && ld_dst >= cols, "cast_rows: bad arguments");
  const size_t total = rows * (size_t)ld_dst;
  hipStream_t st = static_cast<hipStream_t>(stream);
  clear_stale_error();
  const dim3 grid(grid_for(total)), block(256);
  if (src_bf16 && dst_bf16) hipLaunchKernelGGL((cast_rows_kernel<true, true>), grid, block, 0, st, src, dst, rows, cols, ld_src, ld_dst);
  else if (src_bf16) hipLaunchKernelGGL((cast_rows_kernel<true, false>), grid, block, 0, st, src, dst, rows, cols, ld_src, ld_dst);
  else if (dst_bf16) hipLaunchKernelGGL((cast_rows_kernel<false, true>), grid, block, 0, st, src, dst, rows, cols, ld_src, ld_dst);
  else hipLaunchKernelGGL((cast_rows_kernel<false, false>), grid, block, 0, st, src, dst, rows, cols, ld_src, ld_dst);
  return check_launch("cast_rows");
}

int a3d_copy_channel(size_t npix, const float* src, int ld_src, int c_src, float* dst, int ld_dst, int c_dst,
                     void* stream) {
  A3D_CHECK_ARG(npix > 0 && src && dst && c_src >= 0 && c_src < ld_src && c_dst >= 0 && c_dst < ld_dst,
                "copy_channel: bad arguments");
  clear_stale_error();
  hipLaunchKernelGGL(copy_channel_kernel<float>, dim3((unsigned)std::min<size_t>((npix + 255) / 256, 2048)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), src, dst, npix, ld_src, c_src, ld_dst, c_dst);
  return check_launch("copy_channel");
}

int a3d_copy_channel_bf16(size_t npix, const float* src, int ld_src, int c_src, void* dst, int ld_dst, int c_dst, void* stream) {
  A3D_CHECK_ARG(npix > 0 && src && dst && c_src >= 0 && c_src < ld_src && c_dst >= 0 && c_dst < ld_dst,
                "copy_channel_bf16: bad arguments");
  clear_stale_error();
  hipLaunchKernelGGL(copy_channel_kernel<__bf16>, dim3((unsigned)std::min<size_t>((npix + 255) / 256, 2048)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), src, static_cast<__bf16*>(dst), npix, ld_src, c_src, ld_dst, c_dst);
  return check_launch("copy_channel_bf16");
}

// ------------------------------------------------------------------ streams
int a3d_stream_create(int level, void** stream) {
  A3D_CHECK_ARG(stream != nullptr, "stream_create: null output");
  int least = 0, greatest = 0;                        // numerically: greatest priority <= least priority
  if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) return set_error(A3D_ELAUNCH, "stream_create: no priority range");
  const int prio = std::min(least, std::max(greatest, level));
  hipStream_t st = nullptr;
  if (hipStreamCreateWithPriority(&st, hipStreamNonBlocking, prio) != hipSuccess)
    return set_error(A3D_ELAUNCH, "stream_create: hipStreamCreateWithPriority failed");
  *stream = st;
  return A3D_OK;
}

int a3d_stream_destroy(void* stream) {
  A3D_CHECK_ARG(stream != nullptr, "stream_destroy: null stream");
  return hipStreamDestroy(static_cast<hipStream_t>(stream)) == hipSuccess ? A3D_OK : set_error(A3D_ELAUNCH, "stream_destroy failed");
}

}  // extern "C"

namespace a3d {
// ------------------------------------------------------------------ collective stand-in
// A measurement aid, not part of the training path: what a collective costs the kernels it runs beside.  Shaped like one rank's
// share of RCCL's reduce-scatter at N = 8 (src/ann3depth.py:77-92's replacement, dp.py): a few workgroups read `read_bytes`,
// add what they read, write `write_bytes`, and pace themselves to `bytes_per_tick` (s_memrealtime runs at 100 MHz) so that the
// launch lasts as long as the exchange would over xGMI.  bench.py --dp-rank-standin launches it on a second stream wherever a
// data-parallel rank would start a collective.
__global__ __launch_bounds__(256) void comm_standin_kernel(const float* __restrict__ src, size_t read_f4, float* __restrict__ dst,
                                                           size_t write_f4, float f4_per_tick) {
  typedef float f4 __attribute__((ext_vector_type(4)));
  const f4* s4 = reinterpret_cast<const f4*>(src);
  f4* d4 = reinterpret_cast<f4*>(dst);
  const size_t per = (read_f4 + gridDim.x - 1) / gridDim.x, lo = (size_t)blockIdx.x * per, hi = min(read_f4, lo + per);
  const size_t wper = (write_f4 + gridDim.x - 1) / gridDim.x, wlo = (size_t)blockIdx.x * wper, whi = min(write_f4, wlo + wper);
  // a block past the end of what is written (few pieces, many blocks) has wlo > write_f4: its share is empty, not whi - wlo.
  // (Its read share can be empty the same way, hi < lo; then the loop below does not run and nothing is computed from it.)
  const size_t wcnt = whi > wlo ? whi - wlo : 0;
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  constexpr int U = 8;                                  // 8 x 256 x 16 B = 32 KiB per block and round
  f4 acc = {0.f, 0.f, 0.f, 0.f};
  size_t wpos = wlo + threadIdx.x;
  for (size_t i = lo; i < hi; i += 256 * U) {
    f4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t e = i + u * 256 + threadIdx.x;
      v[u] = e < hi ? __builtin_nontemporal_load(s4 + e) : f4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int u = 0; u < U; ++u) acc += v[u];
    // writes keep pace with the reads: after reading a fraction f of its share a block has written the same fraction of what
    // it has to write (reduce-scatter: one piece per eight read; all-reduce stand-in, write_f4 == read_f4: eight per eight)
    const size_t wdue = wlo + (size_t)((double)(min(hi, i + 256 * U) - lo) * (double)wcnt / (double)(hi - lo));
    while (wpos < wdue) {
      __builtin_nontemporal_store(acc, d4 + wpos);
      wpos += 256;
    }
    // pace: this block's share of the rate
    const float due = (float)(i - lo + 256 * U) * (float)gridDim.x / f4_per_tick;
    while ((float)(__builtin_amdgcn_s_memrealtime() - t0) < due) __builtin_amdgcn_s_sleep(8);
  }
}
}  // namespace a3d

extern "C" {

int a3d_comm_standin(const float* src, size_t read_bytes, float* dst, size_t write_bytes, int workgroups, float gbytes_per_s,
                     void* stream) {
  A3D_CHECK_ARG(src && dst && read_bytes >= 16 && write_bytes >= 16 && workgroups >= 1 && workgroups <= 256 && gbytes_per_s > 0.f &&
                    ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0,
                "comm_standin: bad arguments");
  // bytes per 10-ns tick of s_memrealtime: both directions count against the rate
  const float f4_per_tick = gbytes_per_s * 10.f / 16.f * ((float)read_bytes / (float)(read_bytes + write_bytes));
  clear_stale_error();
  hipLaunchKernelGGL(comm_standin_kernel, dim3(workgroups), dim3(256), 0, static_cast<hipStream_t>(stream), src, read_bytes / 16,
                     dst, write_bytes / 16, f4_per_tick);
  return check_launch("comm_standin");
}

}  // extern "C"
