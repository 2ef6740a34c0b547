/* a3d_gradloss.h — extension of the C ABI of liba3d.so (include/a3d.h): the scale-invariant log loss with the gradient-matching
 * term of Eigen & Fergus 2015 (eq. 4), fused into the loss launches.
 *
 * The entry points here have no counterpart in the reference (NON-REFERENCE, --loss-gradient) and keep a prefix of their own,
 * a3dg_: the same library, the same conventions as include/a3d_valid.h (caller-owned device tensors, stream-ordered launches,
 * 0 or a negative A3D_E* code with a3d_last_error()), bound by _lib.py GRADLOSS_SIGNATURES.
 *
 * out / tgt [b, h, w].  Per sample, npix = h w and d_i = masked_log(o_i) - masked_log(t_i), masked_log(v) = log(v + 1e-8) with
 * NaN -> 0 and -inf kept, exactly as in a3d_silog_loss_fwd.
 *   masked = 0: every pixel counts.     masked = 1: a pixel counts iff its target is finite (a3dx_silog_masked_loss_fwd's rule).
 *   A pair is a pixel with its right neighbour in the same row or with the pixel below it; no pair spans the end of a row; a
 *   pair counts iff both of its pixels count.  M = h (w - 1) + (h - 1) w is the number of pairs of the grid.
 *   Over the counting pixels: n their number, s2 = sum d^2, s1 = sum d.  Over the counting pairs: m their number,
 *   sg = sum (d_j - d_i)^2.
 *   silog part:    masked = 0: s2 - c s1^2 with the reference's folded constant c = (float)(0.5 / 4070), whatever npix is;
 *                  masked = 1: r_n (s2 - c_n s1^2), c_n = (float)(0.5 / n), r_n = (float)((double)npix / n), 0 when n = 0
 *   gradient part: r_m sg, r_m = 1 when masked = 0, r_m = (float)((double)M / m) when masked = 1 and 0 when m = 0: holes do not
 *                  shrink the term, as r_n keeps the silog part at full-image magnitude
 *   loss[2] = mean over the batch of the silog parts       loss[3] = mean over the batch of the gradient parts
 *   loss[0] = fl(loss[2] + fl(grad_weight loss[3]))        loss[1] = sum n / (b npix), 1.0f when masked = 0
 *   grad_weight == 0: the gradient part is left out, not multiplied: loss[0] = loss[2] even where sg is not finite (loss[3] is
 *   written all the same).
 * The sums s2, s1 and n keep the partition and the order of a3d_silog_loss_fwd / a3dx_silog_masked_loss_fwd (A3D_SILOG_PARTS
 * parts per sample, the same chunk, the same thread-to-pixel mapping, the last block adds the parts): loss[2] is bit-identical
 * to a3d_silog_loss_fwd (masked = 0) and to a3dx_silog_masked_loss_fwd (masked = 1) on the same [b, h w] tensors at any shape.
 * No floating-point atomics: the same inputs give the same bits on every run.
 *
 * Backward.  g_i = 0 where log(o_i + 1e-8) is NaN or the pixel does not count (a counting pair still pulls on its other pixel).
 * Elsewhere, with inv_b = 1.0f / (float)b, arg = fl(o_i + 1e-8) and every operation below rounded to float32 on its own:
 *   a   = fl(fl(2 d_i) - fl(fl(2 c) s1))                                (c_n for c when masked = 1)
 *   a   = fl(a inv_b)                       masked = 0
 *   a   = fl(fl(a inv_b) r_n)               masked = 1
 *   grad_weight == 0:   g_i = fl(a / arg)   — the sequence of a3d_silog_loss_bwd_ex / a3dx_silog_masked_loss_bwd_ex, bit for bit
 *   grad_weight != 0:   L   = (((0 + [d_i - d_left]) + [d_i - d_right]) + [d_i - d_up]) + [d_i - d_down], each bracket one
 *                             subtraction, a neighbour that does not exist or does not count left out
 *                       q   = fl(fl(fl(2 fl(grad_weight r_m)) L) inv_b)
 *                       g_i = fl(fl(a + q) / arg)
 * dout_bf16 / ld_bf16 as in a3d_silog_loss_bwd_ex.
 *
 * loss: 4 floats.  ws: A3DG_WS_FLOATS(b) floats, [0] the ticket under the rules of A3D_SILOG_WS_FLOATS (zero before the first
 * call, zero again after every call, one workspace serves every batch size up to b), then s2, s1, n, sg, m per sample, then
 * the partial sums.  n and m are whole numbers kept in floats (exact up to 2^24; a pair count above that is the nearest float,
 * and forward and backward both take r_m from that float).
 * A3D_EINVAL before any launch: a NULL pointer (dout_bf16 may be NULL); b, h or w <= 0; h w > 2^24; w > A3DG_MAX_W (the
 * forward keeps a part's window of 1024 + w values of d in LDS, the backward at least three rows); a NaN or negative
 * grad_weight; ld_bf16 < h w with a non-NULL dout_bf16. */
#ifndef A3D_GRADLOSS_H_
#define A3D_GRADLOSS_H_

#include "a3d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define A3DG_MAX_W 2048
#define A3DG_WS_FLOATS(b) ((b) * 5 + 1 + (b) * 5 * A3D_SILOG_PARTS)
int a3dg_silog_grad_loss_fwd(int b, int h, int w, const float* out, const float* tgt, int masked, float grad_weight,
                             float* loss /*4*/, float* ws, void* stream);
int a3dg_silog_grad_loss_bwd_ex(int b, int h, int w, const float* out, const float* tgt, int masked, float grad_weight,
                                const float* ws, float* dout, void* dout_bf16, int ld_bf16, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* A3D_GRADLOSS_H_ */
