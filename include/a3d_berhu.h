/* a3d_berhu.h — extension of the C ABI of liba3d.so (include/a3d.h): the reverse Huber (berHu) loss of Laina et al. 2016 on
 * LINEAR depth, an objective that is finite and differentiable at every real output, where the scale-invariant log loss gives
 * an output at or below zero no gradient at all (include/a3d_gradloss.h: "g_i = 0 where log(o_i + 1e-8) is NaN").
 *
 * The entry points here have no counterpart in the reference (NON-REFERENCE, --loss berhu) and keep a prefix of their own,
 * a3dh_: the same library, the same conventions as include/a3d_gradloss.h (caller-owned device tensors, stream-ordered
 * launches, 0 or a negative A3D_E* code with a3d_last_error(), every refusal before any launch), bound by _lib.py
 * BERHU_SIGNATURES.
 *
 * out / tgt [b, npix] float32.  Every operation below is rounded to float32 on its own (no FMA).  Per sample:
 *   masked = 0: every pixel counts.     masked = 1: a pixel counts iff its target is finite (a3dx_silog_masked_loss_fwd's rule).
 *   n the number of counting pixels.  e = fl(o - t), a = |e|, m = max a over the counting pixels, c = fl(fraction m).
 *   The threshold c is PER SAMPLE, not per batch as in Laina et al.: a sample's loss and gradient do not depend on which
 *   other samples share its batch, so two data-parallel ranks of 32 remain one batch of 64.  c is a constant of the gradient:
 *   nothing is differentiated through the max.
 *   A counting pixel is linear iff a <= c or c == 0, otherwise quadratic.
 *     rho = a                                               (linear)
 *     rho = fl(fl(fl(a a) + fl(c c)) / fl(2 c))             (quadratic)
 *   S = sum rho over the counting pixels, nq the number of quadratic ones.
 *   r_n = 1 when masked = 0, r_n = (float)((double)npix / n) when masked = 1: holes do not shrink the loss, as in the masked
 *   silog loss.  per = fl(r_n S).  n == 0: per = +0.0, c = +0.0 and the sample's gradient row is +0.0.
 *   A sample is POISONED iff some counting a is not finite (a NaN or infinite output; with masked = 0 also a target that is
 *   not finite): its per and c are NaN and every element of its gradient row is NaN; no other sample's row changes;
 *   loss[0], loss[2] and loss[3] are NaN.
 *   loss[0] = (sum per) / (float)b      the samples added in ascending order, starting from 0.0f
 *   loss[1] = (float)(sum n / ((double)b npix)), 1.0f when masked = 0
 *   loss[2] = (sum c) / (float)b        the samples added in ascending order, starting from 0.0f
 *   loss[3] = (float)((double)sum nq / (double)sum n), +0.0 when sum n == 0
 *
 * Launches and the order of every sum.  Forward: two launches of b A3D_SILOG_PARTS workgroups of 256 threads, the maxima
 * first (the threshold exists before any rho does), then the sums.  chunk = ceil(npix / A3D_SILOG_PARTS) rounded up to a
 * multiple of 4; workgroup (sample, part) owns the pixels [part chunk, min(npix, (part + 1) chunk)).  Thread t takes, round
 * after round (r = 0, 1, ...), the four pixels part chunk + 1024 r + 4 t + {0, 1, 2, 3} that lie in the chunk, and adds rho
 * of those that count to ONE accumulator (initially 0.0f) in ascending pixel order.  The 64 accumulators of a wavefront are
 * added as a tree, v[l] += v[l + off] for off = 32, 16, 8, 4, 2, 1; the four wavefronts' sums as ((w0 + w1) + w2) + w3; the
 * last workgroup to arrive (an integer ticket, ws[0]) adds a sample's parts in ascending order starting from 0.0f.  The
 * same thread-to-pixel mapping holds whether the four pixels are read as one 16-byte load (rows that start on a 16-byte
 * address) or one by one.  n and nq are whole numbers below 2^24 kept in floats, exact in any order; a maximum has no order.
 * No workgroup waits for another, and there are no floating-point atomics: the same inputs give the same bits on every run.
 *
 * Backward: one launch, which reads c, n and the poison flag from ws.  With s = fl((1.0f / (float)b) r_n):
 *   g = +0.0 at a pixel that does not count, and where e == 0
 *   g = copysign(s, e)                  (linear)
 *   g = fl(fl(e / c) s)                 (quadratic)
 * dout_bf16 / ld_bf16 as in a3d_silog_loss_bwd_ex: the same gradient rounded once to bf16 in rows of pitch ld_bf16 >= npix,
 * columns npix .. ld_bf16 never written.
 *
 * loss: 4 floats.  ws: A3DH_WS_FLOATS(b) floats, [0] the ticket under the rules of A3D_SILOG_WS_FLOATS (zero before the first
 * call, zero again after every call — after each of the two forward launches —, one workspace serves every batch size up
 * to b), then c, n and the poison flag (0.0f or 1.0f) per sample, then the partial values of the parts.
 * A3D_EINVAL before any launch, each with words of its own: a NULL pointer (dout_bf16 may be NULL); b or npix <= 0;
 * npix > 2^24; masked outside {0, 1}; fraction NaN, <= 0 or > 1; ld_bf16 < npix with a non-NULL dout_bf16. */
#ifndef A3D_BERHU_H_
#define A3D_BERHU_H_

#include "a3d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define A3DH_WS_FLOATS(b) ((b) * 3 + 1 + (b) * 3 * A3D_SILOG_PARTS)
int a3dh_berhu_loss_fwd(int b, int npix, const float* out, const float* tgt, int masked, float fraction, float* loss /*4*/,
                        float* ws, void* stream);
int a3dh_berhu_loss_bwd_ex(int b, int npix, const float* out, const float* tgt, int masked, float fraction, const float* ws,
                           float* dout, void* dout_bf16, int ld_bf16, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* A3D_BERHU_H_ */
