/* a3d_ssi.h — extension of the C ABI of liba3d.so (include/a3d.h): the least-squares scale-and-shift-invariant loss of
 * Ranftl et al. 2020 (MiDaS, L_ssimse) on LINEAR depth.  The depth maps the models train on are min-max scaled per image
 * (tools/data_preprocessor.py), so a checkpoint is judged after a per-image least-squares scale and shift
 * (include/a3d_align.h, --align affine); this is the training objective that matches that protocol: the loss of a sample is
 * what remains of its squared error after the best scale s and shift t have been applied to its OUTPUT.
 *
 * The entry points here have no counterpart in the reference (NON-REFERENCE, --loss ssi) and keep a prefix of their own,
 * a3di_: the same library, the same conventions as include/a3d_berhu.h (caller-owned device tensors, stream-ordered
 * launches, 0 or a negative A3D_E* code with a3d_last_error(), every refusal before any launch), bound by _lib.py
 * SSI_SIGNATURES.
 *
 * out / tgt [b, npix] float32; o and d are a pixel's output and target.  Per sample:
 *   masked = 0: every pixel counts.     masked = 1: a pixel counts iff its target is finite (a3dh_berhu_loss_fwd's rule).
 *   n the number of counting pixels.
 *   A sample is POISONED iff a counting o is not finite or, with masked = 0, a target is not finite.
 *
 * THE FIT, in float64.  S_o, S_d, S_oo, S_od are float64 sums over the counting pixels; each term of S_oo and S_od is the
 * exact float64 product of the two float32 values (what A3DA_AFFINE does).  With every operation rounded to float64 on its
 * own, in the order written:
 *   den = S_oo - (S_o S_o) / n        num = S_od - (S_o S_d) / n
 *   s64 = num / den                   t64 = (S_d - s64 S_o) / n          s = (float)s64, t = (float)t64
 *   A sample is FITTED iff n >= 2 and den > 2^-30 S_oo and s and t are finite.  The floor is a definition, not a
 *   measurement: it calls an output whose relative spread over the sample is below 2^-15 (512 float32 ulps) constant, and it
 *   lies about 2^10 above the worst rounding error den can carry (the longest chain of float64 additions below is about
 *   2^13 at the largest npix, so that error is <= 2^-40 S_oo).
 *   Otherwise the sample is DEGENERATE: s = +0.0, t = (float)(S_d / n) when n >= 1 and t = +0.0 when n = 0.
 *   A poisoned sample is neither: its s and t are NaN.
 *
 * THE LOSS.  Every operation is rounded to float32 on its own (no FMA).  Per counting pixel
 *   q = fl(fl(s o) + t)               (a3da_affine_apply's form)
 *   r = fl(q - d)
 *   S = sum fl(r r)
 *   h = 0.5f when masked = 0, h = (float)(0.5 npix / n) when masked = 1: holes do not shrink the loss, as in the masked silog
 *   and berHu losses.  per = fl(h S); n == 0: per = +0.0.  A sum over the pixels and a mean over the batch, like silog and
 *   berHu, so the reference's learning rates see gradients of the magnitude they were chosen for.
 *   loss[0] = (sum per) / (float)b      loss[2] = (sum s) / (float)b      loss[3] = (sum t) / (float)b
 *     each sum adds the samples in ascending order, starting from 0.0f
 *   loss[1] = (float)(sum n / ((double)b npix)), 1.0f when masked = 0
 *   A poisoned sample's s, t and per are NaN, and with them loss[0], loss[2] and loss[3]; no other sample changes.
 *
 * THE GRADIENT.  s and t minimise the sum, so dL/ds = dL/dt = 0 and the total derivative with respect to o_i is the partial
 * one: nothing is differentiated through the fit, and no assumption is hidden (tests/test_ssi_cpu.py holds the closed form
 * to autograd through an explicit least-squares solve).  With r_n = 1 when masked = 0, r_n = (float)((double)npix / n) when
 * masked = 1, and k = fl((1.0f / (float)b) r_n):
 *   g = fl(fl(s r) k)    at a counting pixel of a fitted sample, r recomputed exactly as in the forward
 *   g = +0.0             at a pixel that does not count, and on every pixel of a degenerate sample
 *   g = NaN              on every pixel of a poisoned sample
 * dout_bf16 / ld_bf16 as in a3dh_berhu_loss_bwd_ex: the same gradient rounded once to bf16 in rows of pitch ld_bf16 >= npix,
 * columns npix .. ld_bf16 never written.
 *
 * Launches and the order of every sum.  Forward: two launches of b A3D_SILOG_PARTS workgroups of 256 threads, with
 * a3dh_berhu_loss_fwd's partition and thread-to-pixel mapping: chunk = ceil(npix / A3D_SILOG_PARTS) rounded up to a
 * multiple of 4; workgroup (sample, part) owns the pixels [part chunk, min(npix, (part + 1) chunk)); thread t takes, round
 * after round (r = 0, 1, ...), the four pixels part chunk + 1024 r + 4 t + {0, 1, 2, 3} that lie in the chunk, and adds
 * those that count to its accumulators (initially 0) in ascending pixel order.  The 64 accumulators of a wavefront are
 * added as a tree, v[l] += v[l + off] for off = 32, 16, 8, 4, 2, 1; the four wavefronts' sums as ((w0 + w1) + w2) + w3; the
 * last workgroup to arrive (an integer ticket, ws[0]) adds a sample's parts in ascending order starting from 0.
 *   1. the four float64 sums, n and the poison flag; the last workgroup solves and writes s, t, n and the flag;
 *   2. S in float32; the last workgroup writes per and the four loss floats.
 * n is a whole number below 2^24 kept in a float, exact in any order.  The same mapping holds whether the four pixels are
 * read as one 16-byte load or one by one.  Backward: one launch over 16-byte groups of the flat tensors where the three
 * base addresses allow, one element at a time otherwise; it reads s, t, n and the flag from ws.
 * No workgroup waits for another, and there are no floating-point atomics: the same inputs give the same bits on every run.
 *
 * loss: 4 floats.  ws: A3DI_WS_FLOATS(b) floats on an 8-byte address.  [0] the ticket under the rules of A3D_SILOG_WS_FLOATS
 * (zero before the first call, zero again after every call — after each of the two forward launches —, one workspace
 * serves every batch size up to b), [1] unused; then four words per sample i at [2 + 4 i ..]: s, t, n and the flag,
 * 0.0f fitted, 1.0f degenerate, 2.0f poisoned; then, from the even offset 2 + 4 b of the CALL's b, the partial values of
 * the parts, ten words per workgroup in the first launch (four float64 sums at even offsets, n, the poison mark), one in
 * the second.
 * A3D_EINVAL before any launch, each with words of its own: a NULL pointer (dout_bf16 may be NULL); b or npix <= 0;
 * npix > 2^24; masked outside {0, 1}; ld_bf16 < npix with a non-NULL dout_bf16; a ws that is not on an 8-byte address. */
#ifndef A3D_SSI_H_
#define A3D_SSI_H_

#include "a3d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define A3DI_WS_FLOATS(b) ((b) * 4 + 2 + (b) * 10 * A3D_SILOG_PARTS)
int a3di_ssi_loss_fwd(int b, int npix, const float* out, const float* tgt, int masked, float* loss /*4*/, float* ws,
                      void* stream);
int a3di_ssi_loss_bwd_ex(int b, int npix, const float* out, const float* tgt, int masked, const float* ws, float* dout,
                         void* dout_bf16, int ld_bf16, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* A3D_SSI_H_ */
