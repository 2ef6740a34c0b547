/* a3d_clip.h — extension of the C ABI of liba3d.so (include/a3d.h): gradient clipping by global norm, per optimizer group.
 *
 * The entry points here have no counterpart in the reference (NON-REFERENCE, --clip-norm): they bound the gradient of ONE
 * optimizer group (one flat buffer, one rate) by its global norm, as tf.clip_by_global_norm does over one optimizer's
 * compute_gradients list, and skip a step whose gradient is not finite.  They keep a prefix of their own, a3dn_: the same
 * library, the same conventions (caller-owned device tensors, stream-ordered launches, 0 or a negative A3D_E* code with
 * a3d_last_error(); every refusal comes before any launch, with words of its own), bound by _lib.py CLIP_SIGNATURES.
 *
 * The definition, for a group with flat gradient g[0..count), the host's grad_scale gs (1 / world size) and clip norm C
 * (C > 0; C = +inf measures and skips, never clips):
 *   S = sum of (double)g[i] * (double)g[i] in float64 (each term is exact: 24-bit significands)
 *   n = |gs| * sqrt(S) in float64
 *   the step is skipped iff S is not finite, that is iff some element is NaN or +-inf (2^27 squares of finite float32
 *     values cannot overflow float64): scale = 0, skip = 1, skipped += 1
 *   otherwise skip = 0, and scale = (float)((double)gs * C / n), rounded once, if n > C; scale = gs, the same bits, if n <= C
 *   norm, as reported, is (float)n: it may be +inf while n is finite, and that is not a skip
 * The optimizer launch that follows reads skip and scale from the device.  On skip it writes nothing: not var, not a slot,
 * not poisoned.  Otherwise it runs its existing rule with grad_scale = scale, the rule "scale == 1 multiplies nothing"
 * included, so C = +inf on one GPU leaves the bits of an unclipped step.
 *
 * Host bookkeeping that cannot know about a skip without a synchronisation advances as on any step: Adam's beta powers
 * and global_step move on a skipped step too.
 *
 * The control block: 32 bytes of device memory on an 8-byte boundary, one per group, zeroed once by the caller.
 *   offset 0   double    sumsq     S
 *   offset 8   float     norm      (float)n
 *   offset 12  float     scale
 *   offset 16  uint32    skip      0 / 1
 *   offset 20  uint32    skipped   running count, only ever incremented by the norm launch
 *   offset 24  8 bytes   reserved, never written */
#ifndef A3D_CLIP_H_
#define A3D_CLIP_H_

#include "a3d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define A3DN_CTL_BYTES 32
#define A3DN_BLOCK_ELEMS 4096 /* floats one block of the norm launch takes before a second block is started */
#define A3DN_MAX_BLOCKS 1024  /* the grid's cap: from A3DN_MAX_BLOCKS * A3DN_BLOCK_ELEMS floats on, blocks take more each */

/* Bytes of workspace a3dn_grad_norm_scale needs for `count` elements: the arrival ticket and one float64 per block.  The
 * caller zeroes the workspace once, at allocation; every launch leaves the ticket at 0 again, and one workspace serves
 * calls of different counts (it must hold the largest). */
size_t a3dn_grad_norm_ws_bytes(size_t count);

/* One launch: S, n, scale and skip of g[0..count) as defined above into ctl words 0..16, and skipped += 1 on a skip.
 * 256-thread blocks, min(A3DN_MAX_BLOCKS, ceil(count / 4 / 1024)) of them; each walks a contiguous range of 16-byte vectors
 * with four float64 accumulators per thread, added in ascending address order; the count % 4 tail is taken by the last
 * block.  Within a block: a fixed shuffle tree per wavefront, then ((w0 + w1) + w2) + w3.  Each block's partial is one 8-byte
 * agent-scope store; the block that arrives last learns it from the ticket's returned value and adds the partials in a
 * fixed order of its own (thread t takes blocks 4t .. 4t + 3 in ascending order, then the same tree as above).  No
 * floating-point atomics, no block waits for another, no trip count depends on a value: the same bits on every run.
 * g is read with ordinary (temporal) loads.
 * A3D_EINVAL before any launch for a NULL pointer, count == 0, g off the 16-byte grid, ctl or ws off the 8-byte grid,
 * a grad_scale that is not finite or is 0, a clip_norm that is NaN or <= 0; A3D_EWORKSPACE for too little workspace. */
int a3dn_grad_norm_scale(size_t count, const float* g, float grad_scale, float clip_norm, void* ctl, void* ws,
                         size_t ws_bytes, void* stream);

/* The four existing rules with grad_scale replaced by the control block a3dn_grad_norm_scale left on the same stream.
 * Each reads skip and scale from the device.  On skip it returns without a store.  Otherwise it is bit for bit the
 * existing entry point called with grad_scale = scale: a3do_momentum_apply (include/a3d_optim.h) and
 * a3d_adam_apply_tf1_flag (include/a3d.h; the general and the frozen kernel, by the same dispatch on the host scalars).
 * Gradient descent has no grad_scale: a3d_sgd_apply and a3dp_sgd_apply_floor (include/a3d_pairwise.h) are matched
 * with lr = fl32(lr * scale), one float32 product formed on the device.  The same refusals as the existing entry points,
 * and A3D_EINVAL for a NULL ctl or one off the 8-byte grid. */
int a3dn_momentum_apply_ctl(size_t count, float* var, float* accum, const float* g, float lr, float momentum,
                            const void* ctl, void* stream);
int a3dn_adam_apply_tf1_ctl(size_t count, float* var, float* m, float* v, const float* g, float lr, float beta1,
                            float beta2, float eps, float beta1_power, float beta2_power, const void* ctl,
                            unsigned int* poisoned, void* stream);
int a3dn_sgd_apply_ctl(size_t count, float* var, const float* g, float lr, const void* ctl, void* stream);
int a3dn_sgd_apply_floor_ctl(size_t count, float* var, const float* g, float lr, float floor, const void* ctl,
                             void* stream);

#ifdef __cplusplus
}
#endif
#endif /* A3D_CLIP_H_ */
