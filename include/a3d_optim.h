/* a3d_optim.h — extension of the C ABI of liba3d.so (include/a3d.h): SGD with momentum for MSDN.
 *
 * include/a3d.h is the fixed surface that stands in for the reference's TensorFlow ops; its optimizer is ApplyAdam
 * (a3d_adam_apply_tf1), which the reference builds with beta2 = 1 so that no weight ever moves.  The per-group rates the
 * reference passes (Eigen et al. 2014: 0.001 / 0.1 / 0.001 / 0.01) were published for SGD with momentum 0.9.  The entry
 * points here have no counterpart in the reference (NON-REFERENCE, --optimizer momentum): they are TensorFlow 1.3's
 * MomentumOptimizer(rate, momentum) without Nesterov (ApplyMomentum).  They keep a prefix of their own, a3do_: the same
 * library, the same conventions (caller-owned device tensors, stream-ordered launches, 0 or a negative A3D_E* code with
 * a3d_last_error()), bound by _lib.py OPTIM_SIGNATURES.
 *
 * The rule, per element, every operation rounded to float32 on its own (no fused multiply-add):
 *   g'     = grad_scale == 1 ? g : g * grad_scale
 *   accum' = accum * momentum + g'
 *   var'   = var - lr * accum'
 * Nothing is special-cased: NaN, infinities, momentum = 0 and lr = 0 come out as this arithmetic decides. */
#ifndef A3D_OPTIM_H_
#define A3D_OPTIM_H_

#include "a3d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The rule above on count elements of var, accum (both updated in place) and g.  One streaming pass in 16-byte pieces,
 * the count % 4 elements behind them one by one.  A3D_EINVAL before any launch for a NULL pointer, count == 0, or a
 * buffer that does not start on a 16-byte boundary. */
int a3do_momentum_apply(size_t count, float* var, float* accum, const float* g, float lr, float momentum,
                        float grad_scale, void* stream);

/* The filter gradient dw[k][n] = sum_m x[m][k] dz[m][n] and the bias gradient db[n] = sum_m dz[m][n] of a dense layer,
 * and the rule above on var_w / accum_w [k][n] and var_b / accum_b [n], in one launch; the gradient is never written.
 * The two-call equivalence: for every accepted shape the results in var_* and accum_* are, bit for bit, those of
 * a3d_dense_bwd_filter into a scratch gradient followed by a3do_momentum_apply on the kernel and on the bias (the same
 * fp32 MFMA 32x32x2 contraction over the batch in ascending order, the same BiasAddGrad walk; below k n = 2^16, where
 * a3d_dense_bwd_filter hands the layer to the implicit-GEMM route, the batch rows are fed in that route's order instead,
 * rows 8u + j and 8u + 4 + j per instruction).  Accepted: 1 <= m <= 64;
 * a larger batch is refused with A3D_EINVAL and a message naming the two-call form.  var_b and accum_b come as a pair or
 * are both NULL (no bias update).  x [m][k], dz [m][n]; the tensors need 4-byte alignment only. */
int a3do_dense_bwd_filter_momentum(int m, int k, int n, const float* x, const float* dz, float* var_w, float* accum_w,
                                   float* var_b, float* accum_b, float lr, float momentum, float grad_scale,
                                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* A3D_OPTIM_H_ */
