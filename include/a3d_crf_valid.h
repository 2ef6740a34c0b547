/* a3d_crf_valid.h — extension of the C ABI of liba3d.so (include/a3d.h) for training DCNF on depth maps with holes.
 *
 * include/a3d.h is the fixed surface that stands in for the reference's TensorFlow ops.  The entry points here have no
 * counterpart in the reference (NON-REFERENCE, --model dcnf with --min-depth / --max-depth) and keep a prefix of their own,
 * a3dv_: the same library, the same conventions (caller-owned device tensors, stream-ordered launches, 0 or a negative
 * A3D_E* code with a3d_last_error()), bound by _lib.py CRF_VALID_SIGNATURES.  a3dx_resize_bilinear_tf1_valid
 * (include/a3d_valid.h) writes NaN where the depth map has no measurement; these two launches take it from there: the mean
 * depth of a superpixel over its measured pixels only, and the CRF's likelihood of the superpixels that have such a mean.
 *
 * The model (Liu et al. 2015) is a Gaussian field over the superpixels: with A = I + D - R from the pair weights, the energy
 * y^T A y - 2 z^T y + z^T z makes y ~ N(mu, A^-1 / 2), mu = A^-1 z.  A superpixel without a target is a variable that is
 * integrated out, not a masked term: the objective is the negative log-likelihood of the observed superpixels alone. */
#ifndef A3D_CRF_VALID_H_
#define A3D_CRF_VALID_H_

#include "a3d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* a3d_superpixel_mean for a one-channel map with holes: x [n,h,w,1] float32 -> y [n,(h/sp)*(w/sp)] float32 and, unless NULL,
 * count [n,(h/sp)*(w/sp)] int32.  A pixel counts iff it is finite (NaN, +inf and -inf are holes).  Per sp x sp block, c is the
 * number of pixels that count (written to count) and
 *   y = (sum of the pixels that count) / (float)c   if c >= max(1, min_count),   NaN otherwise.
 * The sum keeps a3d_superpixel_mean's order (256 threads stride the block, then the block's tree), a hole adding nothing:
 * with every pixel finite y is a3d_superpixel_mean's bits.  One launch.  n <= 0, sp <= 0, h or w no positive multiple of sp,
 * min_count < 0, a NULL x or y: A3D_EINVAL before any launch. */
int a3dv_superpixel_mean_valid(int n, int h, int w, const float* x, int sp, int min_count, float* y, int32_t* count,
                               void* stream);

/* The negative log-likelihood of the observed superpixels under the field, and its gradients.  z, y [n,nsp], r [n,npairs],
 * left, right [npairs] as a3d_crf_loss: A = I + D - R per image, the pairs scattered in order (the last writer owns a cell).
 * O = the superpixels whose y is finite, m = |O|, M the others; P selects the rows of O.  With C = P A^-1 P^T and
 * e = y_O - mu_O:
 *   L = e^T C^-1 e + 1/2 log det C + (m / 2) log pi                                   (no epsilon, no exp)
 * loss_per_image[b] = L_b, loss_mean[0] = sum_b L_b / n (no rescaling by m: it is a likelihood), nobs[b] = m (int32 [n]).
 * dz [n,nsp] and, unless NULL, dr [n,npairs] are the gradients of loss_mean, A NOT held constant.  With u = C^-1 e,
 * q = A^-1 P^T u and, for pair k = (l, r), v = e_l - e_r, t = P A^-1 v:
 *   dL/dz = -2 q        dL/dr_k = 2 (v^T q)(v^T mu) + (v^T q)^2 - 1/2 t^T C^-1 t
 *
 * How it is computed.  C^-1 is the Schur complement A_OO - A_OM A_MM^-1 A_MO, and A^-1 P^T C^-1 P A^-1 = A^-1 - [A_MM^-1]
 * (A_MM^-1 padded with zeros to nsp x nsp).  Hence q_O = e, q_M = yhat_M - mu_M with yhat_M = A_MM^-1 (z_M - A_MO y_O) the
 * field's conditional mean of the missing superpixels, e^T C^-1 e = q^T A q, det C = det A_MM / det A and
 * t^T C^-1 t = S_k(A^-1) - S_k([A_MM^-1]) with S_k(X) = X[l][l] + X[r][r] - X[l][r] - X[r][l].  One wavefront per image runs
 * two eliminations one after the other in the same LDS tile: [A | z | I], then [A_MM | z_M - A_MO y_O | I] (the identity
 * columns only when dr is wanted); log det is the sum of the logs of the pivots.  nsp <= 64.
 *
 * Pivot rule: the loss kernels' (the largest |U[i][k]| of column k wins, the lowest row wins a tie; a NaN is taken at
 * once).  An image is accepted iff every pivot of both eliminations, after its exchange, is finite and > 0 and each
 * elimination exchanged rows an even number of times.  Every symmetric positive definite A that eliminates without an
 * exchange passes (all diagonally dominant ones, so all r >= 0); no image with det A <= 0 or det A_MM <= 0 passes.
 *
 * Edges:
 *   a pair index outside [0,nsp): loss, dz and dr NaN and status 1 for EVERY image (the lists are the batch's), nobs as
 *     counted; the index is skipped, never used;
 *   m = 0 (and no bad index): loss +0.0, the image's rows of dz and dr +0.0, status 0;
 *   A or C not positive (an image that is not accepted, above; a non-finite z or r among them): the image's loss and its
 *     rows of dz and dr NaN, status 1; no other image is touched, loss_mean is NaN;
 *   a pair whose two cells a later pair overwrote: dr +0.0;      a pair of a superpixel with itself: dr 0.
 * The values in the unobserved entries of y (NaN payloads, infinities) change no output bit.  dr = NULL changes no other
 * output bit.  While it runs the kernel parks per-pair intermediates in dr: dr must not alias an input.
 * The same bits on every run.  Two launches (the images, the mean).
 * n <= 0, nsp outside 1 .. 64, npairs <= 0, a NULL pointer other than dr: A3D_EINVAL before any launch. */
int a3dv_crf_loss_observed(int n, int nsp, const float* z, const float* y, const float* r, const int32_t* left,
                           const int32_t* right, int npairs, float* loss_per_image, float* loss_mean, float* dz, float* dr,
                           int32_t* nobs, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* A3D_CRF_VALID_H_ */
