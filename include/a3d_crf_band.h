/* a3d_crf_band.h — extension of the C ABI of liba3d.so (include/a3d.h): DCNF's CRF on fine superpixel grids.
 *
 * include/a3d.h is the fixed surface that stands in for the reference's TensorFlow ops.  The entry points here have no
 * counterpart in the reference (NON-REFERENCE, --model dcnf --unary fcsp --superpixel 20 / 10) and keep a prefix of their
 * own, a3db_: the same library, the same conventions (caller-owned device tensors, stream-ordered launches, 0 or a negative
 * A3D_E* code with a3d_last_error()), bound by _lib.py CRF_BAND_SIGNATURES.
 *
 * The kernels of a3d_crf_loss, a3dp_crf_loss_grad, a3d_crf_map and a3dv_crf_loss_observed eliminate a dense [A | z | I] in
 * LDS with one lane per row and stop at 64 superpixels; the reference's objective multiplies by pi^(nsp/2), which has no
 * float32 value from nsp = 156.  With the superpixels of a rows x cols grid numbered row-major every pair (l, r) of
 * A = I + D - R has |l - r| <= cols: A is banded.  These launches factor A = L D L^T in band storage without pivoting,
 * nsp x (band + 1) floats, and take the entries of A^-1 inside the band from the factor by the Takahashi recurrence, in
 * place.  The objective is the one include/a3d_crf_valid.h defines, every superpixel observed:
 *   L = e^T A e - 1/2 log det A + (nsp / 2) log pi,   e = y - mu,   mu = A^-1 z             (no epsilon, no exp)
 * which is finite at every nsp. */
#ifndef A3D_CRF_BAND_H_
#define A3D_CRF_BAND_H_

#include "a3d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define A3DB_MAX_SP 768   /* superpixels per image: 24 x 32 */
#define A3DB_MAX_BAND 32  /* max |left - right| of a pair */

/* The field's negative log-likelihood of y and its gradients.  z, y [n,nsp], r [n,npairs] float32; left, right [npairs]
 * int32; A = I + D - R per image, the pairs scattered in order (the last writer owns a cell, as a3d_crf_loss), D the row
 * sums of R.  band is the caller's statement of max |left - right| (the lists live on the device: the host cannot look).
 * loss_per_image[b] = L_b as above, log det A the sum of the logs of the pivots; loss_mean[0] = sum_b L_b / n, summed as
 * a3dv_crf_loss_observed sums it.  dz [n,nsp] and, unless NULL, dr [n,npairs] are the gradients of loss_mean, A NOT held
 * constant: with S_k(X) = X[l][l] + X[r][r] - 2 X[l][r] for pair k = (l, r),
 *   dL/dz = -2 e        dL/dr_k = 2 (e_l - e_r)(mu_l - mu_r) + (e_l - e_r)^2 - 1/2 S_k(A^-1)
 * mu [n,nsp], unless NULL, receives A^-1 z; status [n] int32 is 0 for an accepted image, 1 otherwise.
 *
 * Factorisation: L D L^T in band storage, no pivoting.  An image is accepted iff every pivot is finite and > 0 and its
 * loss is finite.  Every r >= 0 makes A strictly diagonally dominant with pivots >= 1.
 *
 * Edges:
 *   a pair index outside [0,nsp) or a pair with |l - r| > band: loss, dz, dr and mu NaN and status 1 for EVERY image (the
 *     lists are the batch's); the pair is skipped, never indexed with;
 *   an image that is not accepted (a pivot <= 0 or not finite; a non-finite z, y or r among them): its loss and its rows of
 *     dz, dr and mu NaN, status 1; no other image is touched, loss_mean is NaN;
 *   a pair that a later pair overwrote: dr +0.0;      a pair of a superpixel with itself: no part in A, dr +0.0.
 * dr = NULL or mu = NULL changes no other output bit.  While it runs the kernel parks one flag per pair in dr: dr must
 * not alias an input.  The same bits on every run; no float atomics.  Two launches (the images, the mean).
 * n <= 0, nsp outside 1 .. A3DB_MAX_SP, band outside 1 .. A3DB_MAX_BAND, npairs <= 0, a NULL pointer other than dr or mu:
 * A3D_EINVAL before any launch. */
int a3db_crf_band_nll(int n, int nsp, int band, const float* z, const float* y, const float* r, const int32_t* left,
                      const int32_t* right, int npairs, float* loss_per_image, float* loss_mean, float* dz, float* dr,
                      float* mu, int32_t* status, void* stream);

/* The field's MAP depths mu = A^-1 z alone, by the same factorisation and solves: the bits a3db_crf_band_nll writes to its
 * mu.  status as there (1 and a NaN row also where a component of mu is not finite).  One launch.  A3D_EINVAL as above. */
int a3db_crf_band_map(int n, int nsp, int band, const float* z, const float* r, const int32_t* left, const int32_t* right,
                      int npairs, float* mu, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* A3D_CRF_BAND_H_ */
