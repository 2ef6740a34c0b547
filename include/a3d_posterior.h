/* a3d_posterior.h — extension of the C ABI of liba3d.so (include/a3d.h): DCNF's field as a distribution at prediction.
 *
 * include/a3d.h is the fixed surface that stands in for the reference's TensorFlow ops.  The entry point here has no
 * counterpart in the reference (NON-REFERENCE, predict --uncertainty / --depths, evaluate --condition) and keeps a prefix of
 * its own, a3dc_ (conditional): the same library, the same conventions (caller-owned device tensors, stream-ordered launches,
 * 0 or a negative A3D_E* code with the library's last-error text), bound by _lib.py POSTERIOR_SIGNATURES.
 *
 * include/a3d_crf_valid.h states the model: y ~ N(mu, A^-1 / 2) over the superpixels, A = I + D - R, mu = A^-1 z.  With O
 * the observed superpixels and M the others, the field's conditional distribution of y_M given y_O is normal with
 *   mean  A_MM^-1 (z_M - A_MO y_O)          covariance  A_MM^-1 / 2.
 * Let A' be A with every observed row and column replaced by the identity's: an off-diagonal cell is kept iff both of its
 * ends are missing, a missing superpixel's diagonal is still 1 + the sum of ALL its pair weights, an observed one's is 1.
 * A' has A's half bandwidth, is positive definite where A is, and its inverse restricted to M x M is A_MM^-1; the solution
 * of A' x = rhs, rhs_i = z_i + sum over observed neighbours j of r_ij y_j on a missing i and 0 on an observed i, is the
 * conditional mean on M.  So the banded L D L^T of include/a3d_crf_band.h, its solves and its in-band inverse run on A'
 * unchanged: no compaction, no renumbering. */
#ifndef A3D_POSTERIOR_H_
#define A3D_POSTERIOR_H_

#include "a3d_crf_band.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The field's mean and variance per superpixel, given the superpixels of y that were measured.  z, y [n,nsp], r [n,npairs]
 * float32; left, right [npairs] int32; band, the scatter (the pairs in order, the last writer owns a cell) and the limits
 * A3DB_MAX_SP and A3DB_MAX_BAND as the banded likelihood's.  A superpixel is observed iff y is given and its entry is
 * finite; y = NULL: nothing is observed.  nobs[b] [n] int32 is the number of observed superpixels of image b.
 *   mean [n,nsp]: y's bits on an observed superpixel, the conditional mean on a missing one;
 *   var  [n,nsp], unless NULL: +0.0 on an observed superpixel, 1/2 (A_MM^-1)_ii on a missing one.
 * var = NULL skips the recurrence and changes no other output bit.
 *
 * Factorisation: L D L^T of A' in band storage, no pivoting.  An image is accepted iff every pivot is finite and > 0, every
 * component of the solution is finite and, where var is asked for, every variance on M is finite and > 0.  status [n] int32
 * is 0 for an accepted image, 1 otherwise.
 *
 * Edges:
 *   a pair index outside [0,nsp) or a pair with |l - r| > band: mean and var NaN and status 1 for EVERY image (the lists are
 *     the batch's); the pair is skipped, never indexed with; nobs is still the count;
 *   an image that is not accepted: its rows of mean and var NaN (the observed entries too), status 1; no other image is
 *     touched;
 *   the values in the unobserved entries of y (NaN payloads, infinities) change no output bit;
 *   nothing observed (y = NULL, or no entry finite): mean is the banded MAP launch's mu bit for bit (the diagonal is summed
 *     over every stored cell, columns ascending, before the masked cells are dropped), var 1/2 (A^-1)_ii;
 *   everything observed: mean is y's bits, var +0.0 everywhere.
 * One launch, no workspace, no float atomics.  The same bits on every run.
 * n <= 0, nsp outside 1 .. A3DB_MAX_SP, band outside 1 .. A3DB_MAX_BAND, npairs <= 0, a NULL pointer other than y or var:
 * A3D_EINVAL before any launch. */
int a3dc_crf_band_posterior(int n, int nsp, int band, const float* z, const float* y, const float* r, const int32_t* left,
                            const int32_t* right, int npairs, float* mean, float* var, int32_t* nobs, int32_t* status,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif /* A3D_POSTERIOR_H_ */
