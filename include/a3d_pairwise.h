/* a3d_pairwise.h — extension of the C ABI of liba3d.so (include/a3d.h) for learning DCNF's pairwise weights.
 *
 * include/a3d.h is the fixed surface that stands in for the reference's TensorFlow ops.  There the CRF matrix A = I + D - R
 * is a constant for the optimizer (TF 1.3 registers no gradient for scatter_nd_update), so the reference's pairwise dense
 * layer keeps its initial draw for ever.  The entry points here have no counterpart in the reference (NON-REFERENCE,
 * --train-pairwise): they carry the gradient of the same loss through A^-1 and log|A| to the pair weights r, on to the
 * dense layer, and keep that layer's weights >= 0 (Liu et al. 2015, eq. 9-14).  They keep a prefix of their own, a3dp_:
 * the same library, the same conventions (caller-owned device tensors, stream-ordered launches, 0 or a negative A3D_E*
 * code with a3d_last_error()), bound by _lib.py PAIR_SIGNATURES. */
#ifndef A3D_PAIRWISE_H_
#define A3D_PAIRWISE_H_

#include "a3d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* a3d_crf_loss plus dr = d loss_mean / d r [n,npairs], A no longer held constant.  Arguments, launches (two) and the
 * outputs loss_per_image, loss_mean and dz as a3d_crf_loss: the SAME BITS on the same inputs (one device body, every
 * operation that feeds them in the same order).  With w = A^-1 z, sd = sqrt(det A), fac = pi^(nsp/2) / (sd + eps),
 * ex = exp(g), Z = fac ex + eps, u = exp(-E) / Z of the loss, and for pair q = (l, r):
 *   S_q    = A^-1[l][l] + A^-1[r][r] - A^-1[l][r] - A^-1[r][l]          (dA / dr_q = (e_l - e_r)(e_l - e_r)^T)
 *   dE_q   = (y_l - y_r)^2       dg_q = -(w_l - w_r)^2       dfac_q = -fac / (sd + eps) (sd / 2) S_q
 *   du_q   = u (-dE_q) - (u / Z) (dfac_q ex + fac ex dg_q)
 *   dr[b,q] = -du_q / (u + eps) / n
 * A^-1 comes out of the loss's own LU, carried over [A | z | I]; one wavefront per image.  Edges:
 *   a pair index outside [0,nsp): NaN for every image and every pair, as loss and dz;
 *   an image whose determinant is negative or whose loss is NaN: its whole row of dr NaN, no other row touched;
 *   a pair whose two cells a later pair overwrote (pairs are scattered in order, the last writer owns both cells): +0.0;
 *   a pair of a superpixel with itself: 0.
 * A NULL dr (or whatever a3d_crf_loss refuses): A3D_EINVAL before any launch.  The same bits on every run. */
int a3dp_crf_loss_grad(int n, int nsp, const float* z, const float* y, const float* r, const int32_t* left,
                       const int32_t* right, int npairs, float eps, float* loss_per_image, float* loss_mean, float* dz,
                       float* dr, void* stream);

/* Backward of the pairwise dense layer k -> 1 (src/models.py:121-127; a3d_pair_similarity has k = 2): sims [n,npairs,k],
 * dr [n,npairs] -> dw[j] = sum_{b,q} dr[b,q] sims[b,q,j] (k floats), db[0] = sum_{b,q} dr[b,q].  One block, a fixed
 * summation order and no atomics: the same bits on every run.  A NaN in dr reaches db and every dw[j].  k outside 1 .. 8,
 * n <= 0, npairs <= 0 or a NULL pointer: A3D_EINVAL before any launch. */
int a3dp_pair_dense_bwd(int n, int npairs, int k, const float* sims, const float* dr, float* dw, float* db, void* stream);

/* Projected gradient descent: v = var - lr * g as a3d_sgd_apply rounds it, then var = v < floor ? floor : v.  A NaN stays
 * a NaN (the comparison is false); floor = 0 is the projection onto beta >= 0.  count == 0 or a NULL pointer: A3D_EINVAL. */
int a3dp_sgd_apply_floor(size_t count, float* var, const float* g, float lr, float floor, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* A3D_PAIRWISE_H_ */
