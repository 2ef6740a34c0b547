/* a3d_texture.h — extension of the C ABI of liba3d.so (include/a3d.h) for DCNF's third pairwise similarity.
 *
 * Liu et al. 2015 define the pairwise potential over K = 3 observations per superpixel pair: colour difference,
 * colour-histogram difference and texture disparity in terms of local binary patterns (LBP).  The reference stops at
 * two (src/models.py:122) and include/a3d.h follows it: a3d_pair_similarity has k = 2.  The entry points here have no
 * counterpart in the reference (NON-REFERENCE, --pairwise-texture): an LBP histogram per superpixel, and the pair
 * similarities with the texture one as the third.  They keep a prefix of their own, a3dt_: the same library, the same
 * conventions (caller-owned device tensors, stream-ordered launches, 0 or a negative A3D_E* code with
 * a3d_last_error()), bound by _lib.py TEXTURE_SIGNATURES.  Every refusal comes before any launch. */
#ifndef A3D_TEXTURE_H_
#define A3D_TEXTURE_H_

#include "a3d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The largest superpixel edge: S_t = sum over the 256 bins of (count_l - count_r)^2 <= 2 (sp sp)^2 < 2^24 for sp <= 53,
 * so a3dt_pair_similarity3 sums it exactly in float32 in any order.  The kernel's grey tile with its halo,
 * (sp + 2)^2 floats, is then at most 55 * 55 * 4 = 12100 bytes of LDS, a static array of that size. */
#define A3DT_MAX_SP 53

/* LBP histogram of every superpixel: x [n,h,w,3] float32 -> hist [n,(h/sp)*(w/sp),256] float32, integer counts.
 *   grey  g = ((x0 + x1) + x2) / 3 in float32, each operation rounded on its own (a3d_pair_similarity's grey value);
 *   code  of pixel (y, x): bit k is set iff g(clamp(y + dy_k, 0, h-1), clamp(x + dx_k, 0, w-1)) >= g(y, x), with
 *         (dy, dx) for k = 0 .. 7: (-1,-1) (-1,0) (-1,+1) (0,+1) (+1,+1) (+1,0) (+1,-1) (0,-1);
 *   bin   the raw 8-bit code.
 * Neighbours are read from the IMAGE, across superpixel borders, and clamped at the image border, where a clamped
 * neighbour can be the pixel itself (the bit is set).  A NaN on either side clears the bit (the comparison is false);
 * -0 >= +0 is true.  Every superpixel's 256 counts sum to sp * sp.  One block per (image, superpixel), integer LDS
 * atomics: the same bits on every run.
 * A NULL pointer, n, h, w or sp <= 0, h or w not a multiple of sp, sp > A3DT_MAX_SP: A3D_EINVAL before any launch. */
int a3dt_superpixel_lbp_hist(int n, int h, int w, const float* x, int sp, float* hist, void* stream);

/* a3d_pair_similarity with the texture similarity as the third: the arguments of a3d_pair_similarity plus lbp_hist
 * [n,P,256] (a3dt_superpixel_lbp_hist's output); dense_w holds 3 floats, sims is [n,npairs,3], r [n,npairs].
 *   sims[..,0], sims[..,1]   the SAME BITS a3d_pair_similarity writes on the same inputs (one device body, the same
 *                            operations in the same order);
 *   sims[..,2] = expf(-gamma * (sqrtf(S_t) / (float)(sp * sp))),  S_t = sum_bins (lbp_l - lbp_r)^2, evaluated in that
 *                            order: the distance of the two FREQUENCY histograms, so the similarity stays inside (0, 1];
 *   r = ((sims0 * w0 + sims1 * w1) + sims2 * w2) + b.
 * A pair index outside [0,P): NaN in the pair's three similarities and its r in every image; other pairs do not notice.
 * What a3d_pair_similarity refuses, a NULL lbp_hist, sp > A3DT_MAX_SP: A3D_EINVAL before any launch. */
int a3dt_pair_similarity3(int n, int h, int w, const float* x, int sp, const float* hist, const float* lbp_hist,
                          const int32_t* left, const int32_t* right, int npairs, const float* dense_w,
                          const float* dense_b, float gamma, float* sims, float* r, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* A3D_TEXTURE_H_ */
