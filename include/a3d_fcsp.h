/* a3d_fcsp.h — extension of the C ABI of liba3d.so (include/a3d.h) for DCNF's fully convolutional unary with
 * superpixel pooling.
 *
 * Liu et al. 2015 (TPAMI, DCNF-FCSP) run the unary convolutions once over the whole image, average the last feature map
 * inside every superpixel and feed those rows to the dense head; the reference cuts patches instead and leaves this open
 * (src/models.py:52).  The two entry points here are the pooling between the last feature map and the dense head, forward
 * and backward; they have no counterpart in the reference (NON-REFERENCE, --unary fcsp).  They keep a prefix of their
 * own, a3df_: the same library, the same conventions (caller-owned device tensors, stream-ordered launches, 0 or a
 * negative A3D_E* code with a3d_last_error()), bound by _lib.py FCSP_SIGNATURES.  Every refusal comes before any launch.
 *
 * Geometry, shared by both: an image grid H x W cut into square superpixels of edge sp, indexed row-major,
 * s = (y / sp) * (W / sp) + x / sp (a3d_superpixel_mean's order), S = (H / sp) * (W / sp) of them; a feature map
 * [n,h,w,C] float32 with pixel stride ld >= C; two int32 tables ymap [H], xmap [W]: image row y belongs to feature row
 * ymap[y], image column x to feature column xmap[x] (the feature map upsampled by the tables).  With
 *   cy(R, i)  = #{ y in [R sp, (R + 1) sp) : ymap[y] == i },   cx(Cc, j) the same over the columns,
 * the weight of cell (i, j) in superpixel s = (R, Cc) is the integer cy cx.  A table entry outside [0, h) (resp. [0, w))
 * makes its pixels contribute nothing, in both directions; the divisor stays sp sp, and nothing outside feat is
 * touched.  The tables need not be monotone for any of this to hold. */
#ifndef A3D_FCSP_H_
#define A3D_FCSP_H_

#include "a3d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The largest superpixel edge.  A block of the forward keeps, per axis, the window's sp table entries, a first-occurrence
 * flag for each, and the sorted list of its distinct in-range cells with their counts: 2 axes x 4 arrays x sp int32 of
 * LDS, filled by one lane per window pixel and axis, so one 64-lane wave serves an axis: sp <= 64, 2 KiB of LDS.  The
 * backward keeps two chunks of 64 counts (512 bytes).  A weight cy cx <= 64^2 = 4096 is exact in float32. */
#define A3DF_MAX_SP 64

/* Superpixel pooling: feat [n,h,w,C] (stride ld) -> pooled [n,S,C] (row stride ldp >= C), the block mean of the
 * upsampled map:
 *   pooled[b, s, c] = ( sum_i sum_j (float)(cy cx) * feat[b, i, j, c] ) / (float)(sp sp)
 * in float32, each operation rounded on its own, the sum started at +0 and taken over the cells in ascending (i, j);
 * cells with cy cx == 0 are SKIPPED, not multiplied by zero: a NaN or infinity in a cell reaches exactly the
 * superpixels that hold a pixel of that cell.  One IEEE division at the end, no reciprocal.  Channels C .. ld-1 of feat
 * and C .. ldp-1 of pooled are neither read nor written.  One block per (image, superpixel), lanes along C; no atomics on
 * floats: the same bits on every run.
 * A NULL pointer; n, h, w, C, H, W or sp <= 0; H or W not a multiple of sp; ld < C; ldp < C; sp > A3DF_MAX_SP:
 * A3D_EINVAL before any launch. */
int a3df_superpixel_pool_fwd(int n, int h, int w, int C, const float* feat, int ld, int H, int W, int sp,
                             const int32_t* ymap, const int32_t* xmap, float* pooled, int ldp, void* stream);

/* Its transpose: dpooled [n,S,C] (row stride ldp) -> dfeat [n,h,w,C] (stride ld),
 *   dfeat[b, i, j, c] = ( sum_s (float)(cy cx) * dpooled[b, s, c] ) / (float)(sp sp)
 * with s ascending and zero weights skipped, in the same arithmetic.  EVERY element of dfeat[.., :C] is written: a cell
 * that no pixel maps to gets +0, so the caller does not pre-zero.  Pad channels are neither read nor written.  A
 * gather, one block per cell: no floating-point atomics, the same bits on every run.
 * Refuses what a3df_superpixel_pool_fwd refuses. */
int a3df_superpixel_pool_bwd(int n, int h, int w, int C, const float* dpooled, int ldp, int H, int W, int sp,
                             const int32_t* ymap, const int32_t* xmap, float* dfeat, int ld, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* A3D_FCSP_H_ */
