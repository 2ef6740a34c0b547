/* a3d_slic.h — extension of the C ABI of liba3d.so (include/a3d.h) for DCNF on SLIC superpixels.
 *
 * Liu et al. 2015 define DCNF over an over-segmentation of the image; the reference cuts square blocks and leaves the rest
 * open (src/models.py:39, :52).  The entry points here segment an image batch in the way GPU SLIC implementations do
 * (gSLIC, Ren & Reid): a pixel may only join one of the 3 x 3 clusters around its home grid cell, so the pair graph stays
 * the grid's and the CRF kernels run unchanged; and they restate, for a label map, the four places that read a
 * superpixel's pixels: the target mean, the colour statistics, the pooling of the unary's feature map and its transpose.
 * None has a counterpart in the reference (NON-REFERENCE, --segmentation slic).  They keep a prefix of their own, a3ds_:
 * the same library, the same conventions (caller-owned device tensors, stream-ordered launches, 0 or a negative A3D_E*
 * code with a3d_last_error()), bound by _lib.py SLIC_SIGNATURES.  Every refusal comes before any launch.  No atomics on
 * floats anywhere: the same bits on every run.
 *
 * Geometry, shared by all: an image H x W, sp dividing both; rows = H / sp, cols = W / sp, S = rows cols superpixels,
 * indexed row-major, s = R cols + C.  The HOME of pixel (y, x) is (y / sp, x / sp).  Its CANDIDATES N(y, x) are the up to
 * nine superpixels (R + dr, C + dc), dr, dc in {-1, 0, 1}, inside the grid, in ascending superpixel index.  Labels are
 * int32 [n,H,W].
 * LABEL CONTRACT of every kernel that reads labels: a pixel counts for superpixel s iff its label is s and s is in
 * N(y, x).  Any other label (negative, >= S, far from home) makes the pixel belong to no superpixel; such a label is never
 * used as an index.  The pixels of s therefore lie in its WINDOW, rows [(R - 1) sp, (R + 2) sp) and columns
 * [(C - 1) sp, (C + 2) sp) clipped to the image, and one block per (image, superpixel) scans that window.
 *
 * THE SUM OF A BLOCK, used wherever floats are added over a window or over 256 bins: the window's pixels are numbered
 * row-major inside the clipped window, q = 0, 1, ...; lane t of 256 starts at +0 and adds the terms q = t, t + 256, ...
 * that count, in ascending q; the 256 partial sums p[] are then folded, p[t] = p[t] + p[t + k] for t < k, k = 128, 64,
 * ..., 1; p[0] is the sum.  Every operation is rounded on its own (no fused multiply-add). */
#ifndef A3D_SLIC_H_
#define A3D_SLIC_H_

#include "a3d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The largest superpixel edge: a window of at most 9 sp sp = 36 864 pixels, whose counts and weights are exact in float32. */
#define A3DS_MAX_SP 64
/* The most cells h w of a feature map the label pooling takes: a block of the forward keeps one int32 count per cell in
 * LDS, 16 KiB. */
#define A3DS_MAX_CELLS 4096
/* The most superpixels S of one image the label pooling takes: a block of the backward keeps one int32 count per
 * superpixel in LDS, 3 KiB. */
#define A3DS_MAX_SUPERPIXELS 768

/* Count and per-channel mean of the pixels that count for every superpixel: x [n,H,W,c] float32, c in 1 .. 4, labels
 * [n,H,W] -> mean [n,S,c], count [n,S] int32.  mean = (the sum of a block, above) / (float)count: one IEEE division.
 * count == 0: the row of mean is NaN.
 * A NULL pointer; n, H, W or sp <= 0; c outside 1 .. 4; H or W not a multiple of sp; sp > A3DS_MAX_SP; more than
 * 2^31 - 1 pixels or superpixels in the batch: A3D_EINVAL before any launch. */
int a3ds_label_mean(int n, int H, int W, int c, const float* x, int sp, const int32_t* labels, float* mean, int32_t* count,
                    void* stream);

/* Colour histogram of the pixels that count for every superpixel: x [n,H,W,3] -> hist [n,S,256] float32 integer counts, the
 * bin of a pixel being a3d_superpixel_hist's (one device function serves both).  Integer LDS atomics: the counts do not
 * depend on the order.  Refuses what a3ds_label_mean refuses (c is 3). */
int a3ds_label_hist(int n, int H, int W, const float* x, int sp, const int32_t* labels, float* hist, void* stream);

/* The centres of a segmentation: x [n,H,W,3], labels -> centres [n,S,5] = (ybar, xbar, c0, c1, c2) of the pixels that
 * count for s, and count [n,S].  The colour means are a3ds_label_mean's bits (the same reduction body).  The coordinate
 * sums are integers, exact: ybar = (float)(sum of y) / (float)count, one rounding each, likewise xbar.
 * count == 0: the row of centres is NOT written (centres is in/out); count is.
 * Refuses what a3ds_label_mean refuses, and 9 sp sp max(H, W) >= 2^24 (the coordinate sums would not be exact in
 * float32). */
int a3ds_slic_update(int n, int H, int W, const float* x, int sp, const int32_t* labels, float* centres, int32_t* count,
                     void* stream);

/* One assignment: x [n,H,W,3], centres [n,S,5] -> labels [n,H,W].  With w = q q, q = compactness / (float)sp (float32, on
 * the host), the distance of pixel (y, x) to candidate k is, each operation rounded on its own,
 *   d_j = x[.., j] - centres[k, 2 + j];   col = (d_0 d_0 + d_1 d_1) + d_2 d_2;
 *   dy = (float)y - centres[k, 0];  dx = (float)x - centres[k, 1];   D_k = col + w * (dy dy + dx dx)
 * and the label is the candidate with the smallest D, ties going to the lowest index.  A candidate whose D is NaN is
 * skipped; with none left the label is the home.
 * ANCHOR: pixel (R sp + sp / 2, C sp + sp / 2) (integer division) always takes its home label, whatever the centres
 * hold: every superpixel keeps at least one pixel and no count of a segmentation is 0.
 * One lane per pixel.  Refuses what a3ds_slic_update refuses, and a compactness that is negative or not finite. */
int a3ds_slic_assign(int n, int H, int W, const float* x, int sp, const float* centres, float compactness, int32_t* labels,
                     void* stream);

/* The segmentation: grid labels (label = home), a3ds_slic_update, then iters x (a3ds_slic_assign, a3ds_slic_update), on
 * the stream in that order: bit for bit what those calls give one by one.  iters = 0 gives the grid and its block means.
 * The first centres are the block centroids R sp + (sp - 1) / 2, which lie between pixels for even sp: on a constant
 * image every pixel's home is strictly nearest and the grid is a fixed point for any iters.
 * Refuses what a3ds_slic_assign refuses, and iters < 0. */
int a3ds_slic_segment(int n, int H, int W, const float* x, int sp, int iters, float compactness, int32_t* labels,
                      float* centres, int32_t* count, void* stream);

/* The pairwise similarities of Liu et al. 2015 from the label statistics, and the pairwise dense layer (2 -> 1): mean3
 * [n,S,3] (a3ds_label_mean of the image), hist [n,S,256] (a3ds_label_hist), count [n,S], left, right [npairs] int32 ->
 * sims [n,npairs,2], r [n,npairs]:
 *   sims0 = expf(-gamma * sqrtf((e_0 e_0 + e_1 e_1) + e_2 e_2)),            e_j = mean3[l, j] - mean3[r, j]
 *   sims1 = expf(-gamma * sqrtf(sum over the 256 bins of f f)),             f = hist[l] / (float)count[l] - hist[r] / (float)count[r]
 *   r     = (sims0 * dense_w[0] + sims1 * dense_w[1]) + dense_b[0]
 * the sum over the bins being the sum of a block (lane t holds bin t).  Both distances are between quantities in [0, 1]
 * (mean colours, frequency histograms), so both similarities lie in (0, 1]; a count of 0 divides by zero and gives NaN, as
 * IEEE has it.  A pair with an index outside [0, S) gets NaN similarities and a NaN r in every image, and nothing is
 * indexed with it.  One block per (image, pair).
 * A NULL pointer; n, S or npairs <= 0; more than 2^31 - 1 (image, pair)s: A3D_EINVAL before any launch. */
int a3ds_pair_similarity(int n, int S, const float* mean3, const float* hist, const int32_t* count, const int32_t* left,
                         const int32_t* right, int npairs, const float* dense_w, const float* dense_b, float gamma,
                         float* sims, float* r, void* stream);

/* a3df_superpixel_pool_fwd (include/a3d_fcsp.h) with a label map in place of the block geometry: feat [n,h,w,C] (pixel
 * stride ld), tables ymap [H], xmap [W], labels [n,H,W], count [n,S] -> pooled [n,S,C] (row stride ldp).  With
 *   cnt(s, i, j) = #{ pixels that count for s with ymap[y] == i and xmap[x] == j, both in range }
 *   pooled[b, s, c] = ( sum over (i, j) ascending, cnt != 0, of (float)cnt * feat[b, i, j, c] ) / (float)count[b, s]
 * in float32, each operation rounded on its own, the sum started at +0; cells with cnt == 0 are SKIPPED, not multiplied
 * by zero.  One IEEE division at the end.  A superpixel with count <= 0 gets +0.  On grid labels with count = sp sp
 * these are a3df_superpixel_pool_fwd's bits.  Pad channels are neither read nor written.  One block per (image,
 * superpixel) forms cnt in LDS by integer atomics; lanes along C.
 * A NULL pointer; n, h, w, C, H, W or sp <= 0; H or W not a multiple of sp; ld < C; ldp < C; sp > A3DS_MAX_SP;
 * h w > A3DS_MAX_CELLS; S > A3DS_MAX_SUPERPIXELS: A3D_EINVAL before any launch. */
int a3ds_label_pool_fwd(int n, int h, int w, int C, const float* feat, int ld, int H, int W, int sp, const int32_t* ymap,
                        const int32_t* xmap, const int32_t* labels, const int32_t* count, float* pooled, int ldp,
                        void* stream);

/* Its exact transpose: dpooled [n,S,C] (row stride ldp) -> dfeat [n,h,w,C] (stride ld),
 *   dfeat[b, i, j, c] = sum over s ascending, cnt != 0 and count[b, s] > 0, of ((float)cnt * dpooled[b, s, c]) / (float)count[b, s]
 * started at +0, one division per term.  EVERY element of dfeat[.., :C] is written: a cell that no pixel maps to gets +0.
 * Pad channels are neither read nor written.  A gather, one block per (image, cell), cnt over the superpixels in LDS.
 * Refuses what a3ds_label_pool_fwd refuses. */
int a3ds_label_pool_bwd(int n, int h, int w, int C, const float* dpooled, int ldp, int H, int W, int sp, const int32_t* ymap,
                        const int32_t* xmap, const int32_t* labels, const int32_t* count, float* dfeat, int ld,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* A3D_SLIC_H_ */
