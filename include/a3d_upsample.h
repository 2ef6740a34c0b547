/* a3d_upsample.h — extension of the C ABI of liba3d.so (include/a3d.h): edge-aware upsampling of a coarse depth map under
 * the guidance of the full-resolution image.
 *
 * The networks predict on coarse grids (MSDN 55 x 74; DCNF 6 x 8, 12 x 16 or 24 x 32) and the only way from there to the
 * image's pixels was the legacy bilinear sampling of a3d_resize_bilinear_tf1 and a3d_depth_metrics, which smears every
 * depth edge over a cell.  Joint bilateral upsampling (Kopf, Cohen, Lischinski, Uyttendaele 2007) weighs the coarse
 * cells around a pixel by their distance AND by how much the image's colour at the cell differs from the colour at the
 * pixel.  It has no learned parameter and no counterpart in the reference (NON-REFERENCE; `predict`, `evaluate
 * --upsample joint`).  One entry point with a prefix of its own, a3du_: the same library, the same conventions
 * (caller-owned device tensors, stream-ordered launches, 0 or a negative A3D_E* code with a3d_last_error()), bound by
 * _lib.py UPSAMPLE_SIGNATURES.  Every refusal comes before any launch. */
#ifndef A3D_UPSAMPLE_H_
#define A3D_UPSAMPLE_H_

#include "a3d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The largest window radius: (2 * 4 + 1)^2 = 81 cells per output pixel. */
#define A3DU_MAX_RADIUS 4

/* depth [n,gh,gw] float32 -> out [n,H,W] float32 under guide [n,H,W,3]: float32, or with guide_u8 != 0 the uint8 pixel
 * values k, read as fl(k / 255) (one IEEE division).  The host supplies four tables; the kernel does no coordinate
 * arithmetic of its own:
 *   cy [H], cx [W] float32: the low-resolution coordinate of every output row and column;
 *   ay [gh], ax [gw] int32: the guide pixel at which cell (i, j) takes its colour, I~(i, j) = guide[b, ay[i], ax[j]].
 * radius R in 1 .. A3DU_MAX_RADIUS; inv2ss = 1 / (2 sigma_s^2) in cells^-2 and inv2sr = 1 / (2 sigma_r^2) in colour
 * units^-2, both >= 0 and finite; inv2sr = 0 switches the range term off (the product with 0 is still formed: a colour
 * that is not finite still makes its exponent not finite).
 *
 * For output pixel p = (y, x) of image b, in float32, every operation rounded on its own (no contraction), cells visited
 * in ascending (i, j):
 *   window centre  q0 = (clamp(floor(cy[y] + 1/2), 0, gh - 1), clamp(floor(cx[x] + 1/2), 0, gw - 1)), clamped as a
 *                  float BEFORE any conversion to an integer (a NaN clamps to 0): a table value of any size stays safe;
 *   window         the cells (i, j) with |i - q0y| <= R, |j - q0x| <= R that lie inside the grid;
 *   exponent       e = ((i - cy[y])^2 + (j - cx[x])^2) * inv2ss + ((dr^2 + dg^2) + db^2) * inv2sr,
 *                  (dr, dg, db) = guide[p] - I~(i, j), the three channels summed in order;
 *   a cell is SKIPPED iff its depth is not finite, or its anchor (ay[i], ax[j]) lies outside [0,H) x [0,W) (the anchor is
 *                  never used as an index then), or its e is not finite;
 *   with e_min the smallest exponent of the remaining cells, w = expf(-(e - e_min)): the common factor cancels in the
 *                  quotient, the best cell has w = 1 exactly, so the denominator is >= 1 for any sigma and the kernel
 *                  never divides by an underflowed sum;
 *   v = (sum w * d) / (sum w), both sums started at +0.  One IEEE division, no reciprocal;
 *   out = min(max(v, d_min), d_max) over the remaining cells: a depth map stays inside the range of the depths it was
 *                  made from;
 *   if no cell remains the pixel is NaN.
 * EVERY element of out is written, nothing else is.  No float atomics: the same bits on every run.  Nothing branches into
 * memory on a value of depth or guide (a skipped cell is a select, not a jump).
 *
 * One workgroup per 8 x 32 tile of output pixels, one launch, no workspace.  The tile's cell range +- R stands in LDS as
 * (d, I~r, I~g, I~b), 16 bytes per cell, read once from memory per tile; each lane reads its own guide pixel once
 * (consecutive lanes, consecutive pixels) and walks its <= 81 cells in a register loop over LDS, twice: a minimum pass,
 * then the sums (the exponents are recomputed, not kept).  Tables for which a tile's range exceeds the 1024 cells of LDS
 * (they are arbitrary: not monotone, out of range) make that tile read its cells from memory instead, same arithmetic.
 *
 * A NULL pointer; n, gh, gw, H, W <= 0; gh or gw above 2^24 (a cell index must be exact in float32); more than 2^31 - 1
 * output pixels or tiles; radius outside 1 .. A3DU_MAX_RADIUS; inv2ss or inv2sr negative or not finite: A3D_EINVAL before
 * any launch. */
int a3du_joint_bilateral_upsample(int n, int gh, int gw, const float* depth, int H, int W, const void* guide, int guide_u8,
                                  const float* cy, const float* cx, const int32_t* ay, const int32_t* ax, int radius,
                                  float inv2ss, float inv2sr, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* A3D_UPSAMPLE_H_ */
