/* a3d_valid.h — extension of the C ABI of liba3d.so (include/a3d.h) for training on depth maps with holes.
 *
 * include/a3d.h is the fixed surface that stands in for the reference's TensorFlow ops; its symbols, the library's a3d_*
 * exports and the binding table ann3depth_amd/_lib.py SIGNATURES are held equal to each other.  The entry points here have
 * no counterpart in the reference (NON-REFERENCE, --min-depth / --max-depth) and keep a prefix of their own, a3dx_: the
 * same library, the same conventions (caller-owned device tensors, stream-ordered launches, 0 or a negative A3D_E* code
 * with a3d_last_error()), bound by _lib.py EXT_SIGNATURES.  Raw Kinect frames and the Make3D laser maps carry pixels without
 * a measurement (k = 0, or the range cap k = 255, in the 8-bit records); these launches keep them out of the resized
 * target and out of the loss. */
#ifndef A3D_VALID_H_
#define A3D_VALID_H_

#include "a3d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* a3d_resize_bilinear_tf1_ex and a3d_warp_bilinear_pair for a depth map with holes.  Arguments as a3d_resize_bilinear_tf1_ex /
 * a3d_warp_bilinear_pair plus two thresholds; tensor 1, the depth map, is required, tensor 0 is treated exactly as there;
 * one launch each.  Per output element of tensor 1, with the four taps tl tr bl br and the weights lx, ly of the plain
 * entry point (a uint8 tap is fl(fl(fl(k / 255) - 0.5) + 0.5)):
 *   a tap value t is valid iff it is finite and min_depth < t <= max_depth   (a3d_depth_metrics' words; the stored
 *                                                                             value, before the table's depth gain)
 *   tl always counts, tr iff lx > 0, bl iff ly > 0, br iff both
 *   every counting tap valid and all four taps finite: exactly the bits the plain entry point writes, gain included
 *   otherwise: NaN (any payload) — no depth is invented across a hole
 * No read leaves the image: coordinates are clamped exactly as in the plain entry points.  A NULL tensor 1, a NaN
 * threshold, min_depth > max_depth: A3D_EINVAL before any launch. */
int a3dx_resize_bilinear_tf1_valid(int n, int h, int w, int c0, const void* x0, int u8_0, int oh0, int ow0, float* y0, int c1,
                                   const void* x1, int u8_1, int oh1, int ow1, float* y1, float min_depth, float max_depth,
                                   void* stream);
int a3dx_warp_bilinear_pair_valid(int n, int h, int w, int c0, const void* x0, int u8_0, int oh0, int ow0, float* y0, int c1,
                                  const void* x1, int u8_1, int oh1, int ow1, float* y1, const float* table, float min_depth,
                                  float max_depth, void* stream);

/* a3d_silog_loss_fwd / a3d_silog_loss_bwd_ex over the pixels that hold a depth (Eigen et al. 2014, section 3.2.2).  A
 * target is valid iff it is finite (the _valid resize above writes NaN into every hole).  Per sample, over its valid pixels: n their number,
 * s2 = sum d^2, s1 = sum d with d = masked_log(o) - masked_log(t), masked_log(v) = log(v + 1e-8) with NaN -> 0 and -inf
 * kept, as in the plain loss (for a target t >= -1e-8 it is logf(t + 1e-8));  c_n = (float)(0.5 / (double)n),
 * r_n = (float)((double)npix / n);
 *   per = r_n (s2 - c_n s1^2), 0 when n = 0;   loss[0] = sum per / b;   loss[1] = sum n / (b npix), the valid fraction
 *   g_i = fl(fl(fl(fl(2 d_i - fl(2 c_n) s1) (1 / b)) r_n) / (o_i + 1e-8)) at valid pixels whose log(o_i + 1e-8) is a number,
 *   0 everywhere else (every pixel of a sample with n = 0 among them)
 * The sums keep the plain kernels' order (A3D_SILOG_PARTS parts per sample, the last block adds them): at npix = 4070 with
 * every target finite loss[0] and the gradient are bit-identical to a3d_silog_loss_fwd / a3d_silog_loss_bwd_ex.
 * loss: 2 floats.  ws: A3DX_SILOG_MASKED_WS_FLOATS(b) floats, [0] the ticket under the rules of A3D_SILOG_WS_FLOATS,
 * then s2, s1, n per sample, then the partial sums.  npix <= 2^24.  dout_bf16 / ld_bf16 as in a3d_silog_loss_bwd_ex. */
#define A3DX_SILOG_MASKED_WS_FLOATS(b) ((b) * 3 + 1 + (b) * 3 * A3D_SILOG_PARTS)
int a3dx_silog_masked_loss_fwd(int b, int npix, const float* out, const float* tgt, float* loss, float* ws, void* stream);
int a3dx_silog_masked_loss_bwd_ex(int b, int npix, const float* out, const float* tgt, const float* ws, float* dout,
                                  void* dout_bf16, int ld_bf16, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* A3D_VALID_H_ */
