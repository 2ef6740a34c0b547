/* a3d_align.h — extension of the C ABI of liba3d.so (include/a3d.h): per-image scale-and-shift alignment of a prediction to
 * a target before it is judged or written.  The depth maps the models train on are min-max scaled per image
 * (tools/data_preprocessor.py), so a checkpoint predicts depth up to an unknown affine map per image; this is the standard
 * protocol for such models: median scaling (SfMLearner, Monodepth2), least-squares scale, least-squares scale and shift
 * (MiDaS), each over the valid pixels of one image.
 *
 * The entry points here have no counterpart in the reference (NON-REFERENCE, --align) and keep a prefix of their own, a3da_:
 * the same library, the same conventions as include/a3d_berhu.h (caller-owned device tensors, stream-ordered launches, 0 or
 * a negative A3D_E* code with a3d_last_error(), every refusal before any launch), bound by _lib.py ALIGN_SIGNATURES.
 *
 * THE PIXEL SET.  pred [n, ph, pw] float32, target [n, th, tw] float32 or (target_u8 != 0) the uint8 pixel values of a
 * converter-written record, as in a3d_depth_metrics.  An image is fitted on exactly the pixels a3d_depth_metrics sums over:
 * the target t is finite, > min_depth and <= max_depth, and p, the prediction sampled at that target pixel, is finite.
 * "Sampled" is a3d_depth_metrics' sampler bit for bit (the legacy align_corners=False mapping with separately rounded
 * operations; the pixel itself when the grids agree): one piece of code, csrc/metrics_common.h.  m is the size of the set.
 *
 * a3da_depth_align.  coef [n, 2] float32 (s, b); count [n] int32 = m; status [n] int32.
 *   A3DA_MEDIAN   b = 0, s = fl(med(t) / med(p)).  med of m values is the element of 0-based rank (m - 1) / 2, the LOWER
 *                 median, no averaging, in the total order of the key k(x) = bits(x) ^ 0x80000000 for x's sign bit clear,
 *                 ~bits(x) otherwise (so -0 sorts before +0); the two medians are taken independently.
 *                 Accepted iff m >= 1, med(p) > 0, and s is finite and > 0.
 *   A3DA_SCALE    b = 0, s = S_pt / S_pp.   Accepted iff m >= 1, S_pp > 0, and s is finite and > 0.
 *   A3DA_AFFINE   s = (S_pt - S_p S_t / m) / (S_pp - S_p S_p / m),  b = (S_t - s S_p) / m  in float64 (s unrounded in b).
 *                 Accepted iff m >= 2, the denominator is > 0, and both coefficients are finite.
 *   S_p, S_t, S_pp, S_pt are float64 sums over the set; each term of S_pp and S_pt is the exact float64 product of the two
 *   float32 values.  A coefficient is rounded to float32 once, at the end, and the tests "finite", "> 0" read that float32.
 *   An image that is not accepted gets coef (1, 0) and status 1 (accepted: 0): its prediction is judged as it is.  count is
 *   written regardless.  No image affects another.
 *
 * Launches and the order of every sum.  The least-squares modes take two launches, as a3d_depth_metrics does: grid
 * (parts, n) of 256 threads, workgroup (part, image) walking a contiguous range of the image's target pixels exactly as
 * metrics_part_kernel does; the sums are added per thread in ascending pixel order, then the 64 lanes of a wavefront as a
 * tree (v[l] += v[l + off], off = 32 .. 1), then the four wavefronts as ((w0 + w1) + w2) + w3; a second launch adds an
 * image's parts in part order and solves.  The same bits on every run.
 * The median is an exact radix selection on the 32-bit key in three digit passes of 11 / 11 / 10 bits.  Each pass is two
 * launches.  The first walks the pixels the same way (re-sampling p), counts the keys that match the digits chosen so far
 * into a histogram in LDS (2048 int32 bins for t and as many for p: 16 KiB) and adds its non-empty bins to the image's
 * histogram in the workspace.  The second, one wavefront per (image, quantity), prefix-scans the 2048 bins, picks the bin
 * that holds the rank and carries the remaining rank to the next pass; after the third pass the key is complete.
 * Integer atomics only, whose result does not depend on their order: no floating-point atomics,
 * no workgroup waits for another, no loop whose trip count depends on a pixel's value.  The answer is exact, and the same
 * bits on every run.
 * A launch that clears the workspace precedes the six: seven launches in all.
 *
 * A3D_EINVAL before any launch, each with words of its own: a NULL pointer; n, ph, pw, th or tw out of range (n <= 65535,
 * th tw < 2^31 - 1024, as a3d_depth_metrics); min_depth or max_depth NaN; a mode that is none of the three.
 * A3D_EWORKSPACE before any launch: ws NULL or ws_bytes < a3da_depth_align_ws_bytes(n, th, tw, mode) (0 for bad arguments).
 *
 * a3da_depth_metrics_aligned: a3d_depth_metrics with the sampled prediction p replaced by q = fl(fl(s p) + b), (s, b) =
 * coef[image], before the finiteness test and the clamp: a valid pixel whose q is not finite (every one whose p is not) is
 * counted in column A3D_METRIC_NONFINITE only.  The same kernel body, the same two launches, the same workspace
 * (a3d_depth_metrics_ws_bytes) and refusals; coef NULL is A3D_EINVAL.  With coef (1, 0) and clamp_lo > 0 the rows are
 * a3d_depth_metrics' bit for bit (1 p + 0 is p except that -0 becomes +0, which the clamp erases).
 *
 * a3da_affine_apply: y[i, j] = fl(fl(s_i x[i, j]) + b_i) for x, y [n, per_image] float32, (s_i, b_i) = coef[i]; y may be x.
 * A value that is not finite stays not finite.  One launch.  A3D_EINVAL: a NULL pointer, n <= 0 or > 65535, per_image <= 0. */
#ifndef A3D_ALIGN_H_
#define A3D_ALIGN_H_

#include "a3d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define A3DA_MEDIAN 0
#define A3DA_SCALE 1
#define A3DA_AFFINE 2

size_t a3da_depth_align_ws_bytes(int n, int th, int tw, int mode);
int a3da_depth_align(int n, int ph, int pw, const float* pred, int th, int tw, const void* target, int target_u8,
                     float min_depth, float max_depth, int mode, float* coef /*[n,2]*/, int* count /*[n]*/,
                     int* status /*[n]*/, void* ws, size_t ws_bytes, void* stream);
int a3da_depth_metrics_aligned(int n, int ph, int pw, const float* pred, int th, int tw, const void* target, int target_u8,
                               float min_depth, float max_depth, float clamp_lo, float clamp_hi, const float* coef /*[n,2]*/,
                               double* rows /*[n,11]*/, void* ws, size_t ws_bytes, void* stream);
int a3da_affine_apply(int n, int per_image, const float* x, const float* coef /*[n,2]*/, float* y, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* A3D_ALIGN_H_ */
