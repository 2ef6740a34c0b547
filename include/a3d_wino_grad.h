/* a3d_wino_grad.h — extension of the C ABI of liba3d.so (include/a3d.h): the filter gradient of a stride-1 3x3 convolution
 * through Winograd F(2x2,3x3) in fp32.
 *
 * The identity of the forward, Y = A^T [ (G g G^T) (.) (B^T d B) ] A, differentiated by the filter:
 *
 *     dg = G^T [ sum over 2x2 tiles of dz  (B^T d B) (.) (A dY A^T) ] G
 *
 * B^T d B is the forward's input transform of x, A dY A^T expands each 2x2 tile of dz to 4x4 with adds alone, and the sixteen
 * sums over tiles are sixteen [c x T] . [T x k] products: 2.25 times fewer multiplies than the direct filter gradient (less
 * where the map's last tile row or column is half empty).  The bias gradient is the column sum of dz.  Every sum has a fixed
 * order (no atomics): two calls on the same operands give the same bits.  Against the direct kernels the result differs by
 * rounding alone, 1e-7 .. 8e-7 rel-L2 on normal operands.
 *
 * a3d_conv2d_bwd_filter itself never takes this route, whatever the descriptor's precision (A3D_PREC_F32_WINOGRAD runs the
 * filter gradient as A3D_PREC_F32 does): the pair below is the route, and names the arithmetic by being called.  It takes
 * descriptors with r = s = 3, stride 1, pad_t and pad_l in {0, 1}, storage 0, precision A3D_PREC_F32 or A3D_PREC_F32_WINOGRAD
 * and tensors within the route's 31-bit row offsets; for ANY OTHER descriptor the call forwards to a3d_conv2d_bwd_filter and the
 * query to a3d_conv2d_bwd_filter_ws_bytes, so a caller needs one code path.  The entry points keep a prefix of their own,
 * a3dwg_: the same library, the same conventions (caller-owned device tensors, stream-ordered launches, 0 or a negative A3D_E*
 * code with a3d_last_error()), bound by _lib.py WINO_GRAD_SIGNATURES. */
#ifndef A3D_WINO_GRAD_H_
#define A3D_WINO_GRAD_H_

#include "a3d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Workspace bytes of the call below: the two transforms, the raw sums of the split tile axis and the bias partials. */
size_t a3dwg_conv2d_bwd_filter_ws_bytes(const a3d_conv_desc* d);
/* dw [3][3][c][k] and, unless db is null, db [k] from x [n][h][w][ldx] and dz [n][ho][wo][ldy].  ws: 16-byte aligned; fewer
 * than the queried bytes is A3D_EWORKSPACE before anything is enqueued.  Nothing outside dw and db is written. */
int a3dwg_conv2d_bwd_filter(const a3d_conv_desc* d, const float* x, const float* dz, float* dw, float* db, void* ws,
                            size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* A3D_WINO_GRAD_H_ */
