/* a3d_wino1d.h — extension of the C ABI of liba3d.so (include/a3d.h): the two gradients of a stride-1 convolution whose window is
 * 5 wide through 1-D Winograd F(4,5) along the width, in fp32.
 *
 * A row of 4 outputs of a 5-tap correlation, y_i = sum_k d_{i+k} g_k, is taken from 8 inputs with 8 multiplies instead of 20:
 *
 *     y = A^T [ (G g) (.) (B^T d) ]              dg = G^T [ sum over tiles (B^T d) (.) (A dy) ]
 *
 * with the interpolation points 0, 1, -1, 2, -2, 1/2, -1/2 and infinity.  The window's rows are not transformed: each of the
 * eight products is a direct r x 1 convolution (its filter gradient) over tensors one quarter as wide, so a gradient executes
 * 8 / 20 of the direct kernel's multiplies (more where the map's last tile of 4 columns is partly empty) and the transformed
 * operand is twice the tensor.  A 2-D transform of a 5x5 window expands it nine times, which costs what the products save.
 * Every sum has a fixed order (no atomics): two calls on the same operands give the same bits.  Against the direct kernels the
 * results differ by rounding alone, about 1e-6 rel-L2 on normal operands (G holds ninths and forty-fifths, nothing is exact).
 * A non-finite input reaches every output of its 8-column window.
 *
 * a3d_conv2d_bwd_data and a3d_conv2d_bwd_filter never take this route: the calls below are the route and name the arithmetic
 * by being called.  They take descriptors with s = 5, stride 1, any r, storage 0, precision A3D_PREC_F32 and transformed planes
 * within 31-bit byte offsets; for ANY OTHER descriptor a call forwards to the a3d_ call of the same name with the same
 * arguments and a query to its query, so a caller needs one code path.  bwd-data reads the filter through U = G g' (taps
 * flipped, channels swapped: eight [r][k][c] tensors); a call that passes a prepared U sets A3D_HINT_W_PREPARED in its
 * descriptor, without the hint the stored filter is transformed into the workspace on every call, with the same bits.  The entry
 * points keep a prefix of their own, a3dl_: the same library, the same conventions (caller-owned device tensors, stream-ordered
 * launches, 0 or a negative A3D_E* code with a3d_last_error()), bound by _lib.py WINO1D_SIGNATURES. */
#ifndef A3D_WINO1D_H_
#define A3D_WINO1D_H_

#include "a3d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Workspace bytes of the call below: the filter transform (unless A3D_HINT_W_PREPARED), the transform of dz, the eight products
 * and the slabs of the tiles two blocks share. */
size_t a3dl_conv2d_bwd_data_ws_bytes(const a3d_conv_desc* d);
/* dx [n][h][w][ldx] from dz [n][ho][wo][ldy] and w [r][5][c][k] (or its prepared form), times (relu_mask > 0) where a mask laid
 * out as dx is given.  ws: 16-byte aligned; fewer than the queried bytes is A3D_EWORKSPACE before anything is enqueued.  Columns
 * >= c of a wider pixel stride are not written. */
int a3dl_conv2d_bwd_data(const a3d_conv_desc* d, const float* dz, const float* w, float* dx, const float* relu_mask, void* ws,
                         size_t ws_bytes, void* stream);

/* Workspace bytes of the call below: the two transforms, the raw sums of the split pixel axis and the bias partials. */
size_t a3dl_conv2d_bwd_filter_ws_bytes(const a3d_conv_desc* d);
/* dw [r][5][c][k] and, unless db is null, db [k] from x [n][h][w][ldx] and dz [n][ho][wo][ldy].  ws as above.  Nothing outside dw
 * and db is written. */
int a3dl_conv2d_bwd_filter(const a3d_conv_desc* d, const float* x, const float* dz, float* dw, float* db, void* ws, size_t ws_bytes,
                           void* stream);

/* Bytes of bwd-data's prepared filter for this descriptor with the hint bit clear; 0: the route does not take the descriptor. */
size_t a3dl_conv2d_bwd_data_prepared_filter_bytes(const a3d_conv_desc* d);
/* The transform of w [r][5][c][k] into a caller-owned, 16-byte aligned buffer of at least that many bytes. */
int a3dl_conv2d_bwd_data_prepare_filter(const a3d_conv_desc* d, const float* w, void* prepared, size_t prepared_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* A3D_WINO1D_H_ */
