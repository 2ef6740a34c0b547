/* a3d_wino_bwd.h — extension of the C ABI of liba3d.so (include/a3d.h): both gradients of a stride-1 3x3 convolution through
 * Winograd F(2x2,3x3) in fp32 as ONE chain of three launches.
 *
 * a3dwg_conv2d_bwd_filter (include/a3d_wino_grad.h) followed by a3d_conv2d_bwd_data under A3D_PREC_F32_WINOGRAD are seven
 * launches: the transforms of x and dz, the sixteen filter-gradient products, their final transform; the input transform of dz,
 * the sixteen bwd-data products, the output transform.  The call below runs the same arithmetic as
 *
 *   1. one transform launch: B^T x B, and B^T dz B together with A dY A^T from one set of loads of dz (the 2x2 tile the
 *      filter gradient expands lies inside the 4x4 window bwd-data transforms for the same tile index);
 *   2. one product launch: one grid whose first blocks are the filter gradient's and whose other blocks are bwd-data's, each
 *      running the body, the tiles and the splits of its own launch;
 *   3. one finishing launch: the filter gradient's final transform (splits added in ascending order, G^T . G, db) and
 *      bwd-data's output transform with its ReLU mask — or with the gradient of a 2x2 max pool fused (a3dwb_pool).
 *
 * dw, db and dx are THE BITS the two calls produce on the same operands: same transforms, same split of the tile axis, same
 * order of every sum.  No atomics: two calls give the same bits.
 *
 * Timing records stay true.  A bracket (a3d_timing_*) measures one kernel, so when the timing list wants the record of either
 * product, the two products run as the two launches they are in the separate calls, each under its own record (mode, m, n, k,
 * splitk as there); launches 1 and 3 are unchanged by that, and so are the results.
 *
 * Taken: r = s = 3, stride 1, pad_t and pad_l in {0, 1}, storage 0, precision A3D_PREC_F32 or A3D_PREC_F32_WINOGRAD, tensors
 * within the routes' 31-bit row offsets.  For ANY OTHER descriptor the call runs exactly a3dwg_conv2d_bwd_filter followed by
 * a3d_conv2d_bwd_data on the descriptor as given (pool must then be null), and the query is the larger of their two queries.
 * Prefix a3dwb_: the same library, the same conventions (caller-owned device tensors, stream-ordered launches, 0 or a negative
 * A3D_E* code with a3d_last_error()), bound by _lib.py WINO_BWD_SIGNATURES. */
#ifndef A3D_WINO_BWD_H_
#define A3D_WINO_BWD_H_

#include "a3d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A 2x2 / stride-2 max pool between this layer's input and the layer below, as a3d_conv2d_pool_fwd recorded it: with it dx is
 * the UNPOOLED gradient [n][h2][w2][c] (dense), h2 / 2 == d->h and w2 / 2 == d->w, holding what
 * a3d_maxpool2x2_bwd_idx(n, h2, w2, c, argmax, y, ldy, <the route's dx>, d->ldx, dx, relu_mask = 1) writes — the zero last row /
 * column of odd extents included.  The pooled-size dx is never stored. */
typedef struct a3dwb_pool {
  const uint8_t* argmax; /* [n][h2/2][w2/2][c] window positions 0..3 */
  const float* y;        /* the pooled map [n][h2/2][w2/2], pixel stride ldy >= c */
  int ldy;
  int h2, w2;            /* the unpooled extents */
} a3dwb_pool;

size_t a3dwb_sizeof_pool(void);

/* Workspace bytes of the call below.  w_prepared: w_or_U will be the transform a3dw_conv2d_bwd_data_prepare_filter wrote (the
 * descriptor of the call then carries A3D_HINT_W_PREPARED); pooled: the call will name a pool (the bytes are the same: the
 * pooled-size dx has no buffer). */
size_t a3dwb_conv2d_bwd_ws_bytes(const a3d_conv_desc* d, int w_prepared, int pooled);
/* dw [3][3][c][k], db [k] unless null, and dx from x [n][h][w][ldx], dz [n][ho][wo][ldy] and the filter w [3][3][c][k] — or,
 * with A3D_HINT_W_PREPARED in d->hints, its prepared bwd-data transform.  relu_mask (laid out as dx, or null) and pool (or null)
 * exclude each other.  ws: 16-byte aligned; one byte fewer than the queried count is A3D_EWORKSPACE before anything is enqueued.
 * Nothing outside dw, db and dx is written. */
int a3dwb_conv2d_bwd(const a3d_conv_desc* d, const float* x, const float* dz, const float* w_or_U, float* dw, float* db, float* dx,
                     const float* relu_mask, const a3dwb_pool* pool, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* A3D_WINO_BWD_H_ */
