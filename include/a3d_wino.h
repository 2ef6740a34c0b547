/* a3d_wino.h — extension of the C ABI of liba3d.so (include/a3d.h) for A3D_PREC_F32_WINOGRAD: the prepared filter of
 * a3d_conv2d_bwd_data.
 *
 * Under A3D_PREC_F32_WINOGRAD (include/a3d.h) the stride-1 3x3 convolutions run as Winograd F(2x2,3x3): both directions read
 * the filter through the transform U = G g G^T, sixteen [c][k] matrices.  The forward's is prepared with
 * a3d_conv2d_fwd_prepared_filter_bytes / a3d_conv2d_fwd_prepare_filter; bwd-data reads another one — the taps flipped and the
 * channels swapped before the transform, sixteen [k][c] matrices — which the pair below prepares.  A call that passes it sets
 * A3D_HINT_W_PREPARED in its descriptor, as the forward does; without the hint the library transforms the stored filter into
 * the workspace on every call.  The caller refreshes the prepared copy whenever the weights change (under the reference's
 * AdamOptimizer(..., beta2 = 1), src/models.py:309, never).  The entry points keep a prefix of their own, a3dw_: the same
 * library, the same conventions (caller-owned device tensors, stream-ordered launches, 0 or a negative A3D_E* code with
 * a3d_last_error()), bound by _lib.py WINO_SIGNATURES. */
#ifndef A3D_WINO_H_
#define A3D_WINO_H_

#include "a3d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the prepared form for this descriptor with the hint bit clear; 0: this bwd-data reads the filter as stored (any
 * precision but A3D_PREC_F32_WINOGRAD, or a geometry the route does not take) and refuses nothing, since it ignores the hint. */
size_t a3dw_conv2d_bwd_data_prepared_filter_bytes(const a3d_conv_desc* d);
/* The transform of w [3][3][c][k] into a caller-owned, 16-byte aligned buffer of at least that many bytes. */
int a3dw_conv2d_bwd_data_prepare_filter(const a3d_conv_desc* d, const float* w, void* prepared, size_t prepared_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* A3D_WINO_H_ */
