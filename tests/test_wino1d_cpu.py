"""The 1-D Winograd F(4,5) route (include/a3d_wino1d.h, csrc/wino1d.hip) on the host: the three matrices against the identity that
defines them; tests/wino1d_ref.py, the route restated in numpy float32, against oracle.tf13_ops in float64 on every case
tests/test_gpu_wino1d.py runs — in rel-L2 and element by element against the same convolution of absolute values, so that one
wrong halo or overhang element cannot hide in a norm —; the two work-division rules; what the library answers for workspaces and
the prepared filter without a GPU; and header, exports and bindings."""
import ctypes

import numpy as np
import pytest

import abi_surface
import wino1d_ref as W1
from oracle import tf13_ops as T

RTOL_F32 = 1e-5
NAMES = {'a3dl_conv2d_bwd_data_ws_bytes', 'a3dl_conv2d_bwd_data', 'a3dl_conv2d_bwd_filter_ws_bytes', 'a3dl_conv2d_bwd_filter',
         'a3dl_conv2d_bwd_data_prepared_filter_bytes', 'a3dl_conv2d_bwd_data_prepare_filter'}


def rel_l2(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def within(got, ref, scale):
    """rel-L2 below RTOL_F32 and |got - ref| <= RTOL_F32 * scale element by element; returns (rel-L2, worst |err| / scale)"""
    r = rel_l2(got, ref)
    err = np.abs(np.asarray(got, np.float64) - ref)
    worst = float((err / np.maximum(scale, 1e-300)).max())
    assert r < RTOL_F32 and (err <= RTOL_F32 * scale).all(), (r, worst)
    return r, worst


def bwd_data_reference(dz, w, xshape, padding, mask=None):
    """dx and its scale |dz| * |w| in float64"""
    f = np.float64
    ref = T.conv2d_bwd_data(dz.astype(f), w.astype(f), xshape, 1, padding)
    scale = T.conv2d_bwd_data(np.abs(dz).astype(f), np.abs(w).astype(f), xshape, 1, padding)
    if mask is not None:
        ref, scale = ref * (mask > 0), scale * (mask > 0)
    return ref, scale


def bwd_filter_reference(x, dz, r, padding):
    """(dw, db) and their scales in float64"""
    f = np.float64
    shape = (r, 5, x.shape[-1], dz.shape[-1])
    return (T.conv2d_bwd_filter(x.astype(f), dz.astype(f), shape, 1, padding),
            T.conv2d_bwd_filter(np.abs(x).astype(f), np.abs(dz).astype(f), shape, 1, padding))


def test_the_matrices_satisfy_the_defining_identity():
    assert W1.defining_forms_hold()
    assert W1.identity_error() < 1e-12
    # B^T holds quarters only: exact in float32; G's ninths are the correctly rounded floats
    assert (W1.BT32.astype(np.float64) == W1.as_array(W1.BT, np.float64)).all()
    assert W1.G32[1, 0] == np.float32(-2.0 / 9.0) and W1.G32[5, 1] == np.float32(16.0 / 45.0)


@pytest.mark.parametrize('case', W1.CASES, ids=W1.case_id)
def test_bwd_data_restated_is_within_the_fp32_bounds(case):
    n, h, w, c, k, r, padding = case[:7]
    _, dz, wt, relu = W1.operands(case, 41)
    for mask in (None, relu):
        ref, scale = bwd_data_reference(dz, wt, (n, h, w, c), padding, mask)
        got = W1.bwd_data(dz, wt, (n, h, w, c), padding, mask)
        print('bwd-data rel-L2 %.3e, worst element %.3e of its scale' % within(got, ref, scale))


@pytest.mark.parametrize('case', W1.CASES, ids=W1.case_id)
def test_bwd_filter_restated_is_within_the_fp32_bounds(case):
    """Measured (rel-L2 / worst element as a multiple of its scale): dw 3.1e-7 .. 1.3e-6 / 2.1e-7 .. 1.4e-6 and db at most
    2.9e-7 / 4e-8 on every case but the smallest; 1x3x5x8x12x5xSAME 3.1e-7 / 8.9e-6.  An outermost tap of that case sums 3
    products (one image, one row, three columns) while it is computed from two tiles' eight plane products, each carrying the
    rounding of a whole 8-column window, so its error follows the windows' energy and its scale the tap's own three products.
    With the final transform in float32 the case measured 1.6e-5 and missed the element bound; the transform's eight terms are
    some twenty times the sum they cancel to, and it runs in double since (wino1d_dw_kernel), which is what holds the case."""
    r, padding = case[5:7]
    x, dz, _, _ = W1.operands(case, 42)
    (dw_ref, db_ref), (dw_scale, db_scale) = bwd_filter_reference(x, dz, r, padding)
    dw, db = W1.bwd_filter(x, dz, r, padding)
    print('dw rel-L2 %.3e, worst element %.3e of its scale' % within(dw, dw_ref, dw_scale))
    print('db rel-L2 %.3e, worst element %.3e of its scale' % within(db, db_ref, db_scale))


def test_the_work_division_rules():
    """conv2d_1 (27 x 37, 96 -> 256, 5 x 5): 64 stream-K blocks a plane from B = 8 up and 8 splits of the filter gradient at
    B = 8, 16 and 32, both exactly one round of the 512 block slots; the cases' single and uneven splits."""
    for B in (8, 16, 32):
        g = W1.bwd_data_geometry(B, 27, 37, 96, 256, 5, 'SAME')
        assert (g['bn'], g['nk'], g['blocks']) == (96, 40, 64) and g['tiles'] == -(-B * 270 // 128)
    assert [W1.grad_splits(480, 256, B * 270) for B in (8, 16, 32)] == [8, 8, 8] and W1.PLANES * 4 * 2 * 8 == W1.BLOCK_SLOTS
    g = W1.bwd_data_geometry(*W1.CASES[-1][:7])
    assert (g['bn'], g['tiles'], g['nk'], g['blocks']) == (128, 1, 10, 2)
    assert W1.bwd_blocks(1, 2) == 1 and W1.bwd_blocks(3, 40) == 30 and W1.bwd_blocks(1000, 40) == 64
    splits = [W1.grad_splits(c[5] * W1.pad4(c[3]), W1.pad4(c[4]), c[0] * W1.geometry(*c[1:3], *c[5:7])[0] * -(-W1.geometry(*c[1:3], *c[5:7])[1] // 4))
              for c in W1.CASES]
    assert splits == [1, 1, 1, 1, 1, 1, 3, 1, 4, 1]
    assert W1.ktile_shares(540, 3) == [6, 6, 5] and W1.ktile_shares(810, 4) == [7, 7, 7, 5]      # the uneven counts of cases 6 and 8


def test_queries():
    """The formulas where the route applies, the direct calls' answers where it does not."""
    from ann3depth_amd import _lib, ops
    lib = _lib.load()
    for case in W1.CASES + [(32, 27, 37, 96, 256, 5, 'SAME', None, None)]:
        n, h, w, c, k, r, padding, ldx, ldy = case
        d = ops.conv_desc(n, h, w, c, k, r, 5, 1, padding, ldx=ldx, ldy=ldy)
        assert lib.a3dl_conv2d_bwd_data_ws_bytes(ctypes.byref(d)) == W1.bwd_data_ws_bytes(*case[:7]), case
        assert lib.a3dl_conv2d_bwd_filter_ws_bytes(ctypes.byref(d)) == W1.bwd_filter_ws_bytes(*case[:7]), case
        assert lib.a3dl_conv2d_bwd_data_prepared_filter_bytes(ctypes.byref(d)) == W1.prepared_bytes(c, k, r), case
        d.hints |= ops.HINT_W_PREPARED
        assert lib.a3dl_conv2d_bwd_data_ws_bytes(ctypes.byref(d)) == W1.bwd_data_ws_bytes(*case[:7], prepared=True), case
    for shape, prec in [((4, 13, 18, 256, 384, 3, 3, 1, 'SAME'), 'fp32'), ((4, 27, 37, 96, 256, 5, 5, 2, 'SAME'), 'fp32'),
                        ((4, 27, 37, 96, 256, 5, 5, 1, 'SAME'), 'bf16'), ((4, 27, 37, 96, 256, 5, 5, 1, 'SAME'), 'fp32w'),
                        ((4, 27, 37, 96, 256, 5, 3, 1, 'SAME'), 'fp32')]:
        d = ops.conv_desc(*shape, precision=prec)
        assert lib.a3dl_conv2d_bwd_data_ws_bytes(ctypes.byref(d)) == lib.a3d_conv2d_bwd_data_ws_bytes(ctypes.byref(d)), shape
        assert lib.a3dl_conv2d_bwd_filter_ws_bytes(ctypes.byref(d)) == lib.a3d_conv2d_bwd_filter_ws_bytes(ctypes.byref(d)), shape
        assert lib.a3dl_conv2d_bwd_data_prepared_filter_bytes(ctypes.byref(d)) == 0, shape
    assert lib.a3dl_conv2d_bwd_data_ws_bytes(None) == 0 and lib.a3dl_conv2d_bwd_filter_ws_bytes(None) == 0


def test_short_workspaces_and_bad_arguments_are_refused_on_the_host():
    """One byte short is A3D_EWORKSPACE before anything is enqueued (host pointers here: a launch would fault)."""
    from ann3depth_amd import _lib, ops
    lib = _lib.load()
    d = ops.conv_desc(2, 7, 8, 8, 12, 5, 5, 1, 'VALID')
    buf = ctypes.create_string_buffer(4096 + 16)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    need = lib.a3dl_conv2d_bwd_data_ws_bytes(ctypes.byref(d))
    assert lib.a3dl_conv2d_bwd_data(ctypes.byref(d), p, p, p, None, p, need - 1, None) == -2 and 'workspace' in _lib.last_error()
    assert lib.a3dl_conv2d_bwd_data(ctypes.byref(d), p, p, p, None, None, need, None) == -2
    assert lib.a3dl_conv2d_bwd_data(ctypes.byref(d), None, p, p, None, p, need, None) == -1
    assert lib.a3dl_conv2d_bwd_data(ctypes.byref(d), p, p, p, None, p + 4, need, None) == -1
    need = lib.a3dl_conv2d_bwd_filter_ws_bytes(ctypes.byref(d))
    assert lib.a3dl_conv2d_bwd_filter(ctypes.byref(d), p, p, p, p, p, need - 1, None) == -2 and 'workspace' in _lib.last_error()
    assert lib.a3dl_conv2d_bwd_filter(ctypes.byref(d), p, None, p, p, p, need, None) == -1
    need = lib.a3dl_conv2d_bwd_data_prepared_filter_bytes(ctypes.byref(d))
    assert lib.a3dl_conv2d_bwd_data_prepare_filter(ctypes.byref(d), p, p, need - 1, None) == -2
    assert lib.a3dl_conv2d_bwd_data_prepare_filter(ctypes.byref(d), p, p + 4, need, None) == -1
    d3 = ops.conv_desc(2, 7, 8, 8, 12, 3, 3, 1, 'VALID')
    assert lib.a3dl_conv2d_bwd_data_prepare_filter(ctypes.byref(d3), p, p, 1 << 20, None) == -1      # the route does not take it
    assert bytes(buf.raw) == bytes(4096 + 16)


def test_header_exports_and_bindings_agree():
    from ann3depth_amd import _lib
    text, code = abi_surface.check('a3dl_', NAMES)
    # each call takes the argument list of the direct call it can replace: a caller switches by name alone
    for name in ('conv2d_bwd_data', 'conv2d_bwd_data_ws_bytes', 'conv2d_bwd_filter', 'conv2d_bwd_filter_ws_bytes'):
        assert _lib.WINO1D_SIGNATURES['a3dl_' + name] == _lib.SIGNATURES['a3d_' + name], name
    for name in ('conv2d_bwd_data_prepared_filter_bytes', 'conv2d_bwd_data_prepare_filter'):
        assert _lib.WINO1D_SIGNATURES['a3dl_' + name] == _lib.WINO_SIGNATURES['a3dw_' + name], name
    for words in ('F(4,5)', 'G^T', 'no atomics', 'A3D_EWORKSPACE', 'forwards to the a3d_ call', 'A3D_HINT_W_PREPARED', 'WINO1D_SIGNATURES'):
        assert words in text, words
