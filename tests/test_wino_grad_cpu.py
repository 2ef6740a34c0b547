"""The Winograd filter-gradient route (include/a3d_wino_grad.h, csrc/wino.hip) on the host: tests/wino_grad_ref.py restates it in
numpy float32.  Held to oracle.tf13_ops in float64 — element for element on ternary operands, with the headroom bound that makes
them exact asserted, and below RTOL_F32 on normal ones — for every case tests/test_gpu_wino_grad.py runs on the GPU; and what the
library answers for the workspace without a GPU."""
import ctypes

import numpy as np
import pytest

import wino_grad_ref as WG
import wino_ref as W
from oracle import tf13_ops as T

RTOL_F32 = 1e-5
# W.CASES, and the 13x18 layers again at the smallest batch whose tile axis is split unevenly (819 tiles: 26 k-tiles dealt to
# five splits as 6 + 6 + 6 + 6 + 2)
CASES = [c[:6] for c in W.CASES] + [(13, 13, 18, 256, 384, 'SAME'), (13, 13, 18, 384, 256, 'SAME')]


def rel_l2(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def reference(x, dz, padding):
    c, k = x.shape[-1], dz.shape[-1]
    return T.conv2d_bwd_filter(x.astype(np.float64), dz.astype(np.float64), (3, 3, c, k), 1, padding)


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_ternary_operands_are_exact_and_within_the_headroom_bound(case):
    n, h, w, c, k, padding = case
    rng = np.random.default_rng(21)
    ho, wo, _, _ = W.geometry(h, w, padding)
    x, dz = W.ternary(rng, (n, h, w, c)), W.ternary(rng, (n, ho, wo, k))
    stats = {}
    dw, db = WG.bwd_filter(x, dz, padding, stats)
    assert stats['max_v'] <= 4 and stats['max_z'] <= 4 and WG.headroom(stats) < 2 ** 22
    dw_ref, db_ref = reference(x, dz, padding)
    np.testing.assert_array_equal(dw, dw_ref)
    np.testing.assert_array_equal(db, db_ref)


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_normal_operands_are_within_the_fp32_bound(case):
    n, h, w, c, k, padding = case
    rng = np.random.default_rng(22)
    ho, wo, _, _ = W.geometry(h, w, padding)
    x = rng.standard_normal((n, h, w, c)).astype(np.float32)
    dz = rng.standard_normal((n, ho, wo, k)).astype(np.float32)
    dw, db = WG.bwd_filter(x, dz, padding)
    dw_ref, db_ref = reference(x, dz, padding)
    assert rel_l2(dw, dw_ref) < RTOL_F32 and rel_l2(db, db_ref) < RTOL_F32


def test_the_split_rule_gives_one_split_and_uneven_ones_on_the_cases():
    """n = 3 of the 13x18 layers is one split with a partial last k-tile (189 tiles), n = 13 five splits of 6, 6, 6, 6 and 2
    k-tiles; the training batches 8, 16 and 32 stay within one round of the block slots."""
    assert WG.splits(256, 384, 189) == 1 and WG.splits(384, 256, 189) == 1
    assert WG.splits(256, 384, 819) == 5 == WG.splits(384, 256, 819) and WG.ktile_shares(819, 5) == [6, 6, 6, 6, 2]
    assert WG.splits(256, 384, 504) == 2 and WG.splits(384, 384, 504) == 3
    for c, k in ((256, 384), (384, 384)):
        for B in (8, 16, 32):
            s = WG.splits(c, k, B * 63)
            assert 16 * -(-c // 128) * -(-k // 128) * s <= WG.BLOCK_SLOTS and min(WG.ktile_shares(B * 63, s)) >= 1
    assert WG.splits(384, 384, 2016) == 3 and WG.splits(256, 384, 2016) == 5
    assert WG.splits(4, 4, 1) == 1


def test_queries():
    """a3dwg_..._ws_bytes for conv2d_3 at B = 32: V + Z + slabs + bias partials by the rule's split count, each rounded up to 256
    bytes; the same answer for an 'fp32w' descriptor; a3d_conv2d_bwd_filter's answer where the route does not apply."""
    from ann3depth_amd import _lib, ops
    lib = _lib.load()

    def up(b):
        return (b + 255) // 256 * 256
    B, c, k = 32, 384, 384
    tiles = B * 7 * 9
    s = WG.splits(c, k, tiles)
    want = up(16 * tiles * c * 4) + up(16 * tiles * k * 4) + up(16 * s * c * k * 4) + up(s * k * 4)
    for prec in ('fp32', 'fp32w'):
        d = ops.conv_desc(B, 13, 18, c, k, 3, 3, 1, 'SAME', precision=prec)
        assert lib.a3dwg_conv2d_bwd_filter_ws_bytes(ctypes.byref(d)) == want <= 200 << 20
    # channels that are no multiple of 4 are padded to whole 16-byte pieces
    d = ops.conv_desc(1, 9, 9, 5, 7, 3, 3, 1, 'SAME')
    assert lib.a3dwg_conv2d_bwd_filter_ws_bytes(ctypes.byref(d)) == 2 * up(16 * 25 * 8 * 4) + up(16 * 8 * 8 * 4) + up(8 * 4)
    for shape, prec in [((B, 27, 37, 96, 256, 5, 5, 1, 'SAME'), 'fp32'), ((B, 13, 18, 384, 256, 3, 3, 2, 'VALID'), 'fp32'),
                        ((B, 13, 18, c, k, 3, 3, 1, 'SAME'), 'bf16'), ((B, 13, 18, c, k, 3, 3, 1, 'SAME'), 'bf16x3')]:
        d = ops.conv_desc(*shape, precision=prec)
        assert lib.a3dwg_conv2d_bwd_filter_ws_bytes(ctypes.byref(d)) == lib.a3d_conv2d_bwd_filter_ws_bytes(ctypes.byref(d)), shape


def test_a_short_workspace_is_refused_on_the_host():
    """One byte short is A3D_EWORKSPACE before anything is enqueued (host pointers here: a launch would fault)."""
    from ann3depth_amd import _lib, ops
    lib = _lib.load()
    d = ops.conv_desc(2, 6, 8, 32, 200, 3, 3, 1, 'VALID')
    need = lib.a3dwg_conv2d_bwd_filter_ws_bytes(ctypes.byref(d))
    buf = ctypes.create_string_buffer(4096 + 16)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    assert lib.a3dwg_conv2d_bwd_filter(ctypes.byref(d), p, p, p, p, p, need - 1, None) == -2
    assert 'workspace' in _lib.last_error()
    assert lib.a3dwg_conv2d_bwd_filter(ctypes.byref(d), None, p, p, p, p, need, None) == -1
    assert bytes(buf.raw) == bytes(4096 + 16)
