"""The Winograd F(2x2,3x3) route (A3D_PREC_F32_WINOGRAD, csrc/wino.hip) on the host: tests/wino_ref.py restates its four stages
in numpy float32.  Held to oracle.tf13_ops in float64 on normal operands (RTOL_F32, the bound the direct fp32 kernels are held to)
and to the integer result on ternary ones, for every case tests/test_gpu_wino.py runs on the GPU; the headroom bound that makes
the ternary cases exact is asserted for each of them.  Also: what the library answers for the new value without a GPU."""
import ctypes

import numpy as np
import pytest

import wino_ref as W
from oracle import tf13_ops as T

RTOL_F32 = 1e-5


def rel_l2(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


@pytest.mark.parametrize('case', W.CASES, ids=lambda c: 'x'.join(map(str, c[:6])))
def test_ternary_operands_are_exact_and_within_the_headroom_bound(case):
    n, h, w, c, k, padding = case[:6]
    rng = np.random.default_rng(5)
    ho, wo, _, _ = W.geometry(h, w, padding)
    x, g, dz = W.ternary(rng, (n, h, w, c)), W.ternary(rng, (3, 3, c, k)), W.ternary(rng, (n, ho, wo, k))
    stats = {}
    y = W.fwd(x, g, padding, stats)
    assert stats['max_v'] <= 4 and stats['max_u'] <= 9 / 4 and W.headroom(stats) < 2 ** 24
    np.testing.assert_array_equal(y, T.conv2d_fwd(x.astype(np.float64), g.astype(np.float64), None, 1, padding))
    dx = W.bwd_data(dz, g, x.shape, padding, stats)
    assert stats['channels'] == k and W.headroom(stats) < 2 ** 24
    np.testing.assert_array_equal(dx, T.conv2d_bwd_data(dz.astype(np.float64), g.astype(np.float64), x.shape, 1, padding))


@pytest.mark.parametrize('case', [(2, 13, 18, 64, 96, 'SAME'), (2, 6, 8, 32, 200, 'VALID'), (1, 9, 9, 5, 7, 'SAME'), (1, 2, 3, 8, 8, 'SAME')],
                         ids=lambda c: 'x'.join(map(str, c)))
def test_normal_operands_are_within_the_fp32_bound(case):
    n, h, w, c, k, padding = case
    rng = np.random.default_rng(6)
    ho, wo, _, _ = W.geometry(h, w, padding)
    x = rng.standard_normal((n, h, w, c)).astype(np.float32)
    g = (rng.standard_normal((3, 3, c, k)) / np.sqrt(9 * c)).astype(np.float32)
    dz = rng.standard_normal((n, ho, wo, k)).astype(np.float32)
    assert rel_l2(W.fwd(x, g, padding), T.conv2d_fwd(x.astype(np.float64), g.astype(np.float64), None, 1, padding)) < RTOL_F32
    assert rel_l2(W.bwd_data(dz, g, x.shape, padding),
                  T.conv2d_bwd_data(dz.astype(np.float64), g.astype(np.float64), x.shape, 1, padding)) < RTOL_F32


def test_queries_of_the_new_value():
    """Workspace and prepared-filter answers for 'fp32w': V + M (+ U unless prepared) where the route applies; the 'fp32' answers
    everywhere else (a 5x5 layer, a strided one, bwd-filter)."""
    from ann3depth_amd import _lib, ops
    lib = _lib.load()

    def q(fn, d):
        return getattr(lib, fn)(ctypes.byref(d))

    def up(b):
        return (b + 255) // 256 * 256
    B, c, k = 32, 384, 384
    tiles = B * 7 * 9
    d = ops.conv_desc(B, 13, 18, c, k, 3, 3, 1, 'SAME', precision='fp32w')
    u, v, m = up(16 * c * k * 4), up(16 * tiles * c * 4), up(16 * tiles * k * 4)
    assert q('a3d_conv2d_fwd_prepared_filter_bytes', d) == u == q('a3dw_conv2d_bwd_data_prepared_filter_bytes', d)
    assert q('a3d_conv2d_bwd_data_ws_bytes', d) == u + v + m
    assert q('a3d_conv2d_fwd_ws_bytes', d) >= u + v + m
    d.hints = ops.HINT_W_PREPARED
    assert q('a3d_conv2d_bwd_data_ws_bytes', d) == v + m <= 99 << 20
    plain = ops.conv_desc(B, 13, 18, c, k, 3, 3, 1, 'SAME')
    assert q('a3dw_conv2d_bwd_data_prepared_filter_bytes', plain) == 0
    for shape in [(B, 27, 37, 96, 256, 5, 5, 1, 'SAME'), (B, 13, 18, 384, 256, 3, 3, 2, 'VALID'), (B, 13, 18, c, k, 3, 3, 1, 'SAME')]:
        d32, dw = ops.conv_desc(*shape), ops.conv_desc(*shape, precision='fp32w')
        fns = ['a3d_conv2d_bwd_filter_ws_bytes']
        if shape[5] != 3 or shape[7] != 1:
            fns += ['a3d_conv2d_fwd_ws_bytes', 'a3d_conv2d_bwd_data_ws_bytes', 'a3d_conv2d_fwd_prepared_filter_bytes',
                    'a3dw_conv2d_bwd_data_prepared_filter_bytes']
        for fn in fns:
            assert q(fn, dw) == q(fn, d32), (fn, shape)


def test_the_extension_header_is_exported_and_bound():
    import os
    import re
    import subprocess
    from ann3depth_amd import _lib
    _lib.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(root, 'include', 'a3d_wino.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(a3dw_[a-z0-9_]+)\s*\(', text))
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert declared == set(re.findall(r' T (a3dw_[a-z0-9_]+)', out)) == set(_lib.WINO_SIGNATURES) and len(declared) == 2
    assert re.search(r'#define A3D_PREC_F32_WINOGRAD 3\b', open(os.path.join(root, 'include', 'a3d.h')).read())


def test_the_prepared_winograd_filter_is_refused_by_the_direct_forwards():
    """The prepared filter of an 'fp32w' descriptor is the Winograd transform: the forwards of that descriptor that run direct
    (fused pool, second output) refuse the hint before anything is enqueued — wide layers and few-channel ones alike."""
    from ann3depth_amd import _lib, ops
    lib = _lib.load()
    out2 = _lib.SecondOutput(1, 8, 1, 0, 0, 8)
    for c in (256, 3):
        d = ops.conv_desc(2, 13, 18, c, 8, 3, 3, 1, 'VALID', precision='fp32w', hints=ops.HINT_W_PREPARED)
        rc = lib.a3d_conv2d_pool_fwd(ctypes.byref(d), None, None, None, None, 8, None, 1, None, 0, None)
        assert rc == -1 and 'plain forward only' in _lib.last_error()
        rc = lib.a3d_conv2d_fwd_ex2(ctypes.byref(d), None, None, None, None, 1, ctypes.byref(out2), None, 0, None)
        assert rc == -1 and 'plain forward only' in _lib.last_error()
