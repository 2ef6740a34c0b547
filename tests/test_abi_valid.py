"""The extension header include/a3d_valid.h, the library's a3dx_* exports and _lib.EXT_SIGNATURES name the same entry
points, as tests/test_abi.py holds include/a3d.h, the a3d_* exports and _lib.SIGNATURES to each other; bad arguments are
refused before any launch (no GPU needed: the checks come first)."""
import ctypes
import re

import abi_surface
from ann3depth_amd import _lib


def test_extension_header_exports_and_bindings_agree():
    text, code = abi_surface.check('a3dx_', {'a3dx_resize_bilinear_tf1_valid', 'a3dx_warp_bilinear_pair_valid',
                                               'a3dx_silog_masked_loss_fwd', 'a3dx_silog_masked_loss_bwd_ex'})
    assert re.search(r'#define A3DX_SILOG_MASKED_WS_FLOATS\(b\) \(\(b\) \* 3 \+ 1 \+ \(b\) \* 3 \* A3D_SILOG_PARTS\)', text)
    for words in ('min_depth < t <= max_depth', 'A3D_EINVAL', 'bit-identical'):
        assert words in text


def test_bad_arguments_are_refused_on_the_host():
    """These calls pass host pointers a launch would fault on: A3D_EINVAL must come first."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.addressof(buf)
    nan = float('nan')

    def resize(x1=p, y1=p, lo=0.0, hi=1.0, n=2):
        return lib.a3dx_resize_bilinear_tf1_valid(n, 4, 4, 3, p, 1, 2, 2, p, 1, x1, 1, 2, 2, y1, lo, hi, None)

    def warp(x1=p, y1=p, lo=0.0, hi=1.0, table=p, c0=3):
        return lib.a3dx_warp_bilinear_pair_valid(2, 4, 4, c0, p, 1, 2, 2, p, 1, x1, 1, 2, 2, y1, table, lo, hi, None)
    for fn in (resize, warp):
        for kw in ({'x1': None}, {'y1': None}, {'lo': nan}, {'hi': nan}, {'lo': 1.0, 'hi': 0.5}):
            assert fn(**kw) == -1, (fn.__name__, kw)
    assert resize(n=0) == -1 and warp(table=None) == -1 and warp(c0=5) == -1
    assert lib.a3dx_silog_masked_loss_fwd(2, 8, p, None, p, p, None) == -1
    assert lib.a3dx_silog_masked_loss_fwd(2, (1 << 24) + 1, p, p, p, p, None) == -1
    assert lib.a3dx_silog_masked_loss_bwd_ex(2, 8, p, p, p, p, p, 4, None) == -1            # a bf16 pitch below npix
