"""The extension header include/a3d_wino_grad.h, the library's a3dwg_* exports and _lib.WINO_GRAD_SIGNATURES name the same entry
points, as tests/test_abi_upsample.py and its siblings hold the other headers; bad arguments are refused before any launch (no
GPU needed: the checks come first)."""
import ctypes

import abi_surface
from ann3depth_amd import _lib, ops

NAMES = {'a3dwg_conv2d_bwd_filter_ws_bytes', 'a3dwg_conv2d_bwd_filter'}


def test_wino_grad_header_exports_and_bindings_agree():
    text, code = abi_surface.check('a3dwg_', NAMES)
    # the other Winograd header keeps its two symbols: the new prefix is not read as a3dw_
    assert {n for n in abi_surface.exports() if n.startswith('a3dw_')} == set(_lib.WINO_SIGNATURES) and len(_lib.WINO_SIGNATURES) == 2
    # the calls take a3d_conv2d_bwd_filter's arguments: a caller switches by name alone
    assert _lib.WINO_GRAD_SIGNATURES['a3dwg_conv2d_bwd_filter'] == _lib.SIGNATURES['a3d_conv2d_bwd_filter']
    assert _lib.WINO_GRAD_SIGNATURES['a3dwg_conv2d_bwd_filter_ws_bytes'] == _lib.SIGNATURES['a3d_conv2d_bwd_filter_ws_bytes']
    for words in ('G^T', 'A dY A^T', 'no atomics', 'A3D_EWORKSPACE', 'forwards to a3d_conv2d_bwd_filter', 'WINO_GRAD_SIGNATURES'):
        assert words in text, words


def test_bad_arguments_are_refused_on_the_host():
    """These calls pass host pointers a launch would fault on: the error must come first, and nothing is written."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.addressof(buf)
    d = ops.conv_desc(2, 6, 8, 32, 200, 3, 3, 1, 'VALID')
    need = lib.a3dwg_conv2d_bwd_filter_ws_bytes(ctypes.byref(d))
    assert need > 0

    def call(desc=d, x=p, dz=p, dw=p, db=p, ws=p, nbytes=need):
        return lib.a3dwg_conv2d_bwd_filter(ctypes.byref(desc) if desc is not None else None, x, dz, dw, db, ws, nbytes, None)
    for kw in ({'x': None}, {'dz': None}, {'dw': None}, {'ws': p + 4}, {'desc': None}):
        assert call(**kw) == -1, kw
    for kw in ({'nbytes': need - 1}, {'nbytes': 0}, {'ws': None}):
        assert call(**kw) == -2, kw
    bad = ops.conv_desc(2, 6, 8, 32, 200, 3, 3, 1, 'VALID')
    bad.ldy = 100                                       # a pixel stride below the channel count
    assert call(desc=bad) == -1
    assert lib.a3dwg_conv2d_bwd_filter_ws_bytes(None) == 0
    assert bytes(buf.raw) == bytes(1 << 12)             # nothing was written
