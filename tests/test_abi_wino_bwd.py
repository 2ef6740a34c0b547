"""The extension header include/a3d_wino_bwd.h, the library's a3dwb_* exports and _lib.WINO_BWD_SIGNATURES name the same entry
points, as tests/test_abi_wino_grad.py and its siblings hold the other headers; a3dwb_pool has the layout the binding passes; bad
arguments are refused before any launch (no GPU needed: the checks come first)."""
import ctypes
import os
import re

import abi_surface
from ann3depth_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {'a3dwb_sizeof_pool', 'a3dwb_conv2d_bwd_ws_bytes', 'a3dwb_conv2d_bwd'}


def test_wino_bwd_header_exports_and_bindings_agree():
    text, code = abi_surface.check('a3dwb_', NAMES)
    # the other two Winograd headers keep their symbols: the new prefix is read as neither a3dw_ nor a3dwg_
    for prefix, theirs in (('a3dw_', _lib.WINO_SIGNATURES), ('a3dwg_', _lib.WINO_GRAD_SIGNATURES)):
        assert {n for n in abi_surface.exports() if n.startswith(prefix)} == set(theirs)
    # x, dz, then a3d_conv2d_bwd_data's w, then a3dwg_conv2d_bwd_filter's dw and db, then dx and relu_mask, the pool, ws, bytes, stream
    P, S = ctypes.c_void_p, ctypes.c_size_t
    assert _lib.WINO_BWD_SIGNATURES['a3dwb_conv2d_bwd'][1] == [ctypes.POINTER(_lib.ConvDesc), P, P, P, P, P, P, P,
                                                                ctypes.POINTER(_lib.WinoBwdPool), P, S, P]
    for words in ('three launches', 'THE BITS', 'A bracket (a3d_timing_*) measures one kernel', 'A3D_EWORKSPACE', 'a3dwg_conv2d_bwd_filter followed by',
                  'never stored', 'WINO_BWD_SIGNATURES'):
        assert words in text, words


def test_the_pool_struct_is_the_one_the_binding_passes():
    lib = _lib.load()
    text = open(os.path.join(ROOT, 'include', 'a3d_wino_bwd.h')).read()
    body = re.search(r'typedef struct a3dwb_pool \{(.*?)\} a3dwb_pool;', re.sub(r'/\*.*?\*/', '', text, flags=re.S), flags=re.S).group(1)
    fields = [f.strip() for f in body.split(';') if f.strip()]
    assert fields == ['const uint8_t* argmax', 'const float* y', 'int ldy', 'int h2, w2']
    assert [n for n, _ in _lib.WinoBwdPool._fields_] == ['argmax', 'y', 'ldy', 'h2', 'w2']
    assert lib.a3dwb_sizeof_pool() == ctypes.sizeof(_lib.WinoBwdPool) == 32
    assert (_lib.WinoBwdPool.y.offset, _lib.WinoBwdPool.ldy.offset, _lib.WinoBwdPool.h2.offset, _lib.WinoBwdPool.w2.offset) == (8, 16, 20, 24)


def test_bad_arguments_are_refused_on_the_host():
    """These calls pass host pointers a launch would fault on: the error must come first, and nothing is written."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.addressof(buf)
    d = ops.conv_desc(2, 6, 8, 32, 200, 3, 3, 1, 'VALID')
    need = lib.a3dwb_conv2d_bwd_ws_bytes(ctypes.byref(d), 0, 0)
    # the chain's buffers: the two routes' own, side by side; a prepared filter saves its transform
    e = ops.conv_desc(2, 6, 8, 32, 200, 3, 3, 1, 'VALID', precision='fp32w')
    assert need == lib.a3dwg_conv2d_bwd_filter_ws_bytes(ctypes.byref(d)) + lib.a3d_conv2d_bwd_data_ws_bytes(ctypes.byref(e)) > 0
    assert need == lib.a3dwb_conv2d_bwd_ws_bytes(ctypes.byref(e), 0, 1)
    assert need - lib.a3dwb_conv2d_bwd_ws_bytes(ctypes.byref(d), 1, 0) == lib.a3dw_conv2d_bwd_data_prepared_filter_bytes(ctypes.byref(e))
    pool = _lib.WinoBwdPool(p, p, 32, 13, 17)

    def call(desc=d, x=p, dz=p, w=p, dw=p, db=p, dx=p, mask=None, pl=None, ws=p, nbytes=need):
        return lib.a3dwb_conv2d_bwd(ctypes.byref(desc) if desc is not None else None, x, dz, w, dw, db, dx, mask,
                                    ctypes.byref(pl) if pl is not None else None, ws, nbytes, None)
    for kw in ({'x': None}, {'dz': None}, {'w': None}, {'dw': None}, {'dx': None}, {'ws': p + 4}, {'desc': None},
               {'mask': p, 'pl': pool}, {'pl': _lib.WinoBwdPool(p, p, 32, 12, 14)}, {'pl': _lib.WinoBwdPool(p, p, 31, 13, 17)},
               {'pl': _lib.WinoBwdPool(None, p, 32, 13, 17)}):
        assert call(**kw) == -1, kw
    for kw in ({'nbytes': need - 1}, {'nbytes': 0}, {'ws': None}, {'pl': pool, 'nbytes': need - 1}):
        assert call(**kw) == -2, kw
    bad = ops.conv_desc(2, 6, 8, 32, 200, 3, 3, 1, 'VALID')
    bad.ldy = 100                                       # a pixel stride below the channel count
    assert call(desc=bad) == -1
    five = ops.conv_desc(2, 11, 9, 16, 24, 5, 5, 1, 'SAME')      # handed on to the two calls: no pool there
    assert call(desc=five, pl=pool) == -1
    assert lib.a3dwb_conv2d_bwd_ws_bytes(ctypes.byref(five), 0, 0) == max(lib.a3d_conv2d_bwd_filter_ws_bytes(ctypes.byref(five)),
                                                                           lib.a3d_conv2d_bwd_data_ws_bytes(ctypes.byref(five)))
    assert lib.a3dwb_conv2d_bwd_ws_bytes(None, 0, 0) == 0
    assert bytes(buf.raw) == bytes(1 << 12)             # nothing was written
