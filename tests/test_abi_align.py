"""The extension header include/a3d_align.h, the library's a3da_* exports and _lib.ALIGN_SIGNATURES name the same entry
points, as tests/test_abi_berhu.py holds include/a3d_berhu.h to its exports and bindings; bad arguments are refused before any
launch (no GPU needed: the checks come first)."""
import ctypes
import re

import abi_surface
from ann3depth_amd import _lib

NAMES = {'a3da_depth_align_ws_bytes', 'a3da_depth_align', 'a3da_depth_metrics_aligned', 'a3da_affine_apply'}


def test_extension_header_exports_and_bindings_agree():
    text, code = abi_surface.check('a3da_', NAMES)
    assert _lib.ALIGN_SIGNATURES['a3da_depth_align_ws_bytes'][0] is ctypes.c_size_t
    # a3da_depth_metrics_aligned is a3d_depth_metrics with coef before rows
    plain = list(_lib.SIGNATURES['a3d_depth_metrics'][1])
    assert _lib.ALIGN_SIGNATURES['a3da_depth_metrics_aligned'][1] == plain[:12] + [ctypes.c_void_p] + plain[12:]
    from ann3depth_amd import ops
    for i, mode in enumerate(ops.ALIGN_MODES):
        assert re.search(rf'#define A3DA_{mode.upper()} {i}\b', text)
    for words in ('LOWER', 'A3D_EINVAL', 'A3D_EWORKSPACE', '-0 sorts before +0', 'no floating-point atomics',
                  'no workgroup waits for another', 'part order', 'bit for bit', 'coef (1, 0) and status 1'):
        assert words in text, words


def test_bad_arguments_are_refused_on_the_host():
    """These calls pass host pointers a launch would fault on: the refusal must come first."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 18)
    p = ctypes.addressof(buf)
    nan = float('nan')
    EINVAL, EWORKSPACE = -1, -2

    def last():
        err = ctypes.create_string_buffer(512)
        lib.a3d_last_error(err, 512)
        return err.value

    def align(n=2, ph=3, pw=4, pred=p, th=6, tw=8, tgt=p, u8=0, lo=0., hi=float('inf'), mode=2, coef=p, count=p, status=p,
              ws=p, ws_bytes=1 << 18):
        return lib.a3da_depth_align(n, ph, pw, pred, th, tw, tgt, u8, lo, hi, mode, coef, count, status, ws, ws_bytes, None)

    def aligned(n=2, ph=3, pw=4, pred=p, th=6, tw=8, tgt=p, u8=0, lo=0., hi=float('inf'), clo=1e-3, chi=float('inf'), coef=p,
                rows=p, ws=p, ws_bytes=1 << 18):
        return lib.a3da_depth_metrics_aligned(n, ph, pw, pred, th, tw, tgt, u8, lo, hi, clo, chi, coef, rows, ws, ws_bytes, None)

    def apply(n=2, per=12, x=p, coef=p, y=p):
        return lib.a3da_affine_apply(n, per, x, coef, y, None)

    def refused(fn, why, code=EINVAL, **kw):
        assert fn(**kw) == code, (fn.__name__, kw)
        assert why in last(), (fn.__name__, kw, last())

    for kw in ({'pred': None}, {'tgt': None}, {'coef': None}, {'count': None}, {'status': None}):
        refused(align, b'depth_align: NULL pointer', **kw)
    for kw in ({'n': 0}, {'n': -2}, {'n': 65536}, {'ph': 0}, {'pw': -1}, {'th': 0}, {'tw': 0}, {'th': 1 << 16, 'tw': 1 << 15}):
        refused(align, b'depth_align: bad shape', **kw)
    for kw in ({'lo': nan}, {'hi': nan}):
        refused(align, b'is NaN', **kw)
    for mode in (-1, 3, 7):
        refused(align, b'unknown mode', mode=mode)
    for mode in (0, 1, 2):
        need = lib.a3da_depth_align_ws_bytes(2, 6, 8, mode)
        assert 0 < need <= 1 << 18
        refused(align, b'depth_align: need', EWORKSPACE, mode=mode, ws_bytes=need - 1)
        refused(align, b'depth_align: need', EWORKSPACE, mode=mode, ws=None)
        assert lib.a3da_depth_align_ws_bytes(2, 480, 640, mode) >= need
    assert lib.a3da_depth_align_ws_bytes(2, 480, 640, 1) > lib.a3da_depth_align_ws_bytes(2, 6, 8, 1)      # more parts
    assert lib.a3da_depth_align_ws_bytes(0, 6, 8, 0) == 0 and lib.a3da_depth_align_ws_bytes(2, 0, 8, 0) == 0
    assert lib.a3da_depth_align_ws_bytes(2, 6, 8, 3) == 0 and lib.a3da_depth_align_ws_bytes(2, 6, 8, -1) == 0

    refused(aligned, b'depth_metrics_aligned: NULL coef', coef=None)
    for kw in ({'n': 0}, {'ph': 0}, {'tw': 0}, {'pred': None}, {'tgt': None}, {'rows': None}):
        refused(aligned, b'depth_metrics_aligned: bad arguments', **kw)
    for kw in ({'lo': nan}, {'chi': nan}, {'clo': 2.0, 'chi': 1.0}):
        refused(aligned, b'depth_metrics_aligned: bad depth range or clamp', **kw)
    need = lib.a3d_depth_metrics_ws_bytes(2, 6, 8)
    refused(aligned, b'depth_metrics_aligned: need', EWORKSPACE, ws_bytes=need - 1)
    refused(aligned, b'depth_metrics_aligned: need', EWORKSPACE, ws=None)

    for kw in ({'x': None}, {'coef': None}, {'y': None}):
        refused(apply, b'affine_apply: NULL pointer', **kw)
    for kw in ({'n': 0}, {'n': -1}, {'n': 65536}, {'per': 0}, {'per': -12}):
        refused(apply, b'affine_apply: bad shape', **kw)
