"""The extension header include/a3d_gradloss.h, the library's a3dg_* exports and _lib.GRADLOSS_SIGNATURES name the same entry
points, as tests/test_abi_valid.py holds include/a3d_valid.h to its exports and bindings; bad arguments are refused before any
launch (no GPU needed: the checks come first)."""
import ctypes
import os
import re

import abi_surface
from ann3depth_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_extension_header_exports_and_bindings_agree():
    text, code = abi_surface.check('a3dg_', {'a3dg_silog_grad_loss_fwd', 'a3dg_silog_grad_loss_bwd_ex'})
    assert re.search(r'#define A3DG_WS_FLOATS\(b\) \(\(b\) \* 5 \+ 1 \+ \(b\) \* 5 \* A3D_SILOG_PARTS\)', text)
    width = re.search(r'#define A3DG_MAX_W (\d+)', text)
    assert width and int(width.group(1)) >= 1024
    for words in ('bit-identical', 'A3D_EINVAL', 'grad_weight == 0', 'grad_weight != 0', 'No floating-point atomics'):
        assert words in text


def test_bad_arguments_are_refused_on_the_host():
    """These calls pass host pointers a launch would fault on: A3D_EINVAL must come first."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.addressof(buf)
    nan = float('nan')
    max_w = int(re.search(r'#define A3DG_MAX_W (\d+)', open(os.path.join(ROOT, 'include', 'a3d_gradloss.h')).read()).group(1))

    def fwd(b=2, h=3, w=5, out=p, tgt=p, masked=1, weight=0.5, loss=p, ws=p):
        return lib.a3dg_silog_grad_loss_fwd(b, h, w, out, tgt, masked, weight, loss, ws, None)

    def bwd(b=2, h=3, w=5, out=p, tgt=p, masked=1, weight=0.5, ws=p, dout=p, d16=None, ld16=0):
        return lib.a3dg_silog_grad_loss_bwd_ex(b, h, w, out, tgt, masked, weight, ws, dout, d16, ld16, None)

    def refused(fn, why, **kw):
        """-1, and by the check meant: every refusal has words of its own in a3d_last_error."""
        assert fn(**kw) == -1, (fn.__name__, kw)
        err = ctypes.create_string_buffer(512)
        lib.a3d_last_error(err, 512)
        assert why in err.value, (fn.__name__, kw, err.value)
    big_h = (1 << 24) // max_w                                              # big_h x max_w is exactly 2^24 pixels
    assert big_h * max_w == 1 << 24
    shared = [(b'bad arguments', kw) for kw in ({'b': 0}, {'h': 0}, {'w': 0}, {'b': -1}, {'h': -3}, {'w': -5}, {'out': None},
                                                {'tgt': None}, {'ws': None})]
    shared += [(b'grad_weight', {'weight': v}) for v in (nan, -0.5, -float('inf'))]
    shared += [(b'A3DG_MAX_W', kw) for kw in ({'h': 1, 'w': max_w + 1}, {'h': 1 << 16, 'w': 1 << 16})]
    # h w > 2^24 with rows the width check lets through: one row too many, one pixel too many, far too many
    shared += [(b'pixels per sample', kw) for kw in ({'h': big_h + 1, 'w': max_w}, {'h': (1 << 24) + 1, 'w': 1},
                                                     {'h': 1 << 30, 'w': 2}, {'h': (1 << 31) - 1, 'w': max_w})]
    # exactly 2^24 pixels pass that check: refused only by the one after it
    shared += [(b'grad_weight', {'h': big_h, 'w': max_w, 'weight': nan}), (b'grad_weight', {'h': 1 << 24, 'w': 1, 'weight': nan})]
    for masked in (0, 1):
        for why, kw in shared:
            refused(fwd, why, masked=masked, **kw)
            refused(bwd, why, masked=masked, **kw)
        refused(fwd, b'bad arguments', masked=masked, loss=None)
        refused(bwd, b'bad arguments', masked=masked, dout=None)
        refused(bwd, b'pitch', masked=masked, d16=p, ld16=14)               # a bf16 pitch below h w = 15
        refused(bwd, b'pitch', masked=masked, d16=p, ld16=0)
        refused(bwd, b'pitch', masked=masked, h=big_h, w=max_w, d16=p, ld16=(1 << 24) - 1)
