"""The extension header include/a3d_berhu.h, the library's a3dh_* exports and _lib.BERHU_SIGNATURES name the same entry points,
as tests/test_abi_gradloss.py holds include/a3d_gradloss.h to its exports and bindings; bad arguments are refused before any
launch (no GPU needed: the checks come first)."""
import ctypes
import re

import abi_surface
from ann3depth_amd import _lib


def test_extension_header_exports_and_bindings_agree():
    text, code = abi_surface.check('a3dh_', {'a3dh_berhu_loss_fwd', 'a3dh_berhu_loss_bwd_ex'})
    assert re.search(r'#define A3DH_WS_FLOATS\(b\) \(\(b\) \* 3 \+ 1 \+ \(b\) \* 3 \* A3D_SILOG_PARTS\)', text)
    for words in ('PER SAMPLE', 'A3D_EINVAL', 'POISONED', 'No workgroup waits for another', 'no floating-point atomics',
                  'ascending order', 'off = 32, 16, 8, 4, 2, 1'):
        assert words in text


def test_bad_arguments_are_refused_on_the_host():
    """These calls pass host pointers a launch would fault on: A3D_EINVAL must come first."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.addressof(buf)
    nan, inf = float('nan'), float('inf')

    def fwd(b=2, npix=15, out=p, tgt=p, masked=1, fraction=0.2, loss=p, ws=p):
        return lib.a3dh_berhu_loss_fwd(b, npix, out, tgt, masked, fraction, loss, ws, None)

    def bwd(b=2, npix=15, out=p, tgt=p, masked=1, fraction=0.2, ws=p, dout=p, d16=None, ld16=0):
        return lib.a3dh_berhu_loss_bwd_ex(b, npix, out, tgt, masked, fraction, ws, dout, d16, ld16, None)

    def refused(fn, why, **kw):
        """-1, and by the check meant: every refusal has words of its own in a3d_last_error."""
        assert fn(**kw) == -1, (fn.__name__, kw)
        err = ctypes.create_string_buffer(512)
        lib.a3d_last_error(err, 512)
        assert why in err.value, (fn.__name__, kw, err.value)
        assert (b'berhu_fwd' if fn is fwd else b'berhu_bwd') in err.value

    shared = [(b'NULL pointer', kw) for kw in ({'out': None}, {'tgt': None}, {'ws': None})]
    shared += [(b'must be positive', kw) for kw in ({'b': 0}, {'npix': 0}, {'b': -1}, {'npix': -15}, {'b': -(1 << 31)})]
    shared += [(b'pixels per sample', kw) for kw in ({'npix': (1 << 24) + 1}, {'npix': (1 << 31) - 1})]
    shared += [(b'neither 0 nor 1', {'masked': v}) for v in (2, -1, 256)]
    shared += [(b'outside (0, 1]', {'fraction': v}) for v in (nan, 0.0, -0.0, -0.2, 1.0000001, 2.0, inf, -inf)]
    # exactly 2^24 pixels pass that check: refused only by one after it
    shared += [(b'outside (0, 1]', {'npix': 1 << 24, 'fraction': nan}), (b'neither 0 nor 1', {'npix': 1 << 24, 'masked': 3})]
    for why, kw in shared:
        refused(fwd, why, **kw)
        refused(bwd, why, **kw)
    for masked in (0, 1):
        refused(fwd, b'NULL pointer', masked=masked, loss=None)
        refused(bwd, b'NULL pointer', masked=masked, dout=None)
        refused(bwd, b'pitch', masked=masked, d16=p, ld16=14)               # a bf16 pitch below npix = 15
        refused(bwd, b'pitch', masked=masked, d16=p, ld16=0)
        refused(bwd, b'pitch', masked=masked, npix=1 << 24, d16=p, ld16=(1 << 24) - 1)
