"""The extension header include/a3d_ssi.h, the library's a3di_* exports and _lib.SSI_SIGNATURES name the same entry points, as
tests/test_abi_berhu.py holds include/a3d_berhu.h to its exports and bindings; bad arguments are refused before any launch
(no GPU needed: the checks come first)."""
import ctypes
import re

import abi_surface
from ann3depth_amd import _lib


def test_extension_header_exports_and_bindings_agree():
    text, code = abi_surface.check('a3di_', {'a3di_ssi_loss_fwd', 'a3di_ssi_loss_bwd_ex'})
    assert re.search(r'#define A3DI_WS_FLOATS\(b\) \(\(b\) \* 4 \+ 2 \+ \(b\) \* 10 \* A3D_SILOG_PARTS\)', text)
    from ann3depth_amd import ops
    for b in (1, 2, 32, 64):
        assert ops.ssi_ws(b, 'cpu').numel() == b * 4 + 2 + b * 10 * ops.SILOG_PARTS and not ops.ssi_ws(b, 'cpu').any()
    for words in ('POISONED', 'FITTED', 'DEGENERATE', 'A3D_EINVAL', 'den > 2^-30 S_oo', 'exact float64 product',
                  'q = fl(fl(s o) + t)', 'g = fl(fl(s r) k)', 'nothing is differentiated through the fit',
                  'No workgroup waits for another', 'no floating-point atomics', 'ascending order', 'off = 32, 16, 8, 4, 2, 1',
                  '((w0 + w1) + w2) + w3', '0.0f fitted, 1.0f degenerate, 2.0f poisoned'):
        assert words in text, words


def test_bad_arguments_are_refused_on_the_host():
    """These calls pass host pointers a launch would fault on: A3D_EINVAL must come first."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 12)
    p = (ctypes.addressof(buf) + 15) & ~15

    def fwd(b=2, npix=15, out=p, tgt=p, masked=1, loss=p, ws=p):
        return lib.a3di_ssi_loss_fwd(b, npix, out, tgt, masked, loss, ws, None)

    def bwd(b=2, npix=15, out=p, tgt=p, masked=1, ws=p, dout=p, d16=None, ld16=0):
        return lib.a3di_ssi_loss_bwd_ex(b, npix, out, tgt, masked, ws, dout, d16, ld16, None)

    def refused(fn, why, **kw):
        """-1, and by the check meant: every refusal has words of its own in a3d_last_error."""
        assert fn(**kw) == -1, (fn.__name__, kw)
        err = ctypes.create_string_buffer(512)
        lib.a3d_last_error(err, 512)
        assert why in err.value, (fn.__name__, kw, err.value)
        assert (b'ssi_fwd' if fn is fwd else b'ssi_bwd') in err.value

    shared = [(b'NULL pointer', kw) for kw in ({'out': None}, {'tgt': None}, {'ws': None})]
    shared += [(b'must be positive', kw) for kw in ({'b': 0}, {'npix': 0}, {'b': -1}, {'npix': -15}, {'b': -(1 << 31)})]
    shared += [(b'pixels per sample', kw) for kw in ({'npix': (1 << 24) + 1}, {'npix': (1 << 31) - 1})]
    shared += [(b'neither 0 nor 1', {'masked': v}) for v in (2, -1, 256)]
    # exactly 2^24 pixels pass that check: refused only by one after it
    shared += [(b'neither 0 nor 1', {'npix': 1 << 24, 'masked': 3})]
    shared += [(b'8-byte address', {'ws': p + 4}), (b'8-byte address', {'npix': 1 << 24, 'ws': p + 12})]
    for why, kw in shared:
        refused(fwd, why, **kw)
        refused(bwd, why, **kw)
    for masked in (0, 1):
        refused(fwd, b'NULL pointer', masked=masked, loss=None)
        refused(bwd, b'NULL pointer', masked=masked, dout=None)
        refused(bwd, b'pitch', masked=masked, d16=p, ld16=14)               # a bf16 pitch below npix = 15
        refused(bwd, b'pitch', masked=masked, d16=p, ld16=0)
        refused(bwd, b'pitch', masked=masked, npix=1 << 24, d16=p, ld16=(1 << 24) - 1)
