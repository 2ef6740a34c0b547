"""The extension header include/a3d_optim.h, the library's a3do_* exports and _lib.OPTIM_SIGNATURES name the same entry points, as
tests/test_abi_ssi.py holds include/a3d_ssi.h to its exports and bindings; bad arguments are refused before any launch (no GPU
needed: the checks come first)."""
import ctypes

import abi_surface
from ann3depth_amd import _lib


def test_extension_header_exports_and_bindings_agree():
    text, code = abi_surface.check('a3do_', {'a3do_momentum_apply', 'a3do_dense_bwd_filter_momentum'})
    for words in ("accum' = accum * momentum + g'", "var'   = var - lr * accum'", "g'     = grad_scale == 1 ? g : g * grad_scale",
                  'no fused multiply-add', 'without Nesterov', 'two-call equivalence', 'bit for bit',
                  'a3d_dense_bwd_filter into a scratch gradient followed by a3do_momentum_apply', 'MFMA 32x32x2', 'ascending order',
                  'BiasAddGrad', '1 <= m <= 64', 'A3D_EINVAL', 'NON-REFERENCE'):
        assert words in text, words


def test_bad_arguments_are_refused_on_the_host():
    """These calls pass host pointers a launch would fault on: A3D_EINVAL must come first."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 12)
    p = (ctypes.addressof(buf) + 15) & ~15

    def apply(count=8, var=p, accum=p + 256, g=p + 512):
        return lib.a3do_momentum_apply(count, var, accum, g, 0.1, 0.9, 1.0, None)

    def fused(m=4, k=3, n=5, x=p, dz=p + 256, var_w=p + 512, accum_w=p + 1024, var_b=p + 1536, accum_b=p + 2048):
        return lib.a3do_dense_bwd_filter_momentum(m, k, n, x, dz, var_w, accum_w, var_b, accum_b, 0.1, 0.9, 1.0, None)

    def refused(fn, why, **kw):
        """-1, and by the check meant: every refusal has words of its own in a3d_last_error."""
        assert fn(**kw) == -1, (fn.__name__, kw)
        err = ctypes.create_string_buffer(512)
        lib.a3d_last_error(err, 512)
        assert why in err.value, (fn.__name__, kw, err.value)

    for kw in ({'var': None}, {'accum': None}, {'g': None}, {'count': 0}):
        refused(apply, b'momentum_apply: bad arguments', **kw)
    for kw in ({'var': p + 4}, {'accum': p + 256 + 4}, {'g': p + 512 + 4}, {'g': p + 8}):      # 4 (and 8) bytes off the 16-byte grid
        refused(apply, b'16-byte aligned', **kw)
    for kw in ({'x': None}, {'dz': None}, {'var_w': None}, {'accum_w': None}, {'m': 0}, {'k': 0}, {'n': -1}):
        refused(fused, b'dense_bwd_filter_momentum: bad arguments', **kw)
    refused(fused, b'come as a pair', var_b=None)
    refused(fused, b'come as a pair', accum_b=None)
    refused(fused, b'a3d_dense_bwd_filter and a3do_momentum_apply', m=65)
    refused(fused, b'at most 64 rows', m=1 << 20)
    refused(fused, b'4-byte aligned', var_w=p + 514)
