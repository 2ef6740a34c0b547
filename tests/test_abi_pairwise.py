"""The extension header include/a3d_pairwise.h, the library's a3dp_* exports and _lib.PAIR_SIGNATURES name the same
entry points, as tests/test_abi.py and tests/test_abi_valid.py hold the other two headers; bad arguments are refused
before any launch (no GPU needed: the checks come first)."""
import ctypes

import abi_surface
from ann3depth_amd import _lib

NAMES = {'a3dp_crf_loss_grad', 'a3dp_pair_dense_bwd', 'a3dp_sgd_apply_floor'}


def test_pairwise_header_exports_and_bindings_agree():
    text, code = abi_surface.check('a3dp_', NAMES)
    # a3d_crf_loss's arguments plus dr
    assert _lib.PAIR_SIGNATURES['a3dp_crf_loss_grad'][1] == (_lib.SIGNATURES['a3d_crf_loss'][1][:-1] + [ctypes.c_void_p] +
                                                           _lib.SIGNATURES['a3d_crf_loss'][1][-1:])
    for words in ('NON-REFERENCE', 'A3D_EINVAL', 'SAME BITS', '+0.0', 'no atomics', 'A NaN stays'):
        assert words in text


def test_bad_arguments_are_refused_on_the_host():
    """These calls pass host pointers a launch would fault on: A3D_EINVAL must come first, and nothing is written."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.addressof(buf)

    def grad(n=2, nsp=48, z=p, y=p, r=p, left=p, right=p, npairs=48, per=p, mean=p, dz=p, dr=p):
        return lib.a3dp_crf_loss_grad(n, nsp, z, y, r, left, right, npairs, 1e-7, per, mean, dz, dr, None)
    for kw in ({'n': 0}, {'n': -1}, {'nsp': 0}, {'nsp': 65}, {'npairs': 0}, {'npairs': -2}, {'z': None}, {'y': None},
               {'r': None}, {'left': None}, {'right': None}, {'per': None}, {'mean': None}, {'dz': None}, {'dr': None}):
        assert grad(**kw) == -1, kw

    def bwd(n=2, npairs=48, k=2, sims=p, dr=p, dw=p, db=p):
        return lib.a3dp_pair_dense_bwd(n, npairs, k, sims, dr, dw, db, None)
    for kw in ({'k': 0}, {'k': 9}, {'k': -1}, {'n': 0}, {'n': -3}, {'npairs': 0}, {'npairs': -1}, {'sims': None},
               {'dr': None}, {'dw': None}, {'db': None}):
        assert bwd(**kw) == -1, kw

    assert lib.a3dp_sgd_apply_floor(4, None, p, 0.1, 0.0, None) == -1
    assert lib.a3dp_sgd_apply_floor(4, p, None, 0.1, 0.0, None) == -1
    assert lib.a3dp_sgd_apply_floor(0, p, p, 0.1, 0.0, None) == -1
    assert 'sgd_floor' in _lib.last_error()
    assert bytes(buf.raw) == bytes(1 << 12)                                     # nothing was written
