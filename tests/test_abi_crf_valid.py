"""The extension header include/a3d_crf_valid.h, the library's a3dv_* exports and _lib.CRF_VALID_SIGNATURES name the same
entry points, as the other tests/test_abi_*.py hold their headers; bad arguments are refused before any launch (no GPU
needed: the checks come first)."""
import ctypes

import abi_surface
from ann3depth_amd import _lib

NAMES = {'a3dv_superpixel_mean_valid', 'a3dv_crf_loss_observed'}


def test_crf_valid_header_exports_and_bindings_agree():
    text, code = abi_surface.check('a3dv_', NAMES)
    # a3d_crf_loss's arguments without eps, plus dr, nobs and status
    base = _lib.SIGNATURES['a3d_crf_loss'][1]
    assert _lib.CRF_VALID_SIGNATURES['a3dv_crf_loss_observed'][1] == base[:8] + base[9:12] + [ctypes.c_void_p] * 3 + base[-1:]
    for words in ('NON-REFERENCE', 'A3D_EINVAL', 'm = 0', '+0.0', 'status 1', 'The same bits on every run', 'Pivot rule',
                  'min_count'):
        assert words in text, words


def test_bad_arguments_are_refused_on_the_host():
    """These calls pass host pointers a launch would fault on: A3D_EINVAL must come first, and nothing is written."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.addressof(buf)

    def loss(n=2, nsp=48, z=p, y=p, r=p, left=p, right=p, npairs=48, per=p, mean=p, dz=p, dr=p, nobs=p, status=p):
        return lib.a3dv_crf_loss_observed(n, nsp, z, y, r, left, right, npairs, per, mean, dz, dr, nobs, status, None)
    for kw in ({'n': 0}, {'n': -1}, {'nsp': 0}, {'nsp': 65}, {'nsp': -3}, {'npairs': 0}, {'npairs': -2}, {'z': None},
               {'y': None}, {'r': None}, {'left': None}, {'right': None}, {'per': None}, {'mean': None}, {'dz': None},
               {'nobs': None}, {'status': None}, {'dr': None, 'n': 0}):
        assert loss(**kw) == -1, kw
    assert 'crf_loss_observed' in _lib.last_error()

    def mean(n=1, h=80, w=120, x=p, sp=40, min_count=0, y=p, count=p):
        return lib.a3dv_superpixel_mean_valid(n, h, w, x, sp, min_count, y, count, None)
    for kw in ({'n': 0}, {'n': -1}, {'sp': 0}, {'sp': -40}, {'h': 81}, {'w': 100}, {'h': 0}, {'w': 0}, {'min_count': -1},
               {'x': None}, {'y': None}):
        assert mean(**kw) == -1, kw
    assert 'superpixel_mean_valid' in _lib.last_error()
    assert bytes(buf.raw) == bytes(1 << 12)                                     # nothing was written
