"""The extension header include/a3d_posterior.h, the library's a3dc_* exports and _lib.POSTERIOR_SIGNATURES name the same
entry point, as the other tests/test_abi_*.py hold their headers; bad arguments are refused before any launch (no GPU
needed: the checks come first)."""
import ctypes

import abi_surface
from ann3depth_amd import _lib

NAMES = {'a3dc_crf_band_posterior'}


def test_posterior_header_exports_and_bindings_agree():
    text, code = abi_surface.check('a3dc_', NAMES)
    assert '#include "a3d_crf_band.h"' in code and '#define' not in code.replace('#define A3D_POSTERIOR_H_', '')
    # a3db_crf_band_nll's inputs (n .. npairs), then mean, var, nobs, status and the stream
    nll = _lib.CRF_BAND_SIGNATURES['a3db_crf_band_nll'][1]
    assert _lib.POSTERIOR_SIGNATURES['a3dc_crf_band_posterior'][1] == nll[:9] + [ctypes.c_void_p] * 5
    for words in ('NON-REFERENCE', 'A3D_EINVAL', '+0.0', 'status 1', 'The same bits on every run', 'no pivoting',
                  'no float atomics', 'no workspace', 'One launch', 'bit for bit', 'A3DB_MAX_SP', 'A3DB_MAX_BAND'):
        assert words in text, words


def test_bad_arguments_are_refused_on_the_host():
    """These calls pass host pointers a launch would fault on: A3D_EINVAL must come first, and nothing is written."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.addressof(buf)

    def post(n=2, nsp=192, band=16, z=p, y=p, r=p, left=p, right=p, npairs=280, mean=p, var=p, nobs=p, status=p):
        return lib.a3dc_crf_band_posterior(n, nsp, band, z, y, r, left, right, npairs, mean, var, nobs, status, None)
    for kw in ({'n': 0}, {'n': -1}, {'nsp': 0}, {'nsp': 769}, {'nsp': -3}, {'band': 0}, {'band': 33}, {'band': -1},
               {'npairs': 0}, {'npairs': -2}, {'z': None}, {'r': None}, {'left': None}, {'right': None}, {'mean': None},
               {'nobs': None}, {'status': None}, {'y': None, 'n': 0}, {'var': None, 'band': 33},
               {'y': None, 'var': None, 'nsp': 769}, {'y': None, 'mean': None}, {'var': None, 'status': None}):
        assert post(**kw) == -1, kw
    assert 'crf_band_posterior' in _lib.last_error()
    assert bytes(buf.raw) == bytes(1 << 12)                                     # nothing was written
