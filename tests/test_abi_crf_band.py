"""The extension header include/a3d_crf_band.h, the library's a3db_* exports and _lib.CRF_BAND_SIGNATURES name the same
entry points, as the other tests/test_abi_*.py hold their headers; bad arguments are refused before any launch (no GPU
needed: the checks come first)."""
import ctypes
import re

import abi_surface
from ann3depth_amd import _lib

NAMES = {'a3db_crf_band_nll', 'a3db_crf_band_map'}


def test_crf_band_header_exports_and_bindings_agree():
    text, code = abi_surface.check('a3db_', NAMES)
    # a3dv_crf_loss_observed's arguments with band after nsp and mu in the place of nobs
    obs = _lib.CRF_VALID_SIGNATURES['a3dv_crf_loss_observed'][1]
    assert _lib.CRF_BAND_SIGNATURES['a3db_crf_band_nll'][1] == obs[:2] + [ctypes.c_int] + obs[2:]
    # a3d_crf_map's with band after nsp
    m = _lib.SIGNATURES['a3d_crf_map'][1]
    assert _lib.CRF_BAND_SIGNATURES['a3db_crf_band_map'][1] == m[:2] + [ctypes.c_int] + m[2:]
    assert re.search(r'#define\s+A3DB_MAX_SP\s+768\b', code) and re.search(r'#define\s+A3DB_MAX_BAND\s+32\b', code)
    for words in ('NON-REFERENCE', 'A3D_EINVAL', '+0.0', 'status 1', 'The same bits on every run', 'no pivoting',
                  'no float atomics', 'band'):
        assert words in text, words


def test_bad_arguments_are_refused_on_the_host():
    """These calls pass host pointers a launch would fault on: A3D_EINVAL must come first, and nothing is written."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.addressof(buf)

    def nll(n=2, nsp=192, band=16, z=p, y=p, r=p, left=p, right=p, npairs=280, per=p, mean=p, dz=p, dr=p, mu=p, status=p):
        return lib.a3db_crf_band_nll(n, nsp, band, z, y, r, left, right, npairs, per, mean, dz, dr, mu, status, None)
    for kw in ({'n': 0}, {'n': -1}, {'nsp': 0}, {'nsp': 769}, {'nsp': -3}, {'band': 0}, {'band': 33}, {'band': -1},
               {'npairs': 0}, {'npairs': -2}, {'z': None}, {'y': None}, {'r': None}, {'left': None}, {'right': None},
               {'per': None}, {'mean': None}, {'dz': None}, {'status': None}, {'dr': None, 'n': 0}, {'mu': None, 'band': 33},
               {'dr': None, 'mu': None, 'nsp': 769}):
        assert nll(**kw) == -1, kw
    assert 'crf_band_nll' in _lib.last_error()

    def mp(n=2, nsp=768, band=32, z=p, r=p, left=p, right=p, npairs=280, mu=p, status=p):
        return lib.a3db_crf_band_map(n, nsp, band, z, r, left, right, npairs, mu, status, None)
    for kw in ({'n': 0}, {'n': -1}, {'nsp': 0}, {'nsp': 769}, {'band': 0}, {'band': 33}, {'npairs': 0}, {'z': None},
               {'r': None}, {'left': None}, {'right': None}, {'mu': None}, {'status': None}):
        assert mp(**kw) == -1, kw
    assert 'crf_band_map' in _lib.last_error()
    assert bytes(buf.raw) == bytes(1 << 12)                                     # nothing was written
