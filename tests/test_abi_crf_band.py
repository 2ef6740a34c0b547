"""The extension header include/a3d_crf_band.h, the library's a3db_* exports and _lib.CRF_BAND_SIGNATURES name the same
entry points, as the other tests/test_abi_*.py hold their headers; bad arguments are refused before any launch (no GPU
needed: the checks come first)."""
import ctypes
import os
import re
import subprocess

from ann3depth_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {'a3db_crf_band_nll', 'a3db_crf_band_map'}


def test_crf_band_header_exports_and_bindings_agree():
    lib = _lib.load()
    text = open(os.path.join(ROOT, 'include', 'a3d_crf_band.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    declared = set(re.findall(r'\b(a3db_[a-z0-9_]+)\s*\(', code))
    assert declared == NAMES
    assert not re.findall(r'\ba3d[a-z]?_[a-z0-9_]+\s*\(', re.sub(r'\ba3db_', 'b_', code))     # nothing of another surface
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(re.findall(r' T (a3db_[a-z0-9_]+)', out)) == declared == set(_lib.CRF_BAND_SIGNATURES)
    others = (set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES) | set(_lib.PAIR_SIGNATURES) | set(_lib.TEXTURE_SIGNATURES)
              | set(_lib.GRADLOSS_SIGNATURES) | set(_lib.CRF_VALID_SIGNATURES) | set(_lib.FCSP_SIGNATURES))
    assert not set(_lib.CRF_BAND_SIGNATURES) & others
    for name in declared:
        assert getattr(lib, name).argtypes == _lib.CRF_BAND_SIGNATURES[name][1]
        assert getattr(lib, name).restype == _lib.CRF_BAND_SIGNATURES[name][0]
        args = re.search(name + r'\s*\((.*?)\)\s*;', code, flags=re.S).group(1)
        assert len(args.split(',')) == len(_lib.CRF_BAND_SIGNATURES[name][1]), name
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
