"""The extension header include/a3d_crf_valid.h, the library's a3dv_* exports and _lib.CRF_VALID_SIGNATURES name the same
entry points, as the other tests/test_abi_*.py hold their headers; bad arguments are refused before any launch (no GPU
needed: the checks come first)."""
import ctypes
import os
import re
import subprocess

from ann3depth_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {'a3dv_superpixel_mean_valid', 'a3dv_crf_loss_observed'}


def test_crf_valid_header_exports_and_bindings_agree():
    lib = _lib.load()
    text = open(os.path.join(ROOT, 'include', 'a3d_crf_valid.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    declared = set(re.findall(r'\b(a3dv_[a-z0-9_]+)\s*\(', code))
    assert declared == NAMES
    assert not re.findall(r'\ba3d[a-z]?_[a-z0-9_]+\s*\(', re.sub(r'\ba3dv_', 'v_', code))     # nothing of another surface
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(re.findall(r' T (a3dv_[a-z0-9_]+)', out)) == declared == set(_lib.CRF_VALID_SIGNATURES)
    others = (set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES) | set(_lib.PAIR_SIGNATURES) | set(_lib.TEXTURE_SIGNATURES)
              | set(_lib.GRADLOSS_SIGNATURES))
    assert not set(_lib.CRF_VALID_SIGNATURES) & others
    for name in declared:
        assert getattr(lib, name).argtypes == _lib.CRF_VALID_SIGNATURES[name][1]
        assert getattr(lib, name).restype == _lib.CRF_VALID_SIGNATURES[name][0]
        args = re.search(name + r'\s*\((.*?)\)\s*;', code, flags=re.S).group(1)
        assert len(args.split(',')) == len(_lib.CRF_VALID_SIGNATURES[name][1]), name
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
