"""The extension header include/a3d_texture.h, the library's a3dt_* exports and _lib.TEXTURE_SIGNATURES name the same
entry points, as tests/test_abi.py, tests/test_abi_valid.py and tests/test_abi_pairwise.py hold the other three headers;
bad arguments are refused before any launch (no GPU needed: the checks come first)."""
import ctypes
import os
import re
import subprocess

from ann3depth_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {'a3dt_superpixel_lbp_hist', 'a3dt_pair_similarity3'}


def test_texture_header_exports_and_bindings_agree():
    lib = _lib.load()
    text = open(os.path.join(ROOT, 'include', 'a3d_texture.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    declared = set(re.findall(r'\b(a3dt_[a-z0-9_]+)\s*\(', code))
    assert declared == NAMES
    assert not re.findall(r'\ba3d[xp]?_[a-z0-9_]+\s*\(', code)              # nothing of the other three surfaces is declared here
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(re.findall(r' T (a3dt_[a-z0-9_]+)', out)) == declared == set(_lib.TEXTURE_SIGNATURES)
    others = set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES) | set(_lib.PAIR_SIGNATURES)
    assert not set(_lib.TEXTURE_SIGNATURES) & others
    for name in declared:
        assert getattr(lib, name).argtypes == _lib.TEXTURE_SIGNATURES[name][1]
        assert getattr(lib, name).restype == _lib.TEXTURE_SIGNATURES[name][0]
    # the siblings' arguments: a3d_superpixel_hist's own, and a3d_pair_similarity's plus lbp_hist after hist
    assert _lib.TEXTURE_SIGNATURES['a3dt_superpixel_lbp_hist'] == _lib.SIGNATURES['a3d_superpixel_hist']
    sim = _lib.SIGNATURES['a3d_pair_similarity'][1]
    assert _lib.TEXTURE_SIGNATURES['a3dt_pair_similarity3'][1] == sim[:6] + [ctypes.c_void_p] + sim[6:]
    for name in declared:                                                   # one argument of the C declaration per binding entry
        args = re.search(name + r'\s*\((.*?)\)\s*;', code, flags=re.S).group(1)
        assert len(args.split(',')) == len(_lib.TEXTURE_SIGNATURES[name][1]), name
    assert re.search(r'#define\s+A3DT_MAX_SP\s+53\b', code)
    for words in ('NON-REFERENCE', 'A3D_EINVAL', 'SAME BITS', 'clamped at the image border', '-0 >= +0', '2^24'):
        assert words in text


def test_bad_arguments_are_refused_on_the_host():
    """These calls pass host pointers a launch would fault on: A3D_EINVAL must come first, and nothing is written."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.addressof(buf)

    def lbp(n=2, h=80, w=120, x=p, sp=40, hist=p):
        return lib.a3dt_superpixel_lbp_hist(n, h, w, x, sp, hist, None)
    for kw in ({'n': 0}, {'n': -1}, {'h': 0}, {'h': -40}, {'w': 0}, {'w': -40}, {'sp': 0}, {'sp': -8}, {'h': 81}, {'w': 100},
               {'sp': 54, 'h': 108, 'w': 108}, {'sp': 64, 'h': 128, 'w': 128}, {'x': None}, {'hist': None}):
        assert lbp(**kw) == -1, kw
    assert 'superpixel_lbp_hist' in _lib.last_error()

    def sim(n=2, h=80, w=120, x=p, sp=40, hist=p, lbp_hist=p, left=p, right=p, npairs=4, dw=p, db=p, sims=p, r=p):
        return lib.a3dt_pair_similarity3(n, h, w, x, sp, hist, lbp_hist, left, right, npairs, dw, db, 1.0, sims, r, None)
    for kw in ({'n': 0}, {'n': -1}, {'h': 0}, {'w': 0}, {'sp': 0}, {'sp': -8}, {'h': 81}, {'w': 100},
               {'sp': 54, 'h': 108, 'w': 108}, {'npairs': 0}, {'npairs': -3}, {'x': None}, {'hist': None}, {'lbp_hist': None},
               {'left': None}, {'right': None}, {'dw': None}, {'db': None}, {'sims': None}, {'r': None}):
        assert sim(**kw) == -1, kw
    assert 'pair_similarity3' in _lib.last_error()
    assert bytes(buf.raw) == bytes(1 << 12)                                     # nothing was written
