"""The extension header include/a3d_texture.h, the library's a3dt_* exports and _lib.TEXTURE_SIGNATURES name the same
entry points, as tests/test_abi.py, tests/test_abi_valid.py and tests/test_abi_pairwise.py hold the other three headers;
bad arguments are refused before any launch (no GPU needed: the checks come first)."""
import ctypes
import re

import abi_surface
from ann3depth_amd import _lib

NAMES = {'a3dt_superpixel_lbp_hist', 'a3dt_pair_similarity3'}


def test_texture_header_exports_and_bindings_agree():
    text, code = abi_surface.check('a3dt_', NAMES)
    # the siblings' arguments: a3d_superpixel_hist's own, and a3d_pair_similarity's plus lbp_hist after hist
    assert _lib.TEXTURE_SIGNATURES['a3dt_superpixel_lbp_hist'] == _lib.SIGNATURES['a3d_superpixel_hist']
    sim = _lib.SIGNATURES['a3d_pair_similarity'][1]
    assert _lib.TEXTURE_SIGNATURES['a3dt_pair_similarity3'][1] == sim[:6] + [ctypes.c_void_p] + sim[6:]
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
