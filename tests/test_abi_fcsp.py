"""The extension header include/a3d_fcsp.h, the library's a3df_* exports and _lib.FCSP_SIGNATURES name the same entry
points, as tests/test_abi_texture.py and its siblings hold the other headers; bad arguments are refused before any launch
(no GPU needed: the checks come first)."""
import ctypes
import re

import abi_surface
from ann3depth_amd import _lib, ops

NAMES = {'a3df_superpixel_pool_fwd', 'a3df_superpixel_pool_bwd'}


def test_fcsp_header_exports_and_bindings_agree():
    text, code = abi_surface.check('a3df_', NAMES)
    assert _lib.FCSP_SIGNATURES['a3df_superpixel_pool_fwd'] == _lib.FCSP_SIGNATURES['a3df_superpixel_pool_bwd']
    cap = int(re.search(r'#define\s+A3DF_MAX_SP\s+(\d+)\b', code).group(1))
    assert cap >= 40 and cap == ops.FCSP_MAX_SP
    for words in ('NON-REFERENCE', 'A3D_EINVAL', 'SKIPPED', 'ascending (i, j)', 'EVERY element', 'One IEEE division', 'LDS'):
        assert words in text


def test_bad_arguments_are_refused_on_the_host():
    """These calls pass host pointers a launch would fault on: A3D_EINVAL must come first, and nothing is written."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.addressof(buf)
    cap = ops.FCSP_MAX_SP

    def call(fn, n=2, h=4, w=9, C=8, a=p, ld=8, H=80, W=120, sp=40, ymap=p, xmap=p, b=p, ldp=8):
        if fn == 'fwd':
            return lib.a3df_superpixel_pool_fwd(n, h, w, C, a, ld, H, W, sp, ymap, xmap, b, ldp, None)
        return lib.a3df_superpixel_pool_bwd(n, h, w, C, b, ldp, H, W, sp, ymap, xmap, a, ld, None)
    bad = ([{k: v} for k in ('n', 'h', 'w', 'C', 'H', 'W', 'sp') for v in (0, -1)]
           + [{'a': None}, {'b': None}, {'ymap': None}, {'xmap': None},
              {'H': 81}, {'W': 100}, {'H': 40, 'W': 60}, {'ld': 7}, {'ldp': 7}, {'C': 9}, {'ld': 0}, {'ldp': -8},
              {'sp': cap + 1, 'H': 2 * (cap + 1), 'W': cap + 1}, {'sp': 2 * cap, 'H': 2 * cap, 'W': 2 * cap}])
    for fn in ('fwd', 'bwd'):
        for kw in bad:
            assert call(fn, **kw) == -1, (fn, kw)
        assert 'superpixel_pool_' + fn in _lib.last_error()
    assert bytes(buf.raw) == bytes(1 << 12)                                     # nothing was written
