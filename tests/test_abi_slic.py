"""The extension header include/a3d_slic.h, the library's a3ds_* exports and _lib.SLIC_SIGNATURES name the same entry
points, as tests/test_abi_fcsp.py and its siblings hold the other headers; bad arguments are refused before any launch (no
GPU needed: the checks come first)."""
import ctypes
import re

import abi_surface
from ann3depth_amd import _lib, ops

NAMES = {'a3ds_label_mean', 'a3ds_label_hist', 'a3ds_slic_update', 'a3ds_slic_assign', 'a3ds_slic_segment',
         'a3ds_pair_similarity', 'a3ds_label_pool_fwd', 'a3ds_label_pool_bwd'}


def test_slic_header_exports_and_bindings_agree():
    text, code = abi_surface.check('a3ds_', NAMES)
    assert _lib.SLIC_SIGNATURES['a3ds_label_pool_fwd'] == _lib.SLIC_SIGNATURES['a3ds_label_pool_bwd']
    for macro, value in (('A3DS_MAX_SP', ops.SLIC_MAX_SP), ('A3DS_MAX_CELLS', ops.SLIC_MAX_CELLS),
                         ('A3DS_MAX_SUPERPIXELS', ops.SLIC_MAX_SUPERPIXELS)):
        assert int(re.search(r'#define\s+' + macro + r'\s+(\d+)\b', code).group(1)) == value
    assert ops.SLIC_MAX_SP >= 40 and ops.SLIC_MAX_CELLS >= 24 * 34 and ops.SLIC_MAX_SUPERPIXELS >= 24 * 32
    for words in ('NON-REFERENCE', 'A3D_EINVAL', 'LABEL CONTRACT', 'ANCHOR', 'SKIPPED', 'EVERY element', 'One IEEE division',
                  'ties going to the lowest index', 'used as an index', 'LDS'):
        assert words in text, words


def test_bad_arguments_are_refused_on_the_host():
    """These calls pass host pointers a launch would fault on: A3D_EINVAL must come first, and nothing is written."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.addressof(buf)
    cap = ops.SLIC_MAX_SP
    geometry = ([{k: v} for k in ('n', 'H', 'W', 'sp') for v in (0, -1)]
                + [{'H': 81}, {'W': 100}, {'H': 40, 'W': 60}, {'sp': cap + 1, 'H': 2 * (cap + 1), 'W': cap + 1},
                   {'n': 1 << 16, 'H': 1 << 8, 'W': 1 << 8, 'sp': 1 << 4}])            # 2^32 pixels
    inexact = [{'H': 64, 'W': 512, 'sp': 64}, {'H': 40 * 1200, 'W': 40, 'sp': 40}]       # 9 sp^2 max(H, W) >= 2^24

    def image(fn, n=2, H=80, W=120, sp=40, c=3, x=p, labels=p, out=p, count=p, iters=2, compactness=0.1):
        if fn == 'label_mean':
            return lib.a3ds_label_mean(n, H, W, c, x, sp, labels, out, count, None)
        if fn == 'label_hist':
            return lib.a3ds_label_hist(n, H, W, x, sp, labels, out, None)
        if fn == 'slic_update':
            return lib.a3ds_slic_update(n, H, W, x, sp, labels, out, count, None)
        if fn == 'slic_assign':
            return lib.a3ds_slic_assign(n, H, W, x, sp, out, compactness, labels, None)
        return lib.a3ds_slic_segment(n, H, W, x, sp, iters, compactness, labels, out, count, None)
    for fn in ('label_mean', 'label_hist', 'slic_update', 'slic_assign', 'slic_segment'):
        bad = geometry + [{'x': None}, {'labels': None}, {'out': None}]
        if fn not in ('label_hist', 'slic_assign'):
            bad.append({'count': None})
        if fn == 'label_mean':
            bad += [{'c': 0}, {'c': 5}, {'c': -1}]
        if fn.startswith('slic'):
            bad += inexact
        if fn in ('slic_assign', 'slic_segment'):
            bad += [{'compactness': -0.5}, {'compactness': float('nan')}, {'compactness': float('inf')}]
        if fn == 'slic_segment':
            bad.append({'iters': -1})
        for kw in bad:
            assert image(fn, **kw) == -1, (fn, kw)
            assert fn in _lib.last_error(), (fn, kw, _lib.last_error())
    for fn in ('label_mean', 'label_hist'):                                    # no coordinate means: not refused for these
        image(fn, x=None, **inexact[0])
        assert 'NULL' in _lib.last_error()
    assert image('slic_update', **inexact[0]) == -1 and '2^24' in _lib.last_error()
    assert image('label_mean', sp=cap + 1, H=cap + 1, W=cap + 1) == -1 and 'A3DS_MAX_SP' in _lib.last_error()

    def pairs(n=2, S=6, npairs=7, mean3=p, hist=p, count=p, left=p, right=p, dw=p, db=p, sims=p, r=p):
        return lib.a3ds_pair_similarity(n, S, mean3, hist, count, left, right, npairs, dw, db, 1.0, sims, r, None)
    for kw in ([{k: v} for k in ('n', 'S', 'npairs') for v in (0, -1)] + [{'n': 1 << 16, 'npairs': 1 << 16}]
               + [{k: None} for k in ('mean3', 'hist', 'count', 'left', 'right', 'dw', 'db', 'sims', 'r')]):
        assert pairs(**kw) == -1, kw
        assert 'pair_similarity' in _lib.last_error()

    def pool(fn, n=2, h=4, w=9, C=8, a=p, ld=8, H=80, W=120, sp=40, ymap=p, xmap=p, labels=p, count=p, b=p, ldp=8):
        if fn == 'fwd':
            return lib.a3ds_label_pool_fwd(n, h, w, C, a, ld, H, W, sp, ymap, xmap, labels, count, b, ldp, None)
        return lib.a3ds_label_pool_bwd(n, h, w, C, b, ldp, H, W, sp, ymap, xmap, labels, count, a, ld, None)
    bad = (geometry + [{k: v} for k in ('h', 'w', 'C') for v in (0, -1)]
           + [{k: None} for k in ('a', 'b', 'ymap', 'xmap', 'labels', 'count')]
           + [{'ld': 7}, {'ldp': 7}, {'C': 9}, {'ld': 0}, {'ldp': -8}, {'h': 64, 'w': 65}, {'h': 1, 'w': 4097},
              {'H': 10 * 24, 'W': 10 * 33, 'sp': 10}])                                    # 792 superpixels
    for fn in ('fwd', 'bwd'):
        for kw in bad:
            assert pool(fn, **kw) == -1, (fn, kw)
            assert 'label_pool_' + fn in _lib.last_error()
        assert pool(fn, h=64, w=65) == -1 and 'A3DS_MAX_CELLS' in _lib.last_error()
        assert pool(fn, H=240, W=330, sp=10) == -1 and 'A3DS_MAX_SUPERPIXELS' in _lib.last_error()
    assert bytes(buf.raw) == bytes(1 << 12)                                     # nothing was written
