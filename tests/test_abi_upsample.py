"""The extension header include/a3d_upsample.h, the library's a3du_* exports and _lib.UPSAMPLE_SIGNATURES name the same
entry point, as tests/test_abi_fcsp.py and its siblings hold the other headers; bad arguments are refused before any
launch (no GPU needed: the checks come first)."""
import ctypes
import math
import re

import abi_surface
from ann3depth_amd import _lib, ops

NAMES = {'a3du_joint_bilateral_upsample'}


def test_upsample_header_exports_and_bindings_agree():
    text, code = abi_surface.check('a3du_', NAMES)
    cap = int(re.search(r'#define\s+A3DU_MAX_RADIUS\s+(\d+)\b', code).group(1))
    assert cap == ops.UPSAMPLE_MAX_RADIUS == 4
    for words in ('NON-REFERENCE', 'A3D_EINVAL', 'SKIPPED', 'ascending (i, j)', 'EVERY element', 'One IEEE division', 'LDS',
                  'No float atomics', 'BEFORE any conversion', 'e_min', 'fl(k / 255)', 'Nothing branches into'):
        assert words in text, words


def test_bad_arguments_are_refused_on_the_host():
    """These calls pass host pointers a launch would fault on: A3D_EINVAL must come first, and nothing is written."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.addressof(buf)

    def call(n=2, gh=3, gw=4, depth=p, H=7, W=9, guide=p, u8=0, cy=p, cx=p, ay=p, ax=p, radius=2, inv2ss=0.5, inv2sr=50.0,
             out=p):
        return lib.a3du_joint_bilateral_upsample(n, gh, gw, depth, H, W, guide, u8, cy, cx, ay, ax, radius, inv2ss, inv2sr,
                                                 out, None)
    bad = ([{k: v} for k in ('n', 'gh', 'gw', 'H', 'W') for v in (0, -1)]
           + [{'radius': r} for r in (0, -1, 5, 81)]
           + [{k: v} for k in ('inv2ss', 'inv2sr') for v in (-1.0, -1e-30, math.inf, -math.inf, math.nan)]
           + [{k: None} for k in ('depth', 'guide', 'cy', 'cx', 'ay', 'ax', 'out')]
           + [{'gh': (1 << 24) + 1}, {'n': 1 << 20, 'H': 1 << 10, 'W': 1 << 10}])
    for u8 in (0, 1):
        for kw in bad:
            assert call(u8=u8, **kw) == -1, kw
            assert 'joint_bilateral_upsample' in _lib.last_error()
    assert bytes(buf.raw) == bytes(1 << 12)                                     # nothing was written
