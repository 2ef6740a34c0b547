"""The extension header include/a3d_upsample.h, the library's a3du_* exports and _lib.UPSAMPLE_SIGNATURES name the same
entry point, as tests/test_abi_fcsp.py and its siblings hold the other headers; bad arguments are refused before any
launch (no GPU needed: the checks come first)."""
import ctypes
import math
import os
import re
import subprocess

from ann3depth_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {'a3du_joint_bilateral_upsample'}


def test_upsample_header_exports_and_bindings_agree():
    lib = _lib.load()
    text = open(os.path.join(ROOT, 'include', 'a3d_upsample.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    declared = set(re.findall(r'\b(a3du_[a-z0-9_]+)\s*\(', code))
    assert declared == NAMES
    assert not re.findall(r'\ba3d[a-z]?_[a-z0-9_]+\s*\(', re.sub(r'\ba3du_', 'u_', code))     # nothing of another surface
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(re.findall(r' T (a3du_[a-z0-9_]+)', out)) == declared == set(_lib.UPSAMPLE_SIGNATURES)
    others = (set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES) | set(_lib.PAIR_SIGNATURES) | set(_lib.TEXTURE_SIGNATURES)
              | set(_lib.GRADLOSS_SIGNATURES) | set(_lib.CRF_VALID_SIGNATURES) | set(_lib.FCSP_SIGNATURES)
              | set(_lib.CRF_BAND_SIGNATURES) | set(_lib.WINO_SIGNATURES))
    assert not set(_lib.UPSAMPLE_SIGNATURES) & others
    for name in declared:
        assert getattr(lib, name).argtypes == _lib.UPSAMPLE_SIGNATURES[name][1]
        assert getattr(lib, name).restype == _lib.UPSAMPLE_SIGNATURES[name][0]
        args = re.search(name + r'\s*\((.*?)\)\s*;', code, flags=re.S).group(1)   # one C argument per binding entry
        kinds = [ctypes.c_void_p if '*' in a else ctypes.c_float if a.split()[0] == 'float' else ctypes.c_int
                 for a in args.split(',')]
        assert kinds == _lib.UPSAMPLE_SIGNATURES[name][1], name
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
