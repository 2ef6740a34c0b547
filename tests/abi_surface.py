"""What every tests/test_abi*.py asks of its C surface, written once: the header under include/, the library's exports and the
binding's dict (_lib.SURFACES) name the same entry points with the same argument lists.  A plain helper module: each test
file passes its own literal set of names and keeps the checks that are its own (macros, workspace sizes, the words a header
must contain, the refusals)."""
import ctypes
import functools
import os
import re
import subprocess

from ann3depth_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {'a3d_conv_desc': _lib.ConvDesc, 'a3dwb_pool': _lib.WinoBwdPool, 'a3d_second_output': _lib.SecondOutput,
           'a3d_example_view': _lib.ExampleView, 'a3d_timing_record': _lib.TimingRecord}
SCALARS = {'int': ctypes.c_int, 'float': ctypes.c_float, 'size_t': ctypes.c_size_t, 'uint64_t': ctypes.c_uint64}
TYPED = {'char': ctypes.c_char_p, 'size_t': ctypes.POINTER(ctypes.c_size_t), 'int': ctypes.POINTER(ctypes.c_int),
         'int32_t': ctypes.POINTER(ctypes.c_int32), 'int64_t': ctypes.POINTER(ctypes.c_int64)}


@functools.lru_cache(maxsize=None)
def exports():
    """Every function liba3d.so defines and exports."""
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    return frozenset(re.findall(r' T (\w+)', out))


def header(surface):
    """(text, text without comments) of a surface's header."""
    text = open(os.path.join(ROOT, 'include', surface.header)).read()
    return text, re.sub(r'/\*.*?\*/', '', text, flags=re.S)


def declared(surface):
    """Every function name the header declares, of whichever surface's prefix."""
    return set(re.findall(r'\b(a3d[a-z]*_[a-z0-9_]+)\s*\(', header(surface)[1]))


def kinds(param):
    """The ctypes types a C parameter may be bound as: one for a scalar, a descriptor pointer or a pointer to floats, bytes
    or void; a pointer to integers may also be typed.  None for a parameter this module does not read (the function's kinds
    then go unchecked, its argument count does not)."""
    words = [w for w in param.replace('*', ' * ').split() if w != 'const']
    if words.count('*') == 1:
        if words[0] in STRUCTS:
            return (ctypes.POINTER(STRUCTS[words[0]]),)
        return (ctypes.c_void_p,) + ((TYPED[words[0]],) if words[0] in TYPED else ())
    return (SCALARS[words[0]],) if len(words) == 2 and words[0] in SCALARS else None


def check(prefix, names):
    """The surface of this prefix declares, exports and binds exactly `names`; returns its header's (text, code)."""
    surface, = [s for s in _lib.SURFACES if s.prefix == prefix]
    lib = _lib.load()
    text, code = header(surface)
    assert declared(surface) == set(names) == set(surface.signatures)           # nothing of another surface's prefix either
    assert all(n.startswith(prefix) for n in names)
    assert {n for n in exports() if n.startswith(prefix)} == set(names)
    for name in names:
        res, args = surface.signatures[name]
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == res, name
        params = re.search(r'\b' + name + r'\s*\((.*?)\)\s*;', code, flags=re.S).group(1).strip()
        may = [] if params in ('', 'void') else [kinds(p) for p in params.split(',')]
        assert len(may) == len(args), name                                         # one C argument per binding entry
        if None not in may:
            assert all(a in k for a, k in zip(args, may)), name
    return text, code
