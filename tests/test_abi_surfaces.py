"""_lib.SURFACES is the whole C surface of liba3d.so: every header under include/ is the header of exactly one entry, no two
entries share a prefix or a name, what load() binds is what the entries list, and each entry passes the checks of
tests/abi_surface.py.  A surface forgotten in the list, or a name written into two dicts, fails here and not at a call."""
import glob
import os

import pytest

import abi_surface
from ann3depth_amd import _lib

IDS = [s.prefix for s in _lib.SURFACES]


@pytest.mark.parametrize('surface', _lib.SURFACES, ids=IDS)
def test_a_surface_shares_nothing_with_the_others(surface):
    abi_surface.check(surface.prefix, set(surface.signatures))
    for other in _lib.SURFACES:
        if other is not surface:
            assert other.prefix != surface.prefix and other.header != surface.header
            assert not set(surface.signatures) & set(other.signatures), other.prefix
            # neither reads the other's names as its own: a3dw_ and a3dwg_ are two prefixes, not one inside the other
            assert not any(n.startswith(surface.prefix) for n in other.signatures), other.prefix
            assert not abi_surface.declared(other) & set(surface.signatures), other.header


def test_the_list_is_the_headers_the_dicts_and_what_load_binds():
    headers = sorted(os.path.basename(h) for h in glob.glob(os.path.join(abi_surface.ROOT, 'include', 'a3d*.h')))
    assert headers == sorted(s.header for s in _lib.SURFACES) and len(set(headers)) == len(_lib.SURFACES)
    dicts = {k: v for k, v in vars(_lib).items() if k.endswith('SIGNATURES')}
    assert sorted(map(id, dicts.values())) == sorted(id(s.signatures) for s in _lib.SURFACES), sorted(dicts)
    listed = [n for s in _lib.SURFACES for n in s.signatures]
    assert len(listed) == len(set(listed))
    bound = {n for n, fn in vars(_lib.load()).items() if n.startswith('a3d') and fn.argtypes is not None}
    assert bound == set(listed)
    assert {n for n in abi_surface.exports() if n.startswith('a3d')} == set(listed)
