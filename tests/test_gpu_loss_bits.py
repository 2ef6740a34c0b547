"""The four loss objectives against tests/golden/loss_bits.json, the bits they gave at the commit that file names: every loss
word, every per-sample workspace word, the ticket, and the digests of dout and of its bf16 copy with the pitch columns.  The
inputs and the launches are tests/golden/make_loss_bits.py's, which wrote the file; a kernel change that promises "same
bits" passes this file unchanged, one that changes a sum's order regenerates it on purpose."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
_spec = importlib.util.spec_from_file_location('make_loss_bits', os.path.join(GOLDEN, 'make_loss_bits.py'))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)
RECORDED = json.load(open(G.FIXTURE))
WORDS = ('loss', 'ws', 'ticket', 'dout_sha256', 'dout16_sha256')


def test_the_fixture_holds_every_case():
    """No case of the generator is missing from the file or changed in it, and the file names its commit."""
    assert [{k: v for k, v in c.items() if k not in WORDS} for c in RECORDED['cases']] == G.cases()
    assert len(RECORDED['commit']) == 40 and int(RECORDED['commit'], 16) >= 0
    assert all(c['ticket'] == '00000000' for c in RECORDED['cases'])


@pytest.mark.parametrize('case', RECORDED['cases'], ids=[c['id'] for c in RECORDED['cases']])
def test_same_bits_as_recorded(case):
    from ann3depth_amd import ops
    got = G.measure(ops, case)
    for k in WORDS:
        assert got[k] == case[k], f'{case["id"]}: {k} differs from commit {RECORDED["commit"][:7]}'
