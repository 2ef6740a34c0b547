"""The planner's answers, pinned.  The six *_ws_bytes queries run the tile / split-K planner on the host, so their values
over a sweep of layer shapes show split factors, stream-K grids and the measured-winner table; every value must equal the
one recorded in tests/golden/plan_table.json.

The fixture is a RECORD of a known-good library, never of the code under test: a change that means to alter a plan
records it again from the build it was reviewed against and shows the difference,

    A3D_LIB=/path/to/known-good/liba3d.so python tests/test_plan_table_cpu.py --record

Each setting runs in a process of its own: the tuning gate (A3D_TUNING) is read once per process."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'plan_table.json')

# the planner as shipped, then one forced branch each (all behind A3D_TUNING=1)
SETTINGS = {
    'default': {},
    'cfg4_splitk3': {'A3D_FORCE_CFG': '4', 'A3D_FORCE_SPLITK': '3'},
    'cfg7_streamk100': {'A3D_FORCE_CFG': '7', 'A3D_FORCE_STREAMK': '100'},
    'cfg10': {'A3D_FORCE_CFG': '10'},
    'bf16_bn64': {'A3D_BF16_BN': '64'},
    'ring_off': {'A3D_RING': '0'},
    'ring_cfg3': {'A3D_RING_CFG': '3'},
}
BATCHES = (1, 2, 3, 4, 8, 16, 32, 64, 128)
X, W, Y = 1, 2, 4                                   # a3d_conv_desc.storage bits
VARIANTS = (('fp32', 0), ('bf16x3', 0), ('bf16', 0), ('bf16', X | W | Y), ('bf16', X | Y), ('bf16', Y))


def conv_cases():
    """(n, h, w, c, k, r, s, stride, padding, ldx, precision, storage)"""
    msdn = [(228, 304, 3, 96, 11, 11, 4, 'VALID', None), (27, 37, 96, 256, 5, 5, 1, 'SAME', None),
            (13, 18, 256, 384, 3, 3, 1, 'SAME', None), (13, 18, 384, 384, 3, 3, 1, 'SAME', None),
            (13, 18, 384, 256, 3, 3, 2, 'VALID', None), (228, 304, 3, 63, 9, 9, 2, 'VALID', None),
            (55, 74, 64, 64, 5, 5, 1, 'SAME', 64), (55, 74, 64, 1, 5, 5, 1, 'SAME', None)]      # as tests/test_abi.py
    odd = [(9, 11, 5, 7, 3, 3, 1, 'SAME', None), (17, 16, 32, 40, 3, 3, 2, 'SAME', None)]
    shapes = [(b,) + s for s in msdn + odd for b in BATCHES]
    h = 100                                          # the DCNF chain (models.DCNF_CONVS) over 768 patches
    for name, ci, co, k in (('conv2d', 3, 64, 11), ('conv2d_1', 64, 256, 5), ('conv2d_2', 256, 256, 3),
                            ('conv2d_3', 256, 256, 3), ('conv2d_4', 256, 256, 3)):
        shapes.append((768, h, h, ci, co, k, k, 1, 'VALID', None))
        h = h - k + 1
        if name in ('conv2d', 'conv2d_1', 'conv2d_4'):
            h //= 2
    cases = [s + v for s in shapes for v in VARIANTS]
    # dense_1 as a 1x1 conv on bf16 tensors: the LDS-DMA kernel's 64-row weight stream, the one split that is not clamped
    cases += [(b, 1, 1, 12288, 4096, 1, 1, 1, 'VALID', None, 'bf16', X | W | Y) for b in BATCHES]
    return cases


def dense_cases():
    """(m, k, n)"""
    return [(m, k, n) for m in (1, 2, 16, 32, 64, 65, 128, 768)
            for k, n in ((12288, 4096), (4096, 4070), (12544, 128), (128, 16), (16, 1), (100, 36))]


def cases_digest():
    return hashlib.sha256(repr((conv_cases(), dense_cases())).encode()).hexdigest()


def plan_table():
    """Every query of every case, in case order, from the library this process loads (A3D_LIB or the tree's)."""
    sys.path.insert(0, ROOT)
    from ann3depth_amd import _lib, ops
    lib = _lib.load()
    out = []
    for c in conv_cases():
        d = ops.conv_desc(*c[:9], ldx=c[9], precision=c[10], storage=c[11])
        out += [int(fn(ctypes.byref(d))) for fn in (lib.a3d_conv2d_fwd_ws_bytes, lib.a3d_conv2d_bwd_data_ws_bytes,
                                                    lib.a3d_conv2d_bwd_filter_ws_bytes)]
    for m, k, n in dense_cases():
        out += [int(fn(m, k, n)) for fn in (lib.a3d_dense_fwd_ws_bytes, lib.a3d_dense_bwd_data_ws_bytes,
                                            lib.a3d_dense_bwd_filter_ws_bytes)]
    return out


def start_child(setting):
    env = {k: v for k, v in os.environ.items() if not (k.startswith('A3D_') and k != 'A3D_LIB')}
    if SETTINGS[setting]:
        env.update(SETTINGS[setting], A3D_TUNING='1')
    return subprocess.Popen([sys.executable, os.path.abspath(__file__), '--print'], env=env, stdout=subprocess.PIPE, text=True)


def all_tables():
    children = {s: start_child(s) for s in SETTINGS}                 # side by side: each spends its time importing
    tables = {}
    for s, child in children.items():
        out, _ = child.communicate()
        assert child.returncode == 0, f'the {s} child failed'
        tables[s] = json.loads(out)
    return tables


def record():
    tables = all_tables()
    values = sorted({v for t in tables.values() for v in t})         # few distinct values: the tables index into them
    index = {v: i for i, v in enumerate(values)}
    with open(FIXTURE, 'w') as f:
        json.dump({'cases': cases_digest(), 'values': values, 'tables': {s: [index[v] for v in t] for s, t in tables.items()}}, f,
                  separators=(',', ':'))
    for s, t in tables.items():
        print(f'{s}: {len(t)} values, {sum(v != 0 for v in t)} non-zero, {len(set(t))} distinct')


@pytest.fixture(scope='module')
def tables():
    return all_tables()


@pytest.fixture(scope='module')
def recorded():
    with open(FIXTURE) as f:
        fx = json.load(f)
    assert fx['cases'] == cases_digest(), 'the case list changed: record the fixture again from a known-good library'
    return {s: [fx['values'][i] for i in t] for s, t in fx['tables'].items()}


def test_the_sweep_is_the_one_that_was_recorded(recorded):
    n = 3 * (len(conv_cases()) + len(dense_cases()))
    assert set(recorded) == set(SETTINGS) and all(len(t) == n for t in recorded.values())
    # the sweep sees the planner: most answers are real slabs, and every forced branch answers differently
    assert sum(v != 0 for v in recorded['default']) > n // 2
    assert len({tuple(t) for t in recorded.values()}) == len(SETTINGS)


@pytest.mark.parametrize('setting', list(SETTINGS))
def test_every_plan_is_the_recorded_one(setting, tables, recorded):
    got, want = tables[setting], recorded[setting]
    assert len(got) == len(want)
    names = ('fwd', 'bwd_data', 'bwd_filter')
    rows = conv_cases() + dense_cases()
    wrong = [(rows[i // 3], names[i % 3], want[i], got[i]) for i in range(len(want)) if got[i] != want[i]]
    assert not wrong, f'{len(wrong)} of {len(want)} workspace answers differ (case, query, recorded, now): {wrong[:5]}'


if __name__ == '__main__':
    if sys.argv[1:] == ['--print']:
        print(json.dumps(plan_table()))
    elif sys.argv[1:] == ['--record']:
        record()
    else:
        sys.exit('usage: test_plan_table_cpu.py --record | --print')
