"""Every kernel, tail and row-group walk of ann3depth_amd/csrc/dense.hip, element by element, each launch held to its own route line.

dense.hip's launches carry no timing record; which instantiation runs is decided by m, n % 4, n % 2, k % 4, pointer alignment and
precision (the fused filter gradient + ApplyAdam: seven launches), and by m, k and n again for the forward (two instantiations, a
split and an unsplit form).  The rows of tests/dense_cases.py state the route each of them expects, and tests/exact_dense_worker.py
— a child process with A3D_TUNING=1 A3D_PLAN_LOG=1 that reads its own stderr — fails a row whose `a3d dense:` line shows another
kernel, grid, split count, span or gpb, exactly as it fails a wrong element.  One child process per group of rows; the last test
asserts that the lines seen name every instantiation dense_cases lists (tests/test_dense_cases_cpu.py: all that dense.hip can
launch), both forms of the forward, gpb == 1 and gpb >= 2 with a short last block for each stream kernel.

Integer operands (exact_ops.dense_case): no tolerance anywhere but the two sigmoid rows, which are held to the float64 sigmoid of
the exact pre-activation within 8 x the largest error of the numpy float32 restatement 1 / (1 + exp(-s)) (at least one ulp of the
output).  Observed on the MI355X: see SIGMOID_OBSERVED below.

That the file bites was checked with mutated copies of dense.hip bound through A3D_LIB, one value changed per build and never an
index, a bound or a stride; each made the rows named here fail (MUTATIONS below)."""
import os
import subprocess
import sys

import pytest

import dense_cases as D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEN = {}            # group -> its ROUTE fields, as the worker printed them


def run_group(group):
    if group in SEEN:
        return SEEN[group]
    env = {k: v for k, v in os.environ.items() if not (k.startswith('A3D_') and k != 'A3D_LIB')}
    env.update(A3D_TUNING='1', A3D_PLAN_LOG='1')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'exact_dense_worker.py'), group], env=env, capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'MISMATCH' not in r.stdout, r.stdout[-3000:]
    done = [ln for ln in r.stdout.splitlines() if ln.startswith('verified ')]
    assert len(done) == 1 and int(done[0].split()[1]) == sum(D.launches(row) for row in D.GROUPS[group]), r.stdout[-2000:]
    SEEN[group] = [ln.split(' | ') for ln in r.stdout.splitlines() if ln.startswith('ROUTE |')]
    return SEEN[group]


@pytest.mark.parametrize('group', list(D.GROUPS))
def test_rows_are_exact_on_the_route_they_expect(group):
    routes = run_group(group)
    assert {r[5] for r in routes} == {row.route['kernel'] for row in D.GROUPS[group]}
    if any(D.is_sigmoid(row) for row in D.GROUPS[group]):
        assert any('act sigmoid' in r[4] for r in routes)
    for row in D.GROUPS[group]:
        mine = [r[4] for r in routes if r[2] == ' '.join(map(str, row.shape))]
        if row in D.REPEATED:
            assert 'three runs' in mine and 'poisoned gradient' in mine, mine
        if row in D.POISONED:
            assert 'poisoned gradient' in mine, mine


def test_every_instantiation_and_regime_was_shown_by_a_route_line():
    """a summary over the groups (a group the run has not been through yet is run here)"""
    routes = [r for group in D.GROUPS for r in run_group(group)]
    by_kernel = {}
    for _, entry, shape, precision, what, kernel, grid, extra, count in routes:
        by_kernel.setdefault(kernel, []).append((shape, extra, grid))
    for kernel in sorted(by_kernel):
        print(f'SHOWN | {kernel} | ' + '; '.join(sorted({f'({s}) {e} {g}'.strip() for s, e, g in by_kernel[kernel]})))
    assert set(by_kernel) == {row.route['kernel'] for row in D.ALL}
    for kernel in (D.F1, D.F2):          # both forms of the forward
        splits = {int(e.split()[1]) for _, e, _ in by_kernel[kernel]}
        assert 1 in splits and max(splits) > 1, (kernel, splits)
    for kernel in (D.SLIM, D.WIDE, D.BF4, D.BF2):
        gpbs = {int(e.split()[1]) for _, e, _ in by_kernel[kernel]}
        assert 1 in gpbs and max(gpbs) >= 2, (kernel, gpbs)
        short = [(s, e, g) for s, e, g in by_kernel[kernel] if int(e.split()[1]) >= 2 and
                 -(-int(s.split()[1]) // 32) % int(e.split()[1]) != 0]          # the last block walks fewer groups than the others
        assert short, kernel


# The sigmoid rows on the MI355X: (largest error of the float32 restatement, of the kernel, largest kernel error / bound).  A record,
# not a bound: the bound is computed from the restatement each run.
SIGMOID_OBSERVED = {
    (4, 64, 16384): (5.47e-08, 5.47e-08, 0.125),       # unsplit: expf in dense_fwd_stream_kernel; 13837 of 65536 differ from numpy's bits
    (33, 132, 8193): (5.47e-08, 5.47e-08, 0.125),      # 3 splits: the split-K reduction's; 59750 of 270369 differ
}

# Mutated copies of dense.hip (never committed), one value changed per build, and the rows each made fail; every other row passed.
MUTATIONS = {
    '`s * p.scale` without the scale in the unsplit epilogue':
        'forward-unsplit: the two dropout variants of all five rows, (4, 64, 16384) .. (64, 68, 32771)',
    'fmaxf(s, -1.f) for the ReLU of the unsplit epilogue':
        'forward-unsplit: the two ReLU variants of all five rows',
    'the fourth wave\'s partial tile left out of the sum at MB == 2':
        'every variant of (33, 132, 8193), (63, 260, 4223), (64, 128, 8200), (64, 256, 4096) and of the unsplit (33, 64, 16388), the '
        'split sigmoid row too; not (64, 68, 32771), whose fourth wave has no rows of W: its tile is zero',
    'the next group\'s m tile requested from the current group\'s row (rn = row_rsrc(g, r))':
        'step 2 of all six gpb == 2 rows, with and without bias slots, and the poisoned launch of the four REPEATED rows; no gpb == 1 '
        'row, and no step 1: beta1 = 0 leaves m = g whatever the slot held, which is why the second step has beta1 = 1/2',
    'gscale ignored in dense_dw_adam_stream_kernel<2, 2>':
        'step 1 of (48, 260, 518), (64, 1028, 4102), (33, 1028, 4100) and the poisoned launch of the last; no other instantiation',
}
