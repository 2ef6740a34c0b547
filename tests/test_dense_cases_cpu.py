"""tests/dense_cases.py held to ann3depth_amd/csrc/dense.hip, without a GPU: the kernels the table's rows expect are exactly
the instantiations the dispatch can launch — a new launch without a row fails here, and so does a row for a kernel that is
gone — and every integer-operand row keeps the headroom of tests/exact_ops.py."""
import os
import re

import numpy as np
import pytest

import dense_cases as D
import exact_ops as E

SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'ann3depth_amd', 'csrc', 'dense.hip')


def launched_instantiations(text):
    """every kernel instantiation dense.hip hands to a launch, spelled as the route line spells it (no blanks)"""
    text = re.sub(r'//[^\n]*', '', text)
    found = {f'dense_dw_adam_stream_kernel<{args}>' for args in re.findall(r'(?<!define )A3D_DW_STREAM\(([^)]*)\)', text)}
    found |= set(re.findall(r'hipLaunchKernelGGL\(\s*\(?\s*((?:dense_dw_adam_rows_kernel|dense_dw_kernel|dense_fwd_stream_kernel)<[^>]*>)', text))
    return {name.replace(' ', '') for name in found}


def dense_half_gradient(cs, dz):
    """the m a second Adam step would leave had it read a zero slot: (grad_scale x^T dz) / 2"""
    return 0.5 * D.GRAD_SCALE * (E.f64(cs.x).T @ E.f64(dz))


def test_the_table_names_exactly_the_kernels_dense_hip_can_launch():
    with open(SOURCE) as f:
        launched = launched_instantiations(f.read())
    expected = {row.route['kernel'] for row in D.ALL}
    assert launched == expected, f'launched without a row: {sorted(launched - expected)}; rows without a launch: {sorted(expected - launched)}'
    assert len(launched) == 10      # 2 forward, 2 plain, 2 rows and 4 stream forms
    assert len(D.ALL) == 32 and len({(r.entry, r.shape, r.precision) for r in D.ALL}) == 32      # a row leaves or arrives on purpose, with this count
    # ... and every row is run by some pytest case of the GPU file, the repeated and the poisoned ones among them
    grouped = [row for rows in D.GROUPS.values() for row in rows]
    assert all(row in grouped for row in D.ALL) and all(row in D.ALL for row in D.POISONED)
    assert {row.route['kernel'] for row in D.REPEATED} == {D.SLIM, D.WIDE, D.BF4, D.BF2}
    assert all(row.route['gpb'] >= 2 for row in D.REPEATED)
    # the poisoned gradient reaches every instantiation that holds the frozen-Adam rule
    assert all(row in D.POISONED for row in D.REPEATED) and len(D.POISONED) == len(D.REPEATED) + 3
    assert {row.route['kernel'] for row in D.POISONED} == {D.SLIM, D.WIDE, D.BF4, D.BF2, D.ROWS4, D.ROWS2, D.PLAIN_ADAM}


def test_the_collector_sees_a_launch_that_is_put_back():
    """the two launches this table's pull request deleted, and a new forward instantiation"""
    with open(SOURCE) as f:
        text = f.read()
    base = launched_instantiations(text)
    dead = text.replace('  else if (stream_ok && n % 2 == 0 && (slots & 7) == 0) A3D_DW_STREAM(2, 2);',
                        '  else if (stream_ok && m <= 32 && n % 4 == 0 && (slots & 15) == 0) A3D_DW_STREAM(4, 1);\n'
                        '  else if (stream_ok && n % 2 == 0 && (slots & 7) == 0) A3D_DW_STREAM(2, 2);')
    assert dead != text and launched_instantiations(dead) - base == {'dense_dw_adam_stream_kernel<4,1>'}
    more = text.replace('hipLaunchKernelGGL(dense_fwd_stream_kernel<2>,', 'hipLaunchKernelGGL(dense_fwd_stream_kernel<3>,')
    assert more != text and launched_instantiations(more) ^ base == {D.F2, 'dense_fwd_stream_kernel<3>'}


def test_the_rows_the_edges_ask_for_are_there():
    """the regimes the rows exist for, stated on the rows' own fields (shape and expected route)"""
    def rows(kernel, **want):
        return [r for r in D.ALL if r.route['kernel'] == kernel and all(r.route.get(f) == v for f, v in want.items())]
    for kernel, batch in ((D.F1, {1, 31, 32}), (D.F2, {33, 63, 64})):
        split = [r for r in rows(kernel) if r.route['splits'] > 1]
        assert batch <= {r.shape[0] for r in split}
        assert {0, 1, 127} <= {r.shape[2] % 128 for r in split} and any(r.shape[2] % 4 for r in split) and any(r.shape[1] % 64 for r in split)
        whole = rows(kernel, splits=1)
        assert any(r.shape[2] > 32768 and r.shape[1] > 64 for r in whole) and any(r.shape[1] <= 64 for r in whole)
    assert any(r.shape[1] == 4 for r in D.FORWARD_UNSPLIT)
    assert {r.route['splits'] > 1 for r in D.SIGMOID} == {True, False}
    plain = rows(D.PLAIN)
    assert {17, 33, 64} <= {r.shape[0] for r in plain} and {1, 127} <= {r.shape[2] % 128 for r in plain}
    assert all(r.shape[1] % 128 and r.shape[1] * r.shape[2] >= 1 << 16 for r in plain)
    for kernel in (D.SLIM, D.WIDE, D.BF4, D.BF2):
        assert rows(kernel, gpb=1), kernel
        multi = rows(kernel, gpb=2)
        assert multi, kernel
        for r in multi:      # a short last block, and a last group of fewer than 32 rows
            groups = -(-r.shape[1] // 32)
            assert r.route['grid'][1] == -(-groups // 2) and groups % 2 == 1 and r.shape[1] % 32
    assert {1, 31} <= {r.shape[0] for r in rows(D.SLIM)}
    for kernel in (D.ROWS4, D.ROWS2, D.PLAIN_ADAM):
        assert all(r.shape[1] % 32 and r.shape[2] % 512 and r.shape[0] in (1, 64) for r in rows(kernel)), kernel
    outside = rows(D.ROWS4) + rows(D.ROWS2) + rows(D.PLAIN_ADAM)
    assert any(r.shape[1] % 4 for r in outside) and any(r.align.get('x') == 4 for r in outside) and any(r.shape[2] % 2 for r in outside)


@pytest.mark.parametrize('row', D.ALL, ids=lambda r: f'{r.entry[4:]}-{"x".join(map(str, r.shape))}-{r.precision}')
def test_every_row_keeps_its_headroom(row):
    """exact_ops.dense_case asserts when it builds the case: integer references, the sum of absolute products (+ twice the bias:
    dropout) below 2^24 in each direction — exact in float32 in any order; ternary operands: exact in bf16"""
    m, k, n = row.shape
    cs = D.case(row)
    assert max(cs.mags) == 1 and max(E.amax(cs.x), E.amax(cs.w), E.amax(cs.dz)) <= 1 <= E.BF16_EXACT
    for a in (cs.x, cs.dz):
        assert np.array_equal(E.bf16_rne(a), a)
    if row.entry == D.FWD:
        assert k * n >= 1 << 20 and k % 4 == 0 and m <= 64
        for bias, act, drop in D.FORWARD_VARIANTS:
            ref = E.require_integers(cs.what, D.forward_reference(cs, bias, act, drop))
            assert E.amax(ref) < E.F32_EXACT
    elif row.entry == D.DW:
        assert E.amax(cs.dw) <= m and E.amax(cs.db) <= m
    else:
        steps = D.adam_steps(cs)
        assert len(steps) == 2 and not np.array_equal(steps[0][0], steps[1][0])
        # the second step moves much of m (one batch row: 4/9 of the ternary products are non-zero), and what it leaves depends on
        # the first step's m: a kernel that dropped the slot's old value, or the new gradient, differs
        assert (steps[1][3] != steps[0][3]).mean() > 0.25 and (steps[1][3] != dense_half_gradient(cs, steps[1][0])).mean() > 0.25
        if row in D.POISONED:
            w, b = D.poison_masks(cs)
            assert w.sum() > k and b.sum() == 2
    E.dense_case.cache_clear()
