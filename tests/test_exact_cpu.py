"""The exact-integer cases of test_gpu_exact.py / exact_forced_worker.py, built on the CPU: building a case asserts the
conditions under which equality with a float32 / bf16 kernel is legitimate (integer reference, 2^24 headroom on the sum of
absolute products, bf16-stored outputs <= 256; tests/exact_ops.py), so they are checked here without a GPU.

And the gap those tests close, on the references themselves: a tensor with ONE element zeroed, or one product missing from one
element, passes the suite's relative-L2 criterion (tests/test_gpu_ops.py: rel_l2 < RTOL_F32 for float32 outputs, < 4e-3 for
bf16 outputs) and fails element-by-element equality.  Likewise for the rounding cases of test_gpu_exact_rounding.py: bf16_rne
against torch's conversion, the conditions of every rounded-store, pool-tie, wide-operand and bf16x3 case, and a truncating
and a round-half-away store, both of which pass rel_l2 < 4e-3 and fail equality."""
import numpy as np
import pytest

import exact_ops as E
from oracle import tf13_ops as T
from test_gpu_ops import RTOL_F32, rel_l2


RTOL_BF16_OUT = 4e-3     # test_gpu_ops.py's tolerance for an output rounded to bf16


@pytest.mark.parametrize('case', E.GENERIC + E.STRIDED_ONE_LAUNCH + E.FEW_CHANNEL + E.FORCED_F32 + [E.FORCED_STRIDED, E.WIDE])
def test_conv_cases_are_exact_in_float32(case):
    E.conv_case(*case)


@pytest.mark.parametrize('case', E.GUARD)
def test_guard_cases_are_exact_in_float32(case):
    n, h, w, c, k, ks, ld = case
    E.conv_case(n, h, w, c, k, ks, 1, 'SAME')


@pytest.mark.parametrize('case', [c for c in E.BF16_ARITH if E.stores_bf16(c)] + E.RING + E.FORCED_F32 + E.POOL_FWD_BF16_STORED
                         + [E.RING_FWD[0], E.RING_BWD_D_96[0], E.RING_BWD_F[0]])
def test_conv_cases_with_bf16_tensors_stay_within_256(case):
    E.conv_case(*case).bf16('y', 'dx')


@pytest.mark.parametrize('case', E.STRIDED_ONE_LAUNCH_BF16)
def test_strided_bwd_data_cases_on_bf16_tensors(case):
    E.conv_case(*case).bf16('dx')


@pytest.mark.parametrize('case', E.POOL_FWD + E.POOL_FWD_BF16_IMAGE)
def test_pool_cases_have_ties_and_a_first_maximum(case):
    """the pooled maps of integer activations: every window has a first maximum, and ties (which a rounding-tolerant check
    has to forgive) are frequent"""
    cs = E.conv_case(*case).bf16('y')
    pooled, arg = cs.pooled
    win = E.pool_windows(np.maximum(cs.y, 0))
    assert ((win == pooled[..., None]).sum(-1) > 1).mean() > 0.02
    assert arg.max() <= 3 and np.array_equal(np.take_along_axis(win, arg[..., None].astype(np.int64), -1)[..., 0], pooled)
    # ... and the by-index gradient of the oracle is MaxPoolGrad + ReluGrad on the activations themselves
    dy = E.ternary(np.random.default_rng(1), pooled.shape)
    y = np.maximum(cs.y, 0)
    np.testing.assert_array_equal(E.pool_grad_reference(arg, pooled, dy, y.shape, True), T.relu_grad(T.maxpool2x2_bwd(y, E.f64(dy)), y))


@pytest.mark.parametrize('case', E.POOLED_BWDF)
def test_pool_fused_filter_gradient_cases(case):
    E.pooled_bwdf_case(*case)


@pytest.mark.parametrize('case', E.BOTH)
def test_one_filter_cases(case):
    E.both_case(*case)


@pytest.mark.parametrize('case', E.DENSE)
def test_dense_cases(case):
    E.dense_case(*case)


@pytest.mark.parametrize('case', E.DENSE_BF16)
def test_dense_cases_on_bf16_tensors(case):
    E.dense_case(*case).bf16()


def test_the_forced_sweep_covers_every_configuration_direction_and_split():
    f32 = E.forced_f32_combos()
    for case in E.FORCED_F32:
        for mode in E.MODES:
            for cfg in range(E.NUM_CFGS):
                mine = [(kind, v) for cs, m, c, kind, v in f32 if (cs, m, c) == (case, mode, cfg)]
                assert [v for kind, v in mine if kind == 'splitk'] == [1, 2, 3, 5]
                grids = [v for kind, v in mine if kind == 'streamk']
                if mode == 0 and cfg in E.TWIN:
                    assert grids == []
                else:
                    M, N, K = E.gemm_dims(case, mode)
                    bm, bn = E.CFG_TILE[E.TWIN.get(cfg, cfg)]
                    assert grids[:3] == [1, 3, 7] and len(grids) == 4
                    assert grids[3] == 1024 or grids[3] > -(-M // bm) * -(-N // bn) * -(-K // 32)
    # K = 288 is 9 k-tiles: factors 2 and 5 leave unequal ranges (5 + 4; 2 + 2 + 2 + 2 + 1)
    assert E.gemm_dims(E.FORCED_F32[1], 0) == (702, 200, 288)
    assert [E.clamped_split(288, 32, s) for s in (1, 2, 3, 5, 64)] == [1, 2, 3, 5, 9]
    assert E.gemm_dims(E.RING_BWD_F[0], 2) == (576, 64, 4232)
    # the rounded-store passes: every pinned bf16 launch with a bf16 result (forward, bwd-data), all column widths, splits and tiles
    rounded = E.forced_bf16_rounded_combos()
    assert {(m, kind, v, s) for cs, m, kind, v, s in rounded if kind == 'bn'} == {(m, 'bn', bn, s) for m in (0, 1) for bn in (64, 128) for s in E.SPLITS_BF16}
    assert sorted(v for cs, m, kind, v, s in rounded if kind == 'ring') == sorted(E.RING_FWD[1] + E.RING_BWD_D[1] + E.RING_BWD_D_96[1])
    assert len(rounded) == 37
    assert E.forced_count() == len(f32) + len(E.forced_bf16_combos()) + len(rounded) == 635


# ---- bf16 rounding, bit for bit ----
def test_bf16_rne_is_torch_s_conversion():
    """all integers in +-70 000, every tie and the neighbours of every tie up to 2^16, and the special values"""
    import torch

    def torch_rne(a):
        return torch.from_numpy(a).to(torch.bfloat16).float().numpy()
    ints = np.arange(-70000, 70001).astype(np.float32)
    np.testing.assert_array_equal(E.bf16_rne(ints), torch_rne(ints))
    # the bf16 grid up to 2^16 (every bit pattern with a zero low half), its midpoints, and the float32 next to each midpoint
    grid = (np.arange(0, 0x4780 + 1, dtype=np.uint32) << 16).view(np.float32)
    assert grid[-1] == 65536.0
    mid = ((grid[:-1].astype(np.float64) + grid[1:].astype(np.float64)) / 2).astype(np.float32)
    assert np.array_equal(mid.astype(np.float64) * 2, grid[:-1].astype(np.float64) + grid[1:])      # midpoints are float32
    near = np.concatenate([mid, np.nextafter(mid, np.float32(np.inf)), np.nextafter(mid, np.float32(-np.inf))])
    near = np.concatenate([near, -near])
    np.testing.assert_array_equal(E.bf16_rne(near), torch_rne(near))
    up = E.bf16_rne(mid) == grid[1:]
    assert up[1:].any() and (~up).any() and np.array_equal(up[1:-1], ~up[2:])      # ties alternate: to the even neighbour
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.finfo(np.float32).max, -np.finfo(np.float32).max, np.nan], np.float32)
    got, want = E.bf16_rne(special), torch_rne(special)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got[-1]) and not np.isnan(got[:-1]).any()
    np.testing.assert_array_equal(got[:-1].view(np.uint32), want[:-1].view(np.uint32))      # the sign of zero included
    assert np.isinf(got[4]) and np.isinf(got[5])                                            # the largest finite float32 rounds to inf


def test_bf16_split_of_12_bit_integers_is_exact():
    a = np.arange(-4095, 4096).astype(np.float32)
    hi, lo = E.bf16_split(a)
    np.testing.assert_array_equal(E.f64(hi) + E.f64(lo), E.f64(a))
    np.testing.assert_array_equal(hi, E.bf16_rne(a))
    assert 0.75 < (lo[np.abs(a) > 256] != 0).mean() < 0.9       # the lo plane is live in four fifths of the wide integers
    odd = np.arange(257, 512, 2).astype(np.float32)
    assert (np.abs(E.bf16_split(odd)[1]) == 1).all() and (np.abs(E.bf16_split(-odd)[1]) == 1).all()


@pytest.mark.parametrize('case', E.ROUNDED_GENERIC + [g[:6] + (1, 'SAME') for g in E.ROUNDED_GUARD] + E.POOL_FWD_BF16_STORED
                         + [E.FORCED_F32[1], E.RING_FWD[0], E.RING_BWD_D_96[0]])
def test_rounded_store_cases(case):
    """a quarter of y and dx changed by the rounding, >= 10 exact ties up and down for each sign (thousands in the large cases)"""
    cs = E.rounded_case(case, 'y', 'dx')
    for name in ('y', 'dx'):
        r, changed, ties = E.rounding_census(getattr(cs, name))
        print(f'{case} {name}: {changed:.1%} rounded, ties {ties}')
        np.testing.assert_array_equal(cs.stored(name, getattr(cs, name)), r)
    if cs.y.size > 1e5:
        assert min(E.rounding_census(cs.y)[2].values()) > 1000
    assert [h < E.F32_EXACT for h in cs.headroom] == [True] * 3


@pytest.mark.parametrize('case', E.ROUNDED_STRIDED)
def test_rounded_store_cases_of_the_strided_bwd_data(case):
    cs = E.rounded_case(case, 'dx')
    if case[5] == 1:      # a quarter of the pixels receive a tap; of those, more than half are rounded
        r, changed, ties = E.rounding_census(cs.dx[:, ::2, ::2])
        assert changed > 0.5 and min(ties.values()) >= 10 and not cs.dx[:, 1::2].any() and not cs.dx[:, :, 1::2].any()


def test_rounded_store_cases_of_the_stencil_and_the_dense_layers():
    shape, mag = E.ROUNDED_BOTH
    E.both_case(*shape, mag=mag)
    for shape in E.DENSE_BF16:
        cs = E.dense_case(*shape, (8, 8, 8), (2.0, 3.0)).rounded_store()
        E.require_rounding(f'{cs.what} 2 y', 2 * cs.y)
        E.require_rounding(f'{cs.what} 3 dx', 3 * cs.dx)
        # tripling does not commute with the rounding (doubling does): a kernel that scales after it rounds differs
        assert (3 * E.f64(E.bf16_rne(cs.dx)) != E.f64(E.bf16_rne(3 * cs.dx))).mean() > 0.25
        np.testing.assert_array_equal(2 * E.f64(E.bf16_rne(cs.dx)), E.f64(E.bf16_rne(2 * cs.dx)))


@pytest.mark.parametrize('case', E.POOL_FWD_BF16_STORED + [g[:6] + (1, 'SAME') for g in E.ROUNDED_GUARD] + E.POOL_FWD_BF16_IMAGE)
def test_rounded_pool_cases_have_ties_the_rounding_created(case):
    """the first maximum of the ROUNDED window is another position than that of the unrounded one in >= 10 windows"""
    cs = E.rounded_case(case, 'y')
    floor = 0 if case in E.POOL_NO_TIES else 10
    for y in (np.maximum(cs.y, 0), cs.y - E.f64(cs.b)):
        pooled, arg = E.rounded_pool(cs, y, floor)
        np.testing.assert_array_equal(pooled, E.f64(E.bf16_rne(E.pool_reference(y)[0])))      # max commutes with the rounding; the position does not
        print(f'{case}: the rounding moves the first maximum of {int((arg != E.pool_reference(y)[1]).sum())} windows')


@pytest.mark.parametrize('case', E.BF16_ARITH)
def test_wide_operand_cases(case):
    """one operand wide (integers up to 4000, half of them no bf16, ties of both parities), the rest ternary: a `bf16` kernel
    must give the oracle on the rounded operand, a `bf16x3` kernel the unrounded oracle"""
    for name, cs in E.wide_variants(case):
        r, x3 = cs.arith_bf16, cs.arith_bf16x3
        reads = {'x': ('y', 'dw'), 'w': ('y', 'dx'), 'dz': ('dw', 'dx')}[name]
        for out in ('y', 'dw', 'dx'):
            np.testing.assert_array_equal(getattr(x3, out), getattr(cs, out))
            E.require_integers(f'{r.what} {out}', getattr(r, out))
            differs = (getattr(r, out) != getattr(cs, out)).mean()
            assert (differs > 0.4) if out in reads else (differs == 0), (name, out, differs)


@pytest.mark.parametrize('case', E.BOTH_WIDE_CASES)
def test_both_wide_bf16x3_cases(case):
    cs = E.conv_case(*case, mags=(E.BOTH_WIDE,) * 3)
    x3 = cs.arith_bf16x3
    for out in ('y', 'dw', 'dx'):
        assert (getattr(x3, out) != getattr(cs, out)).mean() >= 0.5
    # a split by truncation (hi = the upper 16 bits) would multiply other planes: its three products differ from the reference
    hi_t = [(E.f64(v).astype(np.float32).view(np.uint32) & 0xffff0000).view(np.float32) for v in (cs.x, cs.w)]
    lo_t = [E.bf16_rne(v - h) for v, h in zip((cs.x, cs.w), hi_t)]
    trunc = cs.fwd(hi_t[0], hi_t[1], cs.b) + cs.fwd(hi_t[0], lo_t[1]) + cs.fwd(lo_t[0], hi_t[1])
    assert (trunc != x3.y).mean() >= 0.5


def test_few_channel_and_dense_wide_cases():
    for case in E.POOLED_BWDF:
        E.pooled_bwdf_case(*case, xmag=E.WIDE_OPERAND)
    for case in E.POOL_FWD_BF16_IMAGE:
        cs = E.conv_case(*case, mags=(1, E.WIDE_OPERAND, 1))
        assert (cs.arith_bf16.y != cs.y).mean() > 0.9
    for shape in E.DENSE_STREAM_BF16:
        for name, mags in (('x', (E.WIDE_OPERAND, 1, 1)), ('dz', (1, 1, E.WIDE_OPERAND))):
            cs = E.dense_case(*shape, mags)
            E.require_wide(cs.what, getattr(cs, name))
            assert (E.f64(E.bf16_rne(cs.x)).T @ E.f64(E.bf16_rne(cs.dz)) != cs.dw).mean() > 0.5


def rounding_mutants(exact):
    """(truncation, round half away from zero) of the integers `exact` to bf16"""
    bits = np.asarray(exact, np.float32).view(np.uint32)
    trunc = (bits & 0xffff0000).view(np.float32)
    away = ((bits + 0x8000) & 0xffff0000).view(np.float32)
    return E.f64(trunc), E.f64(away)


def test_wrong_rounding_passes_relative_l2_and_fails_equality():
    """conv2d_1's forward, operands up to 8, stored as bf16: a kernel that truncates, or that rounds ties away from zero, is
    within the suite's rel_l2 < 4e-3 of the correctly rounded tensor AND of the float64 result — and fails equality"""
    cs = E.rounded_case(E.GENERIC[0], 'y')
    want = cs.stored('y', cs.y)
    print(f'correct rounding vs float64: rel_l2 {rel_l2(want, cs.y):.2e}')
    for name, mutant in zip(('truncation', 'round half away'), rounding_mutants(cs.y)):
        wrong = (mutant != want).mean()
        print(f'{name}: rel_l2 {rel_l2(mutant, want):.2e} from the rounded tensor, {rel_l2(mutant, cs.y):.2e} from float64, {wrong:.1%} of the elements wrong')
        assert rel_l2(mutant, want) < RTOL_BF16_OUT and rel_l2(mutant, cs.y) < RTOL_BF16_OUT      # the suite's present criterion accepts it
        assert wrong > 0.05
        with pytest.raises(AssertionError):
            np.testing.assert_array_equal(mutant, want)


def test_the_tile_table_here_is_the_library_s():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'ann3depth_amd', 'csrc', 'igemm_cfgs.h')).read()
    body = src[src.index('#define A3D_CFGS(X)'):src.index('// LDS-DMA bf16 kernel')]
    tiles = {int(i): (int(bm), int(bn)) for i, bm, bn in re.findall(r'X\((\d+), (\d+), (\d+),', body)}
    assert tiles == E.CFG_TILE and len(tiles) == E.NUM_CFGS
    assert {int(i): int(t) for i, t in re.findall(r'X\((\d+), \d+, \d+, \d+, \d+, (\d+), [\d.]+f\)', body[body.index('A3D_GLDS_CFGS'):])} == E.TWIN


def mutants(ref, cols, filt, bias, tol):
    """(one element zeroed, one product removed from one element) of the float64 reference `ref` = cols @ filt + bias, each
    chosen as the LARGEST change the relative-L2 criterion `tol` still accepts"""
    budget = 0.9 * tol * np.linalg.norm(ref)
    flat = ref.reshape(-1, ref.shape[-1])
    small = np.abs(flat) * ((np.abs(flat) > 0) & (np.abs(flat) < budget))
    at = np.unravel_index(int(small.argmax()), flat.shape)
    assert small[at] > 0, 'no non-zero element small enough to zero under the criterion'
    zeroed = flat.copy()
    zeroed[at] = 0.0
    # element (row, col) = sum_j cols[row, j] * filt[j, col] + bias[col]: drop the largest product below the budget
    row, col = 0, 0
    prods = cols[row] * filt[:, col]
    assert np.isclose(prods.sum() + bias[col], flat[row, col])
    ok = np.abs(prods) * ((np.abs(prods) > 0) & (np.abs(prods) < budget))
    j = int(ok.argmax())
    assert ok[j] > 0, 'no non-zero product small enough to drop under the criterion'
    dropped = flat.copy()
    dropped[row, col] -= prods[j]
    return zeroed.reshape(ref.shape), dropped.reshape(ref.shape)


def windows_of(cs):
    n, h, w, c, k, ks, st, pad = cs.shape
    ho, pt, pb = T.conv_out_size(h, ks, st, pad)
    wo, pl, pr = T.conv_out_size(w, ks, st, pad)
    xp = np.pad(E.f64(cs.x), ((0, 0), (pt, pb), (pl, pr), (0, 0)))
    return T._windows(xp, ks, ks, st, ho, wo).reshape(n * ho * wo, ks * ks * c), E.f64(cs.w).reshape(ks * ks * c, k)


@pytest.mark.parametrize('case,tol,bf16', [(E.WIDE, RTOL_F32, False), (E.GENERIC[0], RTOL_BF16_OUT, True)])
def test_one_wrong_element_passes_relative_l2_and_fails_equality(case, tol, bf16):
    """conv2d_1's forward at two images (511 488 outputs).  float32: operands up to 8 (a tensor of ternary sums has too small
    a norm for 1e-5 to forgive a difference of 1: ||y|| = 2.3e4); bf16 output: the ternary case, where 4e-3 ||y|| forgives an
    element of magnitude ~80 set to zero."""
    cs = E.conv_case(*case)
    if bf16:
        cs.bf16('y')
    assert cs.y.size >= 5e5
    cols, filt = windows_of(cs)
    for mutant in mutants(cs.y, cols, filt, E.f64(cs.b), tol):
        assert (mutant != cs.y).sum() == 1 and np.array_equal(mutant, np.rint(mutant))
        assert rel_l2(mutant, cs.y) < tol                       # the suite's present criterion accepts it
        with pytest.raises(AssertionError):
            np.testing.assert_array_equal(mutant, cs.y)         # element-by-element equality does not


# ---- operands off the 16-byte grid (test_gpu_exact_offgrid.py) ----
@pytest.mark.parametrize('case', E.OFFGRID_GENERIC + E.OFFGRID_STRIDED + E.OFFGRID_FEW_CHANNEL + E.OFFGRID_POOL)
def test_offgrid_conv_cases_are_exact_in_float32(case):
    cs = E.conv_case(*case)
    assert max(cs.headroom) < E.F32_EXACT
    E.require_integers(cs.what, np.maximum(cs.y, 0))


def test_offgrid_cases_of_the_other_routes():
    for case in E.OFFGRID_POOLED_BWDF:
        E.pooled_bwdf_case(*case)
    for case in E.OFFGRID_BOTH + E.OFFGRID_BOTH_FWD + E.OFFGRID_BOTH_BWD_F:
        E.both_case(*case)
    for case in E.OFFGRID_BF16_STORED:
        assert E.stores_bf16(case)
        E.conv_case(*case).bf16('y', 'dx')
    for case in E.OFFGRID_DENSE + E.OFFGRID_DENSE_ADAM:
        E.dense_case(*case)
    for case in E.OFFGRID_DENSE_BF16:
        E.dense_case(*case).bf16()


@pytest.mark.parametrize('case', E.OFFGRID_BF16_ARITH)
def test_offgrid_wide_cases_tell_the_three_arithmetics_apart(case):
    """an off-grid float32 operand turns a bf16 / bf16x3 request into fp32 arithmetic: with one operand wide, the bf16 reference
    differs from the unrounded one in the outputs that read it, so the record's `prec` decides which one the output must equal"""
    assert case[3] % 4 == 0 and case[4] % 4 == 0
    for name, cs in E.wide_variants(case):
        E.require_wide(f'{cs.what} {name}', getattr(cs, name))
        assert max(cs.headroom) < E.F32_EXACT
        reads = {'x': ('y', 'dw'), 'w': ('y', 'dx'), 'dz': ('dw', 'dx')}[name]
        for out in reads:
            assert (getattr(cs.arith_bf16, out) != getattr(cs, out)).mean() > 0.4
            np.testing.assert_array_equal(getattr(cs.arith_bf16x3, out), getattr(cs, out))


def test_offgrid_sweeps_and_the_refusal_table():
    import os
    import re
    assert E.offgrid_offsets_used()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'a3d.h')).read()
    declared = set(re.findall(r'\b(a3d_\w+)\s*\(', header))
    for cname, operands, image in E.OFFGRID_ENTRIES.values():
        assert cname in declared and (image is None or image in operands)
    for (cname, operand), align in E.REFUSED.items():
        assert cname in declared, f'REFUSED names {cname}, which include/a3d.h does not declare'
        assert align in (4, 8, 16)
        name = operand.split(':')[0]
        assert name == 'ws' or any(c == cname and name in ops for c, ops, _ in E.OFFGRID_ENTRIES.values()), (cname, operand)
    # the header states the contract the table is written from
    for phrase in ('Alignment', 'any multiple of', '16-byte'):
        assert phrase in header
    for entry, (cname, operands, image) in E.OFFGRID_ENTRIES.items():
        sweep = E.offgrid_sweep(entry)
        assert sweep[0] == ('on-grid', {}, 0)
        alone = [offs for _, offs, _ in sweep if len(offs) == 1 and list(offs.values()) == [E.OFFGRID_ALONE]]
        assert [list(o)[0] for o in alone] == list(operands)
        assert [w for _, _, w in sweep if w] == list(E.OFFGRID_WS)
        if image is not None:
            assert ({image: E.OFFGRID_IMAGE} in [offs for _, offs, _ in sweep]) and any(len(offs) == len(operands) for _, offs, _ in sweep)
    # a float32 operand anywhere is refused only where the table says so
    assert E.refused_operands('conv2d_fwd', {'x': 4, 'w': 12, 'y': 8}, 16) == []
    assert E.refused_operands('conv2d_fwd', {}, 4) == ['ws']
    assert E.refused_operands('conv2d_fwd', {'x': 4, 'bias': 4}, 0, {'x': 'bf16', 'w': 'bf16', 'y': 'bf16'}) == ['x']
    assert E.refused_operands('conv2d_bwd_both', {'x': 8, 'dx': 4}, 4) == ['dx']
    assert E.refused_operands('conv2d_bwd_both', {'x': 4, 'dx': 4}, 0, {'dx': 'bf16'}) == ['x']
    assert E.refused_operands('conv2d_bwd_filter_pooled', {'dpool': 8, 'pooled': 4, 'argmax': 1}, 0, {'dpool': 'bf16', 'pooled': 'bf16'}) == ['pooled']
