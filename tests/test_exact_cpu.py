"""The exact-integer cases of test_gpu_exact.py / exact_forced_worker.py, built on the CPU: building a case asserts the
conditions under which equality with a float32 / bf16 kernel is legitimate (integer reference, 2^24 headroom on the sum of
absolute products, bf16-stored outputs <= 256; tests/exact_ops.py), so they are checked here without a GPU.

And the gap those tests close, on the references themselves: a tensor with ONE element zeroed, or one product missing from one
element, passes the suite's relative-L2 criterion (tests/test_gpu_ops.py: rel_l2 < RTOL_F32 for float32 outputs, < 4e-3 for
bf16 outputs) and fails element-by-element equality."""
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
    assert E.forced_count() == len(f32) + len(E.forced_bf16_combos()) == 598


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
