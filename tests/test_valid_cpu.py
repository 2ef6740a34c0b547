"""tests/valid_ref.py, the host reference of the training path for depth maps with holes, pinned without a GPU: to
augment_ref.warp where nothing is invalid, to hand-checked small cases, to the oracle's loss where every target is finite,
and to torch autograd."""
import numpy as np
import pytest
import torch

import augment_ref as R
import valid_ref as V
from oracle import tf13_ops as T

INF = float('inf')
LOSS_SHAPES = [(3, 4070), (2, 7), (65, 33)]       # the shapes tests/test_gpu_masked_loss.py runs


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def eigen_like_table(n, h, w):
    t = R.identity(n)
    t[:, 0], t[:, 1], t[:, 2] = np.float32(0.9), np.float32(0.05), np.float32(1.3)
    t[:, 3], t[:, 4], t[:, 5] = np.float32(-0.05), np.float32(0.9), np.float32(0.7)
    t[:, 10] = np.float32(1 / 0.9)
    return t


@pytest.mark.parametrize('dtype', ['u8', 'f32'])
def test_thresholds_that_admit_everything_give_the_plain_warp(dtype):
    rng = np.random.default_rng(0)
    x = rng.integers(0, 256, (2, 9, 11, 1), dtype=np.uint8)
    if dtype == 'f32':
        x = R.as_float(x) * np.float32(7)
    for table in (R.identity(2), eigen_like_table(2, 9, 11)):
        for oh, ow in ((4, 5), (9, 11), (20, 17)):
            got = V.resize_valid(x, table, oh, ow, -1, INF)
            assert not np.isnan(got).any()
            np.testing.assert_array_equal(bits(got), bits(R.warp(x, table, oh, ow, second=True)))


def test_integer_grid_a_hole_beside_a_tap_does_not_invalidate_it():
    """4 x 4 -> 2 x 2: the taps are the pixels (0, 0), (0, 2), (2, 0), (2, 2) with lx = ly = 0 everywhere."""
    x = (np.arange(16, dtype=np.float32) + 1).reshape(1, 4, 4, 1)
    x[0, 0, 1, 0] = x[0, 1, 0, 0] = x[0, 1, 1, 0] = x[0, 3, 3, 0] = 0          # holes beside the taps, none on one
    got = V.resize_valid(x, R.identity(1), 2, 2, 0, INF)
    np.testing.assert_array_equal(got[0, :, :, 0], np.float32([[1, 3], [9, 11]]))
    x[0, 2, 2, 0] = 0                                                          # a hole ON the tap of output (1, 1)
    got = V.resize_valid(x, R.identity(1), 2, 2, 0, INF)
    assert np.isnan(got[0, 1, 1, 0]) and np.isnan(got).sum() == 1
    np.testing.assert_array_equal(got[0, 0, :, 0], np.float32([1, 3]))
    x[0, 0, 1, 0] = np.nan              # a tap of weight 0 that is not finite: 0 * NaN is NaN in the plain resize too
    got = V.resize_valid(x, R.identity(1), 2, 2, 0, INF)
    assert np.isnan(got[0, 0, 0, 0]) and np.isnan(got).sum() == 2


def test_half_pixel_grid_one_invalid_corner_makes_the_element_nan():
    """3 x 3 -> 2 x 2: sx = sy = 1.5, output (1, 1) reads (1, 1), (1, 2), (2, 1), (2, 2) with lx = ly = 0.5."""
    base = (np.arange(9, dtype=np.float32) + 1).reshape(1, 3, 3, 1)
    plain = V.resize_valid(base, R.identity(1), 2, 2, 0, INF)
    np.testing.assert_array_equal(plain[0, :, :, 0], np.float32([[1, 2.5], [5.5, 7]]))
    for corner in ((1, 1), (1, 2), (2, 1), (2, 2)):
        x = base.copy()
        x[0, corner[0], corner[1], 0] = 0
        got = V.resize_valid(x, R.identity(1), 2, 2, 0, INF)
        assert np.isnan(got[0, 1, 1, 0]), corner
        if corner == (2, 2):                                   # counts for output (1, 1) alone
            assert np.isnan(got).sum() == 1
            np.testing.assert_array_equal(got[0, 0, :, 0], np.float32([1, 2.5]))
    x = base.copy()
    x[0, 0, 2, 0] = 0                                          # (0, 2): tr of output (0, 1) alone, which has lx = 0.5, ly = 0
    got = V.resize_valid(x, R.identity(1), 2, 2, 0, INF)
    assert np.isnan(got[0, 0, 1, 0]) and np.isnan(got).sum() == 1


def test_the_range_cap_of_an_8_bit_record_is_excluded_by_max_depth():
    x = np.full((1, 4, 4, 1), 128, np.uint8)
    x[0, 0, 0, 0], x[0, 2, 2, 0] = 255, 0
    got = V.resize_valid(x, R.identity(1), 2, 2, 0, 0.99)
    assert np.isnan(got[0, 0, 0, 0]) and np.isnan(got[0, 1, 1, 0]) and np.isnan(got).sum() == 2
    assert got[0, 0, 1, 0] == R.u8_lut()[128]
    got = V.resize_valid(x, R.identity(1), 2, 2, 0, INF)       # without the cap k = 255 is a depth of 1.0
    assert got[0, 0, 0, 0] == np.float32(1) and np.isnan(got).sum() == 1
    got = V.resize_valid(x, R.identity(1), 2, 2, 0, 1.0)       # the upper bound is inclusive, the lower exclusive
    assert got[0, 0, 0, 0] == np.float32(1)


def test_the_threshold_is_on_the_stored_value_before_the_depth_gain():
    x = np.full((1, 4, 4, 1), np.float32(0.8))
    t = R.identity(1)
    t[0, 10] = np.float32(2)
    got = V.resize_valid(x, t, 2, 2, 0, 1.0)
    np.testing.assert_array_equal(got, np.full((1, 2, 2, 1), np.float32(1.6)))


def test_without_holes_the_masked_loss_is_the_oracles_at_the_model_grid():
    rng = np.random.default_rng(1)
    o = rng.random((3, 4070)) * 3 - 0.4
    t = rng.random((3, 4070)) * 10 + 0.05
    loss, frac = V.masked_silog_fwd(o, t)
    assert loss == T.silog_loss_fwd(o, t) and frac == 1.0
    np.testing.assert_array_equal(V.masked_silog_bwd(o, t), T.silog_loss_bwd(o, t))


def torch_formula(o, t):
    valid = torch.isfinite(t)
    lo = torch.log(o + 1e-8)
    lo = torch.where(torch.isnan(lo), torch.zeros_like(lo), lo)
    d = torch.where(valid, lo - torch.log(torch.where(valid, t, torch.ones_like(t)) + 1e-8), torch.zeros_like(lo))
    n = valid.sum(dim=1).double()
    npix = o.shape[1]
    per = (npix / n.clamp(min=1)) * ((d * d).sum(dim=1) - (0.5 / n.clamp(min=1)) * d.sum(dim=1) ** 2)
    return torch.where(n > 0, per, torch.zeros_like(per)).mean()


@pytest.mark.parametrize('b,npix', LOSS_SHAPES)
def test_gradient_agrees_with_autograd_of_the_same_formula(b, npix):
    o32, t32 = V.loss_case(b, npix, seed=b)
    o, t = o32.astype(np.float64), t32.astype(np.float64)
    to = torch.from_numpy(o).requires_grad_(True)
    loss = torch_formula(to, torch.from_numpy(t))
    loss.backward()
    got_loss, frac = V.masked_silog_fwd(o, t)
    assert abs(got_loss - loss.item()) <= 1e-9 * abs(loss.item())
    assert frac == np.isfinite(t).mean()
    g = V.masked_silog_bwd(o, t)
    assert V.rel_l2(g, to.grad.numpy()) < 1e-9
    assert (g[~np.isfinite(t)] == 0).all() and (g[o < -1e-8] == 0).all()


@pytest.mark.parametrize('b,npix', LOSS_SHAPES)
def test_float32_run_of_the_formula_sits_well_inside_the_gpu_tolerances(b, npix):
    """The GPU tests hold the kernel to 2e-6 (loss) and 1e-5 rel-L2 (gradient) of the float64 reference, the tolerances of
    tests/test_gpu_ops.py::test_silog_loss: a float32 numpy run of the same formula must itself be well inside them."""
    o, t = V.loss_case(b, npix, seed=b)
    ref, _ = V.masked_silog_fwd(o.astype(np.float64), t.astype(np.float64))
    got, _ = V.masked_silog_fwd(o, t)
    e_loss = abs(float(got) - ref) / abs(ref)
    e_grad = V.rel_l2(V.masked_silog_bwd(o, t), V.masked_silog_bwd(o.astype(np.float64), t.astype(np.float64)))
    print(f'float32 reference b={b} npix={npix}: loss rel err {e_loss:.2e}, gradient rel-L2 {e_grad:.2e}')
    assert e_loss < 1e-6 and e_grad < 5e-6


def test_a_sample_without_a_valid_pixel_and_a_valid_target_of_zero():
    o, t = V.loss_case(3, 40, seed=9)
    assert not np.isfinite(t[-1]).any() and t[0, 0] == 0
    g = V.masked_silog_bwd(o, t)
    assert (g[-1] == 0).all()
    loss3, _ = V.masked_silog_fwd(o.astype(np.float64), t.astype(np.float64))
    loss2, _ = V.masked_silog_fwd(o[:2].astype(np.float64), t[:2].astype(np.float64))
    assert loss3 == pytest.approx(loss2 * 2 / 3, rel=1e-14)              # per = 0: the sample only widens the mean
    # the target 0 counts, with log(0 + 1e-8): moving it to another valid depth changes the loss by that pixel's term
    d00 = np.log(np.float64(o[0, 0]) + 1e-8) - np.log(1e-8)
    assert d00 > 17
    only = np.full((1, 4), np.nan)
    only[0, 0] = 0
    loss, frac = V.masked_silog_fwd(np.full((1, 4), 0.5), only)
    assert frac == 0.25
    dd = np.log(0.5 + 1e-8) - np.log(1e-8)
    assert loss == pytest.approx(4 * (dd * dd - 0.5 * dd * dd), rel=1e-14)       # n = 1: r_n = 4, c_n = 0.5
    assert np.isfinite(g).all() and g[0, 0] != 0
