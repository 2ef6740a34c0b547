"""a3dv_superpixel_mean_valid on the GPU (include/a3d_crf_valid.h): integer-valued depths, so that every sum is exact in
any order, held to numpy bit for bit; all-finite input against a3d_superpixel_mean bit for bit; the count threshold on
both sides, infinities, an empty block, min_count = 0."""
import ctypes

import numpy as np
import pytest
import torch

import crf_observed_ref as V

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = [(2, 80, 120, 40), (2, 240, 320, 40)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def integers_with_holes(n, h, w, seed, hole=0.3):
    """Depths 0 .. 255 (a block's sum stays below 2^24) with `hole` of the pixels NaN."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, (n, h, w, 1)).astype(F)
    x[rng.random((n, h, w, 1)) < hole] = np.nan
    return x


def check(x, sp, min_count):
    from ann3depth_amd import ops
    y, c = ops.superpixel_mean_valid(dev(x), sp, min_count)
    torch.cuda.synchronize()
    y, c = y.cpu().numpy(), c.cpu().numpy()
    y64, c64 = V.superpixel_mean_valid64(x, sp, min_count)
    np.testing.assert_array_equal(c, c64)
    np.testing.assert_array_equal(np.isnan(y), np.isnan(y64))
    fin = ~np.isnan(y64)
    np.testing.assert_array_equal(bits(y[fin]), bits(y64[fin].astype(F)))       # one division of two integers < 2^24: rounding through float64 is innocuous
    return y, c


@pytest.mark.parametrize('min_count', [0, 800, 1200])
@pytest.mark.parametrize('n,h,w,sp', SIZES)
def test_integer_depths_with_holes_are_numpy_bit_for_bit(n, h, w, sp, min_count):
    x = integers_with_holes(n, h, w, h + min_count)
    x[0, :sp, :sp] = np.nan                                              # an all-hole block
    x[1, sp:2 * sp, sp:2 * sp] = F(7)                                    # a block without a hole
    y, c = check(x, sp, min_count)
    cols = w // sp
    assert c[0, 0] == 0 and np.isnan(y[0, 0]) and c[1, cols + 1] == sp * sp and y[1, cols + 1] == 7
    assert min_count == 0 or ((c < min_count).any() and (c >= min_count).any())


@pytest.mark.parametrize('n,h,w,sp', SIZES)
def test_all_finite_input_is_superpixel_mean_bit_for_bit(n, h, w, sp):
    """Not integers: the sums round, and must round as a3d_superpixel_mean's do."""
    from ann3depth_amd import ops
    x = dev(np.random.default_rng(h).random((n, h, w, 1)).astype(F))
    y, c = ops.superpixel_mean_valid(x, sp, sp * sp)
    plain = ops.superpixel_mean(x, sp)
    torch.cuda.synchronize()
    assert torch.equal(y.view(torch.int32), plain.view(n, -1).view(torch.int32)) and (c == sp * sp).all()


def test_the_count_threshold_on_both_sides():
    """Blocks with exactly min_count and min_count - 1 finite pixels; min_count = 0 still wants one pixel."""
    sp, k = 40, 800
    x = np.full((1, 40, 160, 1), np.nan, F)
    blocks = [k, k - 1, 1, 0]
    for j, cnt in enumerate(blocks):
        blk = np.full(sp * sp, np.nan, F)
        blk[np.random.default_rng(j).permutation(sp * sp)[:cnt]] = F(j + 2)
        x[0, :, j * sp:(j + 1) * sp, 0] = blk.reshape(sp, sp)
    y, c = check(x, sp, k)
    assert c[0].tolist() == blocks and y[0, 0] == 2 and np.isnan(y[0, 1:]).all()
    y0, _ = check(x, sp, 0)
    assert y0[0, :3].tolist() == [2, 3, 4] and np.isnan(y0[0, 3])
    y1, _ = check(x, sp, k - 1)
    assert y1[0, :2].tolist() == [2, 3] and np.isnan(y1[0, 2:]).all()


def test_an_infinity_is_a_hole():
    x = integers_with_holes(1, 80, 120, 5, hole=0.0)
    x[0, 0, 0], x[0, 41, 41], x[0, 79, 119] = np.inf, -np.inf, np.inf
    y, c = check(x, 40, 0)
    assert c[0].tolist() == [1599, 1600, 1600, 1600, 1599, 1599] and np.isfinite(y).all()


def test_count_may_be_null_and_guards_stay():
    from ann3depth_amd import _lib
    lib = _lib.load()
    x = dev(integers_with_holes(1, 80, 120, 9))
    ybuf = torch.full((8,), -7.25, device='cuda')
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.a3dv_superpixel_mean_valid(1, 80, 120, x.data_ptr(), 40, 0, ybuf[1:].data_ptr(), None, stream) == 0
    torch.cuda.synchronize()
    want, _ = V.superpixel_mean_valid64(x.cpu().numpy(), 40, 0)
    assert ybuf[0] == -7.25 and ybuf[7] == -7.25
    np.testing.assert_array_equal(bits(ybuf[1:7].cpu().numpy()), bits(want[0].astype(F)))
