"""tests/texture_ref.py checked on the CPU before the GPU tests rely on it: the vectorised LBP against a literal per-pixel
loop, hand-worked images (constant, ramp, a NaN pixel, +-0 ties), the counts of every superpixel, S_t < 2^24 for every case
of tests/test_gpu_texture.py, the float32 similarity inside its derived bound of float64, and R3_BOUND = 8 x measured."""
import numpy as np
import pytest

import dcnf_pair_ref as P
import texture_ref as T

F = np.float32


def rgb(g):
    """A grey image [h, w] as one image [1, h, w, 3] with three equal channels."""
    return np.repeat(np.asarray(g, F)[None, :, :, None], 3, axis=3)


def contrast_image(h, w, sp, seed=0):
    """Superpixels of one value (every code 255) beside superpixels of noise: texture similarities well below 1."""
    rng = np.random.default_rng(seed + h + w + sp)
    x = rng.random((1, h, w, 3)).astype(F)
    board = np.add.outer(np.arange(h // sp), np.arange(w // sp)) % 2                # a checkerboard of the two kinds
    flat = np.kron(board, np.ones((sp, sp), np.int64)).astype(bool)
    x[0, flat] = F(0.5)
    return x


@pytest.mark.parametrize('h,w,sp', [(8, 8, 8), (24, 8, 8), (16, 48, 16)])
def test_vectorised_lbp_is_the_literal_loop(h, w, sp):
    rng = np.random.default_rng(h * w)
    ties = (rng.integers(0, 4, (1, h, w, 3)) / 4).astype(F)
    odd = ties.copy()
    odd[0, 0, 0], odd[0, h - 1, w - 1], odd[0, h // 2, w // 2], odd[0, 1, 2] = np.nan, np.inf, -np.inf, -0.0
    for x in (P.image(h, w, sp, 3), ties, odd):
        np.testing.assert_array_equal(T.lbp_codes(x), T.lbp_codes_loop(x))


def test_a_constant_image_is_code_255_everywhere():
    code = T.lbp_codes(rgb(np.full((9, 7), 0.3)))
    assert (code == 255).all()
    hist = T.lbp_histogram(rgb(np.full((16, 24), 0.3)), 8)
    assert (hist[..., 255] == 64).all() and hist.sum() == 16 * 24


def test_a_ramp_along_x_is_62_inside_and_255_in_column_0():
    """Value = column index.  A pixel's right neighbours (+1 column: bits 2, 3, 4) are larger, the two in its own column
    (bits 1, 5) tie, the left ones (bits 0, 6, 7) are smaller: 4 + 8 + 16 + 2 + 32 = 62, in every row, since the clamp
    at the top and bottom repeats the row.  In column 0 the left neighbours are the clamped column itself and tie too."""
    code = T.lbp_codes(rgb(np.tile(np.arange(10, dtype=F), (6, 1))))[0]
    assert (code[:, 1:-1] == 62).all() and (code[:, 0] == 255).all()
    assert (code[:, -1] == 2 + 32 + 4 + 8 + 16).all()                       # the last column: its right neighbours are itself


def test_a_nan_pixel_clears_its_eight_bits_and_one_bit_in_each_neighbour():
    g = np.full((5, 5), 0.5, F)
    g[2, 2] = np.nan
    code = T.lbp_codes(rgb(g))[0]
    assert code[2, 2] == 0
    for k, (dy, dx) in enumerate(T.OFFSETS):                                # the neighbour at -offset k sees the NaN at offset k
        assert code[2 - dy, 2 - dx] == 255 & ~(1 << k)
    rest = np.ones((5, 5), bool)
    rest[1:4, 1:4] = False
    assert (code[rest] == 255).all()


def test_ties_of_either_zero_set_the_bit():
    g = np.zeros((4, 4), F)
    g[1, 1], g[2, 3] = -0.0, -0.0
    x = rgb(g)
    assert np.signbit(T.grey(x)[0, 1, 1]) and not np.signbit(T.grey(x)[0, 0, 0])      # (-0 + -0) + -0 = -0, / 3 = -0
    assert (T.lbp_codes(x) == 255).all()


@pytest.mark.parametrize('h,w,sp', P.SHAPES)
def test_every_superpixel_counts_its_pixels_and_s_t_stays_exact(h, w, sp):
    nsp = (h // sp) * (w // sp)
    for x in (P.image(h, w, sp, 3), contrast_image(h, w, sp), rgb(np.tile(np.arange(w, dtype=F), (h, 1)))):
        lbp = T.lbp_histogram(x, sp)
        assert lbp.shape == (len(x), nsp, 256) and (lbp >= 0).all() and (lbp == np.floor(lbp)).all()
        assert (lbp.sum(axis=2) == sp * sp).all()
        every = np.arange(nsp)
        S = T.s_t(lbp, np.repeat(every, nsp), np.tile(every, nsp))          # every pair of superpixels there is
        assert S.max() <= 2 * (sp * sp) ** 2 < 2 ** 24
    assert 2 * (T.MAX_SP * T.MAX_SP) ** 2 < 2 ** 24 <= 2 * ((T.MAX_SP + 1) ** 2) ** 2


@pytest.mark.parametrize('h,w,sp', P.SHAPES)
def test_float32_texture_similarity_is_inside_its_derived_bound(h, w, sp):
    nsp = (h // sp) * (w // sp)
    dw, db = T.dense3()
    for x in (P.image(h, w, sp, 3), contrast_image(h, w, sp)):
        hist, lbp = P.histogram(x, sp), T.lbp_histogram(x, sp)
        for gamma in P.GAMMAS:
            left, right = P.pair_lists(nsp, 100)
            s32, r32 = T.similarity3_32(x, sp, hist, lbp, left, right, dw, db, gamma)
            s64, r64 = T.similarity3_64(x, sp, hist, lbp, left, right, dw, db, gamma)
            assert s32.dtype == F and r32.dtype == F and s32.shape == (len(x), 100, 3)
            assert (P.rel_errors(s32[..., 2], s64[..., 2]) <= T.texture_bound(lbp, left, right, gamma, sp)).all()
            assert (s64[..., 2] > 0).all() and (s64[..., 2] <= 1).all()
            s2, _ = P.similarity32(x, sp, hist, left, right, dw[:2], db, gamma)
            np.testing.assert_array_equal(s32[..., :2].view(np.uint32), s2.view(np.uint32))
    if nsp > 1:                                                             # the contrast image does reach below 1
        assert s64[..., 2].min() < 0.9


def test_r_bound_is_eight_times_the_measured_error():
    m = T.measured()
    print('float32 form vs float64: r of three similarities %.3g' % m)
    assert 8 * m <= T.R3_BOUND <= 10 * m
