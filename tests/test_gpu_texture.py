"""a3dt_superpixel_lbp_hist / a3dt_pair_similarity3 on the GPU against tests/texture_ref.py, over dcnf_pair_ref's shapes:
sp = 40 (1600 pixels = 6 * 256 + 64 per block, a 42 x 42 tile), 16 (exactly 256) and 8 (64, 192 idle threads); the model's
240x320, a single superpixel whose every side is clamped, non-square grids.  LBP counts are exact; the first two
similarities are a3d_pair_similarity's bits and so is r with a third weight of 0; the texture similarity is held to its
derived bound and r to 8 x the float32 restatement's measured error (texture_ref's docstring).  Each test prints the worst
figure it saw before it asserts."""
import numpy as np
import pytest
import torch

import dcnf_pair_ref as P
import texture_ref as T
from test_texture_cpu import contrast_image, rgb

pytestmark = pytest.mark.gpu

F = np.float32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def lbp_hist(x, sp):
    """The kernel's histogram between two guard values, which must survive."""
    from ann3depth_amd import ops
    n, h, w, _ = x.shape
    buf = torch.full((n * (h // sp) * (w // sp) * 256 + 2,), -7.25, device='cuda')
    got = ops.superpixel_lbp_hist(dev(x), sp, buf[1:-1].view(n, -1, 256))
    torch.cuda.synchronize()
    assert buf[0] == -7.25 and buf[-1] == -7.25
    return got


def similarity2(x, sp, hist, left, right, w, b, gamma):
    from ann3depth_amd import ops
    sims, r = ops.pair_similarity(dev(x), sp, dev(hist), dev(np.asarray(left, np.int32)), dev(np.asarray(right, np.int32)),
                                  dev(w), dev(b), gamma)
    torch.cuda.synchronize()
    return sims.cpu().numpy(), r.cpu().numpy()


def similarity3(x, sp, hist, lbp, left, right, w, b, gamma):
    from ann3depth_amd import ops
    sims, r = ops.pair_similarity3(dev(x), sp, dev(hist), dev(lbp), dev(np.asarray(left, np.int32)),
                                   dev(np.asarray(right, np.int32)), dev(w), dev(b), gamma)
    torch.cuda.synchronize()
    return sims.cpu().numpy(), r.cpu().numpy()


def odd_values_image(h, w, sp):
    """An image of ties (values k / 4, zeros among them) with NaN, +Inf, -Inf and -0 pixels in the image's corners, on
    both sides of a superpixel border (the image border where the superpixel is the whole image) and in an interior."""
    rng = np.random.default_rng(h + 3 * w + sp)
    x = (rng.integers(0, 4, (1, h, w, 3)) / 4).astype(F)
    odd = [np.nan, np.inf, -np.inf, -0.0]
    spots = [(sp // 2, sp // 2), (sp // 2, sp // 2 + 1), (sp // 2 + 1, sp // 2), (sp // 2 + 2, sp // 2 + 2),      # inside
             (sp - 1, sp - 1), (sp % h, sp % w), (sp - 1, sp % w), (sp % h, sp - 1),      # around a superpixel corner
             (0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)]                      # the corners: three sides clamped
    for i, (yy, xx) in enumerate(spots):                                          # (a later spot wins where two coincide)
        x[0, yy, xx] = odd[(i + 1) % 4] if i < 4 else odd[i % 4]
    return x


@pytest.mark.parametrize('h,w,sp', P.SHAPES)
def test_lbp_histogram_counts_are_exact(h, w, sp):
    rng = np.random.default_rng(sp)
    ties = (rng.integers(0, 3, (3, h, w, 3)) / 2).astype(F)                       # a third of all comparisons tie
    ramp = rgb(np.tile(np.arange(w, dtype=F), (h, 1)))
    cases = [P.image(h, w, sp, 3), P.image(h, w, sp, 3)[2:], rgb(np.full((h, w), 0.3)), ramp, ties,
             contrast_image(h, w, sp), odd_values_image(h, w, sp)]
    for x in cases:
        got = lbp_hist(x, sp)
        want = T.lbp_histogram(x, sp)
        assert torch.equal(got.cpu(), torch.from_numpy(want))
        assert torch.equal(lbp_hist(x, sp), got)                                 # two runs: the same bits
        assert (want.sum(axis=2) == sp * sp).all()
    const = lbp_hist(cases[2], sp).cpu().numpy()
    assert (const[..., 255] == sp * sp).all()
    code = T.lbp_codes(ramp)[0]                  # 62 but for column 0 (the last column's right neighbours are itself: 62 too)
    assert (code[:, 1:] == 62).all() and (code[:, 0] == 255).all()
    got = lbp_hist(ramp, sp).cpu().numpy()
    assert got[..., 62].sum() == h * (w - 1) and got[..., 255].sum() == h
    odd = T.lbp_codes(cases[-1])[0]
    assert odd[0, 0] == 0 and (odd != 255).sum() > 12                             # the NaN corner; the odd values are felt


@pytest.mark.parametrize('gamma', P.GAMMAS)
@pytest.mark.parametrize('h,w,sp', P.SHAPES)
def test_three_similarities_and_pair_weights(h, w, sp, gamma):
    nsp = (h // sp) * (w // sp)
    dw, db = T.dense3()
    dw0 = dw.copy()
    dw0[2] = 0
    worst = np.zeros(2)
    for n in (1, 3):
        x = P.image(h, w, sp, 3)[:n]
        hist, lbp = P.histogram(x, sp), T.lbp_histogram(x, sp)
        for length in (1, 100):
            left, right = P.pair_lists(nsp, length)
            sims, r = similarity3(x, sp, hist, lbp, left, right, dw, db, gamma)
            assert sims.shape == (n, length, 3) and r.shape == (n, length)
            s2, r2 = similarity2(x, sp, hist, left, right, dw[:2], db, gamma)
            np.testing.assert_array_equal(bits(sims[..., :2]), bits(s2))
            _, r0 = similarity3(x, sp, hist, lbp, left, right, dw0, db, gamma)
            np.testing.assert_array_equal(bits(r0), bits(r2))
            s64, r64 = T.similarity3_64(x, sp, hist, lbp, left, right, dw, db, gamma)
            e_t = P.rel_errors(sims[..., 2], s64[..., 2]) / T.texture_bound(lbp, left, right, gamma, sp)
            worst = np.maximum(worst, [e_t.max(), P.r_errors(r, r64).max()])
            if length == 100 or nsp == 1:                         # the first pair is a superpixel with itself
                assert left[0] == right[0]
                assert (bits(sims[:, 0]) == bits(F(1.0))).all()
                assert (bits(r[:, 0]) == bits(((dw[0, 0] + dw[1, 0]) + dw[2, 0]) + db[0])).all()
    # superpixels of one value beside superpixels of noise: texture similarities far below 1, the derived bound alone
    x = contrast_image(h, w, sp)
    hist, lbp = P.histogram(x, sp), T.lbp_histogram(x, sp)
    left, right = P.pair_lists(nsp, 100)
    sims, _ = similarity3(x, sp, hist, lbp, left, right, dw, db, gamma)
    s64, _ = T.similarity3_64(x, sp, hist, lbp, left, right, dw, db, gamma)
    e_t = P.rel_errors(sims[..., 2], s64[..., 2]) / T.texture_bound(lbp, left, right, gamma, sp)
    worst[0] = max(worst[0], e_t.max())
    assert nsp == 1 or s64[..., 2].min() < 0.9
    print(f'pair_similarity3 {h}x{w} sp {sp} gamma {gamma}: texture {worst[0]:.3g} of its bound, '
          f'r {worst[1]:.3g} (bound {T.R3_BOUND:.3g})')
    assert worst[0] <= 1 and worst[1] <= T.R3_BOUND


def test_the_halo_is_read_from_the_image_and_clamped_at_its_border():
    """One random 40 x 40 x 3 tile repeated over 240 x 320, nothing perturbed.  A cell that does not touch the image
    border sees the same tile and the same halo (its neighbours' edges) as every other such cell: their LBP histograms
    are equal and the texture similarity of any two is exactly 1.  A border cell's halo is its own clamped edge."""
    from ann3depth_amd import ops
    h, w, sp = 240, 320, 40
    rows, cols = h // sp, w // sp
    rng = np.random.default_rng(11)
    x = np.tile(rng.random((sp, sp, 3)).astype(F), (rows, cols, 1))[None]
    lbp = lbp_hist(x, sp)
    assert torch.equal(lbp.cpu(), torch.from_numpy(T.lbp_histogram(x, sp)))
    cells = np.arange(rows * cols)
    left, right = np.repeat(cells, len(cells)).astype(np.int32), np.tile(cells, len(cells)).astype(np.int32)
    dw, db = T.dense3()
    sims, _ = ops.pair_similarity3(dev(x), sp, ops.superpixel_hist(dev(x), sp), lbp, dev(left), dev(right), dev(dw), dev(db),
                                   1.0)
    torch.cuda.synchronize()
    t = sims.cpu().numpy()[0, :, 2]

    def inner(c):
        return (0 < c // cols) & (c // cols < rows - 1) & (0 < c % cols) & (c % cols < cols - 1)
    both = inner(left) & inner(right)
    assert both.sum() == 24 * 24 and (bits(t[both]) == bits(F(1.0))).all()
    mixed = ~both & (left != right)
    print(f'periodic image: {int((t[mixed] != 1).sum())} of {int(mixed.sum())} pairs with a border cell differ, '
          f'the least similarity {t[mixed].min():.6f}')
    assert (t[mixed] != 1).any() and (t <= 1).all()
    assert (t[inner(left) != inner(right)] < 1).all()               # an inner cell against a border cell always differs


@pytest.mark.parametrize('bad', [-1, 12, 2 ** 30, -2 ** 31])
def test_a_pair_index_outside_the_grid_is_nan_and_the_other_pairs_do_not_notice(bad):
    h, w, sp, nsp = 24, 32, 8, 12
    x = P.image(h, w, sp, 3)
    hist, lbp = P.histogram(x, sp), T.lbp_histogram(x, sp)
    dw, db = T.dense3()
    left, right = P.pair_lists(nsp, 10)
    clean_s, clean_r = similarity3(x, sp, hist, lbp, left, right, dw, db, 1.0)
    assert np.isfinite(clean_s).all() and np.isfinite(clean_r).all()
    l2, r2 = left.astype(np.int64), right.astype(np.int64)
    l2[3], r2[7] = bad, bad
    sims, r = similarity3(x, sp, hist, lbp, l2.astype(np.int32), r2.astype(np.int32), dw, db, 1.0)
    hit = np.zeros(10, bool)
    hit[[3, 7]] = True
    assert sims.shape == (3, 10, 3) and np.isnan(sims[:, hit]).all() and np.isnan(r[:, hit]).all()
    np.testing.assert_array_equal(bits(sims[:, ~hit]), bits(clean_s[:, ~hit]))
    np.testing.assert_array_equal(bits(r[:, ~hit]), bits(clean_r[:, ~hit]))


def test_the_wrappers_refuse_what_the_kernels_would_misread():
    from ann3depth_amd import ops
    x = dev(P.image(16, 16, 8, 1))
    hist = ops.superpixel_hist(x, 8)
    lbp = ops.superpixel_lbp_hist(x, 8)
    li, ri = dev(np.array([0, 1], np.int32)), dev(np.array([1, 2], np.int32))
    dw, db = dev(T.dense3()[0]), dev(T.dense3()[1])
    with pytest.raises(ValueError):
        ops.superpixel_lbp_hist(x, 5)
    with pytest.raises(ValueError):
        ops.superpixel_lbp_hist(dev(np.zeros((1, 108, 108, 3), F)), 54)
    with pytest.raises(TypeError):
        ops.superpixel_lbp_hist(x.double(), 8)
    with pytest.raises(ValueError):
        ops.superpixel_lbp_hist(x.permute(0, 2, 1, 3), 8)
    with pytest.raises(ValueError):
        ops.superpixel_lbp_hist(x, 8, out=torch.empty((1, 4, 255), device='cuda'))
    with pytest.raises(ValueError):
        ops.pair_similarity3(x, 8, hist, lbp, li, ri, dw[:2], db)           # a two-feature kernel
    with pytest.raises(ValueError):
        ops.pair_similarity3(x, 8, hist, lbp[:, :3], li, ri, dw, db)
    with pytest.raises(TypeError):
        ops.pair_similarity3(x, 8, hist, lbp, li.long(), ri, dw, db)
    with pytest.raises(ValueError):
        ops.pair_similarity3(x, 8, hist, lbp.cpu(), li, ri, dw, db)
