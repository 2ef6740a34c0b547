"""superpixel_mean / superpixel_hist / pair_similarity on the GPU against tests/dcnf_pair_ref.py at their edges: sp = 40
(1600 pixels = 6 * 256 + 64 per block), 16 (exactly 256) and 8 (64, 192 idle threads); the model's 240x320, a single
superpixel, non-square grids; 1 and 3 images; 1, 3 and 4 channels for the mean; gamma 0.25, 1 and 4; pair lists of
length 1 and 100 with repeats and non-neighbours.  Counts are exact; means, colour similarity and r are held to 8 x the
float32 restatement's measured error, the histogram similarity to its derived bound (dcnf_pair_ref's docstring).  Each
test prints the worst figure it saw before it asserts."""
import numpy as np
import pytest
import torch

import dcnf_pair_ref as P

pytestmark = pytest.mark.gpu

F = np.float32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def similarity(x, sp, hist, left, right, w, b, gamma):
    from ann3depth_amd import ops
    sims, r = ops.pair_similarity(dev(x), sp, dev(hist), dev(np.asarray(left, np.int32)),
                                  dev(np.asarray(right, np.int32)), dev(w), dev(b), gamma)
    torch.cuda.synchronize()
    return sims.cpu().numpy(), r.cpu().numpy()


@pytest.mark.parametrize('h,w,sp', P.SHAPES)
def test_block_means(h, w, sp):
    from ann3depth_amd import ops
    worst = 0.0
    for c in P.CHANNELS:
        for n in (1, 3):
            x = P.image(h, w, sp, 3, c)[3 - n:]
            x[0, 0, 0, 0] = F(-3.0)                               # a sign and a value outside [0, 1]
            buf = torch.full((n * (h // sp) * (w // sp) * c + 2,), -7.25, device='cuda')
            got = ops.superpixel_mean(dev(x), sp, buf[1:-1].view(n, -1, c))
            torch.cuda.synchronize()
            assert buf[0] == -7.25 and buf[-1] == -7.25
            worst = max(worst, P.mean_errors(got.cpu().numpy(), x, sp).max())
    print(f'superpixel_mean {h}x{w} sp {sp}: {worst:.3g} (bound {P.MEAN_BOUND:.3g})')
    assert worst <= P.MEAN_BOUND


def edge_image(h, w, k_over):
    """Row-major, the red channel runs through k / k_over for k = 0 .. 255 (k / 256 is exactly the lower edge of bin k),
    then 1.0, values above 1 and negative ones; green and blue stay below one bin's width in every second run."""
    rng = np.random.default_rng(h + w)
    red = np.concatenate([np.arange(256) / k_over, [1.0, 1.5, 4.0, -0.25, -1e-8, 0.99999994, 1 / 512, 255.5 / 256]])
    x = np.zeros((1, h, w, 3), F)
    x[0, :, :, 0] = np.resize(red.astype(F), h * w).reshape(h, w)
    lower = (rng.random((h, w, 2)) / 257).astype(F)
    x[0, :, :, 1:] = np.where((np.arange(h * w).reshape(h, w, 1) // len(red)) % 2 == 1, lower, 0)
    return x


@pytest.mark.parametrize('h,w,sp', P.SHAPES)
def test_histogram_counts_are_exact(h, w, sp):
    from ann3depth_amd import ops
    rng = np.random.default_rng(sp)
    cases = [P.image(h, w, sp, 3), P.image(h, w, sp, 3)[2:], edge_image(h, w, 256), edge_image(h, w, 255),
             (rng.integers(0, 256, (3, h, w, 3)) / 255).astype(F)]
    for x in cases:
        got = ops.superpixel_hist(dev(x), sp).cpu().numpy()
        np.testing.assert_array_equal(got, P.histogram(x, sp))
        assert (got.sum(axis=2) == sp * sp).all() and (got >= 0).all()
    edges = P.histogram(edge_image(h, w, 256), sp)[0]
    assert edges[:, 0].sum() > 0 and (h * w < 264 or edges[:, 255].sum() >= 5)


@pytest.mark.parametrize('gamma', P.GAMMAS)
@pytest.mark.parametrize('h,w,sp', P.SHAPES)
def test_similarities_and_pair_weights(h, w, sp, gamma):
    nsp = (h // sp) * (w // sp)
    dw, db = P.dense()
    worst = np.zeros(3)
    for n in (1, 3):
        x = P.image(h, w, sp, 3)[:n]
        hist = P.histogram(x, sp)
        for length in (1, 100):
            left, right = P.pair_lists(nsp, length)
            sims, r = similarity(x, sp, hist, left, right, dw, db, gamma)
            s64, r64 = P.similarity64(x, sp, hist, left, right, dw, db, gamma)
            e_h = P.rel_errors(sims[..., 1], s64[..., 1]) / P.hist_bound(hist, left, right, gamma)
            worst = np.maximum(worst, [P.rel_errors(sims[..., 0], s64[..., 0]).max(), e_h.max(),
                                       P.r_errors(r, r64).max()])
            if length == 100 or nsp == 1:                         # the first pair is a superpixel with itself
                assert left[0] == right[0]
                assert (bits(sims[:, 0]) == bits(F(1.0))).all()
                assert (bits(r[:, 0]) == bits((dw[0, 0] + dw[1, 0]) + db[0])).all()
    print(f'pair_similarity {h}x{w} sp {sp} gamma {gamma}: colour {worst[0]:.3g} (bound {P.COLOR_BOUND:.3g}), '
          f'histogram {worst[1]:.3g} of its bound, r {worst[2]:.3g} (bound {P.R_BOUND:.3g})')
    assert worst[0] <= P.COLOR_BOUND and worst[1] <= 1 and worst[2] <= P.R_BOUND


@pytest.mark.parametrize('h,w,sp', [(240, 320, 40), (16, 48, 16), (48, 16, 8)])
def test_identical_superpixels_at_different_places_are_exactly_alike(h, w, sp):
    rng = np.random.default_rng(sp)
    x = rng.random((2, h, w, 3)).astype(F)
    nsp, cols = (h // sp) * (w // sp), w // sp
    a, b = 0, nsp - 1
    x[:, (b // cols) * sp:(b // cols + 1) * sp, (b % cols) * sp:(b % cols + 1) * sp] = x[:, :sp, :sp]
    dw, db = P.dense()
    sims, r = similarity(x, sp, P.histogram(x, sp), [a, b, 1], [b, a, 0], dw, db, 4.0)
    assert (bits(sims[:, :2]) == bits(F(1.0))).all() and (sims[:, 2] < 1).all()
    assert (bits(r[:, :2]) == bits((dw[0, 0] + dw[1, 0]) + db[0])).all()


@pytest.mark.parametrize('bad', [-1, 12, 2 ** 30, -2 ** 31])
def test_a_pair_index_outside_the_grid_is_nan_and_the_other_pairs_do_not_notice(bad):
    h, w, sp, nsp = 24, 32, 8, 12
    x = P.image(h, w, sp, 3)
    hist = P.histogram(x, sp)
    dw, db = P.dense()
    left, right = P.pair_lists(nsp, 10)
    clean_s, clean_r = similarity(x, sp, hist, left, right, dw, db, 1.0)
    assert np.isfinite(clean_s).all() and np.isfinite(clean_r).all()
    l2, r2 = left.astype(np.int64), right.astype(np.int64)
    l2[3], r2[7] = bad, bad
    sims, r = similarity(x, sp, hist, l2.astype(np.int32), r2.astype(np.int32), dw, db, 1.0)
    hit = np.zeros(10, bool)
    hit[[3, 7]] = True
    assert np.isnan(sims[:, hit]).all() and np.isnan(r[:, hit]).all()
    np.testing.assert_array_equal(bits(sims[:, ~hit]), bits(clean_s[:, ~hit]))
    np.testing.assert_array_equal(bits(r[:, ~hit]), bits(clean_r[:, ~hit]))
