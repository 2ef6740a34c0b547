"""tests/ssi_ref.py, the host references of include/a3d_ssi.h, against torch autograd (float64) THROUGH an explicit
least-squares solve and against each other; the exactness conditions of the integer cases tests/test_gpu_ssi.py compares bit
for bit; the degenerate rule; and the fit against tests/align_ref.py's exact affine fit (no GPU needed)."""
import numpy as np
import pytest
import torch

import align_ref as A
import ssi_ref as R

F = np.float32


def bits(a):
    return np.ascontiguousarray(np.asarray(a, F)).view(np.uint32)


@pytest.mark.parametrize('masked', [0, 1])
def test_closed_form_gradient_is_autograd_through_the_fit(masked):
    """The envelope-theorem claim: s and t minimise the sum, so the total derivative is the partial one, s r k."""
    o, t = R.case(3, 257, seed=11, masked=masked)
    losses, g, s, sh, flag, n = R.loss64(o, t, masked)
    ot = torch.tensor(o.astype(np.float64), requires_grad=True)
    loss = R.literal_loss(ot, torch.tensor(t.astype(np.float64)), masked)
    loss.backward()
    assert abs(float(loss.detach()) - losses[0]) <= 1e-12 * losses[0] and losses[0] > 0
    scale = np.abs(g).max()
    err = np.abs(g - ot.grad.numpy()).max() / scale
    print(f'closed form against autograd through the solve, masked={masked}: {err:.2e}')
    assert err <= 1e-11                                 # the solve's own conditioning; the forms differ by nothing else
    cnt = R.counting(t, masked)
    assert (g[~cnt] == 0).all() and (g[cnt] != 0).all()
    assert (g[cnt & (o <= 0)] != 0).all() and (cnt & (o <= 0)).any()       # where the log loss has no gradient
    if masked:
        assert flag[1] == R.DEGENERATE and n[1] == 0 and (g[1] == 0).all() and flag[0] == flag[2] == R.FITTED
    else:
        assert (flag == R.FITTED).all()
    # the gradient of a fitted sample is orthogonal to the two directions the fit removes: constants and the output itself
    for i in np.flatnonzero(flag == R.FITTED):
        gi, oi = g[i][cnt[i]], o[i][cnt[i]].astype(np.float64)
        assert abs(gi.sum()) <= 1e-12 * np.abs(gi).sum() and abs((gi * oi).sum()) <= 1e-12 * np.abs(gi * oi).sum()


@pytest.mark.parametrize('b', [1, 2, 4])
def test_integer_cases_are_exact_in_float32(b):
    o, t = R.integer_case(b, 4072, seed=b)
    R.exact_conditions(o, t)
    l64, g64, s64, t64, flag64, n64 = R.loss64(o, t, 1)
    l32, g32, s32, t32, flag32, n32 = R.loss32(o, t, 1)
    np.testing.assert_array_equal(bits(l32), bits(l64))
    np.testing.assert_array_equal(bits(g32), bits(g64))
    assert (s64 == 2).all() and (t64 == 3).all() and (s32 == 2).all() and (t32 == 3).all()
    assert l64[1] == 0.5 and l64[2] == 2 and l64[3] == 3 and l64[0] == np.round(l64[0] * b) / b > 0
    cnt = np.isfinite(t)
    assert set(np.unique(np.abs(g64[cnt]))) == {0, 4 / b, 8 / b, 12 / b}     # s |r| k = 2 {0..3} 2 / b
    assert (bits(g32[~cnt]) == 0).all()


def test_scaling_and_shifting_the_output_changes_nothing_but_the_fit():
    """The feature's point, exactly: 4 o + 8 is exact in float32 on the integer case."""
    o, t = R.integer_case(2, 4072, seed=7)
    o2 = (F(4) * o + F(8)).astype(F)
    a, b = R.loss32(o, t, 1), R.loss32(o2, t, 1)
    np.testing.assert_array_equal(bits(a[0][:2]), bits(b[0][:2]))
    assert (b[2] == a[2] / 4).all() and (b[3] == a[3] - 8 * b[2]).all() and (b[2] == 0.5).all() and (b[3] == -1).all()
    np.testing.assert_array_equal(bits(b[1]), bits(a[1] / F(4)))


def test_float32_restatement_follows_float64_and_poison_stays_in_its_sample():
    for masked in (0, 1):
        o, t = R.case(3, 4070, seed=3, masked=masked)
        ref, b_loss, b_s, b_t, b_grad = R.bound(o, t, masked)
        print(f'ssi float32 restatement (3,4070) masked={masked}: loss bound {b_loss:.2e}, scale {b_s:.2e}, shift {b_t:.2e}, '
              f'gradient {b_grad:.2e}')
        assert 0 < b_loss < 1e-5 and 0 < b_grad < 1e-5 and b_s < 1e-6 and b_t < 1e-6
    o, t = R.case(3, 64, seed=4, masked=0)
    clean = R.loss32(o, t, 0)
    for bad_o, bad_t in ((np.nan, None), (np.inf, None), (None, np.nan), (None, -np.inf)):
        o2, t2 = o.copy(), t.copy()
        if bad_o is not None:
            o2[1, 7] = bad_o
        else:
            t2[1, 7] = bad_t
        for fn in (R.loss32, R.loss64):
            losses, g, s, sh, flag, n = fn(o2, t2, 0)
            assert np.isnan(g[1]).all() and np.isnan(s[1]) and np.isnan(sh[1]) and flag[1] == R.POISONED
            assert np.isnan([losses[0], losses[2], losses[3]]).all() and losses[1] == 1
            assert (flag[[0, 2]] == R.FITTED).all()
        np.testing.assert_array_equal(bits(R.loss32(o2, t2, 0)[1][[0, 2]]), bits(clean[1][[0, 2]]))
    # masked: a hole's target and output poison nobody, a counting output does
    o, t = R.case(3, 64, seed=4, masked=1)
    clean = R.loss32(o, t, 1)
    o2 = o.copy()
    o2[~np.isfinite(t)] = np.inf
    again = R.loss32(o2, t, 1)
    np.testing.assert_array_equal(bits(again[0]), bits(clean[0]))
    np.testing.assert_array_equal(bits(again[1]), bits(clean[1]))
    o2[2, np.flatnonzero(np.isfinite(t[2]))[3]] = np.nan
    assert R.loss32(o2, t, 1)[4].tolist() == [R.FITTED, R.DEGENERATE, R.POISONED]


def test_the_degenerate_rule():
    """A constant output, and one with +-1 ulp of noise, are degenerate: s = 0, t = mean d, no gradient, per = h sum (d - t)^2.
    A relative spread of 1e-3 is fitted."""
    rng = np.random.default_rng(1)
    npix = 4070
    d = (rng.random((1, npix), dtype=F) * F(0.95) + F(0.05)).astype(F)
    const = np.full((1, npix), 0.7, F)
    step = np.spacing(F(0.7))
    noisy = (const + rng.integers(-1, 2, (1, npix)).astype(F) * step).astype(F)
    spread = (const * (1 + 1e-3 * rng.standard_normal((1, npix)))).astype(F)
    for o in (const, noisy):
        assert len(np.unique(o)) == (1 if o is const else 3)
        for fn in (R.loss32, R.loss64):
            losses, g, s, t, flag, n = fn(o, d, 0)
            assert flag[0] == R.DEGENERATE and bits(s)[0] == 0 and (g == 0).all() and (bits(g) == 0).all()
            mean = d.astype(np.float64).mean()
            assert abs(float(t[0]) - mean) <= 2.0 ** -23 * mean
            want = 0.5 * ((d.astype(np.float64) - mean) ** 2).sum()
            assert abs(losses[0] - want) <= 1e-5 * want and losses[2] == 0
    for fn in (R.loss32, R.loss64):
        losses, g, s, t, flag, n = fn(spread, d, 0)
        assert flag[0] == R.FITTED and (g != 0).any() and np.isfinite(s[0]) and s[0] != 0
    # fewer than two counting pixels: one is its own mean, none is nothing
    one = np.array([[np.nan, 0.25, np.inf]], F)
    for fn in (R.loss32, R.loss64):
        losses, g, s, t, flag, n = fn(np.ones((1, 3), F), one, 1)
        assert flag[0] == R.DEGENERATE and t[0] == 0.25 and losses[0] == 0 and n[0] == 1 and (g == 0).all()
        losses, g, s, t, flag, n = fn(np.ones((1, 3), F), np.full((1, 3), np.nan, F), 1)
        assert flag[0] == R.DEGENERATE and t[0] == 0 and s[0] == 0 and losses[0] == 0 and losses[1] == 0 and n[0] == 0


@pytest.mark.parametrize('masked', [0, 1])
def test_scale_and_shift_are_the_affine_alignment_of_the_same_pixels(masked):
    """include/a3d_align.h's A3DA_AFFINE on the same pixel set, computed exactly (fractions) by tests/align_ref.py: the float64
    sums here differ from the exact ones by rounding only, so the float32 coefficients agree or are adjacent."""
    o, t = R.case(2, 15 * 17, seed=21, masked=masked)
    want = A.ref_align(o.reshape(2, 15, 17), t.reshape(2, 15, 17), 'affine', min_depth=-np.inf, max_depth=np.inf)
    assert (want['status'] == 0).all()
    for fn in (R.loss32, R.loss64):
        losses, g, s, sh, flag, n = fn(o, t, masked)
        np.testing.assert_array_equal(n, want['count'])
        got = np.stack([np.asarray(s, F), np.asarray(sh, F)], axis=1)
        assert (A.ulps(got, want['coef']) <= 1).all() and (flag == R.FITTED).all()
