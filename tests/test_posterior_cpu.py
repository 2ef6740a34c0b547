"""The mathematics of include/a3d_posterior.h on the CPU (tests/posterior_ref.py): the precision form on A' against the
covariance form, the tie to the observed-superpixel likelihood's gradient, the claims about A', and the float32
restatement of the kernel against float64.  Draws and grids are crf_band_ref's CASES, every one under every mask."""
import numpy as np
import pytest

import crf_band_ref as R
import crf_observed_ref as V
import posterior_ref as P

PAIRS = [(c, m) for c in R.CASES for m in P.MASKS]


@pytest.mark.parametrize('case,name', PAIRS)
def test_precision_form_on_a_prime_is_the_covariance_form(case, name):
    left, right, n, band = R.pairs(case)
    z, y, r = P.draw(case, name)
    ref, got = P.reference(case, name), P.prec64(z, y, r, left, right)
    np.testing.assert_allclose(got['mean'], ref['mean'], rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(got['var'], ref['var'], rtol=1e-10, atol=1e-12)
    obs = P.mask(case, name)
    assert (got['mean'][obs] == y[obs]).all() and (got['var'][obs] == 0).all() and (got['var'][~obs] > 0).all()
    if name == 'none':
        np.testing.assert_allclose(got['mean'], ref['mu'], rtol=1e-12)


@pytest.mark.parametrize('case,name', [(c, m) for c, m in PAIRS if m not in ('none',)])
def test_mean_minus_mu_is_the_observed_likelihoods_dz(case, name):
    """q = (y_O - mu_O, mean_M - mu_M) is what crf_observed_ref.nll64 returns as -B/2 dz."""
    left, right, n, band = R.pairs(case)
    z, y, r = P.draw(case, name)
    ref = P.reference(case, name)
    dz = V.nll64(z, y, r, left, right)['dz']
    np.testing.assert_allclose(ref['mean'] - ref['mu'], -0.5 * len(z) * dz, rtol=1e-9, atol=1e-13)


@pytest.mark.parametrize('case', R.CASES)
@pytest.mark.parametrize('name', ['row', 'checker', 'random', 'interior', 'one'])
def test_a_prime_keeps_the_band_is_positive_definite_and_has_a_mms_determinant_and_inverse(case, name):
    left, right, n, band = R.pairs(case)
    _, _, r = R.draw(case)
    obs = P.mask(case, name)
    i, j = np.indices((n, n))
    for b in range(len(r)):
        A = R.matrix(r[b], n, left, right)
        Ap = P.masked_matrix(A, obs[b])
        M = ~obs[b]
        assert (Ap[np.abs(i - j) > band] == 0).all()
        assert np.linalg.eigvalsh(A).min() > 0 and np.linalg.eigvalsh(Ap).min() > 0
        amm = A[np.ix_(M, M)]
        np.testing.assert_allclose(np.linalg.slogdet(Ap)[1], np.linalg.slogdet(amm)[1], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(np.linalg.inv(Ap)[np.ix_(M, M)], np.linalg.inv(amm), rtol=1e-10, atol=1e-14)
        # a missing superpixel's diagonal keeps the weights to its observed neighbours; an observed one's is 1
        assert (np.diag(Ap)[M] == np.diag(A)[M]).all() and (np.diag(Ap)[obs[b]] == 1).all()


@pytest.mark.parametrize('case,name', PAIRS)
def test_float32_restatement_is_finite_and_close_to_float64(case, name):
    left, right, n, band = R.pairs(case)
    got, ref = P.restatement(case, name), P.reference(case, name)
    obs = P.mask(case, name)
    z, y, r = P.draw(case, name)
    e = P.measured(case, name)
    print(f'post32 {case} {name}: mean {e[0]:.3g}, var {e[1]:.3g}, bound {P.bound(case, name)}')
    assert not got['status'].any() and np.isfinite(got['mean']).all() and np.isfinite(got['var']).all()
    assert (got['nobs'] == obs.sum(axis=1)).all()
    assert e[0] < 1e-4 and e[1] < 1e-4                                           # float32 on well-conditioned systems
    np.testing.assert_array_equal(got['mean'][obs].view(np.uint32), y[obs].view(np.uint32))
    assert (got['var'][obs].view(np.uint32) == 0).all() and (got['var'][~obs] > 0).all()
    no_var = P.post32(z, y, r, left, right, band, want_var=False)
    np.testing.assert_array_equal(no_var['mean'].view(np.uint32), got['mean'].view(np.uint32))
    if name == 'none':                                                           # the map kernel's operations in its order
        np.testing.assert_array_equal(got['mean'].view(np.uint32), R.restatement(case)['mu'].view(np.uint32))
        by_null = P.post32(z, None, r, left, right, band)
        np.testing.assert_array_equal(by_null['mean'].view(np.uint32), got['mean'].view(np.uint32))
