"""The references of tests/crf_observed_ref.py against each other, without a GPU: the closed-form gradients of the header
include/a3d_crf_valid.h against torch autograd of the literal marginal likelihood, the all-observed case against the
reference's loss with its epsilons removed, the independence from what stands in the unobserved targets, the empty
image, the Schur-complement identities the kernel is organised by, the float32 restatement against float64, and the
superpixel-mean reference on exact integers."""
import numpy as np
import pytest

import crf_loss_ref as L
import crf_map_ref as M
import crf_observed_ref as V

F = np.float32
SMALL = [(3, 4), (6, 8)]


@pytest.mark.parametrize('name', V.MASKS)
@pytest.mark.parametrize('regime', V.REGIMES)
@pytest.mark.parametrize('rows,cols', SMALL)
def test_closed_form_gradients_are_autograds(rows, cols, regime, name):
    left, right = L.pairs(rows, cols)
    z, y, r = V.case(rows, cols, 5, regime, name)
    ref = V.nll64(z, y, r, left, right)
    loss, dz, dr = V.autograd64(z, y, r, left, right)
    e = [abs(loss - ref['mean']), np.abs(dz - ref['dz']).max(), np.abs(dr - ref['dr']).max()]
    print(f'observed nll {rows}x{cols} {regime} {name}: |loss|, |dz|, |dr| differences {e}')
    assert max(e) <= 1e-12 * max(1.0, abs(loss))
    if name != 'none':
        assert np.abs(dz).max() > 1e-3 and np.abs(dr).max() > 1e-3


def test_gradients_with_an_overwritten_and_a_self_pair_and_a_mask_per_image():
    """crf_pair_grad_ref.edge_case (a pair that is overwritten, a self pair) with another mask in each image."""
    import crf_pair_grad_ref as G
    z, y, r, left, right = G.edge_case()
    y = y.copy()
    y[0, 1], y[1, 2] = np.nan, np.nan
    ref = V.nll64(z, y, r, left, right)
    loss, dz, dr = V.autograd64(z, y, r, left, right)
    assert abs(loss - ref['mean']) <= 1e-13 and np.abs(dz - ref['dz']).max() <= 1e-13
    assert np.abs(dr - ref['dr']).max() <= 1e-13
    assert (ref['dr'][:, 0] == 0).all() and (np.abs(ref['dr'][:, 2]) <= 1e-16).all() and ref['nobs'].tolist() == [2, 2]


@pytest.mark.parametrize('regime', V.REGIMES)
@pytest.mark.parametrize('rows,cols', V.GRIDS)
def test_all_observed_is_the_reference_loss_without_its_epsilons(rows, cols, regime):
    """(y - mu)^T A (y - mu) - 1/2 log det A + (n / 2) log pi."""
    left, right = L.pairs(rows, cols)
    z, y, r = L.draw(rows, cols, 5, regime)
    ref = V.nll64(z, y, r, left, right)
    n = rows * cols
    for b in range(5):
        A = M.matrix(r[b], n, left, right)
        d = y[b].astype(np.float64) - np.linalg.solve(A, z[b].astype(np.float64))
        want = d @ A @ d - 0.5 * np.linalg.slogdet(A)[1] + n * V.HALF_LOG_PI
        assert abs(ref['per'][b] - want) <= 1e-11 * ref['scale'][b]
        # and the reference's own loss where neither of its epsilons bites: -log(exp(-E) / Z)
        zb, yb = z[b].astype(np.float64), y[b].astype(np.float64)
        energy = yb @ A @ yb - 2 * zb @ yb + zb @ zb
        logZ = n * V.HALF_LOG_PI - 0.5 * np.linalg.slogdet(A)[1] + zb @ np.linalg.solve(A, zb) - zb @ zb
        assert abs(ref['per'][b] - (energy + logZ)) <= 1e-11 * ref['scale'][b]


@pytest.mark.parametrize('name', ['interior', 'row', 'one'])
def test_what_stands_in_an_unobserved_target_changes_nothing(name):
    left, right = L.pairs(6, 8)
    z, y, r = V.case(6, 8, 5, 'unsaturated', name)
    obs = V.mask(6, 8, name)
    first = V.nll32(z, y, r, left, right)
    for fill in (np.inf, -np.inf, np.array([0xffc01234], np.uint32).view(F)[0]):      # a NaN with a payload
        other = V.nll32(z, V.punch(y, obs, fill), r, left, right)
        for k in ('per', 'dz', 'dr', 'nobs', 'status'):
            np.testing.assert_array_equal(first[k].view(np.uint32) if first[k].dtype == F else first[k],
                                          other[k].view(np.uint32) if other[k].dtype == F else other[k])
    ref = V.nll64(z, y, r, left, right)
    other = V.nll64(z, V.punch(y, obs, np.inf), r, left, right)
    np.testing.assert_array_equal(ref['per'], other['per'])


def test_nothing_observed_is_zero_everywhere():
    left, right = L.pairs(3, 4)
    z, y, r = V.case(3, 4, 5, 'reference', 'none')
    for res in (V.nll64(z, y, r, left, right), V.nll32(z, y, r, left, right)):
        assert (res['per'] == 0).all() and (res['dz'] == 0).all() and (res['dr'] == 0).all() and (res['nobs'] == 0).all()
    # one empty image in a batch: its rows are zero, the others are what they are alone up to the 1 / B of the batch
    z, y, r = (a.copy() for a in V.case(3, 4, 5, 'reference', 'interior'))
    y[2] = np.nan
    ref = V.nll64(z, y, r, left, right)
    keep = [0, 1, 3, 4]
    alone = V.nll64(z[keep], y[keep], r[keep], left, right)
    assert ref['per'][2] == 0 and (ref['dz'][2] == 0).all() and (ref['dr'][2] == 0).all()
    np.testing.assert_allclose(ref['dz'][keep] * 5, alone['dz'] * 4, rtol=1e-13)
    np.testing.assert_allclose(ref['mean'] * 5, alone['mean'] * 4, rtol=1e-13)


@pytest.mark.parametrize('name', ['interior', 'corner', 'row', 'one'])
def test_the_schur_complement_identities(name):
    """C^-1 = A_OO - A_OM A_MM^-1 A_MO;  A^-1 P^T C^-1 P A^-1 = A^-1 - [A_MM^-1];  det C = det A_MM / det A;
    q_O = e and q_M = A_MM^-1 (z_M - A_MO y_O) - mu_M;  e^T C^-1 e = q^T A q."""
    rows, cols = 6, 8
    left, right = L.pairs(rows, cols)
    z, y, r = V.case(rows, cols, 1, 'unsaturated', name)
    O = V.mask(rows, cols, name)
    A = M.matrix(r[0], rows * cols, left, right)
    inv = np.linalg.inv(A)
    C = inv[np.ix_(O, O)]
    Amm_inv = np.linalg.inv(A[np.ix_(~O, ~O)])
    schur = A[np.ix_(O, O)] - A[np.ix_(O, ~O)] @ Amm_inv @ A[np.ix_(~O, O)]
    np.testing.assert_allclose(np.linalg.inv(C), schur, rtol=0, atol=1e-12 * np.abs(schur).max())
    pad = np.zeros_like(A)
    pad[np.ix_(~O, ~O)] = Amm_inv
    np.testing.assert_allclose(inv[:, O] @ np.linalg.solve(C, inv[O, :]), inv - pad, rtol=0, atol=1e-13)
    assert abs(np.linalg.slogdet(C)[1] - (np.linalg.slogdet(A[np.ix_(~O, ~O)])[1] - np.linalg.slogdet(A)[1])) <= 1e-12
    zb, yb = z[0].astype(np.float64), np.where(O, y[0], 0).astype(np.float64)
    mu = inv @ zb
    e = yb[O] - mu[O]
    q = inv[:, O] @ np.linalg.solve(C, e)
    np.testing.assert_allclose(q[O], e, rtol=0, atol=1e-13)
    np.testing.assert_allclose(q[~O], Amm_inv @ (zb[~O] - A[np.ix_(~O, O)] @ yb[O]) - mu[~O], rtol=0, atol=1e-13)
    assert abs(e @ np.linalg.solve(C, e) - q @ A @ q) <= 1e-13


@pytest.mark.parametrize('regime', V.REGIMES + ['pivoting'])
@pytest.mark.parametrize('rows,cols', V.GRIDS)
def test_which_regimes_are_positive_definite(rows, cols, regime):
    """The accuracy regimes of the GPU tests are positive definite in every image; 'pivoting' is not."""
    pd = [V.positive_definite(rows, cols, b, regime) for b in V.BATCHES]
    assert all(pd) if regime in V.REGIMES else not all(pd)


@pytest.mark.parametrize('name', V.MASKS)
@pytest.mark.parametrize('regime', V.REGIMES)
@pytest.mark.parametrize('rows,cols', V.GRIDS)
def test_the_restatement_is_float32_close_to_float64(rows, cols, regime, name):
    """Every accepted image, status 0; the errors the GPU bounds are made of stay where float32 puts them: below 1e-5 of
    the loss's terms, 1e-3 of the gradients (a single observed superpixel leaves gradients that are differences of nearly
    equal numbers)."""
    m_loss, m_dz, m_dr = V.measured(rows, cols, regime, name)
    print(f'observed nll restatement {rows}x{cols} {regime} {name}: loss {m_loss:.3g} dz {m_dz:.3g} dr {m_dr:.3g}')
    for batch in V.BATCHES:
        res = V.restatement(rows, cols, batch, regime, name)
        assert (res['status'] == 0).all() and np.isfinite(res['per']).all()
        assert (res['nobs'] == V.mask(rows, cols, name).sum()).all()
    if name == 'none':
        assert (m_loss, m_dz, m_dr) == (0, 0, 0)
    else:
        assert 0 < m_loss < 1e-5 and 0 < m_dz < 1e-3 and 0 < m_dr < 1e-3


def test_the_restatement_refuses_an_indefinite_image():
    left, right = L.pairs(6, 8)
    z, y, r, det64, _ = L.indefinite_batch()
    res = V.nll32(z, V.punch(y, V.mask(6, 8, 'interior')), r, left, right)
    assert (res['status'][det64 < 0] == 1).all() and np.isnan(res['per'][det64 < 0]).all()


def test_superpixel_mean_reference_on_integers():
    x = np.arange(2 * 4 * 6, dtype=np.float64).reshape(2, 4, 6, 1)
    x[0, 0, 0, 0], x[0, 1, 1, 0], x[1, 2:, 4:, 0] = np.nan, np.inf, -np.inf
    y, c = V.superpixel_mean_valid64(x, 2, 0)
    assert c.tolist() == [[2, 4, 4, 4, 4, 4], [4, 4, 4, 4, 4, 0]]
    assert y[0, 0] == (1 + 6) / 2 and y[0, 1] == (2 + 3 + 8 + 9) / 4 and np.isnan(y[1, 5])
    y3, _ = V.superpixel_mean_valid64(x, 2, 3)
    assert np.isnan(y3[0, 0]) and y3[0, 1] == y[0, 1]
    y4, _ = V.superpixel_mean_valid64(x, 2, 4)
    np.testing.assert_array_equal(np.isnan(y4), c < 4)
