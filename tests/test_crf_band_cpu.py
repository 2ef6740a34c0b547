"""tests/crf_band_ref.py checked on the CPU: the float64 closed forms against autograd of the literal loss, the float32
restatement of the kernel's arithmetic against float64, the band of the model's pair lists, and the overflow of pi^(n/2)
that is the reason the banded form of the objective exists (include/a3d_crf_band.h)."""
import numpy as np
import pytest

import crf_band_ref as R

F = np.float32


@pytest.mark.parametrize('case', ['3x4', '12x16'])
def test_float64_closed_forms_match_autograd_of_the_literal_loss(case):
    left, right, _, _ = R.pairs(case)
    z, y, r = R.draw(case)
    ref = R.reference(case)
    loss, dz, dr = R.autograd64(z, y, r, left, right)
    e = (abs(ref['mean'] - loss) / abs(loss), np.abs(ref['dz'] - dz).max() / np.abs(dz).max(),
         np.abs(ref['dr'] - dr).max() / np.abs(dr).max())
    print(f'crf_band {case}: closed forms against autograd: loss {e[0]:.3g}, dz {e[1]:.3g}, dr {e[2]:.3g}')
    assert max(e) <= 1e-10


def test_overwritten_and_self_pairs_have_no_gradient_in_float64():
    left, right = np.array([0, 1, 2, 1]), np.array([1, 0, 2, 2])
    rng = np.random.default_rng(5)
    z, y = rng.uniform(0.2, 1, (2, 3)), rng.uniform(0.2, 1, (2, 3))
    r = rng.uniform(0, 2, (2, 4))
    assert R.owners(left, right).tolist() == [False, True, False, True]
    ref = R.nll64(z, y, r, left, right)
    loss, dz, dr = R.autograd64(z, y, r, left, right)
    assert abs(ref['mean'] - loss) <= 1e-12 * abs(loss)
    np.testing.assert_allclose(ref['dz'], dz, rtol=1e-10)
    np.testing.assert_allclose(ref['dr'], dr, rtol=1e-10, atol=0)
    assert (ref['dr'][:, [0, 2]] == 0).all()
    got = R.nll32(z, y, r, left, right, 1)
    assert (got['dr'][:, [0, 2]].view(np.uint32) == 0).all() and not got['status'].any()


@pytest.mark.parametrize('case', R.CASES)
def test_the_restatement_stays_within_its_own_bound(case):
    """bound(case) is 8 x the restatement's error: the restatement itself sits at bound / 8, and that figure is float32
    rounding (below 1e-4 at every size), not a mistake in the algebra."""
    assert R.positive_definite(case)
    left, right, n, band = R.pairs(case)
    e = [float(x.max()) for x in R.errors(R.restatement(case), R.reference(case))]
    b = R.bound(case)
    print(f'crf_band {case} (n {n}, band {band}): restatement loss {e[0]:.3g}, dz {e[1]:.3g}, dr {e[2]:.3g}, mu {e[3]:.3g}; '
          f'bound {b}')
    assert not R.restatement(case)['status'].any()
    for x, bx in zip(e, b):
        assert x <= bx / 8 * (1 + 1e-12) and x < 1e-4


@pytest.mark.parametrize('rows,cols', [(6, 8), (12, 16), (24, 32)])
def test_the_band_of_the_models_pair_lists_is_the_number_of_columns(rows, cols):
    from ann3depth_amd import models, ops
    left, right = models.dcnf_pair_indices(rows, cols)
    assert ops.pair_band(left, right) == cols
    assert max(max(left), max(right)) < rows * cols <= ops.BAND_MAX_SP and cols <= ops.BAND_MAX_BAND


def test_pair_band_refuses_what_is_not_a_pair_list():
    from ann3depth_amd import ops
    assert ops.pair_band([3, 0], [1, 9]) == 9
    for bad in (([], []), ([1, 2], [3])):
        with pytest.raises(ValueError):
            ops.pair_band(*bad)


def test_pi_to_the_half_n_overflows_float32_at_192_superpixels_and_the_likelihood_does_not():
    with np.errstate(over='ignore'):
        assert np.isfinite(F(np.pi ** (155 / 2))) and np.isinf(F(np.pi ** (156 / 2))) and np.isinf(F(np.pi ** (192 / 2)))
    assert R.pairs('12x16')[2] == 192
    per = R.restatement('12x16')['per']
    assert np.isfinite(per).all() and per.dtype == F
    np.testing.assert_allclose(per, R.reference('12x16')['per'], rtol=1e-4)
    assert np.isfinite(R.restatement('24x32')['per']).all()
