"""The gradient of the CRF loss with respect to the pair weights without a GPU: tests/crf_pair_grad_ref.py's closed form
against torch float64 autograd of the literal loss, against central differences and against cases worked by hand; its
float32 restatement against crf_loss_ref.loss32 (the same bits where they overlap) and the measured table against the
bound constants the GPU tests use; the dense-layer backward and the floored descent step on exact integers; the float64
descent runs; and the argument checks of ops.crf_loss_grad, ops.pair_dense_bwd and ops.sgd_apply_floor."""
import numpy as np
import pytest
import torch

import crf_loss_ref as L
import crf_pair_grad_ref as G

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---------------------------------------------------------------------------------------------- float64
@pytest.mark.parametrize('regime', ['reference', 'unsaturated'])
@pytest.mark.parametrize('rows,cols', L.GRIDS)
def test_closed_form_is_autograd_of_the_literal_loss(rows, cols, regime):
    """float64 both; the literal loss inverts A and takes det ** .5 through LAPACK, the closed form never differentiates:
    they share no algebra.  1e-12 of ||dr||inf per image: cond(A) <= 1e2 in these regimes, 1e4 u64 would be 1e-12."""
    z, y, r = L.draw(rows, cols, 5, regime)
    left, right = L.pairs(rows, cols)
    want = G.autograd64(z, y, r, left, right)
    got = G.reference(rows, cols, 5, regime)
    err = np.abs(got - want).max(axis=1) / np.abs(want).max(axis=1)
    print(f'{rows}x{cols} {regime}: closed form vs autograd {err.max():.3g}, ||dr||inf {np.abs(want).max(axis=1)}')
    assert np.abs(want).max() > 1e-6 and err.max() <= 1e-12


@pytest.mark.parametrize('eps', [1e-7, 1e-4])
@pytest.mark.parametrize('rows,cols,regime', [(6, 8, 'unsaturated'), (6, 8, 'pivoting'), (3, 4, 'unsaturated'),
                                              (3, 4, 'reference')])
def test_closed_form_matches_central_differences_in_r(rows, cols, regime, eps):
    """d mean / d r by central differences of loss64 itself, step and allowances as
    test_crf_loss_cpu.test_float64_gradient_matches_central_differences (rounding 1e-16 |loss| / h, truncation h^2)."""
    z, y, r = (a[:2].astype(np.float64) for a in L.draw(rows, cols, 5, regime))
    left, right = L.pairs(rows, cols)
    dr = G.grad64(z, y, r, left, right, eps)
    h, num = 1e-5, np.zeros_like(dr)
    for b in range(2):
        for q in range(len(left)):
            rp, rm = r.copy(), r.copy()
            rp[b, q] += h
            rm[b, q] -= h
            num[b, q] = (L.loss64(z, y, rp, left, right, eps)[0] - L.loss64(z, y, rm, left, right, eps)[0]) / (2 * h)
    print(f'max |dr| {np.abs(dr).max():.3g}, max |central difference - dr| {np.abs(num - dr).max():.3g}')
    assert np.abs(dr).max() > 1e-3
    assert np.abs(num - dr).max() <= 1e-6 * np.abs(dr).max() + 1e-9


def test_two_nodes_by_hand():
    """One pair on two nodes: A = [[1 + r, -r], [-r, 1 + r]], det = 1 + 2r, A^-1 = [[1 + r, r], [r, 1 + r]] / (1 + 2r),
    S = 2 / (1 + 2r), w_0 - w_1 = (z_0 - z_1) / (1 + 2r)."""
    z, y, r, eps = np.array([[1.0, 2.0]]), np.array([[1.25, 1.75]]), np.array([[0.75]]), 1e-7
    det = 2.5
    energy = 1.75 * (1.25 ** 2 + 1.75 ** 2) - 2 * 0.75 * 1.25 * 1.75 - 2 * (1.25 + 3.5) + 5.0
    w = np.array([1.75 * 1 + 0.75 * 2, 0.75 * 1 + 1.75 * 2]) / det
    g = z[0] @ w + eps * 9.0 - 5.0
    sd = np.sqrt(det)
    fac, ex = np.pi / (sd + eps), np.exp(g)
    Z = fac * ex + eps
    u = np.exp(-energy) / Z
    dfac = -fac / (sd + eps) * (sd / 2) * (2 / det)
    du = u * -(0.5 ** 2) - (u / Z) * (dfac * ex - fac * ex * (1 / det) ** 2)
    want = -du / (u + eps)
    got = G.grad64(z, y, r, [0], [1], eps)
    assert got.shape == (1, 1) and got[0, 0] == pytest.approx(want, rel=1e-13)
    assert G.grad32(z, y, r, [0], [1], eps)[5][0, 0] == pytest.approx(want, rel=1e-5)


def test_overwritten_and_self_pairs_by_hand():
    """Pairs (0,1), (1,0), (2,2), (1,2) on three nodes.  The second overwrites both cells of the first: the first gets
    exactly +0 and the second the gradient it has without the first.  (2,2) puts r on the diagonal of R, where
    D - R cancels it: dA = 0 and every term of the formula is 0.  A pair that touches an overwritten pair's node only
    ((1,2)) is not affected."""
    z, y, r, left, right = G.edge_case()
    assert G.owners(left, right).tolist() == [False, True, True, True]
    d64 = G.grad64(z, y, r, left, right)
    d32 = G.grad32(z, y, r, left, right)[5]
    alone = G.grad64(z, y, r[:, [1, 3]], [1, 1], [0, 2])
    assert (d64[:, 0] == 0).all() and (bits(d32[:, 0]) == 0).all()                 # +0.0: no sign bit
    np.testing.assert_allclose(d64[:, [1, 3]], alone, rtol=1e-12)
    assert (np.abs(d64[:, [1, 3]]) > 1e-4).all()
    assert (d64[:, 2] == 0).all() and (d32[:, 2] == 0).all()
    want = G.autograd64(z, y, r, left, right)
    np.testing.assert_allclose(d64, want, rtol=1e-11, atol=1e-15)
    assert (want[:, 0] == 0).all() and np.abs(want[:, 2]).max() <= 1e-15
    m = G.dr_errors(d32, d64).max()                                               # the bound the GPU test uses here
    print(f'edge case: float32 restatement vs float64 dr {m:.3g}')
    assert 8 * m <= G.EDGE_BOUND <= 10 * m


# ---------------------------------------------------------------------------------------------- float32
@pytest.mark.parametrize('regime', L.ACCURACY_REGIMES)
@pytest.mark.parametrize('rows,cols', L.GRIDS)
def test_restatement_keeps_the_bits_of_loss32(rows, cols, regime):
    """Carrying the identity through the elimination changes no operation that feeds the loss, dz or the determinant."""
    for batch in (5, 64):
        mean, per, dz, det, swaps, dr = G.restatement(rows, cols, batch, regime)
        mean0, per0, dz0, det0, swaps0 = L.restatement(rows, cols, batch, regime)
        for a, b in ((mean, mean0), (per, per0), (dz, dz0), (det, det0)):
            np.testing.assert_array_equal(bits(a), bits(b))
        np.testing.assert_array_equal(swaps, swaps0)
        assert dr.dtype == F and np.isfinite(dr).all()


@pytest.mark.parametrize('regime', L.ACCURACY_REGIMES)
@pytest.mark.parametrize('rows,cols', L.GRIDS)
def test_bounds_are_eight_times_the_measured_error(rows, cols, regime):
    m = G.measured(rows, cols, regime)
    b = G.BOUNDS[(rows, cols)][regime]
    norms = np.concatenate([np.abs(G.reference(rows, cols, batch, regime)).max(axis=1) for batch in L.BATCHES])
    print(f'{rows}x{cols} {regime}: float32 restatement vs float64 dr {m:.3g}, ||dr64||inf {norms.min():.3g} .. {norms.max():.3g}')
    assert 8 * m <= b <= 10 * m
    assert norms.min() > 1e3 * G.FLT_MIN               # no row is measured against a flushed gradient


def test_restatement_of_a_negative_determinant_is_a_nan_row_and_only_that():
    z, y, r, det64, _ = L.indefinite_batch()
    dr = G.grad32(z, y, r, *L.pairs(6, 8))[5]
    neg = det64 < 0
    assert np.isnan(dr).all(axis=1).tolist() == neg.tolist() and np.isnan(dr).any(axis=1).tolist() == neg.tolist()
    d64 = G.grad64(z, y, r, *L.pairs(6, 8))
    assert np.isnan(d64).all(axis=1).tolist() == neg.tolist()
    assert G.dr_errors(dr[~neg], d64[~neg]).max() <= 1e-3


# ---------------------------------------------------------------------------------------------- dense layer, descent
@pytest.mark.parametrize('k', [1, 2, 3])
@pytest.mark.parametrize('count', [1, 63, 64, 65, 130 * 72])
def test_dense_backward_cases_are_exact_in_float32(count, k):
    """What the GPU test compares bit for bit: integer sums below 2^24, the same in float32 in any order."""
    sims, dr = G.dense_case(count, k)
    dw, db = G.dense_bwd64(sims, dr)
    assert np.abs(sims * np.abs(dr)[..., None]).sum() < 2 ** 24
    assert (dw == np.round(dw)).all() and db == round(db)
    dw32 = (dr[..., None] * sims).sum(axis=(0, 1), dtype=F)
    np.testing.assert_array_equal(dw32.astype(np.float64), dw)
    bad = dr.copy()
    bad[0, count // 2] = np.nan
    dwn, dbn = G.dense_bwd64(sims, bad)
    assert np.isnan(dwn).all() and np.isnan(dbn)


def test_floored_step_by_hand():
    var = np.array([1.0, 0.25, 0.5, -2.0, np.nan, 3.0, 0.0], F)
    g = np.array([2.0, 4.0, 1.0, 0.0, 1.0, np.nan, -1.0], F)
    out = G.sgd_floor32(var, g, 0.25, 0.25)
    #      1 - .5     .25 - 1 -> floor   .5 - .25: exactly the floor   below it   NaN kept   NaN kept   0 + .25
    np.testing.assert_array_equal(bits(out), bits(np.array([0.5, 0.25, 0.25, 0.25, np.nan, np.nan, 0.25], F)))
    assert np.isnan(np.maximum(np.float32(np.nan), 0)) and not np.isnan(np.fmax(np.float32(np.nan), 0))      # why not fmax
    np.testing.assert_array_equal(bits(G.sgd_floor32(var[:4], g[:4], 0.1, -np.inf)), bits(var[:4] - F(0.1) * g[:4]))


@pytest.mark.parametrize('rows,cols,w,b', [(6, 8, (1.0, 1.0), 1.0), (3, 4, (0.3, 0.0), 0.0)])
def test_projected_descent_decreases_the_loss_and_keeps_the_weights_nonnegative(rows, cols, w, b):
    z, y, sims = G.descent_case(rows, cols)
    losses, path = G.descend64(z, y, sims, *L.pairs(rows, cols), w, b, 12)
    print(f'{rows}x{cols} from {w}, {b}: losses {losses}, ends at {path[-1]}')
    assert (np.diff(losses) < 0).all() and losses.max() < 15.5
    assert all((pw >= 0).all() and pb >= 0 for pw, pb in path)


def test_descent_from_zero_weights_is_pinned_at_minus_log_eps_on_the_models_grid():
    """The reference's `+ eps` saturating: r = 0 on 6x8 leaves u far below eps, the loss is -log(eps) = 16.118 and the
    gradient is small.  A property of the loss, documented, not repaired."""
    z, y, sims = G.descent_case(6, 8)
    losses, path = G.descend64(z, y, sims, *L.pairs(6, 8), (0.0, 0.0), 0.0, 3)
    print(f'losses {losses}, after three steps {path[-1]}')
    assert np.abs(losses - -np.log(1e-7)).max() < 1e-2 and (np.diff(losses) <= 0).all()
    assert max(np.abs(path[-1][0]).max(), path[-1][1]) < 1e-2


# ---------------------------------------------------------------------------------------------- argument checks
@pytest.fixture
def no_library(monkeypatch):
    """The checks come before the library: loading it is a failure here."""
    from ann3depth_amd import _lib

    def load():
        raise AssertionError('the library was reached')
    monkeypatch.setattr(_lib, 'load', load)


def crf_args(**kw):
    a = dict(z=torch.zeros((2, 12)), y=torch.zeros((2, 12)), r=torch.zeros((2, 4)),
             left=torch.zeros(4, dtype=torch.int32), right=torch.zeros(4, dtype=torch.int32))
    a.update(kw)
    return [a[k] for k in ('z', 'y', 'r', 'left', 'right')]


@pytest.mark.parametrize('kw', [
    {'y': torch.zeros((2, 11))}, {'y': torch.zeros((3, 12))}, {'y': torch.zeros(24)}, {'r': torch.zeros((3, 4))},
    {'r': torch.zeros((2, 5))}, {'r': torch.zeros(8)}, {'z': torch.zeros(24)}, {'right': torch.zeros(3, dtype=torch.int32)},
    {'left': torch.zeros(0, dtype=torch.int32), 'right': torch.zeros(0, dtype=torch.int32), 'r': torch.zeros((2, 0))},
    {'z': torch.zeros((2, 24))[:, ::2]}, {'y': torch.zeros((12, 2)).t()}, {'r': torch.zeros((2, 8))[:, ::2]},
    {'left': torch.zeros(8, dtype=torch.int32)[::2]}, {'r': torch.zeros((2, 4), device='meta')},
    {'left': torch.zeros(4, dtype=torch.int32, device='meta')}, {'y': torch.zeros((2, 12), device='meta')}])
def test_crf_loss_grad_binding_refuses_tensors_that_do_not_fit(kw, no_library):
    from ann3depth_amd import ops
    with pytest.raises(ValueError, match='crf_loss_grad'):
        ops.crf_loss_grad(*crf_args(**kw))


@pytest.mark.parametrize('kw', [
    {'z': torch.zeros((2, 12), dtype=torch.float64)}, {'y': torch.zeros((2, 12), dtype=torch.bfloat16)},
    {'r': torch.zeros((2, 4), dtype=torch.float16)}, {'left': torch.zeros(4, dtype=torch.int64)},
    {'right': torch.zeros(4)}])
def test_crf_loss_grad_binding_refuses_other_dtypes(kw, no_library):
    from ann3depth_amd import ops
    with pytest.raises(TypeError, match='crf_loss_grad'):
        ops.crf_loss_grad(*crf_args(**kw))


def bwd_args(**kw):
    a = dict(sims=torch.zeros((2, 5, 2)), dr=torch.zeros((2, 5)), dw=torch.zeros((2, 1)), db=torch.zeros(1))
    a.update(kw)
    return [a[k] for k in ('sims', 'dr', 'dw', 'db')]


@pytest.mark.parametrize('kw', [
    {'sims': torch.zeros((2, 5))}, {'sims': torch.zeros((2, 4, 2))}, {'sims': torch.zeros((3, 5, 2))}, {'dr': torch.zeros(10)},
    {'sims': torch.zeros((2, 5, 9)), 'dw': torch.zeros(9)}, {'sims': torch.zeros((2, 5, 0)), 'dw': torch.zeros(0)},
    {'sims': torch.zeros((0, 5, 2)), 'dr': torch.zeros((0, 5))}, {'dw': torch.zeros(3)}, {'db': torch.zeros(2)},
    {'sims': torch.zeros((2, 5, 4))[..., ::2]}, {'dr': torch.zeros((2, 10))[:, ::2]}, {'dw': torch.zeros(4)[::2]},
    {'dr': torch.zeros((2, 5), device='meta')}, {'dw': torch.zeros(2, device='meta')}, {'db': torch.zeros(1, device='meta')}])
def test_pair_dense_bwd_binding_refuses_tensors_that_do_not_fit(kw, no_library):
    from ann3depth_amd import ops
    with pytest.raises(ValueError, match='pair_dense_bwd'):
        ops.pair_dense_bwd(*bwd_args(**kw))


@pytest.mark.parametrize('kw', [{'sims': torch.zeros((2, 5, 2)).double()}, {'dr': torch.zeros((2, 5), dtype=torch.bfloat16)},
                                {'dw': torch.zeros(2, dtype=torch.float16)}, {'db': torch.zeros(1, dtype=torch.int32)}])
def test_pair_dense_bwd_binding_refuses_other_dtypes(kw, no_library):
    from ann3depth_amd import ops
    with pytest.raises(TypeError, match='pair_dense_bwd'):
        ops.pair_dense_bwd(*bwd_args(**kw))


@pytest.mark.parametrize('var,g,exc', [
    (torch.zeros(4), torch.zeros(5), ValueError), (torch.zeros(0), torch.zeros(0), ValueError),
    (torch.zeros(8)[::2], torch.zeros(4), ValueError), (torch.zeros(4), torch.zeros(8)[::2], ValueError),
    (torch.zeros(4), torch.zeros(4, device='meta'), ValueError), (torch.zeros(4).double(), torch.zeros(4), TypeError),
    (torch.zeros(4), torch.zeros(4, dtype=torch.bfloat16), TypeError)])
def test_sgd_apply_floor_binding_refuses_what_does_not_fit(var, g, exc, no_library):
    from ann3depth_amd import ops
    with pytest.raises(exc, match='sgd_apply_floor'):
        ops.sgd_apply_floor(var, g, 0.1, 0.0)
