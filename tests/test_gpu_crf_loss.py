"""a3d_crf_loss on the GPU against the float64 reference of tests/crf_loss_ref.py, at the bounds that module measured
(8 x the error of a float32 restatement of the kernel's own arithmetic, per grid and regime) and at the kernel's edges:
row exchanges, negative determinants, the float32 determinant's range, poisoned images, bad pair indices.  Each test
prints the worst figures it saw before it asserts; the observed figures are kept in crf_loss_ref's docstring."""
import ctypes

import numpy as np
import pytest
import torch

import crf_loss_ref as L

pytestmark = pytest.mark.gpu

F = np.float32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pairs_dev(left, right):
    return dev(np.asarray(left, np.int32)), dev(np.asarray(right, np.int32))


def run(z, y, r, left, right, eps=L.EPSILON):
    from ann3depth_amd import ops
    mean, per, dz = ops.crf_loss(dev(z), dev(y), dev(r), *pairs_dev(left, right), eps)
    torch.cuda.synchronize()
    return mean.cpu().numpy()[0], per.cpu().numpy(), dz.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.mark.parametrize('regime', L.ACCURACY_REGIMES)
@pytest.mark.parametrize('batch', L.BATCHES)
@pytest.mark.parametrize('rows,cols', L.GRIDS)
def test_loss_and_gradient_match_float64(rows, cols, batch, regime):
    """Per image: relative loss error and ||.||inf-relative dz error within crf_loss_ref.bound.  Where the loss is pinned
    at -log(eps) = 16.118 ('reference' on the 6x8 and 8x8 grids) the loss assertion says nothing: ignoring a pair weight
    moves it by 1e-4 of itself at most; those cases rest on dz.  The unsaturated and pivoting draws keep every loss
    below 15.5, and the pivoting draws exchange rows (an odd number of times in some image of every batch >= 5).  The
    mean is mean_kernel's own float32 sum of the kernel's losses, bit for bit."""
    left, right = L.pairs(rows, cols)
    z, y, r = L.draw(rows, cols, batch, regime)
    _, per64, dz64, det64 = L.reference(rows, cols, batch, regime)
    assert np.isfinite(per64).all() and (det64 > 0).all()
    if regime != 'reference':
        assert (per64 < 15.5).all()
    if regime == 'pivoting':
        _, _, _, det32, swaps = L.restatement(rows, cols, batch, regime)
        assert (swaps >= 1).all() and (det32 > 0).all()
        assert batch < 5 or (swaps % 2 == 1).any()
    mean, per, dz = run(z, y, r, left, right)
    e_loss, e_dz = L.errors(per, dz, per64, dz64)
    b_loss, b_dz = L.bound(rows, cols, regime)
    print(f'crf_loss {rows}x{cols} batch {batch} {regime}: loss {e_loss.max():.3g} (bound {b_loss:.3g}), '
          f'dz {e_dz.max():.3g} (bound {b_dz:.3g}), losses {per64.min():.3f} .. {per64.max():.3f}')
    assert np.isfinite(per).all() and np.isfinite(dz).all()
    assert e_loss.max() <= b_loss and e_dz.max() <= b_dz
    assert bits(mean) == bits(L.mean32(per))


@pytest.mark.parametrize('batch', L.LARGE_EPS_BATCHES)
def test_a_large_epsilon_makes_its_terms_count(batch):
    """eps = 1e-4 on the 3x4 'unsaturated' draws: eps * (sum z)^2 is 2e-3 .. 7e-3 in g, a thousand times what it is at
    1e-7 and three hundred times the bound, and u + eps is no longer u.  At eps = 1e-7 that term moves the loss by
    about the bound itself, so nothing else here can be relied on to see it."""
    left, right = L.pairs(3, 4)
    z, y, r = L.draw(3, 4, batch, 'unsaturated')
    _, per64, dz64, _ = L.loss64(z, y, r, left, right, L.LARGE_EPS)
    zsum = z.astype(np.float64).sum(axis=1)
    assert per64.max() < 8.5 and (L.LARGE_EPS * zsum * zsum).min() > 1e-3          # -log(1e-4) = 9.21
    mean, per, dz = run(z, y, r, left, right, L.LARGE_EPS)
    e_loss, e_dz = L.errors(per, dz, per64, dz64)
    b_loss, b_dz = L.LARGE_EPS_BOUND
    print(f'crf_loss 3x4 batch {batch} eps 1e-4: loss {e_loss.max():.3g} (bound {b_loss:.3g}), '
          f'dz {e_dz.max():.3g} (bound {b_dz:.3g})')
    assert e_loss.max() <= b_loss and e_dz.max() <= b_dz
    assert bits(mean) == bits(L.mean32(per))


def test_a_single_superpixel_paired_with_itself():
    """nsp = 1, the pair (0, 0): R = [[r]], A = (1 + r) - r.  r = 0.5 and 2 keep A = 1 exactly; the bound is the 3x4
    grid's: a 1x1 system does a subset of a 12x12 system's operations."""
    z = np.array([[0.75], [0.25], [1.5]], F)
    y = np.array([[0.5], [0.375], [1.0]], F)
    r = np.array([[0.5], [2.0], [0.5]], F)
    mean, per, dz = run(z, y, r, [0], [0])
    _, per64, dz64, det64 = L.loss64(z, y, r, [0], [0])
    np.testing.assert_array_equal(det64, 1.0)
    e_loss, e_dz = L.errors(per, dz, per64, dz64)
    b_loss, b_dz = L.bound(3, 4, 'unsaturated')
    print(f'crf_loss 1x1: loss {e_loss.max():.3g} (bound {b_loss:.3g}), dz {e_dz.max():.3g} (bound {b_dz:.3g})')
    assert (per64 < 15.5).all() and e_loss.max() <= b_loss and e_dz.max() <= b_dz
    assert bits(mean) == bits(L.mean32(per))


def test_a_negative_determinant_is_nan_and_only_that():
    """sqrtf(det) of an indefinite system: loss and dz are NaN exactly where the determinant is negative, whatever the
    number of row exchanges was; the images with det > 0 (two of them reached through an odd number of exchanges) do
    not notice their neighbours.  Alone they are a batch of 4, not 8: dz carries 1 / B, a power of two either way, so
    twice the batch's dz is the same bits."""
    left, right = L.pairs(6, 8)
    z, y, r, det64, swaps = L.indefinite_batch()
    neg = det64 < 0
    assert neg.tolist() == [True, False] * 4 and (swaps[[1, 3]] % 2 == 1).all() and (swaps[[5, 7]] % 2 == 0).all()
    assert (swaps > 0).all()
    mean, per, dz = run(z, y, r, left, right)
    print(f'crf_loss indefinite: det {det64}, exchanges {swaps}, losses {per}')
    assert np.isnan(per).tolist() == neg.tolist()
    assert np.isnan(dz).all(axis=1).tolist() == neg.tolist() and np.isnan(dz).any(axis=1).tolist() == neg.tolist()
    assert np.isnan(mean)
    mean4, per4, dz4 = run(z[~neg], y[~neg], r[~neg], left, right)
    np.testing.assert_array_equal(bits(per[~neg]), bits(per4))
    np.testing.assert_array_equal(bits(dz[~neg] * F(2)), bits(dz4))
    assert np.isfinite(mean4) and (np.abs(dz4) > 1e-30).any()
    _, per64, _, _ = L.loss64(z[~neg], y[~neg], r[~neg], left, right)
    assert np.abs(per4 / per64 - 1).max() <= 1e-3                 # the sign was right: a lost exchange gives NaN here


def test_a_determinant_beyond_float32_is_what_float32_arithmetic_makes_of_it():
    """(8, 8) 'stiff': det(A) ~ 2e80 overflows float32.  The expectation is the float32 restatement's answer, whatever
    that is: the same inf / NaN pattern, finite values within the bound of the 8x8 'unsaturated' regime.  Images 0-2
    have random targets (the energy saturates them), 3-5 constant targets, where the loss is live.  dz below the
    float32 normal range may be 0."""
    left, right = L.pairs(8, 8)
    z, y, r = (a.copy() for a in L.draw(8, 8, 5, 'stiff'))
    z, y, r = np.concatenate([z, z[:1]]), np.concatenate([y, y[:1]]), np.concatenate([r, r[:1]])
    y[3:] = F(0.5)
    z[3:] = (y[3:] + F(0.05) * np.random.default_rng(64).standard_normal((3, 64))).astype(F)
    _, per32, dz32, det32, _ = L.loss32(z, y, r, left, right)
    det64 = L.loss64(z, y, r, left, right)[3]
    assert (det64 > 1e60).all() and np.isinf(det32).all()
    mean, per, dz = run(z, y, r, left, right)
    print(f'crf_loss 8x8 stiff: float32 restatement losses {per32}, kernel {per}')
    np.testing.assert_array_equal(np.isnan(per), np.isnan(per32))
    np.testing.assert_array_equal(np.isinf(per), np.isinf(per32))
    np.testing.assert_array_equal(np.isnan(dz), np.isnan(dz32))
    np.testing.assert_array_equal(np.isinf(dz), np.isinf(dz32))
    fin = np.isfinite(per32)
    fin_dz = np.where(np.isfinite(dz32), dz32, 0).astype(np.float64)
    got_dz = np.where(np.isfinite(dz32), dz, 0)
    e_loss, e_dz = L.errors(per[fin], got_dz[fin], per32[fin].astype(np.float64), fin_dz[fin])
    print(f'  against the restatement: loss {e_loss.max():.3g}, dz {e_dz.max():.3g}, bound {L.STIFF_BOUND}')
    assert e_loss.max() <= L.STIFF_BOUND[0] and e_dz.max() <= L.STIFF_BOUND[1]


def test_poisoned_images_are_not_finite_and_the_others_do_not_notice():
    left, right = L.pairs(6, 8)
    z, y, r = (a.copy() for a in L.draw(6, 8, 5, 'unsaturated'))
    clean_mean, clean_per, clean_dz = run(z, y, r, left, right)
    assert np.isfinite(clean_per).all() and np.isfinite(clean_dz).all() and np.isfinite(clean_mean)
    r[0, 17] = np.nan
    z[2, 40] = np.inf
    y[4, 3] = np.nan
    _, per32, dz32, _, _ = L.loss32(z, y, r, left, right)
    assert (~np.isfinite(per32)).tolist() == [True, False, True, False, True]
    mean, per, dz = run(z, y, r, left, right)
    print(f'crf_loss poisoned: losses {per}, restatement {per32}')
    assert (~np.isfinite(per)).tolist() == (~np.isfinite(per32)).tolist()
    assert not np.isfinite(mean)
    np.testing.assert_array_equal(bits(per[[1, 3]]), bits(clean_per[[1, 3]]))
    np.testing.assert_array_equal(bits(dz[[1, 3]]), bits(clean_dz[[1, 3]]))


def test_two_launches_give_the_same_bits_and_views_are_accepted():
    """The pivoting 8x8 batch of 64 twice; then the same through the views the train step passes: z and y as [B, nsp]
    views of [B * nsp, 1] and [B, nsp, 1] buffers, and leading slices of larger batches (models.DCNFReplica.nll)."""
    from ann3depth_amd import ops
    left, right = pairs_dev(*L.pairs(8, 8))
    z, y, r = (dev(a) for a in L.draw(8, 8, 64, 'pivoting'))
    first = [t.clone() for t in ops.crf_loss(z, y, r, left, right, L.EPSILON)]
    second = ops.crf_loss(z, y, r, left, right, L.EPSILON)
    torch.cuda.synchronize()
    for a, b in zip(first, second):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    zbuf, ybuf = z.reshape(64 * 64, 1).clone(), y.reshape(64, 64, 1).clone()
    third = ops.crf_loss(zbuf.view(64, 64), ybuf.view(64, 64), r, left, right, L.EPSILON)
    for a, b in zip(first, third):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    head = ops.crf_loss(zbuf.view(64, 64)[:16], ybuf.view(64, 64)[:16], r[:16], left, right, L.EPSILON)
    torch.cuda.synchronize()
    assert torch.equal(head[1].view(torch.int32), first[1][:16].view(torch.int32))
    assert torch.equal((head[2] * 0.25).view(torch.int32), first[2][:16].view(torch.int32))      # 1/16 against 1/64


@pytest.mark.parametrize('left,right', [([0, 7], [1, 1]), ([0, 0], [1, -1]), ([2, 0], [1, 1])])
def test_a_pair_index_outside_the_grid_turns_every_image_into_nan_and_is_not_used(left, right):
    """The three index lists of tests/test_gpu_crf_map.py: an index outside [0, nsp) is skipped before anything is
    indexed with it, every image's loss and dz and the mean come back NaN; guard elements stay as they were."""
    from ann3depth_amd import _lib
    lib = _lib.load()
    n, nsp = 3, 2
    z = dev(np.array([[1.0, 2.0]] * n, F))
    y = dev(np.array([[1.1, 1.9]] * n, F))
    r = dev(np.full((n, 2), 0.75, F))
    l, rt = pairs_dev(left, right)
    pbuf = torch.full((n + 2,), -7.25, device='cuda')
    dbuf = torch.full(((n + 2) * nsp,), -7.25, device='cuda')
    mbuf = torch.full((3,), -7.25, device='cuda')
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.a3d_crf_loss(n, nsp, z.data_ptr(), y.data_ptr(), r.data_ptr(), l.data_ptr(), rt.data_ptr(), 2, 1e-7,
                          pbuf[1:].data_ptr(), mbuf[1:].data_ptr(), dbuf[nsp:].data_ptr(), stream)
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.isnan(pbuf[1:1 + n]).all() and torch.isnan(dbuf[nsp:nsp + n * nsp]).all() and torch.isnan(mbuf[1])
    assert pbuf[0] == -7.25 and pbuf[-1] == -7.25 and mbuf[0] == -7.25 and mbuf[2] == -7.25
    assert (dbuf[:nsp] == -7.25).all() and (dbuf[nsp + n * nsp:] == -7.25).all()


def test_valid_pairs_in_any_order_with_a_repeat_match_float64():
    """Explicit pair lists: not the model's, out of order, one edge twice (the later weight counts); 'unsaturated' weights
    on twelve nodes with as many pairs as the 3x4 grid has, held to that grid's bound."""
    rng = np.random.default_rng(12)
    left, right = [0, 7, 5, 9, 0], [2, 1, 11, 5, 2]
    y = rng.random((5, 12)).astype(F)
    z = (y + 0.05 * rng.standard_normal((5, 12))).astype(F)
    r = rng.uniform(2.0, 2.3, (5, 5)).astype(F)
    r[:, 0] = F(0.25)
    _, per64, dz64, _ = L.loss64(z, y, r, left, right)
    np.testing.assert_array_equal(per64, L.loss64(z, y, r[:, 1:], left[1:], right[1:])[1])
    assert np.abs(per64 / L.loss64(z, y, r[:, :4], left[:4], right[:4])[1] - 1).min() > 5e-3      # the first would show
    mean, per, dz = run(z, y, r, left, right)
    e_loss, e_dz = L.errors(per, dz, per64, dz64)
    b_loss, b_dz = L.bound(3, 4, 'unsaturated')
    print(f'crf_loss explicit pairs: loss {e_loss.max():.3g} (bound {b_loss:.3g}), dz {e_dz.max():.3g} (bound {b_dz:.3g})')
    assert np.abs(per64).min() > 1 and e_loss.max() <= b_loss and e_dz.max() <= b_dz
