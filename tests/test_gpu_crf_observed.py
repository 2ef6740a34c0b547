"""a3dv_crf_loss_observed on the GPU (include/a3d_crf_valid.h) against the float64 reference of tests/crf_observed_ref.py:
loss, dz and dr within 8 x the error of the float32 restatement of the kernel's own arithmetic on the same inputs, per
grid, regime and mask (the rule of tests/test_gpu_crf_loss.py; the bounds are computed on the CPU from the restatement),
and every edge the header states.  Grids: 3x4, 6x8 (the model's), 8x8 (nsp = 64 = the kernel's limit, 72 pairs: more than
a wavefront).  Each test prints the worst figures it saw before it asserts."""
import ctypes

import numpy as np
import pytest
import torch

import crf_loss_ref as L
import crf_observed_ref as V
import crf_pair_grad_ref as G

pytestmark = pytest.mark.gpu

F = np.float32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pairs_dev(left, right):
    return dev(np.asarray(left, np.int32)), dev(np.asarray(right, np.int32))


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def run(z, y, r, left, right, pair_grad=True):
    """-> dict(mean, per, dz, dr, nobs, status) as numpy."""
    from ann3depth_amd import ops
    out = ops.crf_loss_observed(dev(z), dev(y), dev(r), *pairs_dev(left, right), pair_grad=pair_grad)
    torch.cuda.synchronize()
    mean, per, dz, dr, nobs, status = (None if t is None else t.cpu().numpy() for t in out)
    return dict(mean=mean[0], per=per, dz=dz, dr=dr, nobs=nobs, status=status)


@pytest.mark.parametrize('name', V.MASKS)
@pytest.mark.parametrize('regime', V.REGIMES)
@pytest.mark.parametrize('batch', V.BATCHES)
@pytest.mark.parametrize('rows,cols', V.GRIDS)
def test_loss_and_gradients_match_float64(rows, cols, batch, regime, name):
    left, right = L.pairs(rows, cols)
    assert V.positive_definite(rows, cols, batch, regime)
    z, y, r = V.case(rows, cols, batch, regime, name)
    ref = V.reference(rows, cols, batch, regime, name)
    got = run(z, y, r, left, right)
    m = int(V.mask(rows, cols, name).sum())
    assert (got['nobs'] == m).all() and (got['status'] == 0).all()
    if name == 'none':
        print(f'crf_loss_observed {rows}x{cols} batch {batch} {regime} none: every output +0')
        assert not bits(got['per']).any() and not bits(got['dz']).any() and not bits(got['dr']).any()
        assert bits(got['mean']) == 0
        return
    e = [x.max() for x in V.errors(got, ref)]
    b = V.bound(rows, cols, regime, name)
    print(f'crf_loss_observed {rows}x{cols} batch {batch} {regime} {name}: loss {e[0]:.3g} (bound {b[0]:.3g}), dz {e[1]:.3g} '
          f'(bound {b[1]:.3g}), dr {e[2]:.3g} (bound {b[2]:.3g}), losses {ref["per"].min():.3f} .. {ref["per"].max():.3f}')
    assert np.isfinite(got['per']).all() and np.isfinite(got['dz']).all() and np.isfinite(got['dr']).all()
    assert e[0] <= b[0] and e[1] <= b[1] and e[2] <= b[2]
    assert bits(got['mean']) == bits(L.mean32(got['per']))


def test_a_mask_of_its_own_in_every_image():
    """Five images of the 6x8 grid with the five masks that observe something, and a sixth with none, in one launch: each
    image is held to its own mask's bound (dz and dr carry the 1 / 6 of this batch, as the reference does)."""
    rows, cols, names = 6, 8, ['all', 'interior', 'corner', 'row', 'one', 'none']
    left, right = L.pairs(rows, cols)
    z, y, r = L.draw(rows, cols, 5, 'unsaturated')
    z, y, r = (np.concatenate([a, a[:1]]) for a in (z, y, r))
    y = np.stack([V.punch(y[i], V.mask(rows, cols, nm)) for i, nm in enumerate(names)])
    ref = V.nll64(z, y, r, left, right)
    got = run(z, y, r, left, right)
    e = V.errors(got, ref)
    print(f'crf_loss_observed mixed masks: loss {e[0]}, dz {e[1]}, dr {e[2]}')
    assert got['nobs'].tolist() == [int(V.mask(rows, cols, nm).sum()) for nm in names] and not got['status'].any()
    for i, nm in enumerate(names[:5]):
        b = V.bound(rows, cols, 'unsaturated', nm)
        assert e[0][i] <= b[0] and e[1][i] <= b[1] and e[2][i] <= b[2], nm
    assert bits(got['per'][5]) == 0 and not bits(got['dz'][5]).any() and not bits(got['dr'][5]).any()


@pytest.mark.parametrize('name', ['all', 'row', 'none'])
def test_without_dr_the_other_outputs_keep_their_bits(name):
    left, right = L.pairs(8, 8)
    z, y, r = V.case(8, 8, 5, 'unsaturated', name)
    a, b = run(z, y, r, left, right), run(z, y, r, left, right, pair_grad=False)
    assert b['dr'] is None
    for k in ('mean', 'per', 'dz'):
        np.testing.assert_array_equal(bits(a[k]), bits(b[k]))
    np.testing.assert_array_equal(a['nobs'], b['nobs'])
    np.testing.assert_array_equal(a['status'], b['status'])


def test_two_launches_give_the_same_bits():
    left, right = L.pairs(8, 8)
    z, y, r = V.case(8, 8, 130, 'reference', 'row')
    a, b = run(z, y, r, left, right), run(z, y, r, left, right)
    for k in ('mean', 'per', 'dz', 'dr'):
        np.testing.assert_array_equal(bits(a[k]), bits(b[k]))


@pytest.mark.parametrize('name', ['interior', 'row', 'one', 'none'])
def test_garbage_in_the_unobserved_targets_changes_no_bit(name):
    left, right = L.pairs(6, 8)
    z, y, r = V.case(6, 8, 5, 'unsaturated', name)
    obs = V.mask(6, 8, name)
    first = run(z, y, r, left, right)
    rng = np.random.default_rng(7)
    junk = np.array([np.inf, -np.inf, np.array([0xffc01234], np.uint32).view(F)[0], np.nan], F)
    other = np.array(y, F)
    other[:, ~obs] = junk[rng.integers(0, 4, (5, int((~obs).sum())))]
    assert not np.array_equal(bits(other), bits(y)) and not np.isfinite(other[:, ~obs]).any()
    second = run(z, other, r, left, right)
    for k in ('mean', 'per', 'dz', 'dr'):
        np.testing.assert_array_equal(bits(first[k]), bits(second[k]))
    np.testing.assert_array_equal(first['nobs'], second['nobs'])


def test_an_indefinite_image_is_nan_with_status_1_and_only_that():
    """crf_loss_ref.indefinite_batch(): images 0, 2, 4, 6 have det A < 0.  Those must come back NaN with status 1; the
    restatement decides for the others (an indefinite A with a positive determinant meets a pivot <= 0 or an odd number
    of exchanges as well); no image notices its neighbours: each is the bits of a launch of its own, up to 1 / B."""
    left, right = L.pairs(6, 8)
    z, y, r, det64, _ = L.indefinite_batch()
    y = V.punch(y, V.mask(6, 8, 'interior'))
    want = V.nll32(z, y, r, left, right)
    got = run(z, y, r, left, right)
    print(f'crf_loss_observed indefinite: det {det64}, status {got["status"]}, restatement {want["status"]}, losses {got["per"]}')
    assert (got['status'][det64 < 0] == 1).all()
    np.testing.assert_array_equal(got['status'], want['status'])
    bad = got['status'] == 1
    assert np.isnan(got['per'][bad]).all() and np.isnan(got['dz'][bad]).all() and np.isnan(got['dr'][bad]).all()
    assert np.isnan(got['mean'])
    # a positive definite image between two indefinite ones: the bits of the same image among accepted neighbours
    zc, yc, rc = V.case(6, 8, 5, 'unsaturated', 'interior')
    z2, y2, r2 = (np.stack([a[0], b[1], a[2], b[3]]) for a, b in ((z, zc), (y, yc), (r, rc)))
    mixed = run(z2, y2, r2, left, right)
    clean = run(zc[:4], yc[:4], rc[:4], left, right)
    assert mixed['status'].tolist() == [1, 0, 1, 0]
    for k in ('per', 'dz', 'dr'):
        np.testing.assert_array_equal(bits(mixed[k][[1, 3]]), bits(clean[k][[1, 3]]))
        assert np.isfinite(mixed[k][[1, 3]]).all()


def test_a_poisoned_z_or_r_is_status_1_for_that_image_only():
    left, right = L.pairs(6, 8)
    z, y, r = (np.array(a) for a in V.case(6, 8, 5, 'unsaturated', 'row'))
    clean = run(z, y, r, left, right)
    r[0, 17] = np.nan
    z[2, 40] = np.inf
    got = run(z, y, r, left, right)
    assert got['status'].tolist() == [1, 0, 1, 0, 0]
    for k in ('per', 'dz', 'dr'):
        assert np.isnan(got[k][[0, 2]]).all()
        np.testing.assert_array_equal(bits(got[k][[1, 3, 4]]), bits(clean[k][[1, 3, 4]]))


@pytest.mark.parametrize('left,right', [([0, 7], [1, 1]), ([0, 0], [1, -1]), ([2, 0], [1, 1])])
def test_a_pair_index_outside_the_grid_turns_every_image_into_nan_and_is_not_used(left, right):
    """The index lists of tests/test_gpu_crf_loss.py; the last image observes nothing and is NaN all the same.  Guard
    elements around every output stay as they were."""
    from ann3depth_amd import _lib
    lib = _lib.load()
    n, nsp = 3, 2
    z, r = dev(np.array([[1.0, 2.0]] * n, F)), dev(np.full((n, 2), 0.75, F))
    y = dev(np.array([[1.1, 1.9], [1.1, np.nan], [np.nan, np.nan]], F))
    l, rt = pairs_dev(left, right)
    pbuf, mbuf = torch.full((n + 2,), -7.25, device='cuda'), torch.full((3,), -7.25, device='cuda')
    dbuf, rbuf = torch.full(((n + 2) * nsp,), -7.25, device='cuda'), torch.full(((n + 2) * 2,), -7.25, device='cuda')
    nbuf, sbuf = (torch.full((n + 2,), -7, dtype=torch.int32, device='cuda') for _ in range(2))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.a3dv_crf_loss_observed(n, nsp, z.data_ptr(), y.data_ptr(), r.data_ptr(), l.data_ptr(), rt.data_ptr(), 2,
                                    pbuf[1:].data_ptr(), mbuf[1:].data_ptr(), dbuf[nsp:].data_ptr(), rbuf[2:].data_ptr(),
                                    nbuf[1:].data_ptr(), sbuf[1:].data_ptr(), stream)
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.isnan(rbuf[2:2 + 2 * n]).all() and torch.isnan(pbuf[1:1 + n]).all() and torch.isnan(mbuf[1])
    assert torch.isnan(dbuf[nsp:nsp + n * nsp]).all()
    assert nbuf.tolist() == [-7, 2, 1, 0, -7] and sbuf.tolist() == [-7, 1, 1, 1, -7]
    assert (rbuf[:2] == -7.25).all() and (rbuf[2 + 2 * n:] == -7.25).all() and mbuf[0] == -7.25 and mbuf[2] == -7.25
    assert pbuf[0] == -7.25 and pbuf[-1] == -7.25 and (dbuf[:nsp] == -7.25).all() and (dbuf[nsp + n * nsp:] == -7.25).all()


def test_an_overwritten_pair_is_plus_zero_and_a_self_pair_is_zero():
    """crf_pair_grad_ref.edge_case(): (0,1) overwritten by (1,0), the self pair (2,2); another superpixel missing in each
    image.  Then 80 pairs over the edges of the 3x4 grid in either direction (more pairs than a wavefront) with its row
    mask.  Both at 8 x the restatement's error on the same inputs."""
    z, y, r, left, right = G.edge_case()
    y = y.copy()
    y[0, 1], y[1, 2] = np.nan, np.nan
    got, ref = run(z, y, r, left, right), V.nll64(z, y, r, left, right)
    e = V.errors(got, ref)
    print(f'crf_loss_observed overwritten / self pair: dr {got["dr"]}, float64 {ref["dr"]}, errors {e}')
    assert (bits(got['dr'][:, 0]) == 0).all() and (got['dr'][:, 2] == 0).all() and not got['status'].any()
    b = [8 * x.max() for x in V.errors(V.nll32(z, y, r, left, right), ref)]      # the restatement on this very case
    assert e[0].max() <= b[0] and e[1].max() <= b[1] and e[2].max() <= b[2]
    rng = np.random.default_rng(80)
    gl, gr = L.pairs(3, 4)
    pick, flip = rng.integers(0, len(gl), 80), rng.random(80) < 0.5
    left, right = np.where(flip, gr[pick], gl[pick]), np.where(flip, gl[pick], gr[pick])
    live = G.owners(left, right)
    assert 0 < live.sum() < 80 and live[64:].any() and not live[64:].all()
    z, y, _ = V.case(3, 4, 5, 'unsaturated', 'row')
    r = rng.uniform(2.0, 2.3, (5, 80)).astype(F)
    got, ref = run(z, y, r, left, right), V.nll64(z, y, r, left, right)
    e, b = V.errors(got, ref), [8 * x.max() for x in V.errors(V.nll32(z, y, r, left, right), ref)]
    print(f'crf_loss_observed 80 pairs, {live.sum()} live: errors {[x.max() for x in e]} (bound {b})')
    assert (bits(got['dr'][:, ~live]) == 0).all() and (got['dr'][:, live] != 0).all()
    assert e[0].max() <= b[0] and e[1].max() <= b[1] and e[2].max() <= b[2]


def test_views_and_leading_slices_are_accepted():
    """z and y as the views the train step passes, and the leading rows of a larger batch (DCNFReplica.nll)."""
    from ann3depth_amd import ops
    left, right = pairs_dev(*L.pairs(6, 8))
    z, y, r = (dev(a) for a in V.case(6, 8, 5, 'unsaturated', 'row'))
    first = ops.crf_loss_observed(z, y, r, left, right)
    zbuf, ybuf = z.reshape(5 * 48, 1).clone(), y.reshape(5, 48, 1).clone()
    second = ops.crf_loss_observed(zbuf.view(5, 48), ybuf.view(5, 48), r, left, right)
    head = ops.crf_loss_observed(zbuf.view(5, 48)[:4], ybuf.view(5, 48)[:4], r[:4], left, right, pair_grad=False)
    torch.cuda.synchronize()
    for a, b in zip(first, second):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(head[1].view(torch.int32), first[1][:4].view(torch.int32)) and head[3] is None
