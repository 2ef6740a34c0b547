"""a3db_crf_band_nll and a3db_crf_band_map on the GPU (include/a3d_crf_band.h) against the float64 reference of
tests/crf_band_ref.py: loss, dz, dr and mu within 8 x the error of the float32 restatement of the kernel's own arithmetic
on the same inputs (the rule of tests/test_gpu_crf_loss.py and tests/test_gpu_crf_observed.py; the bounds are computed on
the CPU), against the dense kernels where those exist, and every edge the header states.  Each test prints the figures it
saw before it asserts."""
import ctypes

import numpy as np
import pytest
import torch

import crf_band_ref as R
import crf_map_ref as M
import crf_observed_ref as V

pytestmark = pytest.mark.gpu

F = np.float32


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def pairs_dev(left, right):
    return dev(np.asarray(left, np.int32)), dev(np.asarray(right, np.int32))


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def run(z, y, r, left, right, band, pair_grad=True, want_mu=True):
    """-> dict(mean, per, dz, dr, mu, status) as numpy."""
    from ann3depth_amd import ops
    out = ops.crf_band_nll(dev(z), dev(y), dev(r), *pairs_dev(left, right), band, pair_grad=pair_grad, want_mu=want_mu)
    torch.cuda.synchronize()
    mean, per, dz, dr, mu, status = (None if t is None else t.cpu().numpy() for t in out)
    return dict(mean=mean[0], per=per, dz=dz, dr=dr, mu=mu, status=status)


def run_map(z, r, left, right, band):
    from ann3depth_amd import ops
    mu, status = ops.crf_band_map(dev(z), dev(r), *pairs_dev(left, right), band)
    torch.cuda.synchronize()
    return mu.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize('case', ['3x4', '6x8', '5x13', '12x16', '3x32', '24x32', 'chain1', 'chain32'])
def test_both_entry_points_match_float64(case):
    import crf_loss_ref as L
    left, right, n, band = R.pairs(case)
    assert R.positive_definite(case)
    z, y, r = R.draw(case)
    ref, b = R.reference(case), R.bound(case)
    got = run(z, y, r, left, right, band)
    mu_map, st_map = run_map(z, r, left, right, band)
    e = [float(x.max()) for x in R.errors(got, ref)]
    e_map = float(R.errors(dict(got, mu=mu_map), ref)[3].max())
    print(f'crf_band {case} (n {n}, band {band}, batch {len(z)}): loss {e[0]:.3g} (bound {b[0]:.3g}), dz {e[1]:.3g} (bound '
          f'{b[1]:.3g}), dr {e[2]:.3g} (bound {b[2]:.3g}), mu {e[3]:.3g} / map {e_map:.3g} (bound {b[3]:.3g}), losses '
          f'{ref["per"].min():.3f} .. {ref["per"].max():.3f}')
    assert not got['status'].any() and not st_map.any()
    assert all(np.isfinite(got[k]).all() for k in ('per', 'dz', 'dr', 'mu')) and np.isfinite(mu_map).all()
    assert e[0] <= b[0] and e[1] <= b[1] and e[2] <= b[2] and e[3] <= b[3] and e_map <= b[3]
    np.testing.assert_array_equal(bits(mu_map), bits(got['mu']))                 # the same solves
    assert bits(got['mean']) == bits(L.mean32(got['per']))


@pytest.mark.parametrize('case', ['6x8', '8x8'])
def test_agrees_with_the_dense_kernels_where_they_reach(case):
    """Every y finite: a3dv_crf_loss_observed computes the same objective by dense pivoted elimination, a3d_crf_map the same
    mu.  Each kernel is within its own bound of float64, so the two are within the sum of them of each other:
    crf_loss_observed's is 8 x its restatement's error on these inputs, crf_map's 16 cond_inf(A) u
    (tests/test_gpu_crf_map.py)."""
    from ann3depth_amd import ops
    left, right, n, band = R.pairs(case)
    z, y, r = R.draw(case)
    ref, b = R.reference(case), R.bound(case)
    ref_v = V.nll64(z, y, r, left, right)
    b_v = [8 * float(x.max()) for x in V.errors(V.nll32(z, y, r, left, right), ref_v)]
    np.testing.assert_allclose(ref_v['per'], ref['per'], rtol=1e-10)             # the two float64 references agree
    np.testing.assert_allclose(ref_v['dr'], ref['dr'], rtol=1e-9, atol=1e-15)
    got = run(z, y, r, left, right, band)
    dense = ops.crf_loss_observed(dev(z), dev(y), dev(r), *pairs_dev(left, right))
    y_map, st = ops.crf_map(dev(z), dev(r), *pairs_dev(left, right))
    torch.cuda.synchronize()
    per_d, dz_d, dr_d = (dense[i].cpu().numpy() for i in (1, 2, 3))
    e = R.errors(got, dict(ref, per=per_d.astype(np.float64), dz=dz_d.astype(np.float64), dr=dr_d.astype(np.float64),
                           mu=y_map.cpu().numpy().astype(np.float64)))
    e = [float(x.max()) for x in e]
    cond = max(M.cond_inf(R.matrix(r[i], n, left, right)) for i in range(len(r)))
    b_map = 16 * cond * M.U
    print(f'crf_band {case} against crf_loss_observed / crf_map: loss {e[0]:.3g} (bounds {b[0]:.3g} + {b_v[0]:.3g}), dz '
          f'{e[1]:.3g} ({b[1]:.3g} + {b_v[1]:.3g}), dr {e[2]:.3g} ({b[2]:.3g} + {b_v[2]:.3g}), mu {e[3]:.3g} ({b[3]:.3g} + '
          f'{b_map:.3g})')
    assert not dense[5].cpu().numpy().any() and not st.cpu().numpy().any() and not got['status'].any()
    assert e[0] <= b[0] + b_v[0] and e[1] <= b[1] + b_v[1] and e[2] <= b[2] + b_v[2] and e[3] <= b[3] + b_map


def test_null_dr_and_null_mu_leave_the_other_bits_alone_and_two_runs_agree():
    left, right, n, band = R.pairs('5x13')
    z, y, r = R.draw('5x13')
    full = run(z, y, r, left, right, band)
    again = run(z, y, r, left, right, band)
    no_dr = run(z, y, r, left, right, band, pair_grad=False)
    no_mu = run(z, y, r, left, right, band, want_mu=False)
    neither = run(z, y, r, left, right, band, pair_grad=False, want_mu=False)
    assert no_dr['dr'] is None and no_mu['mu'] is None and neither['dr'] is None and neither['mu'] is None
    for other in (again, no_dr, no_mu, neither):
        for k in ('mean', 'per', 'dz', 'dr', 'mu', 'status'):
            if other[k] is not None:
                np.testing.assert_array_equal(bits(full[k]) if k != 'status' else full[k],
                                              bits(other[k]) if k != 'status' else other[k], err_msg=k)


@pytest.mark.parametrize('what', ['minus_one', 'nsp', 'too_far'])
def test_a_pair_that_cannot_be_used_turns_every_image_into_nan(what):
    """3x4 with band 4 and one more pair: an index of -1, of nsp, or a pair band + 1 apart.  It is skipped, never indexed
    with; outputs sit in NaN-filled allocations with guard elements on both sides, which stay as they were."""
    from ann3depth_amd import _lib
    lib = _lib.load()
    left, right, n, band = R.pairs('3x4')
    extra = {'minus_one': (-1, 2), 'nsp': (3, n), 'too_far': (1, 1 + band + 1)}[what]
    left, right = np.append(left, extra[0]), np.append(right, extra[1])
    z, y, r = R.draw('3x4')
    r = np.concatenate([r, np.full((3, 1), 0.5, F)], axis=1)
    B, Q = 3, len(left)
    zd, yd, rd = dev(z), dev(y), dev(r)
    l, rt = pairs_dev(left, right)
    g = 5
    per, mean = torch.full((B + 2 * g,), np.nan, device='cuda'), torch.full((1 + 2 * g,), np.nan, device='cuda')
    dz, mu = (torch.full((B * n + 2 * g,), np.nan, device='cuda') for _ in range(2))
    dr = torch.full((B * Q + 2 * g,), np.nan, device='cuda')
    st = torch.full((B + 2 * g,), -7, dtype=torch.int32, device='cuda')
    for t in (per, mean, dz, mu, dr):
        t[:g], t[-g:] = -7.25, -7.25
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.a3db_crf_band_nll(B, n, band, zd.data_ptr(), yd.data_ptr(), rd.data_ptr(), l.data_ptr(), rt.data_ptr(), Q,
                               per[g:].data_ptr(), mean[g:].data_ptr(), dz[g:].data_ptr(), dr[g:].data_ptr(),
                               mu[g:].data_ptr(), st[g:].data_ptr(), stream)
    torch.cuda.synchronize()
    assert rc == 0
    for t in (per, mean, dz, mu, dr):
        assert (t[:g] == -7.25).all() and (t[-g:] == -7.25).all() and torch.isnan(t[g:-g]).all()
    assert st.tolist() == [-7] * g + [1] * B + [-7] * g
    mu2, st2 = run_map(z, r, left, right, band)
    assert np.isnan(mu2).all() and st2.tolist() == [1] * B


def test_outputs_stay_inside_their_allocations():
    """A good call (5x13, batch 3) into NaN-filled buffers with guards: every output element is written, no guard is."""
    from ann3depth_amd import _lib
    lib = _lib.load()
    left, right, n, band = R.pairs('5x13')
    z, y, r = R.draw('5x13')
    B, Q, g = 3, len(left), 7
    zd, yd, rd = dev(z), dev(y), dev(r)
    l, rt = pairs_dev(left, right)
    per, mean = torch.full((B + 2 * g,), np.nan, device='cuda'), torch.full((1 + 2 * g,), np.nan, device='cuda')
    dz, mu, mu2 = (torch.full((B * n + 2 * g,), np.nan, device='cuda') for _ in range(3))
    dr = torch.full((B * Q + 2 * g,), np.nan, device='cuda')
    st, st2 = (torch.full((B + 2 * g,), -7, dtype=torch.int32, device='cuda') for _ in range(2))
    for t in (per, mean, dz, mu, mu2, dr):
        t[:g], t[-g:] = -7.25, -7.25
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.a3db_crf_band_nll(B, n, band, zd.data_ptr(), yd.data_ptr(), rd.data_ptr(), l.data_ptr(), rt.data_ptr(), Q,
                               per[g:].data_ptr(), mean[g:].data_ptr(), dz[g:].data_ptr(), dr[g:].data_ptr(),
                               mu[g:].data_ptr(), st[g:].data_ptr(), stream)
    rc2 = lib.a3db_crf_band_map(B, n, band, zd.data_ptr(), rd.data_ptr(), l.data_ptr(), rt.data_ptr(), Q, mu2[g:].data_ptr(),
                                st2[g:].data_ptr(), stream)
    torch.cuda.synchronize()
    assert rc == 0 and rc2 == 0
    for t in (per, mean, dz, mu, mu2, dr):
        assert (t[:g] == -7.25).all() and (t[-g:] == -7.25).all() and torch.isfinite(t[g:-g]).all()
    assert st.tolist() == st2.tolist() == [-7] * g + [0] * B + [-7] * g
    want = run(z, y, r, left, right, band)
    np.testing.assert_array_equal(bits(dr[g:-g].cpu().numpy().reshape(B, Q)), bits(want['dr']))
    np.testing.assert_array_equal(bits(mu2[g:-g].cpu().numpy().reshape(B, n)), bits(want['mu']))


def test_a_negative_first_pivot_is_nan_with_status_1_for_that_image_only():
    """6x8: superpixel 0 has no pair in the model's lists.  One more pair (0, 1) with r = 0 in images 0 and 2 and r = -10 in
    image 1, whose A[0][0] = 1 - 10 = -9 in any arithmetic: the first pivot.  Images 0 and 2 are the bits they are among
    accepted neighbours."""
    left, right, n, band = R.pairs('6x8')
    assert 0 not in set(left.tolist()) | set(right.tolist())
    left, right = np.append(left, 0), np.append(right, 1)
    z, y, r = R.draw('6x8')
    r = np.concatenate([r, np.zeros((3, 1), F)], axis=1)
    clean = run(z, y, r, left, right, band)
    r[1, -1] = -10.0
    got = run(z, y, r, left, right, band)
    mu_map, st_map = run_map(z, r, left, right, band)
    print(f'crf_band negative pivot: status {got["status"]}, losses {got["per"]}, map status {st_map}')
    assert got['status'].tolist() == [0, 1, 0] and st_map.tolist() == [0, 1, 0] and not clean['status'].any()
    assert np.isnan(got['mean']) and np.isnan(mu_map[1]).all()
    for k in ('per', 'dz', 'dr', 'mu'):
        assert np.isnan(got[k][1]).all(), k
        np.testing.assert_array_equal(bits(got[k][[0, 2]]), bits(clean[k][[0, 2]]), err_msg=k)


def test_an_overwritten_pair_has_dr_plus_zero_and_a_self_pair_too():
    """3x4 plus the pairs (l0, r0) again, reversed, and (5, 5): the first of the doubled pairs no longer owns its cell."""
    left, right, n, band = R.pairs('3x4')
    left, right = np.concatenate([left, [right[0], 5]]), np.concatenate([right, [left[0], 5]])
    z, y, r = R.draw('3x4')
    r = np.concatenate([r, np.array([[0.3, 0.9]] * 3, F)], axis=1)
    live = R.owners(left, right)
    assert not live[0] and live[-2] and not live[-1] and live[1:-1].all()
    ref = R.nll64(z, y, r, left, right)
    b = R.bound_of(z, y, r, left, right, band)
    got = run(z, y, r, left, right, band)
    e = [float(x.max()) for x in R.errors(got, ref)]
    print(f'crf_band overwritten / self pair: dr {got["dr"][0]}, errors {e} (bound {b})')
    assert (bits(got['dr'][:, 0]) == 0).all() and (bits(got['dr'][:, -1]) == 0).all() and (got['dr'][:, live] != 0).all()
    assert not got['status'].any() and all(x <= bx for x, bx in zip(e, b))


def test_a_nan_in_one_images_z_stays_in_that_image():
    left, right, n, band = R.pairs('12x16')
    z, y, r = (np.array(a) for a in R.draw('12x16'))
    clean = run(z, y, r, left, right, band)
    z[1, 100] = np.nan
    got = run(z, y, r, left, right, band)
    mu_map, st_map = run_map(z, r, left, right, band)
    assert got['status'].tolist() == [0, 1, 0] and st_map.tolist() == [0, 1, 0]
    assert np.isnan(got['per'][1]) and np.isnan(got['dz'][1]).all() and np.isnan(got['mu'][1]).all() and np.isnan(mu_map[1]).all()
    for k in ('per', 'dz', 'dr', 'mu'):
        np.testing.assert_array_equal(bits(got[k][[0, 2]]), bits(clean[k][[0, 2]]), err_msg=k)


def test_the_binding_checks_shapes_and_dtypes():
    from ann3depth_amd import ops
    left, right, n, band = R.pairs('3x4')
    z, y, r = (dev(a) for a in R.draw('3x4'))
    l, rt = pairs_dev(left, right)
    for bad in (lambda: ops.crf_band_nll(z, y[:2], r, l, rt, band), lambda: ops.crf_band_nll(z, y, r[:, :3], l, rt, band),
                lambda: ops.crf_band_nll(z, y, r, l, rt, 0), lambda: ops.crf_band_nll(z, y, r, l, rt, 33),
                lambda: ops.crf_band_map(z, r, l, rt[:3], band), lambda: ops.crf_band_map(z.t(), r, l, rt, band)):
        with pytest.raises(ValueError):
            bad()
    for bad in (lambda: ops.crf_band_nll(z.double(), y, r, l, rt, band), lambda: ops.crf_band_map(z, r, l.long(), rt, band)):
        with pytest.raises(TypeError):
            bad()
