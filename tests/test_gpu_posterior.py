"""a3dc_crf_band_posterior on the GPU (include/a3d_posterior.h) against the float64 covariance form of
tests/posterior_ref.py: mean and var within 8 x the error of the float32 restatement of the kernel's own arithmetic on the
same inputs, never less than one ulp (the bounds are computed on the CPU); the cases the header calls exact, bit for bit;
the dense kernel where it reaches; and every edge the header states.  Each test prints the figures it saw before it
asserts."""
import ctypes

import numpy as np
import pytest
import torch

import crf_band_ref as R
import crf_observed_ref as V
import posterior_ref as P

pytestmark = pytest.mark.gpu

F = np.float32


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def pairs_dev(left, right):
    return dev(np.asarray(left, np.int32)), dev(np.asarray(right, np.int32))


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def run(z, y, r, left, right, band, want_var=True):
    """-> dict(mean, var, nobs, status) as numpy."""
    from ann3depth_amd import ops
    out = ops.crf_band_posterior(dev(z), None if y is None else dev(y), dev(r), *pairs_dev(left, right), band,
                                 want_var=want_var)
    torch.cuda.synchronize()
    mean, var, nobs, status = (None if t is None else t.cpu().numpy() for t in out)
    return dict(mean=mean, var=var, nobs=nobs, status=status)


def run_map(z, r, left, right, band):
    from ann3depth_amd import ops
    mu, status = ops.crf_band_map(dev(z), dev(r), *pairs_dev(left, right), band)
    torch.cuda.synchronize()
    return mu.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize('name', P.MASKS)
@pytest.mark.parametrize('case', R.CASES)
def test_mean_and_variance_match_float64(case, name):
    left, right, n, band = R.pairs(case)
    assert R.positive_definite(case)
    z, y, r = P.draw(case, name)
    obs = P.mask(case, name)
    ref, b = P.reference(case, name), P.bound(case, name)
    got = run(z, y, r, left, right, band)
    e = [float(x.max()) for x in P.errors(got, ref)]
    print(f'posterior {case} {name} (n {n}, band {band}, batch {len(z)}, observed {obs.sum(axis=1).tolist()}): mean '
          f'{e[0]:.3g} (bound {b[0]:.3g}, ratio {e[0] / b[0]:.2f}), var {e[1]:.3g} (bound {b[1]:.3g}, ratio {e[1] / b[1]:.2f})')
    assert not got['status'].any() and np.isfinite(got['mean']).all() and np.isfinite(got['var']).all()
    assert got['nobs'].tolist() == obs.sum(axis=1).tolist()
    assert e[0] <= b[0] and e[1] <= b[1]
    np.testing.assert_array_equal(bits(got['mean'])[obs], bits(y)[obs])          # observed entries carry y's bits
    assert (bits(got['var'])[obs] == 0).all() and (got['var'][~obs] > 0).all()


@pytest.mark.parametrize('case', ['3x4', '5x13', '12x16', '24x32', 'chain32'])
def test_nothing_observed_is_the_map_launch_bit_for_bit(case):
    """y = NULL, and y given with no entry finite (NaN, +inf, -inf, payloads): mean is a3db_crf_band_map's mu."""
    left, right, n, band = R.pairs(case)
    z, y, r = P.draw(case, 'none')
    mu, st = run_map(z, r, left, right, band)
    by_null = run(z, None, r, left, right, band)
    by_nan = run(z, y, r, left, right, band)
    junk = np.array(y)
    junk.view(np.uint32)[:, ::3] = 0x7fc12345
    junk[:, 1::3], junk[:, 2::3] = np.inf, -np.inf
    by_junk = run(z, junk, r, left, right, band)
    assert not st.any()
    for other in (by_null, by_nan, by_junk):
        np.testing.assert_array_equal(bits(other['mean']), bits(mu))
        np.testing.assert_array_equal(bits(other['var']), bits(by_null['var']))
        assert other['nobs'].tolist() == [0] * len(z) and not other['status'].any()


def test_everything_observed_gives_y_back_and_zero_variance():
    left, right, n, band = R.pairs('12x16')
    z, y, r = P.draw('12x16', 'all')
    got = run(z, y, r, left, right, band)
    np.testing.assert_array_equal(bits(got['mean']), bits(y))
    assert (bits(got['var']) == 0).all() and got['nobs'].tolist() == [n] * len(z) and not got['status'].any()


def test_hidden_values_null_var_and_a_second_run_change_no_bit():
    """5x13 random: other NaN payloads, +-inf in the hidden entries; var = NULL; the same call again."""
    left, right, n, band = R.pairs('5x13')
    z, y, r = P.draw('5x13', 'random')
    obs = P.mask('5x13', 'random')
    full = run(z, y, r, left, right, band)
    again = run(z, y, r, left, right, band)
    junk = np.array(y)
    hidden = np.flatnonzero(~obs.ravel())
    flat = junk.reshape(-1)
    flat.view(np.uint32)[hidden[0::3]] = 0xffc00001
    flat[hidden[1::3]], flat[hidden[2::3]] = np.inf, -np.inf
    assert not np.isfinite(junk[~obs]).any() and (bits(junk)[obs] == bits(y)[obs]).all()
    other = run(z, junk, r, left, right, band)
    no_var = run(z, y, r, left, right, band, want_var=False)
    assert no_var['var'] is None
    for o in (again, other, no_var):
        np.testing.assert_array_equal(bits(o['mean']), bits(full['mean']))
        np.testing.assert_array_equal(o['nobs'], full['nobs'])
        np.testing.assert_array_equal(o['status'], full['status'])
        if o['var'] is not None:
            np.testing.assert_array_equal(bits(o['var']), bits(full['var']))


@pytest.mark.parametrize('case', ['6x8', '8x8'])
@pytest.mark.parametrize('name', ['row', 'random', 'interior'])
def test_agrees_with_the_dense_kernel_where_it_reaches(case, name):
    """mean - mu = -B/2 dz of a3dv_crf_loss_observed, which conditions by dense pivoted elimination.  Each side is within
    its own bound of float64 (the dense kernel's: 8 x its restatement's dz error on these inputs, relative to ||dz||inf),
    so the two are within the sum of them, each scaled to its own norm."""
    from ann3depth_amd import ops
    left, right, n, band = R.pairs(case)
    z, y, r = P.draw(case, name)
    obs = P.mask(case, name)
    B = len(z)
    ref = P.reference(case, name)
    ref_v = V.nll64(z, y, r, left, right)
    b_v = 8 * float(V.errors(V.nll32(z, y, r, left, right), ref_v)[1].max())
    b_p = P.bound(case, name)[0]
    got = run(z, y, r, left, right, band)
    dense = ops.crf_loss_observed(dev(z), dev(y), dev(r), *pairs_dev(left, right))
    torch.cuda.synchronize()
    q_dense = -0.5 * B * dense[2].cpu().numpy().astype(np.float64)
    q_ref = ref['mean'] - ref['mu']
    assert not dense[5].cpu().numpy().any() and not got['status'].any()
    worst = 0.0
    for i in range(B):
        M = ~obs[i]
        diff = np.abs((got['mean'][i, M].astype(np.float64) - ref['mu'][i, M]) - q_dense[i, M]).max()
        allowed = b_p * np.abs(ref['mean'][i, M]).max() + b_v * np.abs(q_ref[i]).max()
        worst = max(worst, diff / allowed)
        assert diff <= allowed, (i, diff, allowed)
    print(f'posterior {case} {name} against crf_loss_observed: worst difference / (bound {b_p:.3g} x ||mean_M|| + bound '
          f'{b_v:.3g} x ||q||) = {worst:.3f}')


def _guarded(B, n, g=5):
    mean, var = (torch.full((B * n + 2 * g,), np.nan, device='cuda') for _ in range(2))
    nobs, st = (torch.full((B + 2 * g,), -7, dtype=torch.int32, device='cuda') for _ in range(2))
    for t in (mean, var):
        t[:g], t[-g:] = -7.25, -7.25
    return mean, var, nobs, st


@pytest.mark.parametrize('what', ['minus_one', 'nsp', 'too_far'])
def test_a_pair_that_cannot_be_used_turns_every_image_into_nan(what):
    """3x4 with band 4 and one more pair: an index of -1, of nsp, or a pair band + 1 apart.  It is skipped, never indexed
    with; the outputs sit between guard elements, which stay as they were."""
    from ann3depth_amd import _lib
    lib = _lib.load()
    left, right, n, band = R.pairs('3x4')
    extra = {'minus_one': (-1, 2), 'nsp': (3, n), 'too_far': (1, 1 + band + 1)}[what]
    left, right = np.append(left, extra[0]), np.append(right, extra[1])
    z, y, r = P.draw('3x4', 'random')
    r = np.concatenate([r, np.full((3, 1), 0.5, F)], axis=1)
    B, Q, g = 3, len(left), 5
    zd, yd, rd = dev(z), dev(y), dev(r)
    l, rt = pairs_dev(left, right)
    mean, var, nobs, st = _guarded(B, n, g)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.a3dc_crf_band_posterior(B, n, band, zd.data_ptr(), yd.data_ptr(), rd.data_ptr(), l.data_ptr(), rt.data_ptr(), Q,
                                     mean[g:].data_ptr(), var[g:].data_ptr(), nobs[g:].data_ptr(), st[g:].data_ptr(), stream)
    torch.cuda.synchronize()
    assert rc == 0
    for t in (mean, var):
        assert (t[:g] == -7.25).all() and (t[-g:] == -7.25).all() and torch.isnan(t[g:-g]).all()
    assert st.tolist() == [-7] * g + [1] * B + [-7] * g
    assert nobs.tolist() == [-7] * g + P.mask('3x4', 'random').sum(axis=1).tolist() + [-7] * g


def test_outputs_stay_inside_their_allocations():
    """A good call (5x13 checker, batch 3) into NaN-filled buffers with guards: every element is written, no guard is."""
    from ann3depth_amd import _lib
    lib = _lib.load()
    left, right, n, band = R.pairs('5x13')
    z, y, r = P.draw('5x13', 'checker')
    B, Q, g = 3, len(left), 7
    zd, yd, rd = dev(z), dev(y), dev(r)
    l, rt = pairs_dev(left, right)
    mean, var, nobs, st = _guarded(B, n, g)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.a3dc_crf_band_posterior(B, n, band, zd.data_ptr(), yd.data_ptr(), rd.data_ptr(), l.data_ptr(), rt.data_ptr(), Q,
                                     mean[g:].data_ptr(), var[g:].data_ptr(), nobs[g:].data_ptr(), st[g:].data_ptr(), stream)
    torch.cuda.synchronize()
    assert rc == 0
    for t in (mean, var):
        assert (t[:g] == -7.25).all() and (t[-g:] == -7.25).all() and torch.isfinite(t[g:-g]).all()
    assert st.tolist() == [-7] * g + [0] * B + [-7] * g
    assert nobs.tolist() == [-7] * g + P.mask('5x13', 'checker').sum(axis=1).tolist() + [-7] * g
    want = run(z, y, r, left, right, band)
    np.testing.assert_array_equal(bits(mean[g:-g].cpu().numpy().reshape(B, n)), bits(want['mean']))
    np.testing.assert_array_equal(bits(var[g:-g].cpu().numpy().reshape(B, n)), bits(want['var']))


def test_a_negative_first_pivot_is_nan_with_status_1_for_that_image_only():
    """6x8: superpixel 0 has no pair in the model's lists.  One more pair (0, 1) with r = 0 in images 0 and 2 and r = -10 in
    image 1, whose A[0][0] = 1 - 10 = -9 in any arithmetic; superpixels 0 and 1 are hidden, so it is A' 's first pivot."""
    left, right, n, band = R.pairs('6x8')
    assert 0 not in set(left.tolist()) | set(right.tolist())
    left, right = np.append(left, 0), np.append(right, 1)
    z, y, r = P.draw('6x8', 'checker')
    y = np.array(y)
    y[:, :2] = np.nan
    r = np.concatenate([r, np.zeros((3, 1), F)], axis=1)
    clean = run(z, y, r, left, right, band)
    r[1, -1] = -10.0
    got = run(z, y, r, left, right, band)
    print(f'posterior negative pivot: status {got["status"]}, nobs {got["nobs"]}')
    assert got['status'].tolist() == [0, 1, 0] and not clean['status'].any()
    np.testing.assert_array_equal(got['nobs'], clean['nobs'])
    for k in ('mean', 'var'):
        assert np.isnan(got[k][1]).all(), k
        np.testing.assert_array_equal(bits(got[k][[0, 2]]), bits(clean[k][[0, 2]]), err_msg=k)


def test_a_nan_in_one_images_z_stays_in_that_image():
    left, right, n, band = R.pairs('12x16')
    z, y, r = (np.array(a) for a in P.draw('12x16', 'random'))
    hidden = int(np.flatnonzero(~P.mask('12x16', 'random')[1])[3])
    clean = run(z, y, r, left, right, band)
    z[1, hidden] = np.nan
    got = run(z, y, r, left, right, band)
    assert got['status'].tolist() == [0, 1, 0]
    for k in ('mean', 'var'):
        assert np.isnan(got[k][1]).all(), k
        np.testing.assert_array_equal(bits(got[k][[0, 2]]), bits(clean[k][[0, 2]]), err_msg=k)


def test_the_binding_checks_shapes_and_dtypes():
    from ann3depth_amd import ops
    left, right, n, band = R.pairs('3x4')
    z, y, r = (dev(a) for a in P.draw('3x4', 'random'))
    l, rt = pairs_dev(left, right)
    for bad in (lambda: ops.crf_band_posterior(z, y[:2], r, l, rt, band), lambda: ops.crf_band_posterior(z, y[:, :5], r, l, rt, band),
                lambda: ops.crf_band_posterior(z, y, r[:, :3], l, rt, band), lambda: ops.crf_band_posterior(z, y, r, l, rt, 0),
                lambda: ops.crf_band_posterior(z, y, r, l, rt, 33), lambda: ops.crf_band_posterior(z, y, r, l, rt[:3], band),
                lambda: ops.crf_band_posterior(z, y.t().contiguous().t(), r, l, rt, band),
                lambda: ops.crf_band_posterior(z, y, r, l, rt, band, mean=torch.empty((3, n + 1), device='cuda')),
                lambda: ops.crf_band_posterior(z, y, r, l, rt, band, want_var=False, var=torch.empty_like(z)),
                lambda: ops.crf_band_posterior(z, y.cpu(), r, l, rt, band)):
        with pytest.raises(ValueError):
            bad()
    for bad in (lambda: ops.crf_band_posterior(z, y.double(), r, l, rt, band),
                lambda: ops.crf_band_posterior(z.double(), y, r, l, rt, band),
                lambda: ops.crf_band_posterior(z, y, r, l.long(), rt, band),
                lambda: ops.crf_band_posterior(z, y.cpu().numpy(), r, l, rt, band),
                lambda: ops.crf_band_posterior(z, y, r, l, rt, band, var=torch.empty_like(z, dtype=torch.float64))):
        with pytest.raises(TypeError):
            bad()
