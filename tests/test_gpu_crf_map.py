"""a3d_crf_map on the GPU against the float64 reference of tests/crf_map_ref.py.

With u = 2^-24, A the float64 system built from the float32 pair weights and y_hat the kernel's result, every image is
held to
  * the normwise backward error  ||A y_hat - z||inf / (||A||inf ||y_hat||inf + ||z||inf) <= 8 u: the measure a pivoted LU
    answers for, whatever cond(A) is.  A float32 emulation of the algorithm on a CPU stays below 1.6 u; 8 u leaves room
    for another summation order and is seven orders of magnitude below what a wrong solve gives;
  * the forward error  ||y_hat - y||inf / ||y||inf <= 16 cond_inf(A) u, which follows from the first.
Each test prints the worst figures it saw before it asserts."""
import ctypes

import numpy as np
import pytest
import torch

import crf_map_ref as R

pytestmark = pytest.mark.gpu

GRIDS = [(6, 8), (3, 4), (8, 8)]                 # the model's, a small one, and nsp = 64: the limit
REGIMES = {'reference': (-0.1, 0.7), 'unsaturated': (2.0, 2.3), 'indefinite': (-1.4, 1.4), 'stiff': (0.0, 50.0)}
# 'reference' and 'unsaturated' are the two regimes of tests/test_gpu_dcnf.py::test_crf_loss_and_gradient_match_oracle


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pairs_dev(left, right):
    return dev(np.asarray(left, np.int32)), dev(np.asarray(right, np.int32))


def run(z, r, left, right):
    from ann3depth_amd import ops
    y, status = ops.crf_map(dev(z), dev(r), *pairs_dev(left, right))
    torch.cuda.synchronize()
    return y.cpu().numpy(), status.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize('regime', list(REGIMES))
@pytest.mark.parametrize('batch', [1, 5, 64])
@pytest.mark.parametrize('rows,cols', GRIDS)
def test_map_depths_solve_the_float64_system(rows, cols, batch, regime):
    left, right = R.pairs(rows, cols)
    nsp = rows * cols
    lo, hi = REGIMES[regime]
    rng = np.random.default_rng(1000 * nsp + 10 * batch + list(REGIMES).index(regime))
    r = rng.uniform(lo, hi, (batch, len(left))).astype(np.float32)
    z = rng.standard_normal((batch, nsp)).astype(np.float32)
    y_hat, status = run(z, r, left, right)
    want = R.solve(z, r, left, right)
    worst_b = worst_f = worst_c = 0.0
    for b in range(batch):
        A = R.matrix(r[b], nsp, left, right)
        cond = R.cond_inf(A)
        be, fe = R.backward_error(A, y_hat[b], z[b]), R.forward_error(y_hat[b], want[b])
        worst_b, worst_f, worst_c = max(worst_b, be / R.U), max(worst_f, fe / (cond * R.U)), max(worst_c, cond)
    print(f'crf_map {rows}x{cols} batch {batch} {regime}: backward {worst_b:.3f} u, forward {worst_f:.3f} cond u, '
          f'cond_inf <= {worst_c:.3g}')
    assert (status == 0).all() and np.isfinite(y_hat).all()
    assert worst_b <= 8 and worst_f <= 16
    if (rows, cols) == (6, 8) and regime in ('reference', 'unsaturated'):
        assert worst_c <= 20
        assert max(R.forward_error(y_hat[b], want[b]) for b in range(batch)) <= 2e-5


@pytest.mark.parametrize('rows,cols', GRIDS)
def test_no_pair_weights_return_z_bit_for_bit(rows, cols):
    left, right = R.pairs(rows, cols)
    rng = np.random.default_rng(7)
    z = rng.standard_normal((5, rows * cols)).astype(np.float32)
    z[0, 0], z[1, 3] = 0.0, np.float32(1e-42)                       # a zero and a subnormal survive too
    y, status = run(z, np.zeros((5, len(left)), np.float32), left, right)
    np.testing.assert_array_equal(bits(y), bits(z))
    assert (status == 0).all()


def test_a_poisoned_image_is_all_nan_and_the_others_do_not_notice():
    left, right = R.pairs(6, 8)
    rng = np.random.default_rng(8)
    r = rng.uniform(-0.1, 0.7, (5, 48)).astype(np.float32)
    z = rng.standard_normal((5, 48)).astype(np.float32)
    clean, status = run(z, r, left, right)
    assert (status == 0).all()
    r2, z2 = r.copy(), z.copy()
    r2[1, 17] = np.nan
    z2[3, 40] = np.inf
    y, status = run(z2, r2, left, right)
    assert status.tolist() == [0, 1, 0, 1, 0]
    assert np.isnan(y[1]).all() and np.isnan(y[3]).all()
    np.testing.assert_array_equal(bits(y[[0, 2, 4]]), bits(clean[[0, 2, 4]]))


def test_an_exactly_singular_system_is_flagged():
    """Two nodes, one pair, r = -0.5: A = [[.5, .5], [.5, .5]], the second pivot is exactly 0."""
    z = np.array([[1.0, 2.0], [1.0, 2.0]], np.float32)
    r = np.array([[-0.5], [0.75]], np.float32)
    y, status = run(z, r, [0], [1])
    assert status.tolist() == [1, 0]
    assert np.isnan(y[0]).all()
    np.testing.assert_allclose(y[1], R.solve(z[1:], r[1:], [0], [1])[0], rtol=1e-6)


@pytest.mark.parametrize('left,right', [([0, 7], [1, 1]), ([0, 0], [1, -1]), ([2, 0], [1, 1])])
def test_a_pair_index_outside_the_grid_flags_every_image_and_is_not_used(left, right):
    """left / right are the batch's: an index outside [0, nsp) is skipped before anything is indexed with it, and every
    image comes back all-NaN with status 1; guard elements stay as they were."""
    from ann3depth_amd import ops
    n, nsp = 3, 2
    z = dev(np.array([[1.0, 2.0]] * n, np.float32))
    r = dev(np.full((n, 2), 0.75, np.float32))
    ybuf = torch.full(((n + 2) * nsp,), -7.25, device='cuda')
    sbuf = torch.full((n + 2,), -77, dtype=torch.int32, device='cuda')
    y, status = ybuf[nsp:nsp + n * nsp].view(n, nsp), sbuf[1:1 + n]
    ops.crf_map(z, r, *pairs_dev(left, right), y, status)
    torch.cuda.synchronize()
    assert status.tolist() == [1] * n and torch.isnan(y).all()
    assert (ybuf[:nsp] == -7.25).all() and (ybuf[nsp + n * nsp:] == -7.25).all() and sbuf[0] == -77 and sbuf[-1] == -77


def test_the_binding_refuses_output_buffers_of_the_wrong_kind():
    from ann3depth_amd import ops
    left, right = pairs_dev(*R.pairs(3, 4))
    z, r = torch.zeros((2, 12), device='cuda'), torch.zeros((2, 4), device='cuda')
    ok_s = torch.empty((2,), dtype=torch.int32, device='cuda')
    with pytest.raises(ValueError):
        ops.crf_map(z, r, left, right, torch.empty((2, 11), device='cuda'), ok_s)
    with pytest.raises(ValueError):
        ops.crf_map(z, r, left, right, torch.empty((2, 24), device='cuda')[:, ::2], ok_s)
    with pytest.raises(TypeError):
        ops.crf_map(z, r, left, right, torch.empty((2, 12), device='cuda'), torch.empty((2,), device='cuda'))
    with pytest.raises(ValueError):
        ops.crf_map(z, r, left, right, torch.empty((2, 12), device='cuda'),
                    torch.empty((3,), dtype=torch.int32, device='cuda'))
    with pytest.raises(ValueError):
        ops.crf_map(z, r, left, right.cpu())


def test_guards_repeatability_and_null_status():
    from ann3depth_amd import _lib, ops
    lib = _lib.load()
    left, right = R.pairs(8, 8)
    n, nsp = 5, 64
    rng = np.random.default_rng(9)
    r = dev(rng.uniform(-0.1, 0.7, (n, len(left))).astype(np.float32))
    z = dev(rng.standard_normal((n, nsp)).astype(np.float32))
    l, rt = pairs_dev(left, right)
    ybuf = torch.full(((n + 2) * nsp,), -7.25, device='cuda')                   # one guard row on each side
    sbuf = torch.full((n + 2,), -77, dtype=torch.int32, device='cuda')
    y, status = ybuf[nsp:nsp + n * nsp].view(n, nsp), sbuf[1:1 + n]
    ops.crf_map(z, r, l, rt, y, status)
    first_y, first_s = ybuf.clone(), sbuf.clone()
    ops.crf_map(z, r, l, rt, y, status)
    torch.cuda.synchronize()
    assert torch.equal(first_y, ybuf) and torch.equal(first_s, sbuf)            # the same bits on every run
    assert (ybuf[:nsp] == -7.25).all() and (ybuf[nsp + n * nsp:] == -7.25).all()
    assert sbuf[0] == -77 and sbuf[-1] == -77 and (status == 0).all()
    assert torch.isfinite(y).all()
    # status = NULL: y alone
    y2 = torch.full_like(y, 3.0)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.a3d_crf_map(n, nsp, z.data_ptr(), r.data_ptr(), l.data_ptr(), rt.data_ptr(), len(left), y2.data_ptr(), None,
                         stream)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(y2, y)
    # fewer images than the buffers hold: rows past n stay as they were
    y3 = torch.full_like(y, 3.0)
    s3 = torch.full((n,), -5, dtype=torch.int32, device='cuda')
    assert lib.a3d_crf_map(2, nsp, z.data_ptr(), r.data_ptr(), l.data_ptr(), rt.data_ptr(), len(left), y3.data_ptr(),
                           s3.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(y3[:2], y[:2]) and (y3[2:] == 3.0).all() and s3.tolist() == [0, 0, -5, -5, -5]
